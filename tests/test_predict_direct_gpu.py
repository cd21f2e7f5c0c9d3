"""ocf_predict_entries through the library's C entry point, against the NumPy fp64 restatement and the derived
bounds of tests/predict_ref.py, over every compiled instance: the (weight type, H, layout) points of
gather_ref.GRID (the register form: f16 / bf16 at H = 128 (16,1), 256 (32,1), 384 (16,3), 512 (32,2), row-major
and 64x64-blocked; f32 at (32,1) .. (32,4)) and the slab form at H = 640 (a short last slab) and 1024, f32 and f16.

One batch per H (gather_ref.make_batch: B = 20 + 3 padding rows, N = 1000, ~4,000 entries, rows of 0 / 1 / 7 / 255 /
256 / 257 / 700 entries, a -1 row, duplicated columns).  Per point: aux in {-1, 1} x clip off / [0.5, 5] x flag on /
off, and val null.  y is prefilled with NaN (an entry never written is an infinite error) and carries guard elements
past E; row_stats and total are prefilled with NaN too.  tests/test_predict_ref.py shows on the CPU that the bounds
reject seven plausible bugs.

Worst observed error / bound over the grid (MI355X, this file's own run; recorded, not used to set a bound): y 0.0057
(f16; f32 0.0056, bf16 0.0055), row_stats 0.020, total 0.076.  Exact comparisons (guard elements, rows without
entries and padding rows, two runs, y under chunk 64 against 256, y with val null): no mismatch.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gather_ref as G
import predict_ref as P
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

CD = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


@functools.lru_cache(maxsize=None)
def device_case(wt, H, bl):
    """the H fixture, both chunk tables, the packed decoder weight and the hidden rows on the device (shared, never
    written)"""
    fx = G.make_batch(H)
    _, _, po, Woutr = G.weights_for(wt, H, bl)
    h32, hr = P.hidden(fx, wt)
    t = SimpleNamespace(**{k: dev(getattr(fx, k)) for k in ("rows", "rp", "col", "val", "lboff", "flag", "bias_out")})
    cts = {}
    for chunk in (P.CHUNK, P.CHUNK_ALT):
        ct = G.chunks_for(H, chunk)
        cts[chunk] = (ct, SimpleNamespace(**{k: dev(getattr(ct, k)) for k in ("ch_row", "ch_j0", "ch_j1")}))
    return SimpleNamespace(fx=fx, wt=wt, H=H, bl=bl, t=t, cts=cts, W=dev(po), Wr=Woutr, h=dev(h32).to(TD[wt]), hr=hr)


def launch(d, chunk, aux, clip, use_flag, with_val=True):
    """one call on NaN-prefilled outputs -> (y [E + GUARD], row_stats [Bp][4] or None, total [4] or None) on the host
    as float32 bit patterns kept (numpy float32)"""
    fx, t = d.fx, d.t
    ct, ctd = d.cts[chunk]
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    y, cs, rs, tot = nan(fx.E + P.GUARD), nan(ct.n_chunks, 4), nan(fx.Bp, 4), nan(4)
    a = _lib.OcfPredictArgs()
    a.rows, a.rp, a.col, a.lboff = t.rows.data_ptr(), t.rp.data_ptr(), t.col.data_ptr(), t.lboff.data_ptr()
    a.val = t.val.data_ptr() if with_val else None
    a.flag = t.flag.data_ptr() if use_flag else None
    a.ch_row, a.ch_j0, a.ch_j1, a.n_chunks = ctd.ch_row.data_ptr(), ctd.ch_j0.data_ptr(), ctd.ch_j1.data_ptr(), ct.n_chunks
    a.B, a.Bp = fx.B, fx.Bp
    a.h, a.h_dtype, a.ldh, a.H = d.h.data_ptr(), CD[d.wt], d.H, d.H
    a.W, a.w_dtype, a.ldw, a.w_blocked = d.W.data_ptr(), CD[d.wt], d.H, d.bl
    a.bias, a.aux = t.bias_out.data_ptr(), aux
    if clip:
        a.clip, a.clip_lo, a.clip_hi = 1, clip[0], clip[1]
    a.y = y.data_ptr()
    if with_val:
        a.chunk_stats, a.row_stats, a.total = cs.data_ptr(), rs.data_ptr(), tot.data_ptr()
    _lib.call("ocf_predict_entries", a, cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")
    if not with_val:
        assert torch.isnan(rs).all() and torch.isnan(tot).all() and torch.isnan(cs).all()
        return y.cpu().numpy(), None, None
    return y.cpu().numpy(), rs.cpu().numpy(), tot.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("wt,H,bl", P.GRID, ids=P.GRID_IDS)
def test_predict_entries_direct(gpu, wt, H, bl):
    d = device_case(wt, H, bl)
    fx = d.fx
    rep = G.Report()
    for aux in (1.0, -1.0):
        for clip in (None, P.CLIP):
            for use_flag in (True, False):
                what = "aux %g clip %s flag %d" % (aux, "on" if clip else "off", use_flag)
                ct = d.cts[P.CHUNK][0]
                ref = P.reference(fx, ct, d.hr, d.Wr, aux, clip, use_flag)
                y, rs, tot = launch(d, P.CHUNK, aux, clip, use_flag)
                P.check(rep, fx, ref, y, rs, tot, stage=what)
                # two runs are bit-identical
                y2, rs2, tot2 = launch(d, P.CHUNK, aux, clip, use_flag)
                assert same_bits(y, y2) and same_bits(rs, rs2) and same_bits(tot, tot2), what
                # another chunk length: the entries are independent, so y is bit-identical; the statistics are summed in
                # another order and stay within their bounds
                ct2 = d.cts[P.CHUNK_ALT][0]
                y3, rs3, tot3 = launch(d, P.CHUNK_ALT, aux, clip, use_flag)
                assert same_bits(y, y3), what
                P.check(rep, fx, P.reference(fx, ct2, d.hr, d.Wr, aux, clip, use_flag), y3, rs3, tot3,
                        stage=what + " chunk %d" % P.CHUNK_ALT)
            # val null: the same y, no statistics written
            y4, _, _ = launch(d, P.CHUNK, aux, clip, True, with_val=False)
            assert same_bits(y, y4), "aux %g clip %s val null" % (aux, clip)
    for check, r, _ in rep:
        print("PREDICT_RATIO %s | %s | %.4g" % (wt, check, r))
    w, r, i = rep.worst()
    assert not rep.failures(), "worst error / bound %.4g in '%s' at index %s; all: %s" % (r, w, i, rep.failures())
