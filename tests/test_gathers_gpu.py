"""The sparse row gathers, one stage at a time through the library's C entry points, against the NumPy fp64
restatements and derived bounds of tests/gather_ref.py: ocf_gather_encoder, ocf_rows_reduce (RAW / BIAS_ACT /
GRAD_ACT), ocf_gather_decoder (plain, and with the hidden epilogue + the folded row reduction), ocf_gather_encdec
(chunked and row-resident) and ocf_rank_step phases 0 / 1 (the row-resident RAW forms), over every compiled
(weight type, G, PPL) instance: f16 / bf16 at H = 128 (16,1), 256 (32,1), 384 (16,3), 512 (32,2), row-major and
64x64-blocked; f32 at H = 128 (32,1), 256 (32,2), 384 (32,3), 512 (32,4); chunk 64 / 96 / 64 / 256.

One batch per H (gather_ref.make_batch: ~20 rows, ~4,000 entries, rows of 0 / 1 / 7 / 255 / 256 / 257 / 700
entries, a row without inputs, one without targets, duplicates, an exact t + y == 0).  Every output buffer is
filled with NaN (0xFF for bytes) before each launch; every stage's reference starts from the previous stage's
DEVICE output.  tests/test_gather_ref.py shows on the CPU that the bounds reject twelve plausible bugs.

Worst observed error / bound per stage and weight type (MI355X, this file's own run; recorded, not used to set a
bound; the stages that store in a 16-bit dtype sit near 1 by construction: the bound of a rounding is half an ulp,
and so does the fp32 h with dropout: a / keep is correctly rounded, its bound is u |ref|, "1" is 0.9998):

    check                                               f32      f16     bf16
    encoder: part                                     0.328   0.0222    0.054
    reduce: RAW                                       0.342    0.291    0.247
    reduce: a_out                                     0.251    0.251    0.251
    reduce: h                                             1    0.998    0.993
    reduce: hidden delta                              0.423    0.996    0.989
    reduce: db_part                                   0.471     0.47    0.395
    reduce: stats_part                                0.251    0.251    0.251
    decoder: delta_e                                  0.267    0.267    0.267
    decoder: d_out                                        0    0.996    0.995
    decoder: part                                     0.326    0.328    0.326
    decoder: chunk_stats                             0.0226   0.0234   0.0228
    fused: a_out                                       0.25     0.25     0.25
    fused: h                                          0.999    0.998    0.988
    fused: delta_e                                   0.0467    0.059   0.0467
    fused: d_out                                          0    0.992    0.994
    fused: hidden delta                               0.383    0.961    0.987
    fused: db_part                                    0.379    0.375    0.364
    fused: stats_part                               0.00928   0.0155   0.0133
    fused: part                                      0.0277   0.0409   0.0346
    encdec: a_out                                     0.243    0.225     0.24
    encdec: h                                         0.999    0.998    0.988
    encdec: delta_e                                   0.111    0.132    0.111
    encdec: d_out                                         0     0.99    0.987
    encdec: hidden delta                              0.384     0.98    0.988
    encdec: db_part                                   0.364    0.388    0.447
    encdec: stats_part                               0.0165   0.0364    0.037
    rank: encoder row sums                            0.237  0.00553        -
    rank: a_out                                        0.23    0.235        -
    rank: h                                               1    0.998        -
    rank: delta_e                                   0.00663  0.00816        -
    rank: row sums                                    0.241    0.224        -
    rank: stats_part                                0.00641  0.00639        -
    rank: finalized stats                            0.0504   0.0286        -
    Exact comparisons (masks 0 / 1 and equal to the standalone reduction's, delta_e off the targets, d_out
    untouched elsewhere, row_sse, rows without entries, arrival counters, finalized row SSE): no mismatch.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import epilogue_ref as R
import gather_ref as G
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

CD = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SEED, STREAM = 1234, 5
# grid points whose fused launches run tanh on a zero hidden bias: the row without inputs then has h == 0 exactly
# and its engineered target t + y == 0 (sigmoid and the fixture's bias elsewhere)
ZERO_HIDDEN_AT = {("bf16", 256, 1), ("f32", 256, 0), ("f16", 128, 0)}


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def host(t):
    if t is None:
        return None
    return t.float().cpu().numpy().astype(np.float64) if t.is_floating_point() else t.cpu().numpy()


def nan32(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def nan_ct(cd, *shape):
    return nan32(*shape).to(TD[cd])


def ff8(*shape):
    return torch.full(shape, 255, dtype=torch.uint8, device="cuda")


def zeros_u32(n):
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def setp(obj, **kw):
    for k, v in kw.items():
        if torch.is_tensor(v):
            v = v.data_ptr()
        elif isinstance(v, ctypes.Structure):
            v = ctypes.addressof(v)
        setattr(obj, k, v)
    return obj


def run(name, *args):
    _lib.call(name, *args, cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")


def tune(key, value):
    prev = _lib.I32(0)
    _lib.call("ocf_set_tuning", key, int(value), ctypes.byref(prev))
    return prev.value


@functools.lru_cache(maxsize=None)
def device_case(wt, H, bl, chunk=None):
    """the H fixture, its chunk tables and the packed weights on the device (shared by the tests, never written)"""
    fx, ct = G.make_batch(H), G.chunks_for(H, chunk)
    p1, W1r, po, Woutr = G.weights_for(wt, H, bl)
    t = SimpleNamespace(**{k: dev(getattr(fx, k)) for k in ("rows", "rp", "col", "val", "lboff", "xval", "flag", "bias_h",
                                                           "bias_out")})
    for k in ("ch_row", "ch_j0", "ch_j1", "row_cptr"):
        setattr(t, k, dev(getattr(ct, k)))
    t.bias_h0 = torch.zeros_like(t.bias_h)
    t.stats_in = dev(fx.stats_in[:ct.n_chunks])
    has = np.zeros(fx.Bp, bool)
    has[:fx.B] = fx.lens > 0
    return SimpleNamespace(fx=fx, ct=ct, wt=wt, H=H, bl=bl, t=t, W1=dev(p1), Wout=dev(po), W1r=W1r, Woutr=Woutr, has=has)


def gather_args(d, W, **kw):
    a, t = _lib.OcfGatherArgs(), d.t
    setp(a, rows=t.rows, rp=t.rp, col=t.col, val=t.val, lboff=t.lboff, xval=t.xval, flag=t.flag, ch_row=t.ch_row,
         ch_j0=t.ch_j0, ch_j1=t.ch_j1, n_chunks=d.ct.n_chunks, W=W, w_dtype=CD[d.wt], ldw=d.H, w_blocked=d.bl, H=d.H,
         h_dtype=CD[d.wt], d_dtype=CD[d.wt], keep=1.0, m_real=d.fx.B, n_real=d.fx.n_real)
    return setp(a, **kw)


def reduce_args(d, part, mode, **kw):
    r = _lib.OcfRowsReduceArgs()
    setp(r, part=part, row_cptr=d.t.row_cptr, B=d.fx.B, Bp=d.fx.Bp, H=d.H, mode=mode, keep=1.0, h_dtype=CD[d.wt],
         n_real=d.fx.n_real, gscale=G.GSCALE)
    return setp(r, **kw)


def finish(rep, wt, what, share=None):
    """print the worst error / bound of each stage (collected into this file's table), then assert"""
    for check, r, _ in rep:
        print("GATHER_RATIO %s | %s | %.4g" % (wt, check, r))
    w, r, i = rep.worst()
    print("%s: worst error / bound %.4g in '%s' at %s%s" % (what, r, w, i, "" if share is None else
                                                           "; share at a kink / count decision %.5f" % share))
    assert share is None or share <= 0.01, (what, share)
    assert not rep.failures(), "%s: worst error / bound %.4g in '%s' at index %s; all: %s" % (what, r, w, i, rep.failures())


def check_mask_mean(mask, keep, what):
    mean, n = float(mask.mean()), mask.size
    assert abs(mean - keep) <= 5.0 * np.sqrt(keep * (1.0 - keep) / n), (what, mean)       # 5 sigma of n draws


def encoder(d):
    part = nan32(d.ct.n_chunks, d.H)
    run("ocf_gather_encoder", gather_args(d, d.W1, part=part))
    return part


def standalone_bias_act(d, part, act, keep, bias):
    a_out, mask, h = nan32(d.fx.Bp, d.H), ff8(d.fx.Bp, d.H), nan_ct(d.wt, d.fx.Bp, d.H)
    run("ocf_rows_reduce", reduce_args(d, part, _lib.REDUCE_BIAS_ACT, bias=bias, act=_lib.ACT[act], keep=keep, seed=SEED,
                                       stream=STREAM, mask_out=mask if keep < 1.0 else None, a_out=a_out, h_out=h))
    return a_out, mask, h


# =========================================================================================================
# (a) ocf_gather_encoder, (b) ocf_rows_reduce in its three modes on the device partials of (a)
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("wt,H,bl", G.GRID, ids=G.GRID_IDS)
def test_encoder_and_rows_reduce(gpu, wt, H, bl):
    d = device_case(wt, H, bl)
    fx, ct, rep = d.fx, d.ct, G.Report()
    part = encoder(d)
    hp = host(part)
    G.check_encoder(rep, fx, ct, d.W1r, hp)
    out = nan32(fx.Bp, H)
    run("ocf_rows_reduce", reduce_args(d, part, _lib.REDUCE_RAW, out=out))
    G.check_reduce_raw(rep, fx, ct, hp, host(out))
    for act in (R.ACTS if (wt, H, bl) == G.ALL_ACTS_AT else ("sigmoid",)):
        for keep in (1.0, G.KEEP):
            a_out, mask, h = standalone_bias_act(d, part, act, keep, d.t.bias_h)
            G.check_bias_act(rep, fx, ct, wt, act, keep, fx.bias_h, hp, host(a_out), host(mask), host(h))
            if keep < 1.0:
                check_mask_mean(host(mask), G.KEEP32, "mask %s H=%d" % (wt, H))
            # GRAD_ACT: the same partials as a hidden delta's, the forward a / mask fed back, chunk stats -> row stats
            stats4 = int(keep < 1.0)
            hd, db = nan_ct(wt, fx.Bp, H), nan32(fx.Bp, H)
            sp, rs = nan32(fx.Bp, 4), nan32(fx.Bp)
            run("ocf_rows_reduce", reduce_args(d, part, _lib.REDUCE_GRAD_ACT, act=_lib.ACT[act], keep=keep, a_in=a_out,
                                               mask_in=mask if keep < 1.0 else None, h_out=hd, db_part=db,
                                               chunk_stats=d.t.stats_in, stats_part=sp, row_sse=rs, stats4=stats4))
            G.check_grad_act(rep, fx, ct, wt, act, keep, hp, fx.stats_in[:ct.n_chunks], host(a_out), host(mask), host(hd),
                             host(db), host(sp), host(rs), stats4)
    finish(rep, wt, "encoder + reduce %s H=%d blocked=%d" % (wt, H, bl))


# =========================================================================================================
# (c) ocf_gather_decoder, plain form: h given, no hidden epilogue, no folded reduction
# =========================================================================================================
def plain_decoder(d, m, loss):
    fx, ct = d.fx, d.ct
    h = dev(R.round_to(np.array(fx.h_given), d.wt)).to(TD[d.wt])
    o = SimpleNamespace(h=h, part=nan32(ct.n_chunks, d.H), chunk_stats=nan32(ct.n_chunks, 4), delta_e=nan32(fx.E),
                        d_out=nan_ct(d.wt, fx.Bp, G.N_PAD))
    run("ocf_gather_decoder", gather_args(d, d.Wout, h=h, bias=d.t.bias_out, aux=m, part=o.part, chunk_stats=o.chunk_stats,
                                          delta_e=o.delta_e, d_out=o.d_out, ld_d=G.N_PAD, loss=G.LOSS_CODE[loss],
                                          loss_param=G.HUBER_DELTA))
    rep = G.Report()
    # (chunk_stats[c][3] is written under a loss other than MSE only: not asserted under MSE)
    ent = G.check_decoder(rep, fx, ct, d.wt, d.Woutr, host(h), m, loss, host(o.delta_e), host(o.d_out), host(o.part),
                          host(o.chunk_stats))
    return rep, G.kink_share(fx, ent)


@pytest.mark.gpu
@pytest.mark.parametrize("wt,H,bl", G.GRID, ids=G.GRID_IDS)
def test_decoder_plain_mse(gpu, wt, H, bl):
    d = device_case(wt, H, bl)
    for m in (-1.0, 0.5):
        rep, share = plain_decoder(d, m, "mse")
        finish(rep, wt, "decoder mse m=%g %s H=%d blocked=%d" % (m, wt, H, bl), share)


@pytest.mark.gpu
@pytest.mark.parametrize("loss,wt,H,bl", G.LOSS_CASES, ids=["%s-%s-H%d" % c[:3] for c in G.LOSS_CASES])
def test_decoder_plain_losses(gpu, loss, wt, H, bl):
    rep, share = plain_decoder(device_case(wt, H, bl), -1.0, loss)
    finish(rep, wt, "decoder %s %s H=%d blocked=%d" % (loss, wt, H, bl), share)


# =========================================================================================================
# (d) ocf_gather_decoder with the hidden epilogue and the folded reduction; (e) ocf_gather_encdec
# =========================================================================================================
def fused_buffers(d):
    fx, ct, wt = d.fx, d.ct, d.wt
    return SimpleNamespace(a_out=nan32(fx.Bp, d.H), mask_out=ff8(fx.Bp, d.H), h=nan_ct(wt, fx.Bp, d.H),
                           part=nan32(ct.n_chunks, d.H), chunk_stats=nan32(ct.n_chunks, 4), delta_e=nan32(fx.E),
                           d_out=nan_ct(wt, fx.Bp, G.N_PAD), hd=nan_ct(wt, fx.Bp, d.H), db_part=nan32(fx.Bp, d.H),
                           stats_part=nan32(fx.Bp, 4), row_sse=nan32(fx.Bp), row_arrive=zeros_u32(fx.Bp))


def fused_args(d, o, enc_part, act, keep, bias_h, m, loss):
    jr = reduce_args(d, o.part, _lib.REDUCE_GRAD_ACT, act=_lib.ACT[act], keep=keep, a_in=o.a_out, mask_in=o.mask_out,
                     h_out=o.hd, db_part=o.db_part, chunk_stats=o.chunk_stats, stats_part=o.stats_part, row_sse=o.row_sse,
                     stats4=int(loss != "mse"))
    dec = gather_args(d, d.Wout, h=o.h, bias=d.t.bias_out, aux=m, part=o.part, chunk_stats=o.chunk_stats,
                      delta_e=o.delta_e, d_out=o.d_out, ld_d=G.N_PAD, enc_part=enc_part, enc_cptr=d.t.row_cptr,
                      bias_h=bias_h, act=_lib.ACT[act], keep=keep, seed=SEED, stream=STREAM, a_out=o.a_out,
                      mask_out=o.mask_out, jr=jr, row_arrive=o.row_arrive, loss=G.LOSS_CODE[loss],
                      loss_param=G.HUBER_DELTA)
    return dec, jr


def fused_setup(wt, H, bl):
    zero = (wt, H, bl) in ZERO_HIDDEN_AT
    losses = ["mse"] + [ls for ls, w, h, b in G.LOSS_CASES if (w, h, b) == (wt, H, bl)]
    return ("tanh" if zero else "sigmoid"), zero, losses


def host_fused(o):
    return SimpleNamespace(**{k: host(getattr(o, k)) for k in ("a_out", "mask_out", "h", "delta_e", "d_out", "hd",
                                                              "db_part", "stats_part", "row_sse")})


@pytest.mark.gpu
@pytest.mark.parametrize("wt,H,bl", G.GRID, ids=G.GRID_IDS)
def test_decoder_hidden_epilogue_and_folded_reduction(gpu, wt, H, bl):
    d = device_case(wt, H, bl)
    fx, ct = d.fx, d.ct
    act, zero, losses = fused_setup(wt, H, bl)
    bias_dev, bias = (d.t.bias_h0, np.zeros(H)) if zero else (d.t.bias_h, fx.bias_h)
    enc_part = encoder(d)
    _, mask_s, _ = standalone_bias_act(d, enc_part, act, G.KEEP, bias_dev)
    for loss in losses:
        o = fused_buffers(d)
        dec, jr = fused_args(d, o, enc_part, act, G.KEEP, bias_dev, -1.0, loss)
        run("ocf_gather_decoder", dec)
        rep, ho = G.Report(), host_fused(o)
        # a_out / mask_out / h are written by the first chunk of a row: rows without a chunk (no entries, padding)
        # are not promised by the header and not asserted
        G.check_bias_act(rep, fx, ct, wt, act, G.KEEP, bias, host(enc_part), ho.a_out, ho.mask_out, ho.h, rows=d.has,
                         stage="fused")
        rep.exact("fused: mask equals the standalone reduction's", ho.mask_out[d.has], host(mask_s)[d.has])
        ent = G.check_fused(rep, "fused", fx, ct, wt, d.Woutr, act, G.KEEP, -1.0, loss, ho)
        if zero:
            assert ent.tpy[fx.eng] == 0 and ent.live[fx.eng]          # the count differs from the live count
        # the chunks of rows with several chunks hand their partials over through memory (a one-chunk row keeps
        # its sums in registers: its part / chunk_stats rows are not promised)
        multi = np.repeat(np.diff(ct.row_cptr) > 1, np.diff(ct.row_cptr))
        ref, mag, n = G.dec_partials(fx, ct, d.Woutr, ho.delta_e)
        rep.add("fused: part", host(o.part)[multi], ref[multi], G.sum_bound(n[:, None], 0, mag)[multi])
        rep.exact("fused: row_arrive left zero", host(o.row_arrive), 0)
        finish(rep, wt, "fused decoder %s %s H=%d blocked=%d" % (loss, wt, H, bl), G.kink_share(fx, ent))


@pytest.mark.gpu
@pytest.mark.parametrize("wt,H,bl", G.GRID, ids=G.GRID_IDS)
def test_encdec_both_forms(gpu, wt, H, bl):
    d = device_case(wt, H, bl)
    fx, ct = d.fx, d.ct
    act, zero, losses = fused_setup(wt, H, bl)
    bias_dev, bias = (d.t.bias_h0, np.zeros(H)) if zero else (d.t.bias_h, fx.bias_h)
    prev = tune(b"encdec_rowres", -1)
    try:
        for rowres in (0, 1):
            tune(b"encdec_rowres", rowres)
            for loss in losses:
                o = fused_buffers(d)
                enc_part, enc_arrive = nan32(ct.n_chunks, H), zeros_u32(fx.Bp)
                enc = gather_args(d, d.W1, part=enc_part)
                dec, jr = fused_args(d, o, enc_part, act, G.KEEP, bias_dev, 0.5, loss)
                _lib.call("ocf_gather_encdec", enc, dec, enc_arrive.data_ptr(), cur_stream())
                torch.cuda.synchronize()
                _lib.call("ocf_check_async")
                rep, ho = G.Report(), host_fused(o)
                # which form ran: the row-resident one passes no partial through memory.  16-bit weights at H = 384
                # and fp32 at H = 128 / 384 run chunked under either setting
                untouched = bool(torch.isnan(enc_part).all())
                assert untouched == bool(rowres and G.rowres_runs(wt, H)), (wt, H, rowres)
                if not untouched:          # the chunked form's encoder part (its own instance: 4 entries in flight)
                    G.check_encoder(rep, fx, ct, d.W1r, host(enc_part))
                # (a_out / mask_out / h: the rows with entries, as above)
                G.check_hidden_scratch(rep, "encdec", fx, ct, wt, d.W1r, act, G.KEEP, bias, ho, d.has)
                check_mask_mean(ho.mask_out[d.has], G.KEEP32, "encdec mask")
                ent = G.check_fused(rep, "encdec", fx, ct, wt, d.Woutr, act, G.KEEP, 0.5, loss, ho)
                rep.exact("encdec: enc_arrive left zero", host(enc_arrive), 0)
                rep.exact("encdec: row_arrive left zero", host(o.row_arrive), 0)
                finish(rep, wt, "encdec rowres=%d %s %s H=%d blocked=%d" % (rowres, loss, wt, H, bl), G.kink_share(fx, ent))
    finally:
        tune(b"encdec_rowres", prev)


# =========================================================================================================
# (f) ocf_rank_step phases 0 / 1, side = NULL: the row-resident RR_ENC_RAW / RR_DEC_RAW instances
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("wt,bl", [("f16", 1), ("f32", 0)])
@pytest.mark.parametrize("chunk,threads", [(1024, 256), (64, 1024)])
def test_rank_step_row_resident_phases(gpu, wt, bl, chunk, threads):
    H = 256
    d = device_case(wt, H, bl, chunk)
    fx, ct = d.fx, d.ct
    assert (ct.n_chunks <= 2 * fx.B) == (threads == 256)               # ocf_sparse.hip rank_rowres_enc / _dec
    o = fused_buffers(d)
    enc_part, out0, out1, fin = nan32(ct.n_chunks, H), nan32(fx.Bp, H), nan32(fx.Bp, H), nan32(4 + fx.Bp)
    st = _lib.OcfRankStepArgs()
    st.enc = gather_args(d, d.W1, part=enc_part)
    st.enc_sum = reduce_args(d, enc_part, _lib.REDUCE_RAW, out=out0)
    setp(st.hidden, slabs=out0, splits=1, split_stride=fx.Bp * H, M=fx.Bp, N=H, ld=H, bias=d.t.bias_h,
         act=_lib.ACT["sigmoid"], keep=G.KEEP, seed=SEED, stream=STREAM, mask_out=o.mask_out, a_out=o.a_out, h_out=o.h,
         h_dtype=CD[wt], m_real=fx.B, n_real=fx.n_real)
    st.dec = gather_args(d, d.Wout, h=o.h, bias=d.t.bias_out, aux=-1.0, part=o.part, chunk_stats=o.chunk_stats,
                         delta_e=o.delta_e)
    st.dec_sum = reduce_args(d, o.part, _lib.REDUCE_RAW, out=out1, chunk_stats=o.chunk_stats, stats_part=o.stats_part,
                             row_sse=o.row_sse)
    setp(st.stats, stats_part=o.stats_part, n_parts=fx.Bp, row_sse_part=o.row_sse, n_tiles=1, M=fx.Bp, out=fin)
    prev = tune(b"encdec_rowres", 1)
    try:
        rep = G.Report()
        _lib.call("ocf_rank_step", st, 0, cur_stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(enc_part).all()), "phase 0 did not run row-resident"
        v, mag, n = G.row_gather(fx, fx.xval, d.W1r)
        rep.add("rank: encoder row sums", host(out0), v, G.sum_bound(n[:, None], 0, mag))
        _lib.call("ocf_rank_step", st, 1, cur_stream())
        torch.cuda.synchronize()
        _lib.call("ocf_check_async")
        assert bool(torch.isnan(o.part).all()), "phase 1 did not run row-resident"
    finally:
        tune(b"encdec_rowres", prev)
    ho = host_fused(o)
    ho.d_out = None
    # the hidden epilogue runs for every row (ocf_splitk_bias_act's contract): one slab per row
    one = SimpleNamespace(row_cptr=np.arange(fx.Bp + 1, dtype=np.int32))
    G.check_bias_act(rep, fx, one, wt, "sigmoid", G.KEEP, fx.bias_h, host(out0), ho.a_out, ho.mask_out, ho.h, stage="rank")
    check_mask_mean(ho.mask_out, G.KEEP32, "rank mask")
    ho.hd = host(out1)
    ent = G.check_fused(rep, "rank", fx, ct, wt, d.Woutr, "sigmoid", G.KEEP, -1.0, "mse", ho, raw=True)
    f, sp = host(fin), ho.stats_part.astype(np.float64)
    rep.add("rank: finalized stats", f[:3], sp[:, :3].sum(0), G.sum_bound(0, fx.Bp, np.abs(sp[:, :3]).sum(0)))
    rep.exact("rank: finalized slot 3 and row SSE", f[3:], np.concatenate([[0.0], ho.row_sse]))
    finish(rep, wt, "rank step %s chunk=%d (%d threads)" % (wt, chunk, threads), G.kink_share(fx, ent))
