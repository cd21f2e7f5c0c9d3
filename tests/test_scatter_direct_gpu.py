"""ocf_scatter_batch and ocf_epoch_scatter through the library's C entry points, with hand-built arguments, against
the per-rating reference loop of tests/scatter_ref.py: the dense arrays (one memset and several), xval1 / tflag1 /
tflag2, the tile and column counts added onto the caller's, the row tags, the layer-0 input per dtype x feed x both,
the target buckets (never called by the engine), the two column shards and their union, the device split against
its float32 restatement, every selected batch of an epoch plan, batches of 8,192 and 16,384 rows, and the refusals.

Every output buffer is filled with a sentinel before each launch (NaN, 0xFF, -9), has two rows or some entries of
slack past what the call may write, and every comparison is exact; bucket contents are compared per tile as sorted
multisets (their order comes from atomics).  tests/test_scatter_ref.py shows on the CPU that the comparisons made
here reject fourteen plausible defects.

The run on an MI355X (this file's own): 33 tests, all passed, no mismatch in any comparison.
  * B = 8,192 and B = 16,384: the bound B <= 16384 was kept and the dynamic-LDS limit of scatter_flat_kernel and
    bucket_fill_kernel raised to 131,080 bytes; both batches launched and every per-entry output, count and bucket
    equalled the reference.
  * The first run of test_xin found one defect, since fixed in ocf_scatter.hip: with a bf16 layer-0 input and
    feed = 1 the M_in block stayed zero at every live input (1,569 of the train fixture's and 1,464 of the eval
    fixture's elements; f32 and f16 matched).  test_xin's already-clean calls also set the dense outputs, so the
    xin stores are compared with and without the dense stores around them.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scatter_ref as S
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

TD = {_lib.DT_F32: torch.float32, _lib.DT_F16: torch.float16, _lib.DT_BF16: torch.bfloat16}
I_SENT, TAG_BEFORE, RTAG, SLACK = -9, 7, 200, 64
DENSE = ("X", "Min", "Mout", "T", "Mmiss")
IN_KEYS = ("rp1", "col1", "val1", "dup1", "rows1", "keep1", "boff1", "rp2", "col2", "val2", "dup2", "rows2", "pos1",
           "lboff1", "lboff2")


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def nan32(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def ff8(n):
    return torch.full((n,), 255, dtype=torch.uint8, device="cuda")


def ints(n, fill=I_SENT):
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy()


_DEVICE = {}


def inputs_of(c):
    """the case's input arrays on the device (shared by the tests, never written)"""
    if c.name not in _DEVICE:
        _DEVICE[c.name] = {k: dev(getattr(c, k)) for k in IN_KEYS if getattr(c, k) is not None}
    return _DEVICE[c.name]


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return S.reference(CASES[name]())


CASES = {
    "train-pt1": lambda: S.train(1), "train-pt0": lambda: S.train(0), "eval": S.eval_case, "wide": S.wide,
}


def scatter_args(c, **out):
    a = _lib.OcfScatterArgs()
    for k, t in inputs_of(c).items():
        setattr(a, k, t.data_ptr())
    for k in ("s0", "s1", "seed", "stream", "mode", "pass_through", "B", "B_pad", "N", "aux", "ld", "E1", "E2", "n_tiles",
              "tb_nk"):
        setattr(a, k, getattr(c, k))
    for k, v in out.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    return a


def run(a):
    _lib.call("ocf_scatter_batch", ctypes.byref(a), cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")


def eq(got, want, what):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=what)


def dense_expected(c, ref_arr):
    """[B_pad + 2][ld]: the reference in [B][N], zeros around it up to B_pad x ld, the sentinel in the slack rows"""
    want = np.full((c.B_pad + 2, c.ld), np.nan, np.float32)
    want[:c.B_pad] = 0.0
    want[:c.B, :c.N] = ref_arr
    return want


def check_entry_outputs(c, ref, xval1=None, tflag1=None, tflag2=None):
    if xval1 is not None:
        g = host(xval1)
        eq(g[:c.E1], ref.xval1, "xval1")
        assert np.isnan(g[c.E1:]).all(), "xval1 slack"
    if tflag1 is not None:
        g = host(tflag1)
        eq(g[:c.E1], ref.tflag1, "tflag1")
        assert (g[c.E1:] == 255).all(), "tflag1 slack"
    if tflag2 is not None:
        g = host(tflag2)
        eq(g[:c.E2], ref.tflag2, "tflag2")
        assert (g[c.E2:] == 255).all(), "tflag2 slack"


# =========================================================================================================
# train: the dense arrays, the per-entry outputs, the counts, the tags
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("layout", ["contiguous", "separate"])
def test_train_dense_and_entry_outputs(gpu, pt, layout):
    c = S.train(pt)
    ref = ref_of(c.name)
    blk = c.B_pad * c.ld
    if layout == "contiguous":                      # five back-to-back [B_pad][ld] blocks: one memset
        flat = nan32(5 * blk + 2 * c.ld)
        dense = {k: flat[i * blk:(i + 1) * blk] for i, k in enumerate(DENSE)}
    else:                                           # separate allocations, one output null
        dense = {k: nan32(c.B_pad + 2, c.ld) for k in DENSE if k != "Min"}
    xval1, tflag1 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK)
    nt = c.n_tiles * c.tb_nk
    base_tb, base_cc = np.arange(nt + SLACK, dtype=np.int32) % 5 + 1, np.arange(c.N + SLACK, dtype=np.int32) % 7 + 2
    tb_cnt, col_cnt, ecb = dev(base_tb), dev(base_cc), ints(c.E1 + SLACK)
    rtag_in = torch.full((c.N + SLACK,), TAG_BEFORE, dtype=torch.uint8, device="cuda")
    rtag_out = rtag_in.clone()
    run(scatter_args(c, xval1=xval1, tflag1=tflag1, tb_cnt=tb_cnt, col_cnt=col_cnt, ecb=ecb, rtag_in=rtag_in,
                     rtag_out=rtag_out, rtag=RTAG, **dense))
    for k in dense:
        want = dense_expected(c, getattr(ref, k))
        if layout == "contiguous":
            eq(host(dense[k]).reshape(c.B_pad, c.ld), want[:c.B_pad], k)
        else:
            eq(host(dense[k]), want, k)
    if layout == "contiguous":
        assert np.isnan(host(flat[5 * blk:])).all(), "rows past the last dense block"
    check_entry_outputs(c, ref, xval1, tflag1)
    want_tb, want_cc = base_tb.copy(), base_cc.copy()
    want_tb[:nt] += ref.tb_cnt
    want_cc[:c.N] += ref.col_cnt
    eq(host(tb_cnt), want_tb, "tb_cnt (added onto the caller's counts)")
    eq(host(col_cnt), want_cc, "col_cnt (added onto the caller's counts)")
    eq(host(ecb), np.concatenate([ref.ecb, np.full(SLACK, I_SENT, np.int32)]), "ecb")
    for got, live, what in ((rtag_in, ref.live_in, "rtag_in"), (rtag_out, ref.live_out, "rtag_out")):
        want = np.full(c.N + SLACK, TAG_BEFORE, np.uint8)
        want[:c.N][live] = RTAG
        eq(host(got), want, what)


# =========================================================================================================
# the layer-0 input: dtype x feed x both, cleared by the call or already clean
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [_lib.DT_F32, _lib.DT_F16, _lib.DT_BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["train-pt0", "eval"])
def test_xin(gpu, dt, name):
    c = CASES[name]()
    ref = ref_of(name)
    td = TD[dt]
    for feed, both in S.XIN_MODES:
        k = S.xin_blocks(feed, both)
        img = torch.from_numpy(S.xin_image(ref.X, ref.Min, ref.Mmiss, feed, both, S.XB)).to(td)    # rounded once, RNE
        for clean in (0, 1):
            if clean:
                want = torch.zeros(c.B_pad + 2, k * S.XB, dtype=td)
            else:
                want = torch.full((c.B_pad + 2, k * S.XB), float("nan")).to(td)
            buf = want.clone().cuda()                # (the sentinel's bits are the expectation's)
            want[:c.B_pad] = 0
            want[:c.B] = img
            # the already-clean call also takes the dense outputs: the xin stores with and without the dense
            # stores around them (the kernel's xin stores sit where a compiler workaround put them)
            dense = {kk: nan32(c.B_pad + 2, c.ld) for kk in DENSE} if clean else {}
            run(scatter_args(c, xin=buf, xin_dtype=dt, xin_ld=k * S.XB, xin_block=S.XB, feed=feed, both=both,
                             xin_clean=clean, **dense))
            bits = torch.int32 if dt == _lib.DT_F32 else torch.int16
            eq(host(buf.view(bits)), want.view(bits).numpy(), "xin feed %d both %d clean %d" % (feed, both, clean))
            for kk in dense:
                eq(host(dense[kk]), dense_expected(c, getattr(ref, kk)), "%s beside xin feed %d both %d" % (kk, feed, both))


# =========================================================================================================
# the target buckets
# =========================================================================================================
def bucket_buffers(c, n_targets):
    return SimpleNamespace(tile_cnt=torch.cat([torch.zeros(c.n_tiles, dtype=torch.int32, device="cuda"), ints(SLACK)]),
                           bk_ptr=ints(c.n_tiles + 1 + SLACK), bk_cur=ints(c.n_tiles + SLACK),
                           bk_rc=ints(n_targets + SLACK), bk_t=nan32(n_targets + SLACK), bk_m=nan32(n_targets + SLACK))


def check_buckets(c, ref, b, what):
    nt, n = c.n_tiles, int(ref.bk.ptr[-1])
    ptr = host(b.bk_ptr)
    eq(ptr[:nt + 1], ref.bk.ptr, what + ": bk_ptr")
    eq(host(b.bk_cur)[:nt], ref.bk.ptr[1:], what + ": bk_cur")
    eq(host(b.tile_cnt)[:nt], 0, what + ": tile_cnt left zero")
    eq(S.sort_buckets(nt, ptr, host(b.bk_rc), host(b.bk_t), host(b.bk_m)), ref.bk.tri, what + ": triples per tile")
    assert (ptr[nt + 1:] == I_SENT).all() and (host(b.bk_cur)[nt:] == I_SENT).all(), what + ": pointer slack"
    assert (host(b.tile_cnt)[nt:] == I_SENT).all() and (host(b.bk_rc)[n:] == I_SENT).all(), what + ": slack"
    assert np.isnan(host(b.bk_t)[n:]).all() and np.isnan(host(b.bk_m)[n:]).all(), what + ": value slack"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["train-pt1", "train-pt0", "eval", "wide"])
def test_buckets(gpu, name):
    c = CASES[name]()
    ref = ref_of(name)
    n = int(ref.bk.ptr[-1])
    assert n > 0
    b = bucket_buffers(c, n)
    xval1, tflag1, tflag2 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK), ff8(c.E2 + SLACK)
    a = scatter_args(c, xval1=xval1, tflag1=tflag1, tflag2=tflag2, **vars(b))
    run(a)
    check_buckets(c, ref, b, "first call")
    check_entry_outputs(c, ref, xval1, tflag1, tflag2)
    b.bk_rc.fill_(I_SENT)
    b.bk_t.fill_(float("nan"))
    b.bk_m.fill_(float("nan"))
    run(a)                                          # the same counters again: the scan left them ready
    check_buckets(c, ref, b, "second call")
    if name == "wide":                              # (no dense outputs there: the tags and counts with the buckets)
        tb = torch.zeros(c.n_tiles * c.tb_nk, dtype=torch.int32, device="cuda")
        rtag_in = torch.full((c.N,), TAG_BEFORE, dtype=torch.uint8, device="cuda")
        rtag_out = rtag_in.clone()
        run(scatter_args(c, tb_cnt=tb, rtag_in=rtag_in, rtag_out=rtag_out, rtag=RTAG))
        eq(host(tb), ref.tb_cnt, "tb_cnt")
        eq(host(rtag_in) == RTAG, ref.live_in, "rtag_in")
        eq(host(rtag_out) == RTAG, ref.live_out, "rtag_out")
        assert np.isin(host(rtag_in), (RTAG, TAG_BEFORE)).all() and np.isin(host(rtag_out), (RTAG, TAG_BEFORE)).all()


# =========================================================================================================
# eval
# =========================================================================================================
@pytest.mark.gpu
def test_eval_dense_and_flags(gpu):
    c = S.eval_case()
    ref = ref_of("eval")
    dense = {k: nan32(c.B_pad + 2, c.ld) for k in DENSE}
    xval1, tflag1, tflag2 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK), ff8(c.E2 + SLACK)
    tb = torch.zeros(c.n_tiles * c.tb_nk, dtype=torch.int32, device="cuda")
    rtag_in = torch.full((c.N + SLACK,), TAG_BEFORE, dtype=torch.uint8, device="cuda")
    rtag_out = rtag_in.clone()
    run(scatter_args(c, xval1=xval1, tflag1=tflag1, tflag2=tflag2, tb_cnt=tb, rtag_in=rtag_in, rtag_out=rtag_out,
                     rtag=RTAG, **dense))
    for k in DENSE:
        eq(host(dense[k]), dense_expected(c, getattr(ref, k)), k)
    check_entry_outputs(c, ref, xval1, tflag1, tflag2)
    assert not ref.tflag1.any()
    eq(host(tb), ref.tb_cnt, "tb_cnt")
    eq(host(rtag_out), TAG_BEFORE, "rtag_out untouched")
    want = np.full(c.N + SLACK, TAG_BEFORE, np.uint8)
    want[:c.N][ref.live_in] = RTAG
    eq(host(rtag_in), want, "rtag_in")


# =========================================================================================================
# column shards: each against its reference, the union against the full batch
# =========================================================================================================
def run_case_dense(c):
    dense = {k: nan32(c.B_pad + 2, c.ld) for k in DENSE}
    xval1, tflag1 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK)
    col_cnt, ecb = torch.zeros(c.N, dtype=torch.int32, device="cuda"), ints(c.E1 + SLACK)
    run(scatter_args(c, xval1=xval1, tflag1=tflag1, col_cnt=col_cnt, ecb=ecb, **dense))
    out = {k: host(v) for k, v in dense.items()}
    out.update(xval1=host(xval1), tflag1=host(tflag1), col_cnt=host(col_cnt), ecb=host(ecb))
    return out


def check_case_dense(c, ref, out):
    for k in DENSE:
        eq(out[k], dense_expected(c, getattr(ref, k)), c.name + " " + k)
    eq(out["xval1"][:c.E1], ref.xval1, c.name + " xval1")
    eq(out["tflag1"][:c.E1], ref.tflag1, c.name + " tflag1")
    assert np.isnan(out["xval1"][c.E1:]).all() and (out["tflag1"][c.E1:] == 255).all()
    eq(out["col_cnt"], ref.col_cnt, c.name + " col_cnt")
    eq(out["ecb"][:c.E1], ref.ecb, c.name + " ecb")


@pytest.mark.gpu
@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("split", ["host", "device"])
def test_shards(gpu, pt, split):
    full, parts = S.train(pt), S.shards(pt)
    if split == "device":                           # the same seed / stream on both shards
        full = S.with_device_split(full, 0.3, 0.7, S.DEV_SEED, S.DEV_STREAM)
        parts = [S.with_device_split(sh, 0.3, 0.7, S.DEV_SEED, S.DEV_STREAM) for sh in parts]
    ref_full = S.reference(full)
    outs = []
    for sh in parts:
        out = run_case_dense(sh)
        check_case_dense(sh, S.reference(sh), out)
        outs.append(out)
    for k in DENSE:
        got = np.concatenate([o[k][:full.B, :sh.N] for sh, o in zip(parts, outs)], axis=1)
        eq(got, getattr(ref_full, k), "union " + k)
    for k in ("xval1", "tflag1"):
        got = np.full(full.E1, 99, getattr(ref_full, k).dtype)
        for sh, o in zip(parts, outs):
            got[sh.src_e] = o[k][:sh.E1]
        eq(got, getattr(ref_full, k), "union " + k)
    eq(np.concatenate([o["col_cnt"] for o in outs]), ref_full.col_cnt, "union col_cnt")


# =========================================================================================================
# the device split on the full batch
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("s", list(S.DEV_RANGES) + [(1.0, 1.0)], ids=["0.3-0.7", "0.5-0.5", "1-1"])
def test_device_split(gpu, pt, s):
    base = S.train(pt)
    c = S.with_device_split(base, s[0], s[1], S.DEV_SEED, S.DEV_STREAM)
    ref = S.reference(c)
    if s[0] >= 1.0:
        assert c.keep_ref.all()
    else:
        assert 0.2 < c.keep_ref.mean() < 0.8
    out = run_case_dense(c)
    # the flags themselves, at the entries outside the duplicate chains: a live input iff kept (Min holds the
    # flag whatever the rating), and without pass-through a live target iff dropped
    solo = np.ones(c.E1, bool)
    lo = int(c.lboff1[S.T_DUP])
    solo[lo:lo + S.DUP_LEN] = False
    cols = c.col1[c.ei]
    eq((out["Min"][c.eb, cols] != 0)[solo], c.keep_ref[solo] != 0, "keep flags (Min)")
    if not pt:
        eq(out["tflag1"][:c.E1][solo], 1 - c.keep_ref[solo], "keep flags (tflag1)")
    check_case_dense(c, ref, out)


# =========================================================================================================
# ocf_epoch_scatter against the reference (not against ocf_scatter_batch)
# =========================================================================================================
def epoch_args(ep, device, B=None, **over):
    key = "epoch-tables-%d" % ep.pass_through
    if key not in _DEVICE:
        _DEVICE[key] = {k: dev(getattr(ep, k)) for k in ("rp1", "col1", "val1", "dup1", "rows1", "lboff1", "boff1", "keep1",
                                                         "keep_off", "sel", "ebase")}
    t = _DEVICE[key]
    a = _lib.OcfScatterArgs()
    for k in ("rp1", "col1", "val1", "dup1", "rows1", "lboff1", "boff1"):
        setattr(a, k, t[k].data_ptr())
    a.mode, a.pass_through, a.B, a.B_pad, a.N, a.aux, a.ld = 0, ep.pass_through, B or ep.B, B or ep.B, ep.N, -1.0, 304
    a.s0 = a.s1 = 1.0
    if device is None:
        a.keep1 = t["keep1"].data_ptr()
    else:
        a.s0, a.s1, a.seed = device[0], device[1], S.EP_SEED
    e = _lib.OcfEpochScatterArgs()
    e.n_sel, e.sel, e.ebase, e.max_e = len(ep.sel), t["sel"].data_ptr(), t["ebase"].data_ptr(), ep.max_e
    e.keep_off, e.stream_mul, e.ebase0 = t["keep_off"].data_ptr(), S.EP_STREAM_MUL, ep.ebase0
    for k, v in over.items():
        setattr(a if hasattr(a, k) else e, k, v.data_ptr() if torch.is_tensor(v) else v)
    return a, e


@pytest.mark.gpu
@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("device", [None, (0.3, 0.7)], ids=["host", "device"])
def test_epoch_scatter(gpu, pt, device):
    ep = S.epoch(pt)
    want_x, want_t = S.reference_epoch(ep, device)
    xval, tflag = nan32(ep.total + SLACK), ff8(ep.total + SLACK)
    a, e = epoch_args(ep, device)
    e.xval, e.tflag = xval.data_ptr(), tflag.data_ptr()
    _lib.call("ocf_epoch_scatter", ctypes.byref(a), ctypes.byref(e), cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")
    gx, gt = host(xval), host(tflag)
    for s, bi in enumerate(ep.sel):
        lo, hi = int(ep.ebase[s] - ep.ebase0), int(ep.ebase[s + 1] - ep.ebase0)
        eq(gx[lo:hi], want_x[lo:hi], "xval of slot %d (batch %d)" % (s, bi))
        eq(gt[lo:hi], want_t[lo:hi], "tflag of slot %d (batch %d)" % (s, bi))
    assert np.isnan(gx[ep.total:]).all() and (gt[ep.total:] == 255).all(), "bytes outside the selected batches"


# =========================================================================================================
# B = 8,192: the first batch whose offset table is past 64 KB of LDS
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("B", [8192, 16384])
def test_many_rows(gpu, B):
    """8,192 rows: the first offset table past 64 KB; 16,384: the largest batch the entry point admits (131,080 bytes)"""
    c = S.many_rows(B)
    ref = S.reference(c)
    xval1, tflag1 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK)
    tb = torch.zeros(c.n_tiles * c.tb_nk, dtype=torch.int32, device="cuda")
    b = bucket_buffers(c, int(ref.bk.ptr[-1]))
    run(scatter_args(c, xval1=xval1, tflag1=tflag1, tb_cnt=tb, **vars(b)))
    check_entry_outputs(c, ref, xval1, tflag1)
    eq(host(tb), ref.tb_cnt, "tb_cnt")
    check_buckets(c, ref, b, "B = %d" % B)


# =========================================================================================================
# refusals: OcfError, nothing launched
# =========================================================================================================
def empty_case(B):
    """a batch of B rows without an entry (nothing to launch even if a check let it through)"""
    z = np.zeros(B + 1, np.int64)
    return SimpleNamespace(name="empty-%d" % B, mode=0, pass_through=1, B=B, B_pad=B, N=64, ld=64, aux=-1.0,
                           rp1=np.zeros(2, np.int64), col1=np.zeros(1, np.int32), val1=np.zeros(1, np.float32), dup1=None,
                           rows1=np.full(B, -1, np.int32), lboff1=z, boff1=z, pos1=None, keep1=np.zeros(8, np.uint8),
                           s0=1.0, s1=1.0, seed=0, stream=0, E1=0, E2=0, rp2=None, col2=None, val2=None, dup2=None,
                           rows2=None, lboff2=None, n_tiles=1, tb_nk=(B + 63) // 64)


def refused(c, **over):
    xval1, tflag1 = nan32(c.E1 + SLACK), ff8(c.E1 + SLACK)
    a = scatter_args(c, xval1=xval1, tflag1=tflag1, **over)
    with pytest.raises(_lib.OcfError):
        run(a)
    torch.cuda.synchronize()
    assert np.isnan(host(xval1)).all() and (host(tflag1) == 255).all(), "a refused call wrote"


@pytest.mark.gpu
def test_scatter_batch_refusals(gpu):
    c = S.train(1)
    refused(c, B=c.B_pad + 1)
    refused(c, mode=2)
    refused(c, ld=302)
    refused(c, tile_cnt=torch.zeros(c.n_tiles, dtype=torch.int32, device="cuda"))
    tags = torch.full((c.N,), TAG_BEFORE, dtype=torch.uint8, device="cuda")
    for rtag in (0, 256):
        refused(c, rtag_in=tags, rtag_out=tags, rtag=rtag)
    assert (host(tags) == TAG_BEFORE).all()
    cc, ecb = torch.zeros(c.N, dtype=torch.int32, device="cuda"), ints(c.E1 + SLACK)
    ev = S.eval_case()
    refused(ev, col_cnt=cc, ecb=ints(ev.E1 + SLACK))
    refused(empty_case(4097), col_cnt=cc, ecb=ecb)
    assert not host(cc).any() and (host(ecb) == I_SENT).all()
    refused(ev, lboff2=0)


@pytest.mark.gpu
def test_epoch_scatter_refusals(gpu):
    ep = S.epoch(1)
    xval, tflag = nan32(ep.total + SLACK), ff8(ep.total + SLACK)
    big = empty_case(4097)
    t = inputs_of(big)
    cases = [dict(X=nan32(ep.B, 304)),
             dict(B=4097, rows1=t["rows1"], lboff1=t["lboff1"], boff1=t["boff1"]),
             dict(n_sel=65536)]
    for over in cases:
        a, e = epoch_args(ep, None, max_e=0, **over)
        e.xval, e.tflag = xval.data_ptr(), tflag.data_ptr()
        with pytest.raises(_lib.OcfError):
            _lib.call("ocf_epoch_scatter", ctypes.byref(a), ctypes.byref(e), cur_stream())
        torch.cuda.synchronize()
    assert np.isnan(host(xval)).all() and (host(tflag) == 255).all(), "a refused call wrote"
