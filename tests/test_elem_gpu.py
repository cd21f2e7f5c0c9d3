"""The small kernels of csrc/ocf_elem.hip (and ocf_colsum / ocf_pack_input / ocf_dense_targets), each called on
its own with known inputs against the fp64 restatements of tests/epilogue_ref.py: ocf_opt_step, ocf_opt_step_ex,
ocf_bias_opt_from_partials, ocf_stats_finalize, ocf_sumsq, ocf_colsum, ocf_pack_input, ocf_dense_targets.
Sizes sit on both sides of every block / group / grid-cap boundary of the kernels.  Optimizer state is held to
rtol 1e-5 / atol 2e-6 at hyper-parameters where every term of the update is visible (epilogue_ref.HYPER;
tests/test_epilogue_ref.py shows that bar rejects the usual wrong formulas); fixed-order fp32 sums are held to
(number of additions on the longest chain) x 2^-24 x sum |x|; roundings to 16 bits are compared bitwise."""
import numpy as np
import pytest
import torch

import epilogue_ref as R
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream
from test_epilogues_gpu import CD, SENT, TD, assert_buckets, assert_within, bits, dense_targets_call, dev, host

EPS32 = 2.0 ** -24
GRID_CAP = 8192 * 256           # ocf_opt_step launches at most 8,192 blocks of 256: one more element strides


def opt_params(kind, l2=True, gscale=R.GSCALE):
    h = R.hyper(kind, l2, gscale)
    return h, _lib.OcfOptParams(R.OPT_KIND[kind], h["lr"], h["eps"], h["rho"], h["beta2"], h["l2"], h["gscale"])


def sync():
    torch.cuda.synchronize()


def check_state(kind, got, ref, init, what):
    worst = R.opt_worst([host(t) for t in got], ref)
    print("%s: worst |err| / (atol + rtol |ref|) = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)
    for t, x0, r in zip(got[1:], init[1:], ref[1:]):          # slots the optimizer does not have stay as they were
        assert r is not None or np.array_equal(host(t), x0.astype(np.float64)), what


# ---- ocf_opt_step / ocf_opt_step_ex ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID_CAP + 3])
def test_opt_step(gpu, n):
    p0, s10, s20, g = R.opt_inputs((n,), 71, g_std=R.G_STD)
    gd = dev(g)
    for kind in R.OPTS:
        for l2 in (False, True):
            h, opt = opt_params(kind, l2)
            P, S1, S2 = dev(p0), dev(s10), dev(s20)
            _lib.call("ocf_opt_step", P.data_ptr(), gd.data_ptr(), S1.data_ptr() if kind != "sgd" else None,
                      S2.data_ptr() if kind == "adam" else None, n, opt, cur_stream())
            sync()
            ref = R.opt_update(kind, p0, g, s10 if kind != "sgd" else None, s20 if kind == "adam" else None, **h)
            check_state(kind, (P, S1, S2), ref, (p0, s10, s20), "opt_step %s l2=%d n=%d" % (kind, l2, n))
            assert not np.array_equal(host(P), p0.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID_CAP + 3])
def test_opt_step_ex(gpu, n):
    p0, s10, s20, g = R.opt_inputs((n,), 72, g_std=R.G_STD)
    for kind in R.OPTS:
        h, opt = opt_params(kind, True)
        for gdt in ("f32", "bf16"):
            gr = R.round_to(g, gdt)
            gd = dev(gr).to(TD[gdt])
            ref = R.opt_update(kind, p0, gr, s10 if kind != "sgd" else None, s20 if kind == "adam" else None, **h)
            # (the one large size keeps to two pairings, so the case stays within a few seconds)
            for sdt in ((None, "f16", "bf16") if n < 1000 else (("f16",) if gdt == "f32" else ("bf16",))):
                P, S1, S2 = dev(p0), dev(s10), dev(s20)
                Sh = torch.full((n,), SENT, device="cuda").to(TD[sdt]) if sdt else None
                a = _lib.OcfOptStepArgs()
                a.p, a.g, a.g_dtype, a.n, a.opt = P.data_ptr(), gd.data_ptr(), CD[gdt], n, opt
                a.s1 = S1.data_ptr() if kind != "sgd" else None
                a.s2 = S2.data_ptr() if kind == "adam" else None
                if sdt:
                    a.shadow, a.shadow_dtype = Sh.data_ptr(), CD[sdt]
                _lib.call("ocf_opt_step_ex", a, cur_stream())
                sync()
                what = "opt_step_ex %s g=%s shadow=%s n=%d" % (kind, gdt, sdt, n)
                check_state(kind, (P, S1, S2), ref, (p0, s10, s20), what)
                if sdt:         # the shadow is the updated parameter rounded once
                    assert torch.equal(bits(Sh), bits(P.to(TD[sdt]))), what


# ---- ocf_bias_opt_from_partials --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 3, 4, 5, 64, 65, 130])
def test_bias_opt_from_partials(gpu, parts):
    for n in (1, 63, 64, 65, 130):
        ld = n + 5
        rng = np.random.RandomState(1000 * parts + n)
        part = np.full((parts, ld), 1e6, np.float32)                      # columns >= n must not be read
        part[:, :n] = (0.05 / np.sqrt(parts)) * rng.randn(parts, n) + 0.02 / parts
        g = part[:, :n].astype(np.float64).sum(0)
        # the kernel's sum: 4 groups of <= ceil(parts / 4) additions, then two levels
        gtol = (-(-parts // 4) + 2) * EPS32 * np.abs(part[:, :n]).astype(np.float64).sum(0) + 1e-30
        p0, s10, s20 = R.opt_inputs((n + 2,), 73)
        pd = dev(part)
        for kind in R.OPTS:
            h, opt = opt_params(kind, True, gscale=7.0)                   # the partials are already scaled: ignored
            h["gscale"] = 1.0
            what = "bias_opt %s parts=%d n=%d" % (kind, parts, n)
            B, S1, S2 = dev(p0), dev(s10), dev(s20)
            _lib.call("ocf_bias_opt_from_partials", B.data_ptr(), pd.data_ptr(), parts, ld, n,
                      S1.data_ptr() if kind != "sgd" else None, S2.data_ptr() if kind == "adam" else None, None, opt,
                      cur_stream())
            sync()
            ref = R.opt_update(kind, p0[:n], g, s10[:n] if kind != "sgd" else None, s20[:n] if kind == "adam" else None,
                               **h)
            check_state(kind, (B[:n], S1[:n], S2[:n]), ref, (p0[:n], s10[:n], s20[:n]), what)
            for t, x0 in ((B, p0), (S1, s10), (S2, s20)):                 # nothing past n
                assert np.array_equal(host(t)[n:], x0[n:].astype(np.float64)), what
            # the g_out form hands the summed gradient on and leaves the bias and its slots alone
            B, S1, S2 = dev(p0), dev(s10), dev(s20)
            G = torch.full((n + 2,), SENT, device="cuda")
            _lib.call("ocf_bias_opt_from_partials", B.data_ptr(), pd.data_ptr(), parts, ld, n, S1.data_ptr(),
                      S2.data_ptr(), G.data_ptr(), opt, cur_stream())
            sync()
            assert_within(host(G)[:n], g, gtol, what + " g_out")
            assert (G[n:] == SENT).all()
            for t, x0 in ((B, p0), (S1, s10), (S2, s20)):
                assert np.array_equal(host(t), x0.astype(np.float64)), what + " g_out"


# ---- ocf_stats_finalize ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", [1, 255, 256, 257, 1000])
def test_stats_finalize(gpu, n_parts):
    rng = np.random.RandomState(n_parts)
    sp = np.empty((n_parts, 4), np.float32)
    sp[:, 0] = rng.rand(n_parts) * 40
    sp[:, 1] = rng.rand(n_parts) * 9
    sp[:, 2] = rng.randint(0, 3000, n_parts)                              # counts: integer sums are exact in fp32
    sp[:, 3] = 1e9                                                        # unused column, never read
    spd = dev(sp)
    chain = -(-n_parts // 256) + 8                                        # a thread's strided terms + the LDS tree
    tot = sp[:, :3].astype(np.float64).sum(0)
    tol = chain * EPS32 * tot + 1e-30
    for n_tiles in (1, 63, 64, 65):
        for Mr in (4, 130, 256):
            rs = (rng.rand(n_tiles, Mr) * 5).astype(np.float32)
            out = torch.full((4 + Mr + 3,), SENT, device="cuda")
            _lib.call("ocf_stats_finalize", spd.data_ptr(), n_parts, dev(rs).data_ptr(), n_tiles, Mr, out.data_ptr(),
                      cur_stream())
            sync()
            o = host(out)
            what = "stats_finalize parts=%d tiles=%d M=%d" % (n_parts, n_tiles, Mr)
            assert_within(o[:2], tot[:2], tol[:2], what)
            assert o[2] == tot[2] and o[3] == 0.0, what
            rref = rs.astype(np.float64).sum(0)
            assert_within(o[4:4 + Mr], rref, (-(-n_tiles // 64) + 6) * EPS32 * rref + 1e-30, what + " rows")
            assert (o[4 + Mr:] == SENT).all(), what
    out = torch.full((4 + 130,), SENT, device="cuda")                     # no row SSE: out[4:] is left alone
    _lib.call("ocf_stats_finalize", spd.data_ptr(), n_parts, None, 0, 130, out.data_ptr(), cur_stream())
    sync()
    o = host(out)
    assert_within(o[:2], tot[:2], tol[:2], "stats_finalize no rows")
    assert o[2] == tot[2] and o[3] == 0.0 and (o[4:] == SENT).all()


# ---- ocf_sumsq -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 1 << 18, (1 << 18) + 1])
def test_sumsq(gpu, n):
    rng = np.random.RandomState(n % 1000)
    x = rng.randn(n).astype(np.float32)
    x[-1] = 3.0                                                           # the last element counts
    scale = float(np.float32(0.01))
    want = scale * (x.astype(np.float64) ** 2).sum()
    # squares, <= 2 strided terms, two LDS trees of 8, 4 partials per thread, the scale: 24 roundings at most
    tol = 24 * EPS32 * want
    ws = torch.full((1024,), SENT, device="cuda")
    out = torch.tensor([2.5, SENT], device="cuda")
    xd = dev(x)
    for calls in (1, 2):                                                  # accumulates into out[0], call after call
        _lib.call("ocf_sumsq", xd.data_ptr(), n, scale, ws.data_ptr(), out.data_ptr(), cur_stream())
        sync()
        o = host(out)
        ref = 2.5 + calls * want
        assert abs(o[0] - ref) <= calls * (tol + EPS32 * ref), (n, calls, o[0], ref)
        assert o[1] == SENT
    assert o[0] > 2.5 + 1.9 * want


# ---- ocf_colsum ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_colsum(gpu, dt):
    gscale = float(np.float32(R.GSCALE))
    for B in (1, 3, 200):
        for n in (1, 255, 256, 257, 700):
            ld = n + 9
            rng = np.random.RandomState(B * 1000 + n)
            d = R.round_to(rng.randn(B + 2, ld) + 0.3, dt)                # rows >= B and columns >= n: not summed
            out = torch.full((n + 4,), SENT, device="cuda")
            _lib.call("ocf_colsum", dev(d).to(TD[dt]).data_ptr(), CD[dt], ld, B, n, gscale, out.data_ptr(), cur_stream())
            sync()
            o = host(out)
            ref = gscale * d[:B, :n].astype(np.float64).sum(0)
            tol = (B // 2 + 3) * EPS32 * gscale * np.abs(d[:B, :n]).astype(np.float64).sum(0)
            assert_within(o[:n], ref, tol, "colsum %s B=%d N=%d" % (dt, B, n))
            assert (o[n:] == SENT).all()


# ---- ocf_pack_input --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("use_rows", [False, True])
def test_pack_input(gpu, dt, blocks, use_rows):
    n, blk, B, B_pad, ld_src, n_src = 130, 256, 5, 8, 140, 11
    xin_ld = 3 * blk
    rng = np.random.RandomState(7 + blocks)
    src = [dev((rng.randn(n_src, ld_src) * 3).astype(np.float32)) for _ in range(3)]
    rows = torch.tensor([9, 0, 4, 4, 10], dtype=torch.int64, device="cuda")
    xin = torch.full((B_pad, xin_ld), SENT, device="cuda").to(TD[dt])
    ptrs = [s.data_ptr() if i < blocks else None for i, s in enumerate(src)]
    _lib.call("ocf_pack_input", ptrs[0], ptrs[1], ptrs[2], ld_src, B, n, xin.data_ptr(), CD[dt], xin_ld, blk, B_pad,
              rows.data_ptr() if use_rows else None, cur_stream())
    sync()
    want = torch.zeros(B_pad, xin_ld, device="cuda")
    for i in range(blocks):
        want[:B, i * blk:i * blk + n] = (src[i][rows] if use_rows else src[i][:B])[:, :n]
    assert torch.equal(bits(xin), bits(want.to(TD[dt])))                  # rounded once; padding exactly +0


# ---- ocf_dense_targets -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_rows", [False, True])
def test_dense_targets(gpu, use_rows):
    B, n, ld, n_tiles, n_src = 37, 300, 310, 3, 50
    rng = np.random.RandomState(81)
    on = rng.rand(n_src, ld) < 0.15
    T = np.where(on, rng.randint(0, 11, (n_src, ld)) / 2.0, 0.0).astype(np.float32)      # some rated exactly 0
    Mk = np.where(on, -1.0, 0.0).astype(np.float32)
    extra = rng.rand(n_src, ld) < 0.02
    T[extra & ~on] = 1.5                                                                # t != 0, m = 0: an entry
    T[:, 299], Mk[:, 299] = 2.0, -1.0                                                   # the last real column
    assert (T[:, n:] != 0).any() and (on & (T == 0)).any()
    rows = rng.permutation(n_src)[:B].astype(np.int64) if use_rows else None
    want = R.bucket_layout(T, Mk, n_tiles, rows=rows, B=B, N=n)
    assert want[0][-1] > 1024 and want[0][1] < want[0][2] < want[0][3]     # more than one pass of the fill block
    got = dense_targets_call(dev(T), dev(Mk), ld, B, n, n_tiles, dev(rows) if use_rows else None, int(want[0][-1]) + 8)
    assert_buckets(got, want)
