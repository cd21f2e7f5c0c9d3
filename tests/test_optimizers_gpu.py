"""GPU: Adadelta and Adamax (ocf.h OCF_OPTK_ADADELTA / OCF_OPTK_ADAMAX) through every fused weight update.

The elementwise and bias kernels, the row-stream kernel and the generic tile kernel against the fp64 reference of
tests/optim_ref.py within the project's optimizer bar (tests/epilogue_ref.py OPT_RTOL / OPT_ATOL; tests/test_optim_ref.py
shows on the CPU that a correct float32 kernel meets it and every usual mistake misses it); the launch forms (dual-row,
pair, two launches; one-call step; role-split against generic) bit for bit; the fused small-model step against the
layer-wise path; end-to-end fp32 parity with the oracle; checkpoints; and the refusals.  Every test that compares
Adamax with an fp64 reference asserts that the reference takes each branch of max(beta2 * u, |g|) on at least 10 % of
the compared elements (a single element, n = 1, cannot; the bit-for-bit comparisons of two launch forms have no
reference).
"""
import ctypes

import numpy as np
import pytest
import torch

from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream
from tests import optim_ref as R
from tests.test_optim_ws_gpu import _sparse_batch, set_ws
from tests.test_rows_dw_gpu import _gen_for, _row_lists

CD = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dt is None else t.to(dt)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def opt_params(kind, l2=True, gscale=R.GSCALE):
    h = R.hyper2(l2, gscale)
    return h, _lib.OcfOptParams(R.OPT_KIND2[kind], h["lr"], h["eps"], h["rho"], h["beta2"], h["l2"], h["gscale"])


def check_state(kind, got, ref, what, g_eff=None, u0=None, beta2=None):
    """p and both slots within the bar; Adamax: both branches of the max among the compared elements"""
    if kind == "adamax" and g_eff is not None:
        R.assert_max_branches(g_eff, u0, beta2)
    worst = R.opt_worst([host(t) for t in got], ref)
    print("%s: worst |err| / (atol + rtol |ref|) = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)


# ---- 1. elementwise and bias kernels ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [1, 255, 257])
def test_opt_step_and_ex(gpu, kind, n):
    p0, s10, s20, g = R.inputs2(kind, (n,), 71 + n)
    # (one element cannot take both branches: the condition is asserted on the multi-element sizes)
    for l2 in (False, True):
        h, opt = opt_params(kind, l2)
        ge = R.eff_grad(g, p0, h["gscale"], h["l2"]) if n > 1 else None
        P, S1, S2, gd = dev(p0), dev(s10), dev(s20), dev(g)
        _lib.call("ocf_opt_step", P.data_ptr(), gd.data_ptr(), S1.data_ptr(), S2.data_ptr(), n, opt, cur_stream())
        torch.cuda.synchronize()
        ref = R.opt_update2(kind, p0, g, s10, s20, **h)
        check_state(kind, (P, S1, S2), ref, "opt_step %s l2=%d n=%d" % (kind, l2, n), ge, s20, h["beta2"])
        assert not np.array_equal(host(P), p0.astype(np.float64)) and not np.array_equal(host(S2), s20.astype(np.float64))
        # ocf_opt_step_ex: bf16 gradient, the 16-bit shadow = the updated weight rounded once
        gr = dev(g).to(torch.bfloat16)
        g16 = gr.float().cpu().numpy()
        for sdt in ("f16", "bf16"):
            P, S1, S2 = dev(p0), dev(s10), dev(s20)
            Sh = torch.full((n,), -3.0, device="cuda").to(TD[sdt])
            a = _lib.OcfOptStepArgs()
            a.p, a.g, a.g_dtype, a.n, a.opt = P.data_ptr(), gr.data_ptr(), _lib.DT_BF16, n, opt
            a.s1, a.s2, a.shadow, a.shadow_dtype = S1.data_ptr(), S2.data_ptr(), Sh.data_ptr(), CD[sdt]
            _lib.call("ocf_opt_step_ex", a, cur_stream())
            torch.cuda.synchronize()
            ref = R.opt_update2(kind, p0, g16, s10, s20, **h)
            ge = R.eff_grad(g16, p0, h["gscale"], h["l2"]) if n > 1 else None
            check_state(kind, (P, S1, S2), ref, "opt_step_ex %s l2=%d n=%d %s" % (kind, l2, n, sdt), ge, s20, h["beta2"])
            assert torch.equal(Sh.view(torch.int16), P.to(TD[sdt]).view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("parts", [1, 5, 65])
def test_bias_opt_from_partials(gpu, kind, parts):
    for n in (1, 255, 257):
        ld = n + 5
        rng = np.random.RandomState(1000 * parts + n)
        part = np.full((parts, ld), 1e6, np.float32)                      # columns >= n must not be read
        part[:, :n] = (0.05 / np.sqrt(parts)) * rng.randn(parts, n)
        g = part[:, :n].astype(np.float64).sum(0)
        p0, s10, s20 = R.inputs2(kind, (ld,), 5 * parts + n, g_std=None)
        pd = dev(part)
        for l2 in (False, True):
            h, opt = opt_params(kind, l2, gscale=7.0)                     # the partials are already scaled: ignored
            h["gscale"] = 1.0
            B, S1, S2 = dev(p0), dev(s10), dev(s20)
            _lib.call("ocf_bias_opt_from_partials", B.data_ptr(), pd.data_ptr(), parts, ld, n, S1.data_ptr(),
                      S2.data_ptr(), None, opt, cur_stream())
            torch.cuda.synchronize()
            ref = R.opt_update2(kind, p0[:n], g, s10[:n], s20[:n], **h)
            # the fixed-order fp32 sum of the partials against fp64: parts additions of 2^-24 on sum |x|, as a
            # gradient error; through the update it stays far inside the bar (|dp/dg| <= lr / u ~ 2.5 at most)
            ge = R.eff_grad(g, p0[:n], 1.0, h["l2"]) if n > 1 else None
            check_state(kind, (B[:n], S1[:n], S2[:n]), ref, "bias_opt %s parts=%d n=%d l2=%d" % (kind, parts, n, l2),
                        ge, s20[:n], h["beta2"])
            for t, x0 in ((B, p0), (S1, s10), (S2, s20)):                 # nothing past n
                assert np.array_equal(host(t)[n:], x0[n:].astype(np.float64))


# ---- 2. / 4. ocf_gemm EPI_OPTIM directly -------------------------------------------------------------------
def _gemm_optim(cd, M, N, K, opt, A, Bm, state, sparse=None, colsum=False, shadow=True, s2=True, extra=None):
    """ocf_gemm EPI_OPTIM on [K][M] x [K][N]; A dense (a tensor) or sparse (None, with the sp_* descriptor);
    returns [P, S1, S2, shadow or None, colsum or None]"""
    P, S1, S2 = (t.clone() for t in state)
    sdt = {_lib.DT_F16: torch.float16, _lib.DT_BF16: torch.bfloat16}.get(cd) if shadow else None
    Sh = P.to(sdt) if sdt is not None else None
    cs = torch.full((M,), -7.0, device="cuda") if colsum else None
    a = _lib.OcfGemmArgs()
    a.compute_dtype = cd
    a.A, a.a_dtype, a.a_col, a.lda = (A if A is not None else Bm).data_ptr(), cd, 1, M
    a.B, a.b_dtype, a.b_col, a.ldb = Bm.data_ptr(), cd, 1, N
    a.M, a.N, a.K, a.splits, a.epi = M, N, K, 1, _lib.EPI_OPTIM
    a.p, a.ld_out, a.s1 = P.data_ptr(), N, S1.data_ptr()
    a.s2 = S2.data_ptr() if s2 else None
    a.opt = opt
    if Sh is not None:
        a.p_shadow, a.shadow_blocked = Sh.data_ptr(), 0
    if cs is not None:
        a.sp_colsum = cs.data_ptr()
    if sparse is not None:
        a.a_sparse = 1
        for k, v in sparse.items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    for k, v in (extra or {}).items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    _lib.call("ocf_gemm", a, cur_stream())
    torch.cuda.synchronize()
    return [P, S1, S2, Sh, cs]


def _count(key):
    """a launch counter of the library (ocf_set_tuning "rows_count" / "optim_ws_count"), read and reset"""
    c = ctypes.c_int(-1)
    _lib.call("ocf_set_tuning", key, 0, ctypes.byref(c))
    return c.value


def _state(kind, M, N, seed):
    p, s1, s2 = R.inputs2(kind, (M, N), seed, g_std=None)
    return p, s1, s2


def _gscale_for(G):
    """|g * gscale| ~ 0.2 on the rows that have a gradient (about 0.4 of them: the others take the decayed branch
    of Adamax's max): P(|g| > u) ~ 0.7 there for u in [0.02, 0.12), so ~0.3 of all elements take |g|"""
    live = G[np.abs(G).sum(1) > 0]
    return float(np.float32(0.2 / live.std()))


_ROWS_CACHE = {}


def _rows_case(shape, cdn):
    """the sparse batch, its row lists, B and the fp64 gradient of a (shape, dtype) case, built once"""
    key = (shape, cdn)
    if key not in _ROWS_CACHE:
        M, N, K, krows = shape
        sp, dense = _sparse_batch(M, K, krows, seed=M + K + N, col_frac=0.6)
        bptr, ent, rptr, rent = _row_lists(sp, M, K)
        spr = dict(sp, sp_bptr=bptr, sp_ent=ent, sp_rowptr=rptr, sp_rowent=rent)
        g = torch.Generator().manual_seed(K + N)
        Bm = torch.randn(K, N, generator=g).to(TD[cdn]).cuda()
        G = dense.astype(np.float64).T @ host(Bm)
        _ROWS_CACHE[key] = (spr, dense, Bm, G)
    return _ROWS_CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cdn", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(384, 128, 64, 40), (384, 256, 64, 40), (384, 384, 64, 40), (384, 512, 256, 200)])
def test_rows_kernel_vs_fp64(gpu, shape, cdn, kind):
    M, N, K, krows = shape
    spr, dense, Bm, G = _rows_case(shape, cdn)
    p0, s10, s20 = _state(kind, M, N, seed=M + N)
    gs = _gscale_for(G)
    h, opt = opt_params(kind, True, gscale=gs)
    ref = R.opt_update2(kind, p0, G, s10, s20, **h)
    ge = R.eff_grad(G, p0, gs, h["l2"])
    empty = ~(dense != 0).any(0)
    assert empty[128:256].all() and 0 < empty.sum() < M                  # a whole 128-row tile without entries
    state = (dev(p0), dev(s10), dev(s20))
    prev = ctypes.c_int(0)
    try:
        for lng in (0, 1):
            _lib.call("ocf_set_tuning", b"rows_long", lng, ctypes.byref(prev) if lng == 0 else None)
            _lib.call("ocf_set_tuning", b"rows_count", 0, None)
            P, S1, S2, Sh, cs = _gemm_optim(CD[cdn], M, N, K, opt, None, Bm, state, sparse=spr, colsum=True)
            what = "rows %s %s %s long=%d" % (kind, cdn, shape, lng)
            assert _count(b"rows_count") == 1, what + ": the row-stream kernel did not run"
            check_state(kind, (P, S1, S2), ref, what, ge, s20, h["beta2"])
            if Sh is not None:
                assert torch.equal(Sh.view(torch.int16), P.to(Sh.dtype).view(torch.int16)), what
            want_cs = dense.astype(np.float64).sum(0) * np.float64(np.float32(gs))
            np.testing.assert_allclose(host(cs), want_cs, rtol=1e-5, atol=1e-7, err_msg=what)
            # rows without entries: no identity there -- the slots moved (to the reference, checked above), and
            # under Adamax so did p (m != 0)
            e = torch.from_numpy(empty).cuda()
            assert not torch.equal(S1[e], state[1][e]) and not torch.equal(S2[e], state[2][e]), what
            if kind == "adamax":
                assert (P[e] != state[0][e]).float().mean() > 0.99, what
    finally:
        _lib.call("ocf_set_tuning", b"rows_long", prev.value, None)


def _dense_operands(cdn, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(K, M, generator=g).to(TD[cdn]).cuda()
    Bm = torch.randn(K, N, generator=g).to(TD[cdn]).cuda()
    return A, Bm


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cdn", ["f16", "bf16"])
def test_role_split_matches_generic_bitwise(gpu, cdn, kind):
    M, N, K = 128, 128, 64
    A, Bm = _dense_operands(cdn, M, N, K, seed=M + K)
    state = tuple(dev(x) for x in _state(kind, M, N, seed=3))
    _, opt = opt_params(kind, True, gscale=0.05 / np.sqrt(K))
    prev = set_ws(0)
    try:
        _count(b"optim_ws_count")
        ref = _gemm_optim(CD[cdn], M, N, K, opt, A, Bm, state, colsum=True)
        assert _count(b"optim_ws_count") == 0, "the generic kernel's run took the role-split kernel"
        set_ws(1)
        got = _gemm_optim(CD[cdn], M, N, K, opt, A, Bm, state, colsum=True)
        assert _count(b"optim_ws_count") == 1, "the role-split kernel did not run"
    finally:
        set_ws(prev)
    for r, x in zip(ref, got):
        assert torch.equal(r, x)
    assert not torch.equal(ref[0], state[0]) and not torch.equal(ref[2], state[2])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cdn", ["f16", "f32"])
def test_generic_kernel_vs_fp64(gpu, cdn, kind):
    M, N, K = 384, 256, 192
    A, Bm = _dense_operands(cdn, M, N, K, seed=21)
    G = host(A).T @ host(Bm)
    gs = float(np.float32(0.1 / G.std()))          # every row has a gradient: P(|g| > u) ~ 0.5 at u ~ 0.07
    p0, s10, s20 = _state(kind, M, N, seed=9)
    h, opt = opt_params(kind, True, gscale=gs)
    prev = set_ws(0)
    try:
        _count(b"optim_ws_count")
        P, S1, S2, Sh, cs = _gemm_optim(CD[cdn], M, N, K, opt, A, Bm, (dev(p0), dev(s10), dev(s20)), colsum=True)
        assert _count(b"optim_ws_count") == 0 and _count(b"rows_count") == 0    # the generic tile kernel
    finally:
        set_ws(prev)
    ref = R.opt_update2(kind, p0, G, s10, s20, **h)
    check_state(kind, (P, S1, S2), ref, "generic %s %s" % (kind, cdn), R.eff_grad(G, p0, gs, h["l2"]), s20, h["beta2"])
    if Sh is not None:
        assert torch.equal(Sh.view(torch.int16), P.to(Sh.dtype).view(torch.int16))


# ---- 3. launch forms through the engine, bit for bit -----------------------------------------------------------
def _snapshot(eng, hist):
    return ([hist[k][0] for k in sorted(hist)], [t.clone() for t in eng.W] + [t.clone() for t in eng.b] +
            [s.clone() for sw, sb in eng.slots for s in sw + sb if s is not None] +
            [t.clone() for t in eng.Wsh if t is not None])


def _assert_same(out):
    for o in out[1:]:
        assert out[0][0] == o[0]
        for a, b in zip(out[0][1], o[1]):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cd,shape", [("float16", (900, 4000, 40000, 128, 0.5)),
                                      ("float32", (1682, 943, 100000, 256, 0.0))])
def test_rows_dual_bit_identical(gpu, cd, shape, kind):
    """the dual-row launch against two row-stream launches, and the dual launch really ran (one per step)"""
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    rows, cols, nnz, B, skew = shape
    out = []
    try:
        for dual in (0, 1):
            _lib.call("ocf_set_tuning", b"rows_dual", dual, None)
            _lib.call("ocf_set_tuning", b"rows_dual_count", 0, None)
            rd, gen = _gen_for(rows, cols, nnz, B, skew, seed=13)
            om = omni_model(1, 500 if cd != "float32" else 200, cols, B, dense_activation="sigmoid",
                            use_causal_info=False, dropout_probability=0.2, compute_dtype=cd, seed=4)
            m = om.model
            m.compile(R.our_opt2(kind), "mean_squared_error", metrics=["mae"])
            n = min(4, gen.num_batches)
            h = m.fit_generator(gen, n, epochs=1, verbose=0).history
            torch.cuda.synchronize()
            cnt = ctypes.c_int(-1)
            _lib.call("ocf_set_tuning", b"rows_dual_count", 0, ctypes.byref(cnt))
            assert cnt.value == (n if dual else 0), (dual, cnt.value)
            assert om.engine.tb is not None and "sp_rowptr" in om.engine.tb
            out.append(_snapshot(om.engine, h))
            del om, m
    finally:
        _lib.call("ocf_set_tuning", b"rows_dual", 1, None)
    _assert_same(out)
    assert all(np.isfinite(v) for v in out[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
def test_rows_dual_large_bit_identical(gpu, chunked_encdec, kind):
    """large weights: the pair launch against the dual-row launch against two launches"""
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    out = []
    try:
        for large, in_dec in ((0, False), (0, True), (1, True)):
            _lib.call("ocf_set_tuning", b"rows_dual_large", large, None)
            _lib.call("ocf_set_tuning", b"rows_dual_count", 0, None)
            rd, gen = _gen_for(2000, 30000, 300000, 256, 0.5, seed=21)
            om = omni_model(1, 500, 30000, 256, dense_activation="sigmoid", use_causal_info=False,
                            dropout_probability=0.2, compute_dtype="float16", seed=4)
            eng = om.engine
            eng.reduce_in_decoder = in_dec
            m = om.model
            m.compile(R.our_opt2(kind), "mean_squared_error", metrics=["mae"])
            n = min(4, gen.num_batches)
            h = m.fit_generator(gen, n, epochs=1, verbose=0).history
            torch.cuda.synchronize()
            cnt = ctypes.c_int(-1)
            _lib.call("ocf_set_tuning", b"rows_dual_count", 0, ctypes.byref(cnt))
            assert cnt.value == (n if large else 0), (large, cnt.value)
            assert eng._dec_reduced == in_dec
            out.append(_snapshot(eng, h))
            del om, m, eng
    finally:
        _lib.call("ocf_set_tuning", b"rows_dual_large", 1, None)
    _assert_same(out)


def _fast_run(fast, steps):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    from tests.parity import dataset
    data = dataset(rows=1200, cols=700, nnz=50000)
    np.random.seed(21)
    rd = data_reader(data.num_cols, data.train.n_rows, dataset=data, eval_mode="fixed_split", rng="numpy")
    om = omni_model(1, 500, data.num_cols, 128, dense_activation="sigmoid", use_causal_info=False,
                    dropout_probability=0.2, compute_dtype="bfloat16", seed=3)
    m = om.model
    m.compile(O.Adamax(lr=0.002), "mean_squared_error", metrics=["mae", "accurate_RMSE"])
    eng = om.engine
    eng.fast_steps = fast
    gen = rd.data_gen(128, [0.5, 0.9], "train", True, None, -1, pass_through_input_training=False)
    assert gen.num_batches >= steps
    n0 = eng.step_count
    h = m.fit_generator(gen, steps, epochs=1, verbose=0).history
    torch.cuda.synchronize()
    ready = eng._plan is not None and eng._plan.get("ready")
    return _snapshot(eng, h), ready, eng.step_count - n0, m.optimizer.iterations


@pytest.mark.gpu
def test_one_call_step_refreshes_adamax_lr(gpu):
    """the one-call step against the general path over seven steps of one fit_generator call, Adamax in bf16:
    lr_t = lr / (1 - beta_1^t) changes every step, so optimizer scalars frozen at the plan's first step fail this"""
    a, ready, n, it = _fast_run(True, 7)
    b, ready_g, n_g, it_g = _fast_run(False, 7)
    assert ready and not ready_g and n == n_g == 7 and it == it_g == 7
    _assert_same([a, b])


# ---- 5. fused small-model step against the layer-wise path and the oracle ----------------------------------------
def _mlp_oracle(kind, layers, H, act, k, n, N, B, w0, data, u, vs=0.1):
    """tests/test_mlp_step_gpu.py::_oracle for the two kinds (its table of largest steps does not know them): the
    fp64 replay of Keras' fit loop and the per-element rounding envelope env += step * min(2, c * r), r the running
    maximum of CHAIN_ROUNDINGS * u * G / |g| (the operand rounding relative to the gradient), capped at a step of the
    opposite sign.  The largest step and the conditioning c, from the updates themselves:
      Adamax    |m'| <= u' (1 - beta_1^t) / beta_2^t, so |step| <= lr / beta_2^t <= 1.01 lr; a relative error r of
                every g moves m' / u' by at most 2 (1 - beta_1^t) r: c = 3, that file's factor, covers it.
      Adadelta  from zero slots |u| <= sqrt(d + eps) / sqrt(1 - rho) with d' <= rho d + (1 - rho) u^2 (4.5e-4, 6.3e-4,
                8.9e-4 for lr = 1); the relative error e_t of u obeys e_t <= r (g) + r (sqrt a') + e_(t-1) (sqrt d),
                e_1 = 2 r: e_t <= 2 t r, and c_t = 2 t + 1 leaves the same margin of one r as 3 does over 2."""
    from oracle.model_oracle import OmniOracle
    from tests.parity import CHAIN_ROUNDINGS
    x, om_, t = data
    ora = OmniOracle([k * N] + [H] * layers + [N], activation=act).set_params(w0[0::2], w0[1::2])
    o = R.oracle_opt2(kind)
    split = int(n * (1 - vs))
    np.random.seed(42)
    idx = np.arange(split)
    np.random.shuffle(idx)
    losses, sizes = [], []
    env = [np.zeros_like(p) for p in ora.params()]
    rmax = [np.zeros_like(p) for p in ora.params()]
    d_max, total = 0.0, 0.0
    for s in range(-(-split // B)):
        sel = idx[s * B:(s + 1) * B]
        xin = np.concatenate([a[sel] for a in x], 1)
        loss, _, gW, gb = ora.loss_and_grads(xin, om_[sel], t[sel])
        grads = [g for pair in zip(gW, gb) for g in pair]
        GW, Gb = ora.grad_magnitudes(xin, om_[sel], t[sel], u=u)
        if kind == "adamax":
            step, c = 1.01 * o.lr, 3.0
        else:
            ustep = np.sqrt(d_max + o.eps) / np.sqrt(1.0 - o.rho)
            d_max = o.rho * d_max + (1.0 - o.rho) * ustep * ustep
            step, c = o.lr * ustep, 2.0 * (s + 1) + 1.0
        total += step
        for j, (g, G) in enumerate(zip(grads, [z for pair in zip(GW, Gb) for z in pair])):
            rmax[j] = np.maximum(rmax[j], CHAIN_ROUNDINGS * u * G / np.maximum(np.abs(g), 1e-30))
            env[j] += step * np.minimum(2.0, c * rmax[j])
        losses.append(loss)
        sizes.append(len(sel))
        ora.set_flat(o.step(ora.params(), grads))
    sse = 0.0
    for s0 in range(split, n, B):
        sel = np.arange(s0, min(n, s0 + B))
        y, _ = ora.forward(np.concatenate([a[sel] for a in x], 1), om_[sel])
        sse += float(((y - t[sel]) ** 2).sum())
    return float(np.dot(losses, sizes) / np.sum(sizes)), sse / ((n - split) * N), ora.params(), env, total


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cd", ["float32", "float16"])
def test_fused_mlp_step_matches_layerwise(gpu, monkeypatch, cd, kind):
    """three steps (360 training rows, B = 128) of Model.fit through ocf_mlp_step and through the layer-wise path.
    fp32: tests/test_mlp_step_gpu.py's bars for Adam against the layer-wise path (1e-5 relative on loss and
    val_loss, 5e-5 on every weight).  f16: the two paths round their operands at different points, so they are not
    compared weight by weight with each other; each is held to that file's 16-bit bars against the fp64 oracle
    (_mlp_oracle): loss and val_loss within 1e-2, every weight within 1e-5 + its rounding envelope -- tight wherever
    the gradient is well conditioned -- and, as tests/parity.py asks of the bulk, the 99th / 99.9th percentile
    errors within 0.02 / 0.15 of the sum of the largest steps."""
    import tests.test_mlp_step_gpu as T
    from oracle.model_oracle import AdamOracle
    from tests.parity import UNIT_ROUNDOFF
    old = T._opt
    monkeypatch.setattr(T, "_opt", lambda name: (lambda: R.our_opt2(name), AdamOracle) if name in R.KINDS else old(name))
    layers, H, act, k, n, N, B = 2, 160, "sigmoid", 2, 400, 100, 128
    args = (layers, H, act, kind, cd, k, n, N, B)
    a = T._fit(*args, fused=True)
    b = T._fit(*args, fused=False)
    assert a[3] and not b[3]
    for x, w0 in zip(a[2], a[1]):
        assert not np.array_equal(x, w0)
    if cd == "float32":
        assert abs(a[0]["loss"][0] - b[0]["loss"][0]) <= 1e-5 * b[0]["loss"][0]
        assert abs(a[0]["val_loss"][0] - b[0]["val_loss"][0]) <= 1e-5 * b[0]["val_loss"][0]
        for x, y in zip(a[2], b[2]):
            assert np.abs(x - y).max() <= 5e-5, float(np.abs(x - y).max())
        return
    loss_o, val_o, p, env, total = _mlp_oracle(kind, layers, H, act, k, n, N, B, a[1], a[4], UNIT_ROUNDOFF[cd])
    for name, run in (("fused", a), ("layer-wise", b)):
        hist, w = run[0], run[2]
        errs = [np.abs(g - o) for g, o in zip(w, p)]
        worst = max(float((e / (1e-5 + v)).max()) for e, v in zip(errs, env))
        q99, q999 = np.quantile(np.concatenate([e.ravel() for e in errs]), [0.99, 0.999]) / total
        print("%s %s f16 against the oracle: loss %.3g / val_loss %.3g relative, worst |err| / (1e-5 + envelope) %.3g, "
              "99th / 99.9th percentile error %.3g / %.3g of the steps' sum %.3g"
              % (kind, name, abs(hist["loss"][0] - loss_o) / loss_o, abs(hist["val_loss"][0] - val_o) / val_o, worst,
                 q99, q999, total))
        assert abs(hist["loss"][0] - loss_o) <= 1e-2 * loss_o, (name, hist["loss"][0], loss_o)
        assert abs(hist["val_loss"][0] - val_o) <= 1e-2 * val_o, (name, hist["val_loss"][0], val_o)
        for i, (e, v) in enumerate(zip(errs, env)):
            assert (e <= 1e-5 + v).all(), (name, i, float(e.max()), int((e > 1e-5 + v).sum()))
        assert q99 <= 0.02 and q999 <= 0.15, (name, float(q99), float(q999))


# ---- 6. end-to-end parity in exact fp32 ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_parity_with_oracle(gpu, monkeypatch, kind):
    from tests import parity
    our, ora = parity.our_opt, parity.oracle_opt
    monkeypatch.setattr(parity, "our_opt", lambda n, lr=None: R.our_opt2(n, lr) if n in R.KINDS else our(n, lr))
    made = []

    def oracle_opt(n, lr=None):
        made.append(R.oracle_opt2(n, lr) if n in R.KINDS else ora(n, lr))
        return made[-1]

    monkeypatch.setattr(parity, "oracle_opt", oracle_opt)
    res = parity.run_parity("float32", kind, 1, "sigmoid")
    if kind == "adamax":      # the fp64 reference's max over the steps after the first (from u = 0 every |g| wins)
        lo, hi = made[-1].branch_fractions()
        print("adamax max branches: decayed u %.3f, |g| %.3f" % (lo, hi))
        assert lo >= 0.1 and hi >= 0.1, (lo, hi)
    print(kind, res.max_param_err())
    parity.assert_fp32(res)


# ---- 7. checkpoints ----------------------------------------------------------------------------------------
def _ckpt_model(kind, seed=4):
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    rd, gen = _gen_for(900, 4000, 40000, 128, 0.5, seed=13)
    om = omni_model(1, 200, 4000, 128, dense_activation="sigmoid", use_causal_info=False, dropout_probability=0.2,
                    compute_dtype="float16", seed=seed)
    om.model.compile(R.our_opt2(kind) if kind in R.KINDS else kind, "mean_squared_error", metrics=["mae"])
    return om, gen


def _full_state(eng):
    return [t.clone() for t in eng.W + eng.b + [s for sw, sb in eng.slots for s in sw + sb if s is not None]
            + [w for w in eng.Wsh if w is not None]]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
def test_checkpoint_round_trip(gpu, tmp_path, kind):
    from safetensors.numpy import load_file, save_file
    a, ga = _ckpt_model(kind)
    a.model.fit_generator(ga, 2, epochs=1, verbose=0)
    path = str(tmp_path / "ck.safetensors")
    a.model.save(path)
    saved = _full_state(a.engine)
    a.model._train_one(ga)
    torch.cuda.synchronize()
    want = _full_state(a.engine)
    t = load_file(path)
    assert bytes(bytearray(t["opt/name"])).decode("ascii") == kind and int(t["opt/iterations"][0]) == 2
    old = str(tmp_path / "old.safetensors")
    save_file({k: v for k, v in t.items() if k != "opt/name"}, old)          # a file from before the field
    for p in (path, old):
        b, gb = _ckpt_model(kind)
        b.model.fit_generator(gb, 2, epochs=1, verbose=0)
        eb = b.engine
        for x in eb.W + eb.b:
            x.add_(0.125)
        for sw, sb in eb.slots:
            for s in sw + sb:
                s.mul_(3.0).add_(1.0)
        b.model.optimizer.iterations = 17
        b.model.load(p)
        torch.cuda.synchronize()
        assert b.model.optimizer.iterations == 2
        for x, y in zip(saved, _full_state(eb)):
            assert torch.equal(x, y)
        b.model._train_one(gb)
        torch.cuda.synchronize()
        for x, y in zip(want, _full_state(eb)):
            assert torch.equal(x, y)
        assert not torch.equal(want[0], saved[0])


@pytest.mark.gpu
def test_checkpoint_of_another_optimizer_is_refused(gpu, tmp_path):
    a, _ = _ckpt_model("adam")
    path = str(tmp_path / "adam.safetensors")
    a.model.save(path)
    b, _ = _ckpt_model("adamax")
    before = _full_state(b.engine)
    with pytest.raises(ValueError, match="optimizer state of 'adam'"):
        b.model.load(path)
    assert b.model.optimizer.iterations == 0
    for x, y in zip(before, _full_state(b.engine)):            # nothing was touched: weights, slots, shadows
        assert torch.equal(x, y)
    b.model.load(path, with_optimizer=False)                                  # the weights alone are welcome


# ---- 8. refusals -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    n = 64
    p0, s10, s20, g = R.inputs2("adamax", (n,), 1)
    P, S1, S2, gd = dev(p0), dev(s10), dev(s20), dev(g)

    def untouched():
        torch.cuda.synchronize()
        return np.array_equal(host(P), p0.astype(np.float64)) and np.array_equal(host(S1), s10.astype(np.float64))

    # a kind outside the enum
    for bad in (6, -1, 99):
        opt = _lib.OcfOptParams(bad, 0.01, 1e-8, 0.9, 0.999, 0, 1.0)
        with pytest.raises(_lib.OcfError, match="unknown optimizer kind"):
            _lib.call("ocf_opt_step", P.data_ptr(), gd.data_ptr(), S1.data_ptr(), S2.data_ptr(), n, opt, cur_stream())
        assert untouched()
    # a new kind without its second slot
    for kind in R.KINDS:
        _, opt = opt_params(kind)
        with pytest.raises(_lib.OcfError, match="both optimizer slots"):
            _lib.call("ocf_opt_step", P.data_ptr(), gd.data_ptr(), S1.data_ptr(), None, n, opt, cur_stream())
        assert untouched()
    # ocf_gemm EPI_OPTIM: dense operands (the role-split gate) and row lists (the row-stream gate)
    M, N, K, krows = 384, 128, 64, 40
    spr, dense, Bm, G = _rows_case((M, N, K, krows), "f16")
    A, _ = _dense_operands("f16", M, N, K, seed=5)
    for kind in R.KINDS:
        state = tuple(dev(x) for x in _state(kind, M, N, seed=2))
        _, opt = opt_params(kind)
        for sparse, Ad in ((None, A), (spr, None)):
            with pytest.raises(_lib.OcfError, match="both optimizer slots"):
                _gemm_optim(_lib.DT_F16, M, N, K, opt, Ad, Bm, state, sparse=sparse, s2=False)
            bad = _lib.OcfOptParams(7, 0.01, 1e-8, 0.9, 0.999, 0, 1.0)
            with pytest.raises(_lib.OcfError, match="unknown optimizer kind"):
                _gemm_optim(_lib.DT_F16, M, N, K, bad, Ad, Bm, state, sparse=sparse)
        # the folded output-bias update runs the weight's kernel instance: it needs both of its slots too
        cb = dict(cb_p=torch.zeros(M, device="cuda"), cb_s1=torch.zeros(M, device="cuda"), cb_op=opt)
        with pytest.raises(_lib.OcfError, match="both optimizer slots"):
            _gemm_optim(_lib.DT_F16, M, N, K, opt, None, Bm, state, sparse=spr, colsum=True, extra=cb)
        with pytest.raises(_lib.OcfError, match="both optimizer slots"):
            _gemm_optim(_lib.DT_F16, M, N, K, opt, A, Bm, state, colsum=True, extra=cb)
        # live-row records skip rows: only where a zero gradient is the identity (Adagrad, l2 = 0)
        rec = torch.zeros(M // 128 * _lib.LIVE_REC, dtype=torch.uint8, device="cuda")
        h = R.hyper2(False)
        o2 = _lib.OcfOptParams(R.OPT_KIND2[kind], h["lr"], h["eps"], h["rho"], h["beta2"], 0.0, 1.0)
        with pytest.raises(_lib.OcfError, match="row_live"):
            _gemm_optim(_lib.DT_F16, M, N, K, o2, None, Bm, state, sparse=spr, extra=dict(row_live=rec))
    # the multi-GPU layouts
    for kind in R.KINDS:
        om, _ = _ckpt_model(kind)
        with pytest.raises(NotImplementedError):
            om.model.enable_data_parallel(0, 2)
        with pytest.raises(NotImplementedError):
            om.model.enable_feature_parallel(0, 2)
        assert om.model.dp is None and om.model.fp is None
        ok, _ = _ckpt_model("adagrad")
        ok.model.enable_feature_parallel(0, 2)
        with pytest.raises(NotImplementedError):
            ok.model.compile(R.our_opt2(kind), "mean_squared_error")
        ok.model.fp = None
        ok.model.dp = object()                       # (stands for a DataParallel: compile must refuse before using it)
        with pytest.raises(NotImplementedError):
            ok.model.compile(R.our_opt2(kind), "mean_squared_error")
        ok.model.dp = None
        assert isinstance(ok.model.optimizer, O.Adagrad)
        ok.engine.dp_world = 2
        with pytest.raises(NotImplementedError):
            ok.engine.set_optimizer(R.our_opt2(kind))
        ok.engine.dp_world = 1
