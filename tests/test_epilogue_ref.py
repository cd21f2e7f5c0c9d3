"""CPU checks of tests/epilogue_ref.py at the GPU tests' own inputs and hyper-parameters: (1) a correct float32
kernel (the float32 restatement of opt_update_k) sits inside the optimizer tolerance with a factor 10 to spare,
(2) every deliberately wrong variant misses it by at least 5x for every optimizer it applies to, so
tests/test_epilogues_gpu.py and tests/test_elem_gpu.py would catch a subtly wrong kernel, (3) the activations and
the masked-MSE arithmetic agree with oracle/model_oracle.py."""
import numpy as np
import pytest

import epilogue_ref as R
from oracle.model_oracle import (AdagradOracle, AdamOracle, RMSpropOracle, SGDOracle, act_fwd, act_grad_from_out,
                                 batch_metrics)


def _input_sets():
    """(name, p, s1, s2, raw g in float32) of the GEMM test (per compute dtype) and of the elementwise tests"""
    out = []
    for cd in ("f32", "f16", "bf16"):
        A, B = R.optim_operands(cd)
        g = (A.astype(np.float64).T @ B.astype(np.float64)).astype(np.float32)     # fp32 accumulator
        out.append(("gemm-" + cd,) + R.opt_inputs((R.M, R.N), 22) + (g,))
    out.append(("elem",) + R.opt_inputs((257,), 23, g_std=R.G_STD))
    return out


INPUTS = _input_sets()


@pytest.mark.parametrize("kind", R.OPTS)
@pytest.mark.parametrize("l2", [False, True])
def test_float32_restatement_is_well_inside_the_tolerance(kind, l2):
    for name, p, s1, s2, g in INPUTS:
        h = R.hyper(kind, l2)
        ref = R.opt_update(kind, p, g, s1, s2, **h)
        got = R.opt_update(kind, p, g, s1, s2, dtype=np.float32, **h)
        assert all(x is None or x.dtype == np.float32 for x in got)
        worst = R.opt_worst(got, ref)
        assert worst <= 0.1, (name, kind, worst)


@pytest.mark.parametrize("variant", sorted(R.WRONG_OPT))
def test_wrong_optimizer_variants_miss_the_tolerance(variant):
    for kind in R.WRONG_OPT[variant]:
        for l2 in ([True] if "l2" in variant else [False, True]):
            for name, p, s1, s2, g in INPUTS:
                h = R.hyper(kind, l2)
                ref = R.opt_update(kind, p, g, s1, s2, **h)
                bad = R.opt_update(kind, p, g, s1, s2, variant=variant, **h)
                miss = R.opt_worst(bad, ref)
                assert miss >= 5.0, (variant, kind, l2, name, miss)


def test_wrong_variants_cover_every_optimizer():
    assert {k for v in R.WRONG_OPT.values() for k in v} == set(R.OPTS)
    assert R.GSCALE != 1.0 and all(R.HYPER[k] for k in ("lr", "eps", "rho", "beta2", "l2"))


@pytest.mark.parametrize("variant", R.WRONG_ACT)
def test_wrong_backward_variants_miss_the_product_tolerance(variant):
    """GRAD_ACT's inputs: delta [M][K] ~ randn times W [N][K] ~ 0.05 randn, keep 0.8"""
    rng = np.random.RandomState(5)
    A = rng.randn(R.M, R.K)
    W = 0.05 * rng.randn(R.N, R.K)
    d = A @ W.T
    tol = R.product_tol(R.K, np.abs(A) @ np.abs(W).T, d) / 0.8
    mask = (rng.rand(R.M, R.N) < 0.8).astype(np.uint8)
    for name in (["sigmoid"] if variant == "sigmoid_grad_as_tanh" else R.ACTS):
        a = R.a_in_for(name, (R.M, R.N), rng)
        ref = R.grad_act(name, d, a, mask, 0.8)
        bad = R.grad_act(name, d, a, mask, 0.8, variant=variant)
        assert (np.abs(bad - ref) / tol).max() >= 5.0, (variant, name)


def test_optimizers_agree_with_the_oracle():
    """one step from the oracle's zero slots (Keras: accumulators start at 0) is the same arithmetic"""
    rng = np.random.RandomState(1)
    p, g = rng.randn(50), rng.randn(50)
    z = np.zeros(50)
    cases = [("sgd", SGDOracle(lr=0.05), 0.05, {}), ("adagrad", AdagradOracle(lr=0.05, epsilon=1e-2), 0.05, {}),
             ("rmsprop", RMSpropOracle(lr=0.05, rho=0.9, epsilon=1e-2), 0.05, {}),
             ("adam", AdamOracle(lr=0.05, beta_1=0.9, beta_2=0.99, epsilon=1e-2),
              0.05 * np.sqrt(1 - 0.99) / (1 - 0.9), {})]
    for kind, ora, lr, _ in cases:
        want = ora.step([p], [g])[0]
        # (hyper-parameters pass through float32, as the kernels take them: 6e-8 relative each, 1.5e-6 on
        # 1 - beta2 = 0.01; compared on the step p_new - p)
        got = R.opt_update(kind, p, g, z, z, lr=lr, eps=1e-2, rho=0.9, beta2=0.99)[0]
        np.testing.assert_allclose(got - p, want - p, rtol=1e-5, atol=0, err_msg=kind)


def test_sgd_rejects_momentum_and_nesterov():
    """Keras 2.0.4's SGD has momentum and Nesterov momentum; the library implements neither and says so"""
    from omnidirectional_collaborative_filtering_amd import _lib, optimizers as O
    for kw in (dict(momentum=0.9), dict(nesterov=True), dict(momentum=0.9, nesterov=True)):
        with pytest.raises(ValueError, match="momentum"):
            O.SGD(lr=0.01, **kw)
    with pytest.raises(TypeError):
        O.SGD(lr=0.01, rho=0.9)                       # unknown keywords are no longer swallowed
    o = O.SGD(lr=0.05, momentum=0.0, decay=0.5, nesterov=False)
    assert isinstance(O.get("sgd"), O.SGD) and O.get("sgd").lr == pytest.approx(0.01)
    sp = o.step_params(gscale=2.0, l2=1e-2)
    assert (sp.kind, sp.gscale) == (_lib.OPT_SGD, 2.0) and sp.lr == pytest.approx(0.05) and o.n_slots == 0
    o.iterations = 2
    assert o.step_params().lr == pytest.approx(0.05 / 2.0)


def test_sgd_oracle_decay():
    ora = SGDOracle(lr=0.1, decay=0.5)
    p = [np.ones(3)]
    p = ora.step(p, [np.ones(3)])          # lr
    np.testing.assert_allclose(p[0], 0.9)
    p = ora.step(p, [np.ones(3)])          # lr / (1 + 0.5 * 1)
    np.testing.assert_allclose(p[0], 0.9 - 0.1 / 1.5)


@pytest.mark.parametrize("name", R.ACTS)
def test_activations_agree_with_the_oracle(name):
    rng = np.random.RandomState(2)
    z = 3.0 * rng.randn(64, 33)
    z[0, :4] = [0.0, -0.0, 30.0, -30.0]
    a = R.act(name, z)
    np.testing.assert_allclose(a, act_fwd(name, z), rtol=1e-15, atol=0)
    np.testing.assert_allclose(R.act_grad(name, a), act_grad_from_out(name, a, z), rtol=1e-15, atol=0)
    mask = (rng.rand(64, 33) < 0.8).astype(np.float64)
    np.testing.assert_allclose(R.dropout_fwd(a, mask, 0.8), a * (mask / 0.8), rtol=1e-15)
    d = rng.randn(64, 33)
    np.testing.assert_allclose(R.grad_act(name, d, a, mask, 0.8),
                               d * (mask / 0.8) * act_grad_from_out(name, a, z), rtol=1e-15)
    assert np.isfinite(R.act(name, np.array([1e4, -1e4, 100.0, -100.0]))).all()


def test_masked_mse_agrees_with_batch_metrics():
    rng = np.random.RandomState(3)
    B, N = 40, 77
    on = rng.rand(B, N) < 0.2
    t = np.where(on, rng.randint(1, 11, (B, N)) / 2.0, 0.0)
    t[on & (rng.rand(B, N) < 0.05)] = 0.0                    # ratings of exactly 0
    for aux in (-1.0, 1.0):
        m = np.where(on, aux, 0.0)
        y = 0.4 * rng.randn(B, N)
        s = R.masked_mse(y, t, m)
        np.testing.assert_array_equal(s["yhat"], m * y)
        np.testing.assert_allclose(s["d"], (m * y - t) * m, rtol=0, atol=0)
        bm = batch_metrics(t, m * y, N, B, 4.5)
        scale = N * B / s["count"]
        assert s["count"] == np.count_nonzero(t + m * y)
        np.testing.assert_allclose(s["sse"] / (B * N), bm["loss"], rtol=1e-12)
        np.testing.assert_allclose(s["sae"] / (B * N), bm["mean_absolute_error"], rtol=1e-12)
        np.testing.assert_allclose(s["sse"] / (B * N) * scale, bm["accurate_MSE"], rtol=1e-12)
        np.testing.assert_allclose(np.sqrt(s["row_sse"] / N * scale).mean(), bm["accurate_RMSE"], rtol=1e-12)
    # an entry with m = 0, t != 0 is counted; t = m = 0 is no entry
    s = R.masked_mse(np.full((1, 3), 0.3), np.array([[2.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]))
    assert s["count"] == 2 and s["sse"] == pytest.approx(4.0 + 0.09) and s["d"][0, 0] == 0.0


def test_bucket_layout():
    T = np.zeros((3, 260), np.float32)
    Mk = np.zeros((3, 260), np.float32)
    T[0, 5], Mk[0, 5] = 2.5, -1
    Mk[2, 3] = -1                       # rated exactly 0
    T[1, 127], Mk[1, 127] = 1.0, -1
    T[1, 128] = 3.0                     # t != 0, m = 0
    T[0, 259], Mk[0, 259] = 4.0, -1
    ptr, rc, bt, bm = R.bucket_layout(T, Mk, 3)
    assert ptr.tolist() == [0, 3, 4, 5]
    assert rc.tolist() == [(0 << 7) | 5, (1 << 7) | 127, (2 << 7) | 3, (1 << 7) | 0, (0 << 7) | 3]
    assert bt.tolist() == [2.5, 1.0, 0.0, 3.0, 4.0] and bm.tolist() == [-1, -1, -1, 0, -1]
    ptr2, rc2, _, _ = R.bucket_layout(T, Mk, 3, rows=[2, 0], B=2)
    assert ptr2.tolist() == [0, 2, 2, 3] and rc2.tolist() == [(0 << 7) | 3, (1 << 7) | 5, (1 << 7) | 3]
