"""CPU: the Adadelta / Adamax references of tests/optim_ref.py and the Python optimizer surface.

 * the float32 restatement of opt_update_k's operation order sits at or below half the project's optimizer bar
   (tests/epilogue_ref.py OPT_RTOL / OPT_ATOL) against the fp64 reference, and every deliberately wrong variant
   at or above 5x the bar (the factor of tests/test_epilogue_ref.py) -- so the GPU tests' bar is attainable and
   rejects each mistake; the inputs take both branches of Adamax's max;
 * the fp64 reference against torch.optim.Adadelta / Adamax over four steps from zero slots;
 * optimizers.Adadelta / Adamax: defaults, n_slots, get(), step_params with and without decay, strict keywords;
 * the end-to-end fp32 bar (tests/parity.py FP32_ABS) is attainable: the oracle in float32 against float64.
"""
import math

import numpy as np
import pytest

from tests import optim_ref as R
from tests.epilogue_ref import OPT_ATOL, OPT_RTOL

SHAPE = (64, 257)


def _case(kind, l2):
    p, s1, s2, g = R.inputs2(kind, SHAPE, seed=7)
    h = R.hyper2(l2=l2)
    ref = R.opt_update2(kind, p, g, s1, s2, **h)
    return p, s1, s2, g, h, ref


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_restatement_within_half_the_bar(kind, l2):
    p, s1, s2, g, h, ref = _case(kind, l2)
    got = R.opt_update2(kind, p, g, s1, s2, dtype=np.float32, **h)
    assert all(x.dtype == np.float32 for x in got)
    w = R.opt_worst(got, ref)
    print("%s l2=%s fp32 restatement: %.4f of the bar" % (kind, l2, w))
    assert w <= 0.5, w


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("kind,variant", [(k, v) for k in R.KINDS for v in R.WRONG2[k]])
def test_wrong_variants_rejected(kind, variant, l2):
    p, s1, s2, g, h, ref = _case(kind, l2)
    bad = R.opt_update2(kind, p, g, s1, s2, variant=variant, **h)
    w = R.opt_worst(bad, ref)
    print("%s %s l2=%s: %.1f x the bar" % (kind, variant, l2, w))
    assert w >= 5.0, (variant, w)


@pytest.mark.parametrize("l2", [False, True])
def test_inputs_take_both_branches_of_the_max(l2):
    p, s1, s2, g, h, _ = _case("adamax", l2)
    R.assert_max_branches(R.eff_grad(g, p, h["gscale"], h["l2"]), s2, h["beta2"])
    # a unit-scale gradient would not: |g * gscale| ~ 3e-3 never reaches beta2 * u >= 0.0198
    lo, hi = R.max_branches(R.eff_grad(g / R.G_STD, p, h["gscale"], 0.0), s2, h["beta2"])
    assert hi < 0.01


def test_bar_is_the_projects():
    assert (OPT_RTOL, OPT_ATOL) == (1e-5, 2e-6) and R.OPT_RTOL is OPT_RTOL and R.OPT_ATOL is OPT_ATOL


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_matches_torch_optim(kind):
    """four steps from zero slots in fp64; torch puts Adamax's eps inside the max, Keras after it: eps = 1e-12"""
    import torch
    rng = np.random.RandomState(3)
    p0 = rng.randn(50)
    grads = [rng.randn(50) for _ in range(4)]
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    if kind == "adadelta":
        hp = dict(lr=1.0, rho=0.95, eps=1e-8)
        to = torch.optim.Adadelta([tp], lr=1.0, rho=0.95, eps=1e-8)
    else:
        hp = dict(lr=0.002, rho=0.9, beta2=0.999, eps=1e-12)
        to = torch.optim.Adamax([tp], lr=0.002, betas=(0.9, 0.999), eps=1e-12)
    p, s1, s2 = p0.copy(), np.zeros(50), np.zeros(50)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.tensor(g, dtype=torch.float64)
        to.step()
        h = dict(hp)
        if kind == "adamax":
            h["lr"] = hp["lr"] / (1.0 - 0.9 ** t)
        # (opt_update2 passes its scalars through float32, as the kernel receives them; not here: fp64 throughout)
        p, s1, s2 = _update_fp64_scalars(kind, p, g, s1, s2, **h)
    err = float(np.abs(p - tp.detach().numpy()).max())
    assert err <= 1e-15, err            # (a few fp64 ulps of |p| ~ 1: the two write the quotient in another order)


def _update_fp64_scalars(kind, p, g, s1, s2, lr, eps, rho, beta2=0.0):
    if kind == "adadelta":
        a = rho * s1 + (1.0 - rho) * (g * g)
        u = (g * np.sqrt(s2 + eps)) / np.sqrt(a + eps)
        return p - lr * u, a, rho * s2 + (1.0 - rho) * (u * u)
    m = rho * s1 + (1.0 - rho) * g
    u = np.maximum(beta2 * s2, np.abs(g))
    return p - (lr * m) / (u + eps), m, u


@pytest.mark.parametrize("kind", R.KINDS)
def test_fp64_scalar_form_is_opt_update2(kind):
    """the helper above is opt_update2 but for the float32 rounding of the scalars"""
    p, s1, s2, g = R.inputs2(kind, (40,), seed=2, g_std=1.0)
    h = dict(lr=0.5, eps=0.25, rho=0.75, beta2=0.5)                  # exact in float32
    a = R.opt_update2(kind, p, g, s1, s2, **h)
    b = _update_fp64_scalars(kind, *(np.asarray(x, np.float64) for x in (p, g, s1, s2)), **h)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- the Python surface -----------------------------------------------------------------------------------
def test_surface_defaults_and_get():
    from omnidirectional_collaborative_filtering_amd import _lib, optimizers as O
    a = O.Adadelta()
    assert (a.lr, a.rho, a.epsilon, a.decay, a.n_slots, a.kind) == (1.0, 0.95, 1e-8, 0.0, 2, 4)
    assert (_lib.OPT_ADADELTA, _lib.OPT_ADAMAX) == (4, 5)
    x = O.Adamax()
    assert (x.lr, x.beta_1, x.beta_2, x.epsilon, x.decay, x.n_slots, x.kind) == (0.002, 0.9, 0.999, 1e-8, 0.0, 2, 5)
    assert isinstance(O.get("adadelta"), O.Adadelta) and isinstance(O.get("Adamax"), O.Adamax)
    assert O.get(x) is x
    assert a.get_config() == {"lr": 1.0, "rho": 0.95, "epsilon": 1e-8, "decay": 0.0}
    assert x.get_config() == {"lr": 0.002, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-8, "decay": 0.0}
    # which optimizers' scalars change with the step (the engine's one-call step freezes the others')
    assert not a.scalars_change and x.scalars_change and O.Adam().scalars_change and not O.Adagrad().scalars_change
    assert O.Adadelta(decay=0.1).scalars_change and O.Adagrad(decay=0.1).scalars_change
    with pytest.raises(ValueError):
        O.get("nadam")


@pytest.mark.parametrize("decay", [0.0, 0.25])
def test_step_params_over_three_iterations(decay):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    a, x = O.Adadelta(lr=0.5, rho=0.9, epsilon=1e-6, decay=decay), O.Adamax(lr=0.004, beta_1=0.8, beta_2=0.99, decay=decay)
    for it in range(3):
        a.iterations = x.iterations = it
        lr_d = 1.0 / (1.0 + decay * it) if decay else 1.0
        oa, ox = a.step_params(gscale=2.0, l2=0.5), x.step_params(gscale=3.0)
        assert (oa.kind, oa.gscale, oa.l2, oa.beta2) == (4, 2.0, 0.5, 0.0)
        assert oa.lr == pytest.approx(0.5 * lr_d, rel=1e-6) and oa.rho == pytest.approx(0.9, rel=1e-6)
        assert oa.eps == pytest.approx(1e-6, rel=1e-6)
        assert (ox.kind, ox.gscale, ox.l2) == (5, 3.0, 0.0)
        assert ox.lr == pytest.approx(0.004 * lr_d / (1.0 - 0.8 ** (it + 1)), rel=1e-6)
        assert ox.rho == pytest.approx(0.8, rel=1e-6) and ox.beta2 == pytest.approx(0.99, rel=1e-6)
        assert ox.eps == pytest.approx(1e-8, rel=1e-6)


@pytest.mark.parametrize("cls", ["Adadelta", "Adamax"])
def test_unknown_keyword_raises(cls):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    with pytest.raises(TypeError):
        getattr(O, cls)(momentum=0.9)
    with pytest.raises(TypeError):
        getattr(O, cls)(clipnorm=1.0)


def test_train_accepts_the_names():
    from omnidirectional_collaborative_filtering_amd import train
    assert {"adadelta", "adamax"} <= set(train.OPTIMIZERS)
    assert train.KERAS_LR == {"adadelta": 1.0, "adamax": 0.002}
    # not given (None, in DEFAULTS as on the command line): the reference's 0.005, or Keras' default for the two
    assert train.DEFAULTS["learning_rate"] is None and train.REFERENCE_LR == 0.005
    with pytest.raises(ValueError, match="optimizer must be one of"):
        train.run(dict(train.DEFAULTS, optimizer="nadam"))


# ---- the end-to-end fp32 bar is attainable -------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_oracle_within_a_tenth_of_the_parity_bar(kind):
    """OmniOracle in float32 against float64 over four steps (B = 128, H = 100, tests.parity.dataset(), Keras'
    default hyper-parameters): every parameter within FP32_ABS / 10, so tests.parity.assert_fp32 can hold"""
    from oracle.model_oracle import OmniOracle
    from tests.parity import FP32_ABS, dataset, dense
    data = dataset()
    N, B, H = data.num_cols, 128, 100
    rng = np.random.RandomState(77)
    order = rng.permutation(data.train.n_rows)
    base = OmniOracle([N, H, N], activation="sigmoid", dtype=np.float32).init(11)   # (float32 start: exact in both)
    w0, b0 = [w.copy() for w in base.W], [b.copy() for b in base.b]
    out = {}
    for dt in (np.float64, np.float32):
        ora = OmniOracle([N, H, N], activation="sigmoid", dtype=dt).set_params(w0, b0)
        opt = R.oracle_opt2(kind)
        for s in range(4):
            rows = order[s * B:(s + 1) * B]
            m_in, m_out, x, t, m_miss = dense(data.train, rows, N, -1.0)
            _, _, gW, gb = ora.loss_and_grads(x.astype(dt), m_out.astype(dt), t.astype(dt))
            grads = [g for pair in zip(gW, gb) for g in pair]
            ora.set_flat(opt.step(ora.params(), grads))
        assert all(p.dtype == dt for p in ora.params())
        if kind == "adamax" and dt is np.float64:      # both branches of the max among the compared elements
            lo, hi = opt.branch_fractions()
            print("adamax max branches: decayed u %.3f, |g| %.3f" % (lo, hi))
            assert lo >= 0.1 and hi >= 0.1, (lo, hi)
        out[dt] = [np.asarray(p, np.float64) for p in ora.params()]
    worst = max(float(np.abs(a - b).max()) for a, b in zip(out[np.float64], out[np.float32]))
    print("%s: float32 oracle against float64, worst parameter error %.3g" % (kind, worst))
    assert math.isfinite(worst) and worst <= FP32_ABS / 10, worst
