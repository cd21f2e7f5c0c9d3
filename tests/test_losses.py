"""CPU: the training losses other than MSE (losses.py, Model.compile(loss=...)): name / parameter validation,
the checkpoint round trip of the objective, the multi-GPU layouts' refusal, the C prototype and constants, and
the fp64 reference of the GPU tests (tests/loss_ref.py) against torch.autograd."""
import os
import subprocess

import numpy as np
import pytest
import torch

from omnidirectional_collaborative_filtering_amd import _lib, losses

import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def host_engine(monkeypatch):
    """engines on host tensors (no GPU here): nothing in these tests launches a kernel"""
    from omnidirectional_collaborative_filtering_amd import engine as E
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(E, "cur_stream", lambda: None)


def _model(**kw):
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    return omni_model(1, 24, 40, 16, dense_activation="sigmoid", use_causal_info=False, compute_dtype="float32",
                      seed=3, device=torch.device("cpu"), **kw)


def test_loss_names_aliases_and_codes():
    for name, cls, code in (("mean_squared_error", losses.MeanSquaredError, 0), ("mse", losses.MeanSquaredError, 0),
                            ("mean_absolute_error", losses.MeanAbsoluteError, 1), ("mae", losses.MeanAbsoluteError, 1),
                            ("MAE", losses.MeanAbsoluteError, 1), ("huber", losses.Huber, 2),
                            ("logcosh", losses.LogCosh, 3)):
        lo = losses.get(name)
        assert type(lo) is cls and lo.code == code
    assert (_lib.LOSS_MSE, _lib.LOSS_MAE, _lib.LOSS_HUBER, _lib.LOSS_LOGCOSH) == (0, 1, 2, 3)
    assert losses.get("huber").param == 1.0                      # the default delta
    assert losses.get("huber", {"delta": 2.5}).param == 2.5
    assert losses.get("huber", {"delta": 1e30}).param == 1e30
    h = losses.Huber(0.75)
    assert losses.get(h) is h
    # the gradient scale's numerator: MSE's kernels carry e * m (the 2 is folded into gscale), the others rho'(e) * m
    assert losses.get("mse").grad_num == 2.0
    assert all(losses.get(n).grad_num == 1.0 for n in ("mae", "huber", "logcosh"))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), "x", None])
def test_bad_huber_delta_is_a_value_error(bad):
    with pytest.raises(ValueError):
        losses.get("huber", {"delta": bad})
    with pytest.raises(ValueError):
        _model().model.compile("adagrad", "huber", loss_params={"delta": bad})


def test_compile_validation():
    m = _model().model
    for name in ("mean_absolute_error", "mae", "huber", "logcosh", "mean_squared_error", "mse"):
        m.compile("adagrad", name)
        assert m.loss == losses.get(name) and m.engine.loss == m.loss
    m.compile("adagrad", "huber", loss_params={"delta": 2.5})
    assert m.engine.loss.code == _lib.LOSS_HUBER and m.engine.loss.param == 2.5
    m.compile("adagrad", losses.Huber(0.5))
    assert m.engine.loss.param == 0.5
    for bad in ("no_such_loss", "hubber", "", 7):
        with pytest.raises(ValueError):
            m.compile("adagrad", bad)
    with pytest.raises(ValueError):                 # a parameter the loss does not take
        m.compile("adagrad", "mae", loss_params={"delta": 1.0})
    with pytest.raises(ValueError):
        m.compile("adagrad", "huber", loss_params={"delta": 1.0, "beta": 2.0})
    with pytest.raises(NotImplementedError):        # a Keras loss that touches unobserved entries: not built
        m.compile("adagrad", "categorical_crossentropy")
    assert m.engine.loss.param == 0.5               # a refused compile changes nothing


def test_gradient_scale_follows_the_loss():
    om = _model()
    e = om.engine
    om.model.compile("adagrad", "mse")
    assert e._gscale() == 2.0 / (16 * 40)
    om.model.compile("adagrad", "logcosh")
    assert e._gscale() == 1.0 / (16 * 40)


def test_checkpoint_round_trip_keeps_the_objective(tmp_path):
    from safetensors.numpy import load_file, save_file
    a = _model().model
    a.compile("adagrad", "huber", loss_params={"delta": 2.5})
    p = str(tmp_path / "ck.safetensors")
    a.save(p)
    b = _model().model
    b.compile("adagrad", "mean_squared_error")
    b.load(p)
    assert b.loss == losses.Huber(2.5) and b.engine.loss == losses.Huber(2.5)
    assert b.engine._gscale() == 1.0 / (16 * 40)
    for x, y in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(x, y)
    c = _model().model
    c.compile("adagrad", "logcosh")
    c.save(p)
    b.load(p)
    assert b.loss == losses.LogCosh()
    # weights only: the compiled objective stays
    b.compile("adagrad", "mae")
    b.load(p, with_optimizer=False)
    assert b.loss == losses.MeanAbsoluteError()
    # a file from before the losses existed (no loss/ entries) means the squared loss
    t = {k: v for k, v in load_file(p).items() if not k.startswith("loss/")}
    save_file(t, p)
    b.load(p)
    assert b.loss == losses.MeanSquaredError() and b.engine._gscale() == 2.0 / (16 * 40)


def test_multi_gpu_layouts_refuse_other_losses():
    """the feature-parallel rank step and DataParallel reduce their statistics without the sum of rho: they raise
    rather than train MSE under another loss's name"""
    om = _model()
    om.model.compile("adagrad", "huber")
    with pytest.raises(NotImplementedError, match="huber"):
        om.model.enable_data_parallel(0, 2)
    om = _model()
    om.engine.comm = lambda t: None                  # a column-sharded engine
    with pytest.raises(NotImplementedError, match="logcosh"):
        om.model.compile("adagrad", "logcosh")
    om.model.compile("adagrad", "mean_squared_error")
    om = _model()
    om.engine.dp_world = 2                           # an engine under parallel.DataParallel
    with pytest.raises(NotImplementedError, match="mean_absolute_error"):
        om.model.compile("adagrad", "mae")
    # the C ABI: ocf_rank_step with a loss other than MSE is an argument error
    a = _lib.OcfRankStepArgs()
    a.dec.loss = _lib.LOSS_HUBER
    with pytest.raises(_lib.OcfError, match="OCF_LOSS_MSE"):
        _lib.call("ocf_rank_step", a, 1, None)


def test_unknown_loss_codes_are_argument_errors():
    g = _lib.OcfGatherArgs()
    for f in ("rows", "rp", "col", "lboff", "ch_row", "ch_j0", "ch_j1", "W", "part", "flag", "val", "h", "bias",
              "chunk_stats"):
        setattr(g, f, 8)
    g.H, g.ldw, g.n_chunks = 128, 128, 1
    g.loss = 9
    with pytest.raises(_lib.OcfError, match="unknown loss code 9"):
        _lib.call("ocf_gather_decoder", g, None)
    g.loss, g.loss_param = _lib.LOSS_HUBER, 0.0
    with pytest.raises(_lib.OcfError, match="delta"):
        _lib.call("ocf_gather_decoder", g, None)
    with pytest.raises(_lib.OcfError, match="unknown loss code 4"):
        _lib.call("ocf_masked_loss", 4, 0.0, 8, 8, None, 4, 1, 4, None, 0, 8, None)
    with pytest.raises(_lib.OcfError, match="delta"):
        _lib.call("ocf_masked_loss", _lib.LOSS_HUBER, -1.0, 8, 8, None, 4, 1, 4, None, 0, 8, None)
    m = _lib.OcfMlpStepArgs()
    m.loss = -1
    with pytest.raises(_lib.OcfError):
        _lib.call("ocf_mlp_step", m, None)


def test_loss_abi_is_plain_c(tmp_path):
    """the new prototype, constants and struct fields compile from C (gcc -std=c99, no C++ / HIP headers) and link"""
    src = tmp_path / "loss.c"
    src.write_text(r'''
#include "ocf.h"
#if OCF_LOSS_MSE != 0 || OCF_LOSS_MAE != 1 || OCF_LOSS_HUBER != 2 || OCF_LOSS_LOGCOSH != 3
#error "loss codes"
#endif
int drive(OcfCtx* ctx, const float* pred, const float* t, const float* mo, float* grad, float* stats, float** gW,
          float** gb, float* sums, void* stream) {
  OcfGatherArgs g = {0};
  OcfGemmArgs e = {0};
  OcfMlpStepArgs s = {0};
  OcfRowsReduceArgs r = {0};
  if (g.loss != OCF_LOSS_MSE || e.loss != OCF_LOSS_MSE || s.loss != OCF_LOSS_MSE || r.stats4) return 2;
  g.loss = OCF_LOSS_HUBER; g.loss_param = 2.5f;
  e.loss = OCF_LOSS_LOGCOSH; e.loss_param = 0.f;
  s.loss = OCF_LOSS_MAE; s.loss_param = 0.f;
  r.stats4 = 1;
  return ocf_masked_loss(OCF_LOSS_HUBER, 2.5f, pred, t, mo, 333, 128, 333, grad, 333, stats, stream)
      || ocf_backward(ctx, grad, 333, 128, 1.f / (128 * 333), gW, gb, stream)
      || ocf_loss_sum(stats, 128, sums, stream);
}
int main(void) { return 0; }
''')
    exe = tmp_path / "loss"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), _lib.LIB_PATH, "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _torch_rho(loss, e, d):
    a = e.abs()
    if loss == "mae":
        return a
    if loss == "huber":
        return torch.where(a <= d, 0.5 * e * e, d * (a - 0.5 * d))
    return torch.log(torch.cosh(e))                  # (the residuals here are far from cosh's overflow)


@pytest.mark.parametrize("loss,delta", loss_ref.LOSSES, ids=loss_ref.LOSS_IDS)
@pytest.mark.parametrize("layers,dropout", [(1, None), (2, 0.25)])
def test_reference_against_autograd(loss, delta, layers, dropout):
    """tests/loss_ref.LossOracle (the GPU tests' fp64 reference) against torch.autograd on a 16 x 24 batch: loss and
    every gradient, with the l2 penalty and (two layers) dropout masks"""
    rng = np.random.RandomState(4)
    B, N, H = 16, 24, 10
    dims = [N] + [H] * layers + [N]
    x = (rng.rand(B, N) < 0.4) * rng.randint(1, 6, (B, N)).astype(np.float64)
    m_out = -1.0 * ((rng.rand(B, N) < 0.5) & (x == 0))
    t = np.where(m_out != 0, rng.randint(1, 6, (B, N)), 0.0)
    dm = [(rng.rand(B, H) < 0.75).astype(np.float64) for _ in range(layers)] if dropout else None
    ora = loss_ref.LossOracle(dims, loss, delta, activation="tanh", dropout=dropout, l2=1e-3).init(2)
    # biases off zero and an output layer large enough for residuals on both Huber branches
    ora.b = [rng.uniform(-0.5, 0.5, b.shape) for b in ora.b]
    ora.W[-1] = ora.W[-1] * 8.0
    lo, y, gW, gb = ora.loss_and_grads(x, m_out, t, drop_masks=dm)
    e = (y - t)[m_out != 0]
    if loss == "huber":
        assert 0.1 <= np.mean(np.abs(e) <= delta) <= 0.9
    assert np.abs(e).min() > 1e-6                    # no residual on a kink
    W = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ora.W]
    b = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in ora.b]
    h = torch.tensor(x)
    for i in range(layers):
        h = torch.tanh(h @ W[i] + b[i])
        if dm is not None:
            h = h * torch.tensor(dm[i]) / (1.0 - dropout)
    yt = torch.tensor(m_out) * (h @ W[-1] + b[-1])
    lt = _torch_rho(loss, yt - torch.tensor(t), delta if delta is not None else 1.0).sum() / (B * N)
    lt = lt + sum(1e-3 * (w * w).sum() for w in W)
    lt.backward()
    assert abs(lo - float(lt.detach())) <= 1e-12 * abs(float(lt.detach()))
    for g, p in zip(gW + gb, W + b):
        np.testing.assert_allclose(g, p.grad.numpy(), rtol=1e-10, atol=1e-14)


def test_reference_functions():
    e = np.array([0.0, 1e-30, -1e-4, 2.5, -2.5, np.nextafter(2.5, 3), 3.0, -50.0, 1e4])
    assert np.array_equal(loss_ref.drho("mae", e), np.sign(e)) and loss_ref.drho("mae", 0.0) == 0.0
    np.testing.assert_allclose(loss_ref.rho("huber", e, 2.5)[3:6], [3.125, 3.125, 3.125], rtol=1e-15)
    np.testing.assert_allclose(loss_ref.rho("logcosh", e[:7]), np.log(np.cosh(e[:7])), rtol=1e-9, atol=1e-16)
    assert np.isfinite(loss_ref.rho("logcosh", e)).all()
    np.testing.assert_allclose(loss_ref.rho("logcosh", 1e4), 1e4 - np.log(2.0), rtol=1e-15)
    # huber with a huge delta is half the squared loss
    np.testing.assert_array_equal(loss_ref.rho("huber", e, 1e30), 0.5 * e * e)
    np.testing.assert_array_equal(2.0 * loss_ref.drho("huber", e, 1e30), loss_ref.drho("mse", e))


def test_train_driver_takes_the_loss_options():
    from omnidirectional_collaborative_filtering_amd import train
    assert train.DEFAULTS["model_loss"] == "mean_squared_error" and train.DEFAULTS["huber_delta"] == 1.0
    seen = {}
    orig = train.run
    train.run = lambda cfg: seen.update(cfg)
    try:
        train.main(["--loss", "huber", "--huber-delta", "2.5"])
        assert seen["model_loss"] == "huber" and seen["huber_delta"] == 2.5
        train.main([])
        assert seen["model_loss"] == "mean_squared_error" and seen["huber_delta"] == 1.0
    finally:
        train.run = orig
