"""fp64 reference for the training losses other than MSE (compile(loss=...): mean_absolute_error, huber,
logcosh) and the loops that drive the GPU model and the reference over the same batches.

With e = m * y - t over all B * N elements (rho(0) = 0, so only the live target entries count):

    loss = sum rho(e) / (B N) + l2 penalty          dL/dy_full = rho'(e) * m / (B N)

    mae      rho = |e|                                       rho' = sign(e), 0 at e = 0
    huber    rho = e^2 / 2 (|e| <= d), d (|e| - d / 2)       rho' = clamp(e, -d, d)
    logcosh  rho = |e| + log1p(exp(-2 |e|)) - ln 2           rho' = tanh e

LossOracle is checked against torch.autograd in tests/test_losses.py, so it does not certify itself.
"""
from __future__ import annotations

import numpy as np

import parity
from oracle.model_oracle import OmniOracle, act_fwd, act_grad_from_out

LOSSES = [("mae", None), ("huber", 2.5), ("logcosh", None)]
LOSS_IDS = ["mae", "huber2.5", "logcosh"]


def rho(loss, e, delta=1.0):
    e = np.asarray(e, np.float64)
    a = np.abs(e)
    if loss == "mse":
        return e * e
    if loss == "mae":
        return a
    if loss == "huber":
        return np.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))
    if loss == "logcosh":
        return a + np.log1p(np.exp(-2.0 * a)) - np.log(2.0)
    raise ValueError(loss)


def drho(loss, e, delta=1.0):
    e = np.asarray(e, np.float64)
    if loss == "mse":
        return 2.0 * e
    if loss == "mae":
        return np.sign(e)
    if loss == "huber":
        return np.clip(e, -delta, delta)
    if loss == "logcosh":
        return np.tanh(e)
    raise ValueError(loss)


class LossOracle(OmniOracle):
    """OmniOracle with the loss of the table above in place of Keras' mean_squared_error"""

    def __init__(self, dims, loss, delta=1.0, shift=0.0, **kw):
        """shift (sensitivity runs only): rho' is evaluated at e + shift * (|h| |W_out| + |b_out|) |m| -- every
        residual moved by `shift` units of the magnitude that an operand rounding of unit roundoff 1 would move
        it by (OmniOracle.grad_magnitudes' ymag); shift = +-u shows how far the weights move when the residuals
        are only known to 16-bit operand accuracy (for mae: which signs are undetermined)"""
        super().__init__(dims, **kw)
        self.loss, self.delta, self.shift = loss, float(delta if delta is not None else 1.0), float(shift)

    def residuals(self, x_in, out_mask, targets, drop_masks=None):
        """e at the live entries (out_mask != 0 or target != 0) of the batch"""
        y, _ = self.forward(x_in, out_mask, drop_masks)
        T = np.asarray(targets, self.dtype)
        live = (np.asarray(out_mask) != 0) | (T != 0)
        return (y - T)[live]

    def loss_and_grads(self, x_in, out_mask, targets, drop_masks=None):
        dt = self.dtype
        y, (hs, zs, _) = self.forward(x_in, out_mask, drop_masks)
        T = np.asarray(targets, dt)
        Bn, N = T.shape
        e = y - T
        loss = np.sum(rho(self.loss, e, self.delta)) / dt(Bn * N)
        if self.l2 is not None:
            loss = loss + sum(self.l2 * np.sum(w * w) for w in self.W)
        L = len(self.W) - 1
        eg = e
        if self.shift:
            eg = e + self.shift * (np.abs(hs[L]) @ np.abs(self.W[L]) + np.abs(self.b[L])) * np.abs(out_mask)
        g = drho(self.loss, eg, self.delta) * np.asarray(out_mask, dt) / dt(Bn * N)      # dL/dy_full
        gW, gb = [None] * (L + 1), [None] * (L + 1)
        gW[L] = hs[L].T @ g
        gb[L] = g.sum(0)
        d = g @ self.W[L].T
        for i in range(L - 1, -1, -1):
            if drop_masks is not None and drop_masks[i] is not None:
                d = d * (np.asarray(drop_masks[i], dt) / dt(1.0 - self.dropout))
                a_pre = act_fwd(self.activation, zs[i])
            else:
                a_pre = hs[i + 1]
            d = d * act_grad_from_out(self.activation, a_pre, zs[i])
            gW[i] = hs[i].T @ d
            gb[i] = d.sum(0)
            if i > 0:
                d = d @ self.W[i].T
        if self.l2 is not None:
            gW = [gw + 2.0 * self.l2 * w for gw, w in zip(gW, self.W)]
        return loss, y, gW, gb


def compile_loss(model, opt, loss, delta, **kw):
    model.compile(opt, loss, loss_params={"delta": delta} if loss == "huber" else None, **kw)


def _oracle_for(loss, delta, dims, act, dropout, w0, shift=0.0):
    cls_kw = dict(activation=act, dropout=dropout, dtype=np.float64)
    if loss == "mse":
        return OmniOracle(dims, **cls_kw).set_params(w0[0::2], w0[1::2])
    return LossOracle(dims, loss, delta, shift=shift, **cls_kw).set_params(w0[0::2], w0[1::2])


def _stats_of(res, ora, xin, m_out, t, dm):
    """the conditions the tests assert on the reference: min |e| and the Huber branch shares per step"""
    if isinstance(ora, LossOracle):
        a = np.abs(ora.residuals(xin, m_out, t, dm))
        res.min_abs_e.append(float(a.min()))
        res.frac_quadratic.append(float(np.mean(a <= ora.delta)))


def run_generator(loss, delta, compute_dtype, opt_name, H, steps=3, B=128, dropout=0.2, lr=None, data=None,
                  eval_rmse=True, layers=1, act="sigmoid", model_hook=None, sensitivity=False):
    """parity.run_parity's loop (generator path: fit_generator one step at a time, the device dropout masks read
    back, the fp64 reference replaying the same rows, compute_full_RMSE on the test split) with the loss compiled
    in; returns a parity.Result with min_abs_e / frac_quadratic per step and the engine's decoder launch counts"""
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = data if data is not None else parity.dataset()
    N = data.num_cols
    np.random.seed(77)
    rd = data_reader(N, data.train.n_rows, dataset=data, eval_mode="fixed_split")
    om = omni_model(layers, H, N, B, dense_activation=act, use_causal_info=False, compute_dtype=compute_dtype,
                    seed=11, dropout_probability=dropout)
    if model_hook is not None:
        model_hook(om)
    m = om.model
    compile_loss(m, parity.our_opt(opt_name, lr), loss, delta, metrics=["mae", "accurate_RMSE"])
    w0 = m.get_weights()
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True)
    masks, gpu_losses = [], []
    for _ in range(steps):
        hist = m.fit_generator(gen, 1, epochs=1, verbose=0)
        gpu_losses.append(hist.history["loss"][0])
        if dropout:
            masks.append([mk[:B, :H].cpu().numpy().astype(np.float64) for mk in om.engine.mask])
    w_gpu = m.get_weights()
    launches = dict(om.engine.gather_launches)
    ora = _oracle_for(loss, delta, [N] + [H] * layers + [N], act, dropout, w0)
    opt = parity.oracle_opt(opt_name, lr)
    res = parity.Result(min_abs_e=[], frac_quadratic=[])
    losses = []
    for bi in range(steps):
        dm = masks[bi] if dropout else None
        _, m_out, x, t, _ = parity.dense(data.train, gen.rows_host[bi], N, -1.0)
        _stats_of(res, ora, x, m_out, t, dm)
        lo, _, gW, gb = ora.loss_and_grads(x, m_out, t, drop_masks=dm)
        losses.append(lo)
        ora.set_flat(opt.step(ora.params(), [g for pair in zip(gW, gb) for g in pair]))
    # the reference's own sensitivity to residuals known only to operand accuracy u (16-bit modes): the same
    # replay with every residual shifted by +u / -u of its rounding magnitude; per weight the larger movement
    res.sensitivity = None
    u = parity.UNIT_ROUNDOFF[compute_dtype]
    if sensitivity and loss != "mse":
        moved = None
        for sgn in (1.0, -1.0):
            o2 = _oracle_for(loss, delta, [N] + [H] * layers + [N], act, dropout, w0, shift=sgn * u)
            opt2 = parity.oracle_opt(opt_name, lr)
            for bi in range(steps):
                _, m_out, x, t, _ = parity.dense(data.train, gen.rows_host[bi], N, -1.0)
                _, _, gW, gb = o2.loss_and_grads(x, m_out, t, drop_masks=masks[bi] if dropout else None)
                o2.set_flat(opt2.step(o2.params(), [g for pair in zip(gW, gb) for g in pair]))
            d = np.concatenate([np.abs(a - b).ravel() for a, b in zip(o2.params(), ora.params())])
            moved = d if moved is None else np.maximum(moved, d)
        res.sensitivity = moved
    rmse_g = rmse_o = None
    if eval_rmse:
        np.random.seed(99)
        tgen = rd.data_gen(B, None, "test", True, None, -1, return_target_count=True)
        nb = min(2, rd.test_set_size // B)
        sse, cnt = m.evaluate_sse(tgen, nb)
        rmse_g = float(np.sqrt(sse / cnt))
        sse_o, cnt_o = 0.0, 0
        for bi in range(nb):
            rows = tgen.rows_host[bi]
            _, _, x, _, _ = parity.dense(data.test_in, rows, N, -1.0)
            _, mo, _, t, _ = parity.dense(data.test_tgt, rows, N, -1.0)
            y, _ = ora.forward(x, mo)
            sse_o += float(((y - t) ** 2).sum())
            cnt_o += int(data.test_tgt.row_lengths()[rows].sum())
        assert cnt == cnt_o
        rmse_o = float(np.sqrt(sse_o / cnt_o))
    res.__dict__.update(loss_g=float(np.mean(gpu_losses)), loss_o=float(np.mean(losses)), step_losses_g=gpu_losses,
                        step_losses_o=losses, rmse_g=rmse_g, rmse_o=rmse_o, w=w_gpu, ora=ora, env=None, om=om, gen=gen,
                        w0=w0, masks=masks, lr=opt.lr, launches=launches)
    return res


def run_dense(loss, delta, compute_dtype, opt_name, layers, H, steps=3, B=128, dropout=0.2, causal=False, act="tanh",
              data=None):
    """train_on_batch on the dense data_gen arrays (the layer-wise GEMM path with the masked-loss epilogue's dense
    target mode): the same rows through the fp64 reference.  causal: k = 2 input blocks [x, missing-data mask]."""
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = data if data is not None else parity.dataset()
    N = data.num_cols
    om = omni_model(layers, H, N, B, dense_activation=act, use_causal_info=causal, compute_dtype=compute_dtype,
                    seed=11, dropout_probability=dropout)
    m = om.model
    compile_loss(m, parity.our_opt(opt_name), loss, delta)
    w0 = m.get_weights()
    k = 1 + int(causal)
    ora = _oracle_for(loss, delta, [k * N] + [H] * layers + [N], act, dropout, w0)
    opt = parity.oracle_opt(opt_name)
    order = np.random.RandomState(3).permutation(data.train.n_rows)
    res = parity.Result(min_abs_e=[], frac_quadratic=[])
    gl, ol = [], []
    for s in range(steps):
        rows = order[s * B:(s + 1) * B]
        _, m_out, x, t, m_miss = parity.dense(data.train, rows, N, -1.0)
        ins = [x, m_miss, m_out] if causal else [x, m_out]
        gl.append(m.train_on_batch([np.asarray(a, np.float32) for a in ins], np.asarray(t, np.float32)))
        dm = [mk[:B, :H].cpu().numpy().astype(np.float64) for mk in om.engine.mask] if dropout else None
        xin = np.concatenate([x, m_miss], 1) if causal else x
        _stats_of(res, ora, xin, m_out, t, dm)
        lo, _, gW, gb = ora.loss_and_grads(xin, m_out, t, drop_masks=dm)
        ol.append(lo)
        ora.set_flat(opt.step(ora.params(), [g for pair in zip(gW, gb) for g in pair]))
    # the masked test loss of one more batch through test_on_batch (the loss's own value, no update)
    rows = order[steps * B:(steps + 1) * B]
    _, m_out, x, t, m_miss = parity.dense(data.train, rows, N, -1.0)
    ins = [x, m_miss, m_out] if causal else [x, m_out]
    gl.append(m.test_on_batch([np.asarray(a, np.float32) for a in ins], np.asarray(t, np.float32)))
    ol.append(ora.loss_and_grads(np.concatenate([x, m_miss], 1) if causal else x, m_out, t)[0])
    res.__dict__.update(step_losses_g=gl, step_losses_o=ol, rmse_g=None, rmse_o=None, w=m.get_weights(), ora=ora,
                        om=om, lr=opt.lr)
    return res
