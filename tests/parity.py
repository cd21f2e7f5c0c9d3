"""Shared training-parity harness for the -m gpu tests: run the GPU engine through the reference's
API (data_reader.data_gen -> omni_model -> compile -> fit_generator, train.py:131-158), replay the
same batches through the NumPy fp64 oracle (oracle/model_oracle.py), and compare.

Tolerances (stated here, used by every parity test):
  * exact-fp32 mode (v_mfma_f32_32x32x2_f32): per-step loss within 1e-5 relative, masked test RMSE
    within 1e-5, every weight and bias within FP32_ABS = 1e-5 (max-abs, no quantile);
  * f16 / bf16 MFMA operands: loss and RMSE within 2e-3 / 1e-2 relative; every weight within a
    per-element running-error envelope (adagrad_envelope): an Adagrad update is lr * g / sqrt(sum g^2),
    which amplifies the operand rounding of g by G_i / |g_i| (G = the gradient's magnitude sum,
    OmniOracle.grad_magnitudes).  Elements with a well-conditioned gradient must match tightly;
    only elements whose gradient is within rounding distance of zero may differ by up to 2 lr per
    step (the update's sign there is not determined by 16-bit operands); and the bulk must sit far
    inside: 99th / 99.9th percentile errors within 0.02 / 0.15 of lr * steps.
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle.batch_oracle import scatter_rows_numpy
from oracle.model_oracle import AdagradOracle, AdamOracle, OmniOracle, RMSpropOracle, SGDOracle  # noqa: F401

FP32_ABS = 1e-5
UNIT_ROUNDOFF = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8, "float32": 2.0 ** -24}
# roundings along the longest gradient chain of the 16-bit path: W shadow, h, delta, dh operands
CHAIN_ROUNDINGS = 4


def dataset(rows=700, cols=333, nnz=14000, seed=5):
    from omnidirectional_collaborative_filtering_amd.dataset import split_ratings, synthetic_ratings
    r, c, v = synthetic_ratings(rows, cols, nnz, half_stars=True, seed=seed)
    return split_ratings(r, c, v, rows, cols, rng=np.random.RandomState(seed))


def dense(csr, rows, N, aux):
    return scatter_rows_numpy(csr.row_ptr, csr.col, csr.val, rows, N, aux=aux)


def oracle_opt(name, lr=None):
    return {"adagrad": lambda: AdagradOracle(lr=lr or 0.005, epsilon=1e-8),
            "rmsprop": lambda: RMSpropOracle(lr=lr or 0.001),
            "adam": lambda: AdamOracle(lr=lr or 0.001),
            "sgd": lambda: SGDOracle(lr=lr or 0.05)}[name]()


def our_opt(name, lr=None):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    return {"adagrad": lambda: O.Adagrad(lr=lr or 0.005, epsilon=1e-8), "rmsprop": lambda: O.RMSprop(lr=lr or 0.001),
            "adam": lambda: O.Adam(lr=lr or 0.001), "sgd": lambda: O.SGD(lr=lr or 0.05)}[name]()


class Result:
    """loss_g / loss_o: mean per-step loss (GPU history / oracle); step_losses_*: per step;
    rmse_g / rmse_o: compute_full_RMSE on the test split; w: GPU weights (Keras list); ora: the oracle
    after the same steps; env: per-parameter Adagrad tolerance envelopes (16-bit modes) or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def max_param_err(self):
        out = []
        for i, (wg, wo) in enumerate(zip(self.w[0::2], self.ora.W)):
            out.append(("W%d" % i, float(np.abs(wg - wo).max())))
        for i, (bg, bo) in enumerate(zip(self.w[1::2], self.ora.b)):
            out.append(("b%d" % i, float(np.abs(bg - bo).max())))
        return out


def sparse_batch(csr, rows, N, aux=-1.0):
    """the batch (inputs X, output mask, targets) of a pass-through train batch with data_sparsity
    [1, 1] as scipy CSR [B, N] (data_reader.py:158-169 writes X = T = rating, M_out = aux at every
    rating of the row); duplicate-free data only (last-write-wins needs the dense scatter)"""
    import scipy.sparse as sp
    assert csr.dup is None, "sparse_batch: duplicate (row, col) entries need scatter_rows_numpy"
    lens = csr.row_lengths()[rows]
    ip = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ip[1:])
    take = np.concatenate([np.arange(csr.row_ptr[r], csr.row_ptr[r + 1]) for r in rows])
    col, val = csr.col[take], csr.val[take].astype(np.float64)
    X = sp.csr_matrix((val, col, ip), shape=(len(rows), N))
    Mo = sp.csr_matrix((np.full(len(col), aux), col, ip), shape=(len(rows), N))
    return X, Mo, X


def run_parity(compute_dtype, opt_name, layers, act, steps=4, B=128, H=100, aux_type=None, causal=False,
               gather=True, sparse_dw=None, dropout=None, data=None, n_rows=None, lr=None, eval_rmse=True,
               envelope=False, model_hook=None, sparse_oracle=False, eval_batches=None, l2=None):
    """`steps` training steps through fit_generator (one call per step, so the engine's Philox
    dropout masks engine.mask[l][:B, :H] can be read back after each and fed to the oracle as Keras'
    Dropout draw, model.py:72-73), then the oracle on the same rows (the generator exposes its epoch
    plan) and compute_full_RMSE of both models on identical test batches (train.py:225-255).
    sparse_oracle: the oracle's sparse-batch form (OmniOracle.loss_and_grads_sparse; one hidden
    layer, no aux inputs) for the ML-20M / Netflix widths; eval_batches: test batches evaluated.
    """
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = data if data is not None else dataset()
    N = data.num_cols
    np.random.seed(77)
    rd = data_reader(N, n_rows or data.train.n_rows, dataset=data, eval_mode="fixed_split")
    om = omni_model(layers, H, N, B, dense_activation=act, use_causal_info=causal, compute_dtype=compute_dtype,
                    seed=11, dropout_probability=dropout, l2_weight_regulatization=l2)
    m = om.model
    om.engine.use_sparse = gather
    if sparse_dw is not None:
        om.engine.sparse_dw = sparse_dw
    if model_hook is not None:
        model_hook(om)
    m.compile(our_opt(opt_name, lr), "mean_squared_error", metrics=["mae", "accurate_MSE", "accurate_RMSE"])
    w0 = m.get_weights()
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, aux_type, -1, pass_through_input_training=True)
    masks, gpu_losses = [], []
    for _ in range(steps):
        hist = m.fit_generator(gen, 1, epochs=1, verbose=0)
        gpu_losses.append(hist.history["loss"][0])
        if dropout:
            masks.append([mk[:B, :H].cpu().numpy().astype(np.float64) for mk in om.engine.mask])
    w_gpu = m.get_weights()
    live_rows_used = bool(om.engine._rtag_live)        # (the eval batches below reset it)
    k = 1 + int(causal)
    ora = OmniOracle([k * N] + [H] * layers + [N], activation=act, dropout=dropout, l2=l2,
                     dtype=np.float64).set_params(w0[0::2], w0[1::2])
    opt = oracle_opt(opt_name, lr)
    u = UNIT_ROUNDOFF[compute_dtype]
    env = None
    if envelope:
        if opt_name != "adagrad":
            raise ValueError("the rounding envelope is derived for Adagrad")
        env = [np.zeros_like(p) for p in ora.params()]
        rmax = [np.zeros_like(p) for p in ora.params()]
    losses = []
    for bi in range(steps):
        dm = masks[bi] if dropout else None
        if sparse_oracle:
            assert layers == 1 and not causal and aux_type is None
            X, Mo, T = sparse_batch(data.train, gen.rows_host[bi], N)
            out = ora.loss_and_grads_sparse(X, Mo, T, drop_masks=dm, u=u if envelope else None)
            loss, _, gW, gb = out[:4]
            if envelope:
                GW, Gb = out[4], out[5]
        else:
            m_in, m_out, x, t, m_miss = dense(data.train, gen.rows_host[bi], N, -1.0)
            xin = np.concatenate([x, m_miss if aux_type == "causal" else m_in], 1) if causal else x
            loss, _, gW, gb = ora.loss_and_grads(xin, m_out, t, drop_masks=dm)
            if envelope:
                GW, Gb = ora.grad_magnitudes(xin, m_out, t, drop_masks=dm, u=u)
        grads = [g for pair in zip(gW, gb) for g in pair]
        if envelope:
            for j, (g, G) in enumerate(zip(grads, [x for pair in zip(GW, Gb) for x in pair])):
                r = CHAIN_ROUNDINGS * u * G / np.maximum(np.abs(g), 1e-30)
                rmax[j] = np.maximum(rmax[j], r)
                # g/sqrt(a) with a = sum of squares of the (equally perturbed) gradients so far
                env[j] += opt.lr * np.minimum(2.0, 3.0 * rmax[j])
        losses.append(loss)
        ora.set_flat(opt.step(ora.params(), grads))
    rmse_g = rmse_o = None
    if eval_rmse:
        np.random.seed(99)
        tgen = rd.data_gen(B, None, "test", True, aux_type, -1, return_target_count=True)
        nb = rd.test_set_size // B if eval_batches is None else min(eval_batches, rd.test_set_size // B)
        sse, cnt = m.evaluate_sse(tgen, nb)
        rmse_g = float(np.sqrt(sse / cnt))
        sse_o, cnt_o = 0.0, 0
        for bi in range(nb):
            rows = tgen.rows_host[bi]
            if sparse_oracle:
                sse_o += _sparse_eval_sse(ora, data, rows, N)
                cnt_o += int(data.test_tgt.row_lengths()[rows].sum())
                continue
            mi, _, x, _, mm = dense(data.test_in, rows, N, -1.0)
            _, mo, _, t, mm2 = dense(data.test_tgt, rows, N, -1.0)
            miss = np.maximum(np.abs(mm), np.abs(mm2)) * -1.0
            xin = np.concatenate([x, miss if aux_type == "causal" else mi], 1) if causal else x
            y, _ = ora.forward(xin, mo)
            sse_o += float(((y - t) ** 2).sum())
            cnt_o += int(data.test_tgt.row_lengths()[rows].sum())
        assert cnt == cnt_o
        rmse_o = float(np.sqrt(sse_o / cnt_o))
    return Result(loss_g=float(np.mean(gpu_losses)), loss_o=float(np.mean(losses)), step_losses_g=gpu_losses,
                  step_losses_o=losses, rmse_g=rmse_g, rmse_o=rmse_o, w=w_gpu, ora=ora, env=env, om=om, gen=gen,
                  live_rows_used=live_rows_used, w0=w0,
                  reader=rd, masks=masks, lr=opt.lr)


def replay_train_draws(lens, n_rows, B, sparsity, shuffle=True):
    """The reference's own NumPy calls for one training generator, in its order (independent of the
    product's restatement in BatchGenerator.plan): np.random.permutation of the row set
    (data_reader.py:326-327), then per batch np.random.uniform for the row sparsities (:120) and one
    np.random.choice([0, 1], p=[1-s, s]) per row (:130).  Returns (rows [nb][B], keep [nb] -> bool
    per entry of the batch in CSR order)."""
    order = np.random.permutation(n_rows) if shuffle else np.arange(n_rows)
    nb = n_rows // B
    rows, keeps = [], []
    for bi in range(nb):
        r = order[bi * B:(bi + 1) * B]
        s = np.random.uniform(low=sparsity[0], high=sparsity[1], size=B)
        k = [np.random.choice([0, 1], size=int(lens[x]), p=[1 - s[j], s[j]]) for j, x in enumerate(r)]
        rows.append(r)
        keeps.append(np.concatenate(k).astype(bool) if k else np.zeros(0, bool))
    return rows, keeps


def with_duplicates(rows, cols, nnz, dup_frac=0.03, half_stars=True, seed=0):
    """synthetic ratings with the reference's own data hazards: a fraction of (row, col) pairs rated twice
    with a different value (data_reader.py:158-166 resolves them last-write-wins, per array), some
    ratings of exactly 0.0 (they still set the masks), and every row's list in random order (not
    column order) -- as a fixed split (rating-level 80/10/10, TrainValidTestSplit.py:74-103)"""
    from omnidirectional_collaborative_filtering_amd.dataset import split_ratings, synthetic_ratings
    r, c, v = synthetic_ratings(rows, cols, nnz, half_stars=half_stars, seed=seed)
    g = np.random.RandomState(seed + 1)
    d = g.choice(len(r), int(dup_frac * len(r)), replace=False)
    r = np.concatenate([r, r[d]])
    c = np.concatenate([c, c[d]])
    v = np.concatenate([v, (g.randint(1, 11, len(d)) / 2.0).astype(np.float32)])
    v[g.choice(len(v), max(1, len(v) // 500), replace=False)] = 0.0
    p = g.permutation(len(r))
    data = split_ratings(r[p], c[p], v[p], rows, cols, rng=np.random.RandomState(seed))
    assert data.train.dup is not None, "the split must keep duplicate (row, col) pairs in train"
    return data


def aux_model_input(aux_type, x, m_in, m_miss):
    """the first dense layer's input for a data_gen batch (model.py:47-56 concatenates in the order of
    data_reader.py:341-361): x alone (aux None), [x, mask_to_feed] (causal: the missing-data mask; dropout:
    the input mask; zeros: zeros) or [x, m_in, m_miss] (both, use_both_masks)"""
    if aux_type is None:
        return x
    feed = {"causal": m_miss, "dropout": m_in, "both": m_in, "zeros": np.zeros_like(m_in)}[aux_type]
    return np.concatenate([x, feed] + ([m_miss] if aux_type == "both" else []), 1)


def run_semantics_parity(rd, B, H, steps, sparsity, pass_through, aux, compute_dtype, dropout, seed, oracle_batch,
                         eval_batches=4, envelope=False, lr=0.005, epoch_lists=True, aux_type=None):
    """The DEFAULT training path (data_reader with rng='numpy' -> fit_generator, one hidden layer,
    aux None = k=1 row gathers, the per-epoch row lists and scatter outputs, row-stream dW with
    live-row skipping) on the reference's data semantics: reciprocal split with s<1, pass-through
    on or off, duplicate (row, col) ratings, unsorted lists.  With aux_type (causal / dropout / zeros /
    both) the generator feeds the aux-mask inputs and the model concatenates them (use_causal_info,
    use_both_masks for 'both': k = 2 / 3 input blocks, the dense scatter + MFMA path).
    oracle_batch(bi, rows) -> (x, m_out, t) is the oracle's dense batch, x already the concatenated
    model input (reference goldens or scatter_rows_numpy over the replayed draws).
    Per step: loss and accurate_MSE (count_nonzero(T + y) denominators) vs the oracle; after the run
    every weight, and compute_full_RMSE on the test split (train.py:243-255)."""
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    from omnidirectional_collaborative_filtering_amd.optimizers import Adagrad
    from oracle.model_oracle import batch_metrics
    N = rd.num_items
    k = 1 + int(aux_type is not None) + int(aux_type == "both")
    om = omni_model(1, H, N, B, dense_activation="sigmoid", use_causal_info=aux_type is not None,
                    use_both_masks=aux_type == "both", compute_dtype=compute_dtype, seed=11,
                    dropout_probability=dropout)
    m = om.model
    om.engine.epoch_row_lists = om.engine.epoch_scatter = epoch_lists
    m.compile(Adagrad(lr=lr, epsilon=1e-8), "mean_squared_error", metrics=["accurate_MSE"])
    w0 = m.get_weights()
    np.random.seed(seed)
    gen = rd.data_gen(B, sparsity, "train", True, aux_type, aux, pass_through_input_training=pass_through)
    assert gen.r.rng == "numpy"
    steps = min(steps, gen.num_batches)
    masks, gl, gm = [], [], []
    for _ in range(steps):
        hist = m.fit_generator(gen, 1, epochs=1, verbose=0)
        gl.append(hist.history["loss"][0])
        gm.append(hist.history["accurate_MSE"][0])
        if dropout:
            masks.append([om.engine.mask[0][:B, :H].cpu().numpy().astype(np.float64)])
    e = om.engine
    if k > 1:                              # aux-mask inputs: the dense k-block scatter + MFMA path
        assert e.k == k and not e.sparse_ok and e.gt is None
    elif epoch_lists:
        # the default path really ran: row gathers, the epoch's row lists + scatter outputs, live-row records
        assert e.gt is not None and "xval" in e.gt and "flag" in e.gt, "epoch scatter outputs not used"
        assert getattr(gen, "_rl", None) is not None
    else:                                  # per-step ocf_scatter_batch + ocf_row_lists
        assert e.gt is not None and getattr(gen, "_rl", None) is None
    if k == 1:
        assert e.tb is not None and "sp_rowptr" in e.tb
        assert e._rtag_live == (e.row_skip == "always" or getattr(gen, "_rl", None) is None or
                                not gen.gather_tables(0)["rows_dense"]), "live-row records expected (Adagrad, l2 = 0)"
    w_gpu = m.get_weights()
    ora = OmniOracle([k * N, H, N], activation="sigmoid", dropout=dropout, dtype=np.float64).set_params(w0[0::2],
                                                                                                       w0[1::2])
    opt = AdagradOracle(lr=lr, epsilon=1e-8)
    u = UNIT_ROUNDOFF[compute_dtype]
    env = [np.zeros_like(p) for p in ora.params()] if envelope else None
    rmax = [np.zeros_like(p) for p in ora.params()] if envelope else None
    losses, mets = [], []
    for bi in range(steps):
        dm = masks[bi] if dropout else None
        x, mo, t = oracle_batch(bi, gen.rows_host[bi])
        loss, y, gW, gb = ora.loss_and_grads(x, mo, t, drop_masks=dm)
        mets.append(batch_metrics(t, y, N, B, 1.0)["accurate_MSE"])
        grads = [g for pair in zip(gW, gb) for g in pair]
        if envelope:
            GW, Gb = ora.grad_magnitudes(x, mo, t, drop_masks=dm, u=u)
            for j, (g, G) in enumerate(zip(grads, [z for pair in zip(GW, Gb) for z in pair])):
                rmax[j] = np.maximum(rmax[j], CHAIN_ROUNDINGS * u * G / np.maximum(np.abs(g), 1e-30))
                env[j] += opt.lr * np.minimum(2.0, 3.0 * rmax[j])
        losses.append(loss)
        ora.set_flat(opt.step(ora.params(), grads))
    # compute_full_RMSE over test batches; the oracle replays the test permutation itself
    np.random.seed(seed + 1)
    tgen = rd.data_gen(B, None, "test", True, aux_type, aux, return_target_count=True)
    nb = min(eval_batches, rd.test_set_size // B)
    sse, cnt = m.evaluate_sse(tgen, nb)
    np.random.seed(seed + 1)
    order = np.random.permutation(rd.test_set_size)
    data = rd.data
    sse_o, cnt_o = 0.0, 0
    for bi in range(nb):
        rows = order[bi * B:(bi + 1) * B]
        assert np.array_equal(rows, tgen.rows_host[bi])
        mi, _, xe, _, mm1 = scatter_rows_numpy(data.test_in.row_ptr, data.test_in.col, data.test_in.val, rows, N,
                                               aux=aux)
        _, mo, _, te, mm2 = scatter_rows_numpy(data.test_tgt.row_ptr, data.test_tgt.col, data.test_tgt.val, rows, N,
                                               aux=aux)
        # fixed split (data_reader.py:250-266): the missing-data mask covers the input and the target ratings
        miss = np.where((mm1 != 0) | (mm2 != 0), aux, 0.0)
        y, _ = ora.forward(aux_model_input(aux_type, xe, mi, miss), mo)
        sse_o += float(((y - te) ** 2).sum())
        cnt_o += int(data.test_tgt.row_lengths()[rows].sum())          # data_reader.py:268: every list entry
    assert cnt == cnt_o, (cnt, cnt_o)
    return Result(loss_g=float(np.mean(gl)), loss_o=float(np.mean(losses)), step_losses_g=gl, step_losses_o=losses,
                  step_mse_g=gm, step_mse_o=mets, rmse_g=float(np.sqrt(sse / cnt)), rmse_o=float(np.sqrt(sse_o / cnt_o)),
                  w=w_gpu, ora=ora, env=env, om=om, gen=gen, reader=rd, masks=masks, lr=opt.lr)


def _sparse_eval_sse(ora, data, rows, N):
    """compute_full_RMSE's squared error of one test batch (train.py:243-252) from the sparse
    forward: inputs from test_in, predictions only at the test_tgt entries (elsewhere y = T = 0)"""
    import scipy.sparse as sp
    X, _, _ = sparse_batch(data.test_in, rows, N)
    h = ora.forward_hidden_sparse(X)
    Tt, _, _ = sparse_batch(data.test_tgt, rows, N)
    coo = Tt.tocoo()
    y = -1.0 * (np.einsum("ij,ji->i", h[coo.row], ora.W[1][:, coo.col]) + ora.b[1][coo.col])
    return float(((y - coo.data) ** 2).sum())


def assert_fp32(res, loss_rel=FP32_ABS, rmse_abs=FP32_ABS, w_abs=FP32_ABS):
    """the exact-fp32 bar: per-step loss, test RMSE, and the max-abs error of every parameter"""
    for lg, lo in zip(res.step_losses_g, res.step_losses_o):
        assert abs(lg - lo) <= loss_rel * abs(lo), (lg, lo)
    for mg, mo in zip(getattr(res, "step_mse_g", []), getattr(res, "step_mse_o", [])):
        assert abs(mg - mo) <= loss_rel * abs(mo), ("accurate_MSE", mg, mo)
    if res.rmse_g is not None:
        assert abs(res.rmse_g - res.rmse_o) <= rmse_abs, (res.rmse_g, res.rmse_o)
    for name, err in res.max_param_err():
        assert err <= w_abs, (name, err)


def assert_low_precision(res, tol):
    """16-bit operands: loss / RMSE within `tol` relative; every parameter inside its Adagrad
    rounding envelope (+ FP32_ABS); returns the worst |error| / envelope ratio"""
    for lg, lo in zip(res.step_losses_g, res.step_losses_o):
        assert abs(lg - lo) <= tol * abs(lo), (lg, lo)
    for mg, mo in zip(getattr(res, "step_mse_g", []), getattr(res, "step_mse_o", [])):
        assert abs(mg - mo) <= tol * abs(mo), ("accurate_MSE", mg, mo)
    if res.rmse_g is not None:
        assert abs(res.rmse_g - res.rmse_o) <= tol * res.rmse_o, (res.rmse_g, res.rmse_o)
    worst = 0.0
    got = list(res.w)
    want = res.ora.params()
    errs, envs = [], []
    for j, (g, o, e) in enumerate(zip(got, want, res.env)):
        err = np.abs(g - o)
        lim = FP32_ABS + e
        ratio = float((err / lim).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, ("param %d" % j, float(err.max()), int((err > lim).sum()))
        errs.append(err.ravel())
        envs.append(np.asarray(e).ravel())
    err, env = np.concatenate(errs), np.concatenate(envs)
    _record_envelope_stats(res, err, env)
    # the envelope bounds every element; the bulk must sit far inside it: in units of lr * steps, the 99th /
    # 99.9th percentile errors within 0.02 / 0.15 (measured: f16 <= 4.5e-4 / 5.4e-3, bf16 <= 3.0e-3 / 4.6e-2,
    # profiles/r03c_envelope_stats.jsonl; the runs are seeded and the kernels deterministic)
    unit = float(getattr(res, "lr", None) or 0.005) * max(1, len(res.step_losses_o))
    q99, q999 = np.quantile(err, [0.99, 0.999]) / unit
    assert q99 <= 0.02 and q999 <= 0.15, ("error quantiles / (lr * steps)", float(q99), float(q999))
    return worst


# How loose the 16-bit envelope is in practice (OCF_PARITY_STATS=path: one JSON line per checked run): the
# envelope is lr * min(2, 3 r) per step, so it is wide only where r -- the operand rounding relative to the
# gradient -- is large; these lines give the share of elements where it exceeds half a step and the error
# quantiles in units of lr * steps.
def _record_envelope_stats(res, err, env):
    path = os.environ.get("OCF_PARITY_STATS")
    if not path:
        return
    lr = float(getattr(res, "lr", None) or 0.005)
    steps = max(1, len(getattr(res, "step_losses_o", []) or [1]))
    unit = lr * steps
    line = {"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "elements": int(err.size),
            "loose_frac": float(np.mean(env > 0.5 * unit)),
            "err_p50": float(np.quantile(err, 0.5) / unit), "err_p99": float(np.quantile(err, 0.99) / unit),
            "err_p999": float(np.quantile(err, 0.999) / unit), "err_max": float(err.max() / unit),
            "unit": "lr * steps"}
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")
