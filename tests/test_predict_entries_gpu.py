"""GPU: per-entry predictions for generator batches (Model.predict_entries, Engine.predict_entries, the
save_test_predictions leg of train.py) on the 600 x 200 half-star split of test_topk_gpu.py, B = 100, H = 100 and
500: against Model.predict's dense output at the same positions, against evaluate_sse, the clipped RMSE, an
arbitrary queries CSR on a train generator, a two-hidden-layer model with the causal mask input (the dense
layer-0 path), the documented order, side effects on training, the refusals, and train.run's file.

Bounds.  predict and predict_entries accumulate the same H products and one bias in fp32, in different orders: each
lies within gather_ref.sum_bound(H, 1, sum |h||w| + |b|) of the exact value of its operands, and so does their
difference at the errors both have in practice (the bound is the worst case of one of them; the measured ratio is
printed).  In 16 bits the operands are the rounded ones (the shadow is the master rounded once, predict rounds the
master while staging), and h, stored in the compute dtype by two encoder forms, may differ by one rounding:
+ sum round_tol(h) |w|.
Worst observed |predict_entries - predict| / bound (MI355X, this file's own run; recorded, not used to set a bound):
fp32 0.062 (H = 100) / 0.019 (H = 500), f16 3.3e-4, bf16 4.2e-5.
"""
import numpy as np
import pytest
import torch

import epilogue_ref as R
import gather_ref as G
import parity

B, N, ROWS = 100, 200, 600
CDN = {"float32": "f32", "float16": "f16", "bfloat16": "bf16"}


def _split():
    from omnidirectional_collaborative_filtering_amd.dataset import split_ratings, synthetic_ratings
    r, c, v = synthetic_ratings(ROWS, N, 9000, half_stars=True, seed=2)
    return split_ratings(r, c, v, ROWS, N, rng=np.random.RandomState(2))


def _model(cd, H, layers=1, causal=False, act="sigmoid", steps=2, dropout=None):
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = _split()
    np.random.seed(4)
    rd = data_reader(N, ROWS, dataset=data, eval_mode="fixed_split")
    kw = {} if dropout is None else dict(dropout_probability=dropout)
    om = omni_model(layers, H, N, B, act, use_causal_info=causal, compute_dtype=cd, seed=8, **kw)
    om.model.compile(parity.our_opt("adagrad", 0.05), "mean_squared_error")
    aux = "causal" if causal else None
    if steps:
        om.model.fit_generator(rd.data_gen(B, [1.0, 1.0], "train", True, aux, -1, pass_through_input_training=True),
                               steps, verbose=0)
    return data, rd, om, aux


def _entry_bound(e, cd, H, bidx, cols):
    """per entry: the bound of the module docstring, from the engine's hidden rows of the batch just run and the
    decoder operands as both routes read them"""
    w = e.get_weights()
    Wr = R.round_to(w[-2], CDN[cd]).astype(np.float64)                 # [H, N]
    h = e.h[-1][:B, :H].float().cpu().numpy().astype(np.float64)
    wa = np.abs(Wr[:, cols].T)
    mag = (np.abs(h[bidx]) * wa).sum(1) + np.abs(w[-1].astype(np.float64)[cols])
    return G.sum_bound(H, 1, mag) + (R.round_tol(CDN[cd], h[bidx]) * wa).sum(1)


def _against_predict(m, e, cd, H, make_gen, steps, queries=None, aux=-1.0):
    """batch by batch: Model.predict on the generator's dense batch (the output mask = aux at the asked positions)
    against predict_entries on a fresh generator of the same batches; returns the pieces per batch"""
    gd, gp = make_gen(), make_gen()
    out, worst = [], 0.0
    for s in range(steps):
        inputs, _ = next(gd)[:2]
        rows = gd.rows_host[s]
        if queries is not None:
            mask = np.zeros((B, N), np.float32)
            for b, r in enumerate(rows):
                mask[b, queries.col[queries.row_ptr[r]:queries.row_ptr[r + 1]]] = aux
            inputs = list(inputs[:-1]) + [torch.as_tensor(mask, device="cuda")]
        dense = m.predict(inputs).cpu().numpy().astype(np.float64)
        p = m.predict_entries(gp, 1, queries=queries)
        assert np.array_equal(gp.rows_host[s], rows)
        pr, pc, py = p["rows"].cpu().numpy(), p["cols"].cpu().numpy(), p["predictions"].cpu().numpy()
        where = {int(r): b for b, r in enumerate(rows)}
        bidx = np.array([where[int(r)] for r in pr], np.int64)
        tol = _entry_bound(e, cd, H, bidx, pc)
        ratio, i = G.worst(py, dense[bidx, pc], tol)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (cd, H, s, ratio, i)
        out.append((p, rows, tol))
    print("PREDICT_ENTRIES vs predict: %s H=%d worst error / bound %.4g" % (cd, H, worst))
    return out


def _expected_order(csr, batches):
    lens = csr.row_lengths()
    rows = np.concatenate([np.repeat(r, lens[r]) for r in batches])
    cols = np.concatenate([csr.col[csr.row_ptr[x]:csr.row_ptr[x + 1]] for r in batches for x in r])
    vals = np.concatenate([csr.val[csr.row_ptr[x]:csr.row_ptr[x + 1]] for r in batches for x in r])
    return rows, cols, vals


@pytest.mark.gpu
@pytest.mark.parametrize("H", [100, 500])
@pytest.mark.parametrize("cd", ["float32", "float16", "bfloat16"])
def test_test_split_against_predict_and_evaluate_sse(gpu, cd, H):
    data, rd, om, aux = _model(cd, H)
    m, e = om.model, om.engine
    steps = 3
    test = lambda: rd.data_gen(B, None, "test", False, aux, -1, return_target_count=True)
    got = _against_predict(m, e, cd, H, test, steps)
    assert e.gt is not None                                           # the generator (row-gather) path ran
    # one call over all batches: the documented order, the same values, and evaluate_sse's sums
    g = test()
    p = m.predict_entries(g, steps)
    rows, cols, vals = _expected_order(data.test_tgt, g.rows_host[:steps])
    assert data.test_tgt.dup is None or not (data.test_tgt.dup >= 0).any()
    assert p["rows"].dtype == torch.int64 and p["cols"].dtype == torch.int32 and p["predictions"].is_cuda
    assert np.array_equal(p["rows"].cpu().numpy(), rows) and np.array_equal(p["cols"].cpu().numpy(), cols)
    assert np.array_equal(p["targets"].cpu().numpy(), vals)
    py = p["predictions"].cpu().numpy()
    assert np.array_equal(py, np.concatenate([q["predictions"].cpu().numpy() for q, _, _ in got]))
    sse, count = m.evaluate_sse(test(), steps)
    assert p["count"] == count == len(py)
    err = py.astype(np.float64) - vals
    if cd == "float32":
        assert abs(p["sse"] - sse) <= 1e-5 * abs(sse), (p["sse"], sse)
    else:
        tol = np.concatenate([t for _, _, t in got])
        bound = (2.0 * np.abs(err) * tol + tol * tol).sum() + 2.0 * G.sum_bound(len(err), steps * B, (err * err).sum())
        assert abs(p["sse"] - sse) <= bound, (p["sse"], sse, bound)
    # the returned statistics are those of the returned predictions
    assert abs(p["sse"] - (err * err).sum()) <= G.sum_bound(len(err), steps * B, (err * err).sum())
    assert abs(p["sae"] - np.abs(err).sum()) <= G.sum_bound(len(err), steps * B, np.abs(err).sum())
    assert abs(p["rmse"] - np.sqrt(p["sse"] / len(err))) <= 1e-12
    # clipped: the RMSE is that of the returned (clipped) predictions
    c = m.predict_entries(test(), steps, clip=(1.0, 4.0))
    cy = c["predictions"].cpu().numpy()
    assert np.array_equal(cy, np.clip(py, np.float32(1.0), np.float32(4.0))) and (cy != py).any()
    cerr = cy.astype(np.float64) - c["targets"].cpu().numpy()
    assert abs(c["rmse"] - np.sqrt((cerr * cerr).mean())) <= 1e-5 * c["rmse"]
    assert c["rmse"] != p["rmse"]


@pytest.mark.gpu
@pytest.mark.parametrize("cd", ["float32", "float16"])
def test_queries_on_a_train_generator(gpu, cd):
    """an arbitrary queries CSR (unsorted columns, a duplicate, rows without queries), with and without values, on a
    train generator with data_sparsity [1, 1]"""
    from omnidirectional_collaborative_filtering_amd.dataset import RatingsCSR
    H = 100
    data, rd, om, aux = _model(cd, H)
    m, e = om.model, om.engine
    rng = np.random.RandomState(7)
    n = 4000
    qr, qc = rng.randint(0, ROWS, n), rng.randint(0, N, n)
    qr[qr % 7 == 3] = 5                                               # some rows without queries, one long row
    qv = (rng.randint(1, 11, n) / 2.0).astype(np.float32)
    steps = 2
    for vals in (qv, None):
        q = RatingsCSR.from_coo(qr, qc, vals, ROWS)
        np.random.seed(12)
        st = np.random.get_state()

        def train():
            np.random.set_state(st)                                   # the same permutation for every generator
            g = rd.data_gen(B, [1.0, 1.0], "train", True, aux, -1, pass_through_input_training=True)
            g._start()                                                # (the epoch plan is drawn at the first pull)
            return g
        got = _against_predict(m, e, cd, H, train, steps, queries=q)
        g = train()
        p = m.predict_entries(g, steps, queries=q)
        rows, cols, _ = _expected_order(RatingsCSR(q.row_ptr, q.col, np.zeros(q.nnz, np.float32)), g.rows_host[:steps])
        assert np.array_equal(p["rows"].cpu().numpy(), rows) and np.array_equal(p["cols"].cpu().numpy(), cols)
        assert len(rows) > 500 and len(np.unique(rows)) < steps * B
        if vals is None:
            assert p["targets"] is None and p["sse"] is None and p["rmse"] is None
        else:
            err = p["predictions"].cpu().numpy().astype(np.float64) - p["targets"].cpu().numpy()
            assert abs(p["sse"] - (err * err).sum()) <= G.sum_bound(len(err), steps * B, (err * err).sum())
    with pytest.raises(ValueError, match="queries has"):
        m.predict_entries(train(), 1, queries=RatingsCSR.from_coo(qr[qr < 50], qc[qr < 50], None, 50))


@pytest.mark.gpu
def test_deeper_model_with_causal_mask(gpu):
    """two hidden layers, tanh, k = 2 input blocks: the dense layer-0 path, h[L-1] from the hidden GEMM"""
    cd, H = "float32", 100
    data, rd, om, aux = _model(cd, H, layers=2, causal=True, act="tanh")
    m, e = om.model, om.engine
    assert e.k == 2 and len(e.H) == 2
    _against_predict(m, e, cd, H, lambda: rd.data_gen(B, None, "valid", False, aux, -1), 2)
    assert e.gt is None                                               # no row gathers: the dense layer-0 path


def _train_four(with_predictions):
    data, rd, om, aux = _model("float16", 64, steps=0, dropout=0.2)
    m, e = om.model, om.engine
    np.random.seed(6)
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True)
    for _ in range(4):
        m._train_one(gen)
        if with_predictions:
            m.predict_entries(rd.data_gen(B, None, "test", False, None, -1), 1)
            m.predict_entries(rd.data_gen(B, None, "valid", False, None, -1), 1, clip=(0.5, 5.0))
    assert e.gt is not None or e.step_paths["one_call"] > 0          # the row-gather path
    stats = e.take_stats()
    torch.cuda.synchronize()
    tensors = list(e.W) + list(e.b) + [t for t in e.Wsh if t is not None]
    tensors += [t for sw, sb in e.slots for t in list(sw) + list(sb) if t is not None]
    return stats, [t.detach().cpu().view(torch.uint8).numpy().copy() for t in tensors], (e.step_count, m.optimizer.iterations)


@pytest.mark.gpu
def test_predictions_leave_training_untouched(gpu):
    s0, w0, c0 = _train_four(False)
    s1, w1, c1 = _train_four(True)
    assert s0.shape == s1.shape and s0.shape[0] == 4 and np.array_equal(s0, s1)
    assert c0 == c1
    assert len(w0) == len(w1) and all(np.array_equal(a, b) for a, b in zip(w0, w1))


@pytest.mark.gpu
def test_refusals(gpu):
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from test_rank_rowres_gpu import _NoComm
    e = Engine(200, [64], 128, compute_dtype="float16", seed=1, shard=(0, 200, 800), comm=_NoComm())
    with pytest.raises(ValueError, match="feature-parallel"):
        e.predict_entries(dict(n_chunks=0, E=0))
    data, rd, om, aux = _model("float32", 100, steps=0)
    with pytest.raises(ValueError, match="valid or test"):
        om.model.predict_entries(rd.data_gen(B, [1.0, 1.0], "train", True, None, -1), 1)
    with pytest.raises(ValueError, match="lo <= hi"):
        om.model.predict_entries(rd.data_gen(B, None, "test", False, None, -1), 1, clip=(5.0, 0.5))


@pytest.mark.gpu
def test_train_run_saves_test_predictions(gpu, tmp_path):
    from omnidirectional_collaborative_filtering_amd import train
    from omnidirectional_collaborative_filtering_amd.dataset import synthetic_fixed_split
    data = synthetic_fixed_split("ml100k", seed=0)
    outs = {}
    for name, clip in (("plain", None), ("clipped", [1.0, 4.0])):
        path = str(tmp_path / name / "test_predictions.npz")
        cfg = dict(train.DEFAULTS)
        cfg.update(synthetic="ml100k", max_epochs=1, batch_size=128, num_hidden_units=500, patience=0,
                   model_save_path=str(tmp_path), compute_dtype="float32", seed=4, save_test_predictions=path,
                   clip_predictions=clip)
        out = train.run(cfg)
        f = np.load(path)
        want = int(data.test_tgt.row_lengths()[np.concatenate(out["manual_test_rows"])].sum())
        assert len(f["predictions"]) == len(f["cols"]) == len(f["ratings"]) == len(f["row_keys"]) == want
        keys = np.asarray(data.test_tgt.keys)[np.concatenate(out["manual_test_rows"])]
        assert set(f["row_keys"].tolist()) <= set(keys.tolist())
        rmse = float(np.sqrt(((f["predictions"].astype(np.float64) - f["ratings"]) ** 2).mean()))
        assert abs(out["predicted_test_RMSE"] - out["manual_test_RMSE"]) <= 1e-5 * out["manual_test_RMSE"]
        if clip is None:
            assert "clipped_test_RMSE" not in out
            assert abs(rmse - out["manual_test_RMSE"]) <= 1e-5 * out["manual_test_RMSE"]
        else:
            assert abs(rmse - out["clipped_test_RMSE"]) <= 1e-5 * rmse
            assert f["predictions"].min() >= 1.0 and f["predictions"].max() <= 4.0
        outs[name] = out
    same = lambda a, b: abs(a - b) <= 1e-5 * abs(b)
    assert same(outs["plain"]["manual_test_RMSE"], outs["clipped"]["manual_test_RMSE"])
    # nothing changes when the path is unset
    cfg = dict(train.DEFAULTS)
    cfg.update(synthetic="ml100k", max_epochs=1, batch_size=128, num_hidden_units=500, patience=0,
               model_save_path=str(tmp_path), compute_dtype="float32", seed=4)
    out = train.run(cfg)
    assert "predicted_test_RMSE" not in out and same(out["manual_test_RMSE"], outs["plain"]["manual_test_RMSE"])
