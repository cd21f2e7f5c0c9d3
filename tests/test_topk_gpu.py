"""GPU: recommendations from the decoder GEMM (ocf_topk, Engine.topk, Model.recommend_* / evaluate_ranking).

The selection is checked bit for bit against the NumPy reference (tests/ranking_ref.py) applied to predict_dense's
own output -- indices equal, values bitwise equal, for every forced group count, k at both ends of its range, all
three compute dtypes and all three exclusion forms -- then for ties, short rows and padding, independently against
the fp32 oracle, for the ranking statistics, for side effects on training, and for the feature-parallel refusal."""
import numpy as np
import pytest
import torch

import parity
import ranking_ref
from oracle.batch_oracle import scatter_rows_numpy
from oracle.model_oracle import OmniOracle

KS = (1, 10, 128)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _groups(n_tiles):
    return sorted({1, 2, 3, n_tiles})


def _engine(B, N, H, cd, seed=3, act="tanh"):
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    e = Engine(N, [H], B, k_blocks=1, activation=act, compute_dtype=cd, seed=seed)
    rng = np.random.RandomState(seed)
    x = rng.rand(B, N) * (rng.rand(B, N) < 0.2)
    z = np.zeros((B, N), np.float32)
    e.load_dense([x], z, z)
    e.forward(training=False)
    return e


def _predict(e):
    out = torch.empty(e.B, e.N, device=e.dev, dtype=torch.float32)
    e.predict_dense(torch.ones(e.B, e.N, device=e.dev), out)
    return out.cpu().numpy()


def _segment_form(csr, rows, N, dev):
    """Engine.topk's row-segment exclusion of dataset rows `rows` (-1: none) + the tensors it points into"""
    col_s, _, _, tptr = csr.tile_index(N)
    t = dict(ex_rows=torch.as_tensor(np.asarray(rows, np.int32), device=dev),
             ex_rp=torch.as_tensor(csr.row_ptr.astype(np.int64), device=dev),
             ex_tptr=torch.as_tensor(np.ascontiguousarray(tptr, np.int32), device=dev),
             ex_col=torch.as_tensor(np.ascontiguousarray(col_s, np.int32), device=dev), ex_ntiles=tptr.shape[1] - 1)
    return t


def _check_exact(e, scores, k, groups, exclude, excluded):
    idx, val = e.topk(k, exclude=exclude, groups=groups)
    ri, rv = ranking_ref.select(scores, k, excluded, n_real=e.N)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(idx, ri), (k, groups, np.argwhere(idx != ri)[:4])
    assert np.array_equal(_bits(val), _bits(rv)), (k, groups)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [100, 500])
@pytest.mark.parametrize("N", [333, 1500])
@pytest.mark.parametrize("B", [100, 256])
@pytest.mark.parametrize("cd", ["float32", "float16", "bfloat16"])
def test_topk_is_bit_identical_to_predict(gpu, cd, B, N, H):
    e = _engine(B, N, H, cd)
    scores = _predict(e)
    rng = np.random.RandomState(11)
    dense = rng.rand(B, N) < 0.3
    dense_t = torch.as_tensor(dense.astype(np.float32), device=e.dev)
    data = parity.with_duplicates(300, N, 30 * 300 if N > 1000 else 6000, seed=4)
    rows = rng.randint(0, 300, B)
    rows[B // 2] = -1
    seg = _segment_form(data.train, rows, N, e.dev)
    seg_ex = ranking_ref.csr_excluded(data.train, rows, N)
    assert seg_ex.sum() > B
    for groups in _groups(e.n_tiles):
        for k in KS:
            _check_exact(e, scores, k, groups, None, None)
            _check_exact(e, scores, k, groups, dense_t, dense)
            _check_exact(e, scores, k, groups, seg, seg_ex)
    _check_exact(e, scores, 10, None, seg, seg_ex)        # the library's own group count


@pytest.mark.gpu
def test_more_candidates_than_the_merge_stages(gpu):
    """130 column groups x k = 128 candidates per row are more than the merge launch stages in LDS (16,384): it
    then works on the workspace itself.  Same exact check."""
    B, N, H = 100, 130 * 128 - 7, 100
    e = _engine(B, N, H, "float16")
    scores = _predict(e)
    dense = np.random.RandomState(3).rand(B, N) < 0.3
    dense_t = torch.as_tensor(dense.astype(np.float32), device=e.dev)
    assert e.n_tiles * 128 > 16384
    _check_exact(e, scores, 128, e.n_tiles, None, None)
    _check_exact(e, scores, 128, e.n_tiles, dense_t, dense)
    _check_exact(e, scores, 100, None, dense_t, dense)


@pytest.mark.gpu
def test_ties_are_ordered_by_column(gpu):
    B, N, H = 100, 1500, 100
    e = _engine(B, N, H, "float16")
    w = e.get_weights()
    # all-zero decoder: every row's list is its first k eligible columns
    e.set_weights([w[0], w[1], np.zeros_like(w[2]), np.zeros_like(w[3])])
    rng = np.random.RandomState(2)
    dense = rng.rand(B, N) < 0.3
    dense_t = torch.as_tensor(dense.astype(np.float32), device=e.dev)
    for groups in _groups(e.n_tiles):
        for ex_t, ex in ((None, np.zeros((B, N), bool)), (dense_t, dense)):
            idx, val = e.topk(10, exclude=ex_t, groups=groups)
            want = np.stack([np.nonzero(~ex[b])[0][:10] for b in range(B)])
            assert np.array_equal(idx.cpu().numpy(), want), groups
            assert np.array_equal(_bits(val.cpu().numpy()), _bits(np.zeros((B, 10))))
    # equal scores at the k-th place that later, larger ones push out: the largest columns among them must leave
    b3 = np.zeros_like(w[3])
    b3[[200, 700, 701, 1300, 1499]] = 1.0
    b3[900] = 2.0
    e.set_weights([w[0], w[1], np.zeros_like(w[2]), b3])
    scores = _predict(e)
    for groups in _groups(e.n_tiles):
        for k in (4, 10, 128):
            _check_exact(e, scores, k, groups, None, None)
            _check_exact(e, scores, k, groups, dense_t, dense)
    # equal scores inside a tile (j, j + 1), across tiles (j, j + 128) and across groups: one decoder column and
    # one bias copied to all of them, pushed to the top of every row by the bias
    tie = [37, 38, 165, 700, 1400, 1499]
    w2, b2 = w[2].copy(), w[3].copy()
    w2[:, tie] = w2[:, [tie[0]]]
    b2[tie] = 50.0
    e.set_weights([w[0], w[1], w2, b2])
    scores = _predict(e)
    assert all(np.array_equal(_bits(scores[:, tie[0]]), _bits(scores[:, c])) for c in tie)
    for groups in _groups(e.n_tiles):
        idx, _ = e.topk(10, groups=groups)
        assert np.array_equal(idx.cpu().numpy()[:, :6], np.tile(tie, (B, 1))), groups
        _check_exact(e, scores, 10, groups, None, None)
        _check_exact(e, scores, 4, groups, dense_t, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("cd", ["float32", "bfloat16"])
def test_short_rows_padding_and_guard_rows(gpu, cd):
    B, N, k = 100, 130, 10
    e = _engine(B, N, 100, cd)
    scores = _predict(e)
    ex = np.random.RandomState(5).rand(B, N) < 0.3
    ex[0] = True
    ex[0, [3, 77, 129]] = False          # three eligible columns, one of them in the last (padded) tile
    ex[1] = True                         # none
    ex_t = torch.as_tensor(ex.astype(np.float32), device=e.dev)
    for groups in (1, 2):
        idx = torch.full((B + 8, k + 6), 12345, device=e.dev, dtype=torch.int32)
        val = torch.full((B + 8, k + 6), 777.0, device=e.dev, dtype=torch.float32)
        e.topk(k, exclude=ex_t, groups=groups, out=(idx, val))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        assert (idx[B:] == 12345).all() and (val[B:] == 777.0).all()            # rows >= B never written
        assert (idx[:, k:] == 12345).all() and (val[:, k:] == 777.0).all()      # nor columns >= k
        ri, rv = ranking_ref.select(scores, k, ex, n_real=N)
        assert np.array_equal(idx[:B, :k], ri) and np.array_equal(_bits(val[:B, :k]), _bits(rv))
        assert sorted(idx[0, :3].tolist()) == [3, 77, 129] and (idx[0, 3:k] == -1).all()
        assert np.isneginf(val[0, 3:k]).all() and (idx[1, :k] == -1).all() and np.isneginf(val[1, :k]).all()
        assert idx[:B, :k].max() < N
    # without exclusions the padding columns (130 .. 255) still never appear, at k = 128 with 130 real columns
    idx, val = e.topk(128)
    assert idx.max().item() < N and idx.min().item() >= 0 and torch.isfinite(val).all()


def _assert_against_oracle(items, scores, s_ref, eligible, k):
    """every position of every row: value within the fp32 bar of the oracle's score there, index eligible, and
    no better than 2 bars below the oracle's own k-th eligible score"""
    bar = lambda s: parity.FP32_ABS + parity.FP32_ABS * np.abs(s)
    Bn = items.shape[0]
    for b in range(Bn):
        el = np.nonzero(eligible[b])[0]
        assert len(el) >= k
        kth = np.sort(s_ref[b, el])[::-1][k - 1]
        for j in range(k):
            c = int(items[b, j])
            assert 0 <= c < s_ref.shape[1] and eligible[b, c], (b, j, c)
            s = s_ref[b, c]
            assert abs(float(scores[b, j]) - s) <= bar(s), (b, j, float(scores[b, j]), s)
            assert s >= kth - 2 * bar(kth), (b, j, s, kth)
        assert len(set(items[b].tolist())) == k


@pytest.mark.gpu
def test_recommend_generator_against_oracle(gpu):
    """one hidden layer on the generator (row-gather) path, trained a few steps, fp32"""
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = parity.dataset()
    N, B, H, k = data.num_cols, 128, 100, 10
    np.random.seed(3)
    rd = data_reader(N, 700, dataset=data, eval_mode="fixed_split")
    om = omni_model(1, H, N, B, "sigmoid", use_causal_info=False, compute_dtype="float32", seed=5)
    m = om.model
    m.compile(parity.our_opt("adagrad", 0.05), "mean_squared_error")
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True)
    m.fit_generator(gen, 3, verbose=0)
    steps = 2
    vg = rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1)
    rows, items, scores = m.recommend_generator(vg, steps, k=k, exclude_seen=True)
    assert om.engine.gt is not None                                  # the row-gather path ran
    rows, items, scores = rows.cpu().numpy(), items.cpu().numpy(), scores.cpu().numpy()
    assert rows.shape == (steps * B,) and items.shape == scores.shape == (steps * B, k)
    assert np.array_equal(rows, vg.rows_host[:steps].ravel())
    w = m.get_weights()
    ora = OmniOracle([N, H, N], activation="sigmoid").set_params(w[0::2], w[1::2])
    _, _, x, _, _ = scatter_rows_numpy(data.valid_in.row_ptr, data.valid_in.col, data.valid_in.val, rows, N, aux=-1.0)
    s_ref, _ = ora.forward(x, np.ones((len(rows), N)))
    _assert_against_oracle(items, scores, np.asarray(s_ref, np.float64),
                           ~ranking_ref.csr_excluded(data.valid_in, rows, N), k)
    # exclude_seen=False: the same rows again (a fresh generator), nothing excluded
    vg2 = rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1)
    _, items2, scores2 = m.recommend_generator(vg2, 1, k=k, exclude_seen=False)
    _assert_against_oracle(items2.cpu().numpy(), scores2.cpu().numpy(), np.asarray(s_ref[:B], np.float64),
                           np.ones((B, N), bool), k)


@pytest.mark.gpu
def test_recommend_on_batch_against_oracle(gpu):
    """three hidden layers on the dense path (the Jester shape, scaled down), trained a few steps, fp32"""
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    rng = np.random.RandomState(1)
    B, N, H, k = 128, 100, 64, 10
    om = omni_model(3, H, N, B, dense_activation="tanh", use_causal_info=True, compute_dtype="float32", seed=3,
                    rating_range=20)
    m = om.model
    m.compile(parity.our_opt("rmsprop"), "mean_squared_error")
    for _ in range(3):
        d = np.where(rng.rand(B, N) < 0.5, rng.uniform(-10, 10, (B, N)), 0.0)
        drop = rng.rand(B, N) < 0.5
        x, t = np.where(drop, d, 0.0), np.where(~drop, d, 0.0)
        m.train_on_batch([x, 1.0 * (x != 0), 1.0 * (t != 0)], t)
    d = np.where(rng.rand(B, N) < 0.5, rng.uniform(-10, 10, (B, N)), 0.0)
    obs = 1.0 * (d != 0)
    items, scores = m.recommend_on_batch([d, obs, np.ones((B, N))], k=k, exclude=obs)
    assert om.engine.gt is None                                      # the dense path ran
    w = m.get_weights()
    ora = OmniOracle([2 * N, H, H, H, N], activation="tanh").set_params(w[0::2], w[1::2])
    s_ref, _ = ora.forward(np.concatenate([d, obs], 1), np.ones((B, N)))
    _assert_against_oracle(items.cpu().numpy(), scores.cpu().numpy(), np.asarray(s_ref, np.float64), obs == 0, k)


def _split():
    from omnidirectional_collaborative_filtering_amd.dataset import split_ratings, synthetic_ratings
    r, c, v = synthetic_ratings(600, 200, 9000, half_stars=True, seed=2)
    return split_ratings(r, c, v, 600, 200, rng=np.random.RandomState(2))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 20])
def test_evaluate_ranking(gpu, k):
    from omnidirectional_collaborative_filtering_amd import metrics
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = _split()
    N, B = data.num_cols, 128
    np.random.seed(4)
    rd = data_reader(N, 600, dataset=data, eval_mode="fixed_split")
    m = omni_model(1, 64, N, B, "sigmoid", use_causal_info=False, compute_dtype="float32", seed=8).model
    m.compile(parity.our_opt("adagrad", 0.05), "mean_squared_error")
    m.fit_generator(rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True), 2, verbose=0)
    valid = lambda: rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1)
    steps = 2
    tgt = data.valid_tgt
    seen_nrel = {}
    for rel_min in (None, 3.0):
        g = valid()
        got = [m._rank_batch(g, k, True, rel_min, True) for _ in range(steps)]
        rows = np.concatenate([r.cpu().numpy() for r, _ in got])
        items = np.concatenate([t[0].cpu().numpy() for _, t in got])
        rank = np.concatenate([t[2].cpu().numpy() for _, t in got])
        assert rank.shape == (steps * B, 4) and (rank[:, 3] == 0).all()
        ref = []
        for b, r in enumerate(rows):
            sl = slice(tgt.row_ptr[r], tgt.row_ptr[r + 1])
            cols, vals = tgt.col[sl], tgt.val[sl]
            ref.append(ranking_ref.row_rank(items[b], cols if rel_min is None else cols[vals >= rel_min]))
        ref = np.array(ref, np.float64)
        assert np.array_equal(rank[:, 0], ref[:, 0]) and np.array_equal(rank[:, 2], ref[:, 2])
        assert np.abs(rank[:, 1] - ref[:, 1]).max() <= 1e-6
        seen_nrel[rel_min] = ref[:, 2]
        assert ref[:, 2].max() > 0
        d = m.evaluate_ranking(valid(), steps, k=k, relevance_min=rel_min)
        assert d == metrics.ranking_from_rows(rank[:, 0], rank[:, 1], rank[:, 2], k)
        want = ranking_ref.ranking_metrics(ref[:, 0], ref[:, 1], ref[:, 2], k)
        assert d["rows"] == want["rows"] and set(d) == {"hit_rate@%d" % k, "recall@%d" % k, "ndcg@%d" % k, "rows"}
        for key in want:
            assert abs(d[key] - want[key]) <= 1e-6, key
    assert (seen_nrel[3.0] <= seen_nrel[None]).all() and (seen_nrel[3.0] < seen_nrel[None]).any()
    with pytest.raises(ValueError, match="valid or test"):
        m.evaluate_ranking(rd.data_gen(B, [1.0, 1.0], "train", True, None, -1), 1, k=k)


def _train_four(with_recommendations):
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = _split()
    N, B = data.num_cols, 128
    np.random.seed(6)
    rd = data_reader(N, 600, dataset=data, eval_mode="fixed_split")
    om = omni_model(1, 64, N, B, "sigmoid", use_causal_info=False, dropout_probability=0.2, compute_dtype="float16",
                    seed=9)
    m, e = om.model, om.engine
    m.compile(parity.our_opt("adagrad", 0.05), "mean_squared_error")
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True)
    for _ in range(4):
        m._train_one(gen)
        if with_recommendations:
            m.recommend_generator(rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1), 1, k=10)
            m.evaluate_ranking(rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1), 1, k=10)
    assert e.gt is not None or e.step_paths["one_call"] > 0          # the row-gather path
    stats = e.take_stats()
    torch.cuda.synchronize()
    tensors = list(e.W) + list(e.b) + [t for t in e.Wsh if t is not None]
    tensors += [t for sw, sb in e.slots for t in list(sw) + list(sb) if t is not None]
    return stats, [t.detach().cpu().view(torch.uint8).numpy().copy() for t in tensors], (e.step_count, m.optimizer.iterations)


@pytest.mark.gpu
def test_recommendations_leave_training_untouched(gpu):
    s0, w0, c0 = _train_four(False)
    s1, w1, c1 = _train_four(True)
    assert s0.shape == s1.shape and s0.shape[0] == 4 and np.array_equal(s0, s1)
    assert c0 == c1
    assert len(w0) == len(w1) and all(np.array_equal(a, b) for a, b in zip(w0, w1))


@pytest.mark.gpu
def test_feature_parallel_engine_is_refused(gpu):
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from test_rank_rowres_gpu import _NoComm
    e = Engine(200, [64], 128, compute_dtype="float16", seed=1, shard=(0, 200, 800), comm=_NoComm())
    with pytest.raises(ValueError, match="feature-parallel"):
        e.topk(10)
