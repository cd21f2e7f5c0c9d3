"""GPU: per-column top-K (the transposed ocf_topk: Engine.encode_rows / topk_columns, Model.encode_rows /
recommend_columns / evaluate_ranking_columns).

The lists are checked bit for bit against the NumPy selection (tests/ranking_ref.py) over the engine's own scores
-- predict_dense of every catalogue batch, transposed -- for all three compute dtypes, every forced group count and
k at both ends of its range; the three M-side operand forms against each other; ties, short lists, guard rows and
padding; the columns= subset against the full call; the Model methods against the fp32 oracle; the per-column
ranking counts against the NumPy reference; side effects on training; the feature-parallel refusal.

Bitwise equality with predict_dense HOLDS on the MI355X (measured: largest difference 0 over every case below): the
operands are the same bits, a product does not depend on which factor is A, and both kernels add the products in
the same K order."""
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


def _reader(data, rows):
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    return data_reader(data.num_cols, rows, dataset=data, eval_mode="fixed_split")


def _seg(dcsr, Rp):
    t = dcsr.tiles(Rp)
    return dict(ex_rp=dcsr.rp, ex_tptr=t["t_tptr"], ex_col=t["t_col"], ex_ntiles=t["t_ntiles"])


def _seen_matrix(seen, R):
    """[columns, R] bool from the transposed input CSR"""
    out = np.zeros((seen.n_rows, R), bool)
    out[np.repeat(np.arange(seen.n_rows), seen.row_lengths()), seen.col] = True
    return out


def _catalogue_scores(e, rd, split="train"):
    """(codes table, S [R, N]): the engine's own scores of every catalogue row -- the encode loop restated with
    predict_dense (all-ones mask) after each batch -- and encode_rows' table from a fresh generator"""
    gen = rd.catalogue_gen(e.B, split)
    R = gen.n
    S = np.zeros((gen.num_batches * e.B, e.N), np.float32)
    out = torch.empty(e.B, e.N, device=e.dev, dtype=torch.float32)
    ones = torch.ones(e.B, e.N, device=e.dev)
    for bi in range(gen.num_batches):
        assert gen.next_batch_index() == bi
        e.load_batch(gen.scatter_args(bi, engine_args=e.scatter_args()), gen.targets(bi, e.N),
                     gather=gen.gather_tables(bi))
        e.forward(training=False)
        e._finish_deferred_encoder()
        e.predict_dense(ones, out)
        S[bi * e.B:(bi + 1) * e.B] = out.cpu().numpy()
    codes = e.encode_rows(rd.catalogue_gen(e.B, split))
    return codes, S[:R], R


def _check_exact(e, codes, R, scores_t, k, groups, exclude, excluded, ref=None, **kw):
    idx, val = e.topk_columns(codes, R, k, exclude=exclude, groups=groups, **kw)
    ri, rv = ref if ref is not None else ranking_ref.select(scores_t, k, excluded, n_real=R)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.shape == ri.shape
    assert np.array_equal(idx, ri), (k, groups, np.argwhere(idx != ri)[:4])
    assert np.array_equal(_bits(val), _bits(rv)), (k, groups)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [100, 500])
@pytest.mark.parametrize("R", [130, 700])
@pytest.mark.parametrize("N", [333, 1500])
@pytest.mark.parametrize("B", [100, 256])
@pytest.mark.parametrize("cd", ["float32", "float16", "bfloat16"])
def test_columns_are_bit_identical_to_predict(gpu, cd, B, N, R, H):
    """every returned value is S's at its index, indices distinct / eligible / < R, descending with ties by
    ascending index, nothing eligible left out above the k-th: all of it is equality with the reference selection
    over S transposed.  R = 130 and 700 leave a tail batch (all but 700 / 100) and padding rows (R_p = 256, 768)."""
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    data = parity.dataset(rows=R, cols=N, nnz=R * max(N // 10, 30), seed=7)
    rd = _reader(data, R)
    e = Engine(N, [H], B, k_blocks=1, activation="tanh", compute_dtype=cd, seed=3)
    codes, S, n = _catalogue_scores(e, rd)
    assert n == R and codes.shape == (-(-R // 128) * 128, e.Hp[0])
    assert not codes[R:].any().item()                       # rows at or beyond R are zero
    assert torch.equal(codes[R - 1], e.h[0][(R - 1) % B])               # the last batch's last real row
    St = np.ascontiguousarray(S.T)
    cat = rd.catalogue("train")
    seen = _seen_matrix(cat["seen"].host, R)
    seg = _seg(cat["seen"], codes.shape[0])
    assert seen.sum() == data.train.nnz
    for k in KS:
        refs = (ranking_ref.select(St, k, None, n_real=R), ranking_ref.select(St, k, seen, n_real=R))
        for groups in _groups(codes.shape[0] // 128):
            _check_exact(e, codes, R, St, k, groups, None, None, ref=refs[0])
            _check_exact(e, codes, R, St, k, groups, seg, seen, ref=refs[1])
    _check_exact(e, codes, R, St, 10, None, seg, seen)      # the library's own group count


def _forms_engine(cd, H, N=333, B=100, R=130):
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    data = parity.dataset(rows=R, cols=N, nnz=R * 40, seed=7)
    rd = _reader(data, R)
    e = Engine(N, [H], B, k_blocks=1, activation="tanh", compute_dtype=cd, seed=3)
    codes, S, n = _catalogue_scores(e, rd)
    return e, rd, codes, np.ascontiguousarray(S.T), n


@pytest.mark.gpu
@pytest.mark.parametrize("cd", ["float16", "bfloat16"])
def test_m_side_forms_agree_bitwise(gpu, cd):
    """row-major shadow, fp32 master (rounded while staging) and 64x64-blocked shadow: the same lists, bit for bit"""
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    e, rd, codes, St, R = _forms_engine(cd, 100)
    assert e._wblk(1) == 0 and e.Wsh[1] is not None
    seg = _seg(rd.catalogue("train")["seen"], codes.shape[0])
    # a second engine with the same weights and the blocked shadow layout (it only serves as the M operand)
    e2 = Engine(e.N, [100], e.B, k_blocks=1, activation="tanh", compute_dtype=cd, seed=3)
    e2.shadow_blocked = True
    e2.set_weights(e.get_weights())
    e2._refresh_shadows()
    assert e2._wblk(1) == 1 and torch.equal(e2.W[1], e.W[1]) and not torch.equal(e2.Wsh[1], e.Wsh[1])
    for k in (1, 10, 128):
        for groups in (1, 2):
            base = [t.cpu().numpy() for t in e.topk_columns(codes, R, k, exclude=seg, groups=groups)]
            for eng, kw in ((e, dict(master=True)), (e2, dict()), (e2, dict(master=True))):
                got = [t.cpu().numpy() for t in eng.topk_columns(codes, R, k, exclude=seg, groups=groups, **kw)]
                assert np.array_equal(got[0], base[0]) and np.array_equal(_bits(got[1]), _bits(base[1])), (k, kw)
    _check_exact(e2, codes, R, St, 10, None, None, None)


@pytest.mark.gpu
def test_blocked_shadow_of_a_wide_model(gpu):
    """H = 600 (Hp = 640 > 512): the engine's own shadows are blocked, the dense path encodes"""
    e, rd, codes, St, R = _forms_engine("float16", 600)
    assert e._wblk(1) == 1
    for k in (10, 128):
        _check_exact(e, codes, R, St, k, 2, None, None)
        _check_exact(e, codes, R, St, k, 1, None, None, master=True)


@pytest.mark.gpu
def test_ties_short_lists_and_guard_rows(gpu):
    e, rd, codes, St, R = _forms_engine("float16", 100)
    N, Rp, k = e.N, codes.shape[0], 10
    w = e.get_weights()
    zero = [7, 130, 332]                                    # columns whose decoder row is zero: score = bias[u]
    w2, b2 = w[2].copy(), w[3].copy()
    w2[:, zero] = 0.0
    b2[zero] = [0.25, -1.5, 3.0]
    e.set_weights([w[0], w[1], w2, b2])
    rng = np.random.RandomState(5)
    ex = rng.rand(N, R) < 0.3
    ex[0] = True
    ex[0, [3, 77, 129]] = False                             # column 0 has seen all but three candidates
    ex[1] = True                                            # column 1 all of them
    ex_t = torch.zeros(N, Rp, device=e.dev)
    ex_t[:, :R] = torch.as_tensor(ex.astype(np.float32))
    for groups in (1, 2):
        idx = torch.full((N + 8, k + 6), 12345, device=e.dev, dtype=torch.int32)
        val = torch.full((N + 8, k + 6), 777.0, device=e.dev, dtype=torch.float32)
        e.topk_columns(codes, R, k, exclude=ex_t, groups=groups, out=(idx, val))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        assert (idx[N:] == 12345).all() and (val[N:] == 777.0).all()            # rows >= C never written
        assert (idx[:, k:] == 12345).all() and (val[:, k:] == 777.0).all()      # nor columns >= k
        for u, b in zip(zero, (0.25, -1.5, 3.0)):           # the k smallest eligible positions, each at bias[u]
            assert np.array_equal(idx[u, :k], np.nonzero(~ex[u])[0][:k]), u
            assert np.array_equal(_bits(val[u, :k]), _bits(np.full(k, b))), u
        assert sorted(idx[0, :3].tolist()) == [3, 77, 129] and (idx[0, 3:k] == -1).all()
        assert np.isneginf(val[0, 3:k]).all() and (idx[1, :k] == -1).all() and np.isneginf(val[1, :k]).all()
        assert idx[:N, :k].max() < R
    # the padding rows of the table (130 .. 255) never appear, at k = 128 with 130 candidates
    idx, val = e.topk_columns(codes, R, 128)
    assert idx.shape == (N, 128) and idx.max().item() < R and idx.min().item() >= 0 and torch.isfinite(val).all()
    for u in zero:
        assert np.array_equal(idx[u].cpu().numpy(), np.arange(128))


@pytest.mark.gpu
@pytest.mark.parametrize("cd", ["float32", "float16"])
def test_columns_subset_equals_the_full_call(gpu, cd):
    e, rd, codes, St, R = _forms_engine(cd, 100)
    cat = rd.catalogue("valid")
    seg = _seg(cat["seen"], codes.shape[0])
    h = cat["held"].tiles(codes.shape[0])
    rel = dict(rel_rp=cat["held"].rp, rel_col=h["t_col"], rel_val=h["t_val"], rel_min=3.0)
    cols = [5, 300, 332, 128, 127, 256, 5]                  # 256 .. 332: the last, partial row tile of the full call
    for k in (10, 128):
        full = [t.cpu().numpy() for t in e.topk_columns(codes, R, k, exclude=seg, relevance=rel)]
        for columns in (cols, torch.as_tensor(cols), list(range(140))):       # 140: a partial tile of the subset
            sub = [t.cpu().numpy() for t in e.topk_columns(codes, R, k, columns=columns, exclude=seg, relevance=rel)]
            sel = np.asarray(columns)
            assert sub[0].shape == (len(sel), k) and sub[2].shape == (len(sel), 4)
            assert np.array_equal(sub[0], full[0][sel]) and np.array_equal(_bits(sub[1]), _bits(full[1][sel]))
            assert np.array_equal(_bits(sub[2]), _bits(full[2][sel]))
    with pytest.raises(ValueError, match="columns = indices"):
        e.topk_columns(codes, R, 10, columns=[333])


def _assert_against_oracle(items, scores, s_ref, eligible, k):
    """every position of every list: value within the fp32 bar of the oracle's score there, index eligible, and
    no better than 2 bars below the oracle's own k-th eligible score (test_topk_gpu.py's bars)"""
    bar = lambda s: parity.FP32_ABS + parity.FP32_ABS * np.abs(s)
    for b in range(items.shape[0]):
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


def _trained(causal, cd="float32", seed=5, steps=3, data=None, dropout=None):
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    data = parity.dataset() if data is None else data
    N, B, H = data.num_cols, 128, 100
    np.random.seed(3)
    rd = _reader(data, data.train.n_rows)
    kw = dict(dropout_probability=dropout) if dropout else {}
    om = omni_model(1, H, N, B, "sigmoid", use_causal_info=causal, compute_dtype=cd, seed=seed, **kw)
    m = om.model
    m.compile(parity.our_opt("adagrad", 0.05), "mean_squared_error")
    aux = "causal" if causal else None
    gen = rd.data_gen(B, [1.0, 1.0], "train", True, aux, -1, pass_through_input_training=True)
    m.fit_generator(gen, steps, verbose=0)
    return data, rd, om, aux


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True])
def test_model_methods_against_oracle(gpu, causal):
    """fp32, a few training steps, both splits: codes and lists against the oracle run on the catalogue inputs"""
    data, rd, om, aux = _trained(causal)
    m, N, H, k = om.model, data.num_cols, 100, 10
    w = m.get_weights()
    ora = OmniOracle([(2 if causal else 1) * N, H, N], activation="sigmoid").set_params(w[0::2], w[1::2])
    bar = lambda s: parity.FP32_ABS + parity.FP32_ABS * np.abs(s)
    for split in ("valid", "test"):
        keys_ref, inputs, seen, _ = data.catalogue(split)
        R = len(keys_ref)
        m_in, _, x, _, m_miss = scatter_rows_numpy(inputs.row_ptr, inputs.col, inputs.val, np.arange(R), N, aux=-1.0)
        s_ref, (hs, _, _) = ora.forward(parity.aux_model_input(aux, x, m_in, m_miss), np.ones((R, N)))
        s_ref_t = np.ascontiguousarray(np.asarray(s_ref, np.float64).T)          # [columns, candidates]
        keys, codes = m.encode_rows(rd, split, auxilliary_mask_type=aux)
        assert list(keys) == list(keys_ref) and tuple(codes.shape) == (R, H) and codes.dtype == torch.float32
        assert (np.abs(codes.cpu().numpy() - hs[1]) <= bar(hs[1])).all()
        eligible = ~_seen_matrix(seen, R)
        keys, items, scores = m.recommend_columns(rd, split, k=k, auxilliary_mask_type=aux)
        assert list(keys) == list(keys_ref) and tuple(items.shape) == tuple(scores.shape) == (N, k)
        _assert_against_oracle(items.cpu().numpy(), scores.cpu().numpy(), s_ref_t, eligible, k)
        sel = [0, 17, 332]
        _, items2, scores2 = m.recommend_columns(rd, split, k=k, exclude_seen=False, columns=sel,
                                                 auxilliary_mask_type=aux)
        _assert_against_oracle(items2.cpu().numpy(), scores2.cpu().numpy(), s_ref_t[sel], np.ones((3, R), bool), k)
    assert (om.engine.gt is not None) == (not causal)          # the row-gather path / the dense path encoded


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 20])
def test_ranking_per_column(gpu, k):
    from omnidirectional_collaborative_filtering_amd import metrics
    data, rd, om, _ = _trained(False, steps=2)
    m, N = om.model, data.num_cols
    nrel_seen = {}
    for split, rows_want in (("valid", 327), ("test", None)):
        cat, codes = m._encode_catalogue(rd, split, None, -1)
        held = cat["held"].host
        for rel_min in (None, 3.0):
            items, _, rank = [t.cpu().numpy() for t in m._rank_columns(cat, codes, k, rel_min)]
            assert rank.shape == (N, 4) and (rank[:, 3] == 0).all()
            ref = []
            for u in range(N):
                sl = slice(held.row_ptr[u], held.row_ptr[u + 1])
                cols, vals = held.col[sl], held.val[sl]
                ref.append(ranking_ref.row_rank(items[u], cols if rel_min is None else cols[vals >= rel_min]))
            ref = np.array(ref, np.float64)
            assert np.array_equal(rank[:, 0], ref[:, 0]) and np.array_equal(rank[:, 2], ref[:, 2])
            assert np.abs(rank[:, 1] - ref[:, 1]).max() <= 1e-6
            assert ref[:, 2].max() > 0
            nrel_seen[split, rel_min] = ref[:, 2]
            d = m.evaluate_ranking_columns(rd, split, k=k, relevance_min=rel_min)
            assert d == metrics.ranking_from_rows(rank[:, 0], rank[:, 1], rank[:, 2], k)
            want = ranking_ref.ranking_metrics(ref[:, 0], ref[:, 1], ref[:, 2], k)
            assert d["rows"] == want["rows"] == int((ref[:, 2] > 0).sum())
            assert set(d) == {"hit_rate@%d" % k, "recall@%d" % k, "ndcg@%d" % k, "rows"}
            if rel_min is None and rows_want is not None:
                assert d["rows"] == rows_want
            for key in want:
                assert abs(d[key] - want[key]) <= 1e-6, key
        assert (nrel_seen[split, 3.0] <= nrel_seen[split, None]).all()
        assert (nrel_seen[split, 3.0] < nrel_seen[split, None]).any()
    with pytest.raises(ValueError, match="valid' or 'test"):
        m.evaluate_ranking_columns(rd, "train", k=k)


def _train_four(with_columns):
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.dataset import split_ratings, synthetic_ratings
    from omnidirectional_collaborative_filtering_amd.model import omni_model
    r, c, v = synthetic_ratings(600, 200, 9000, half_stars=True, seed=2)
    data = split_ratings(r, c, v, 600, 200, rng=np.random.RandomState(2))
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
        if with_columns:
            m.encode_rows(rd, "valid")
            m.recommend_columns(rd, "valid", k=10)
            m.evaluate_ranking_columns(rd, "test", k=10)
    assert e.gt is not None or e.step_paths["one_call"] > 0          # the row-gather path
    stats = e.take_stats()
    torch.cuda.synchronize()
    tensors = list(e.W) + list(e.b) + [t for t in e.Wsh if t is not None]
    tensors += [t for sw, sb in e.slots for t in list(sw) + list(sb) if t is not None]
    rng = np.random.get_state()
    return (stats, [t.detach().cpu().view(torch.uint8).numpy().copy() for t in tensors],
            (e.step_count, m.optimizer.iterations), (rng[0], rng[1].copy(), rng[2], rng[3], rng[4]))


@pytest.mark.gpu
def test_column_calls_leave_training_untouched(gpu):
    s0, w0, c0, r0 = _train_four(False)
    s1, w1, c1, r1 = _train_four(True)
    assert s0.shape == s1.shape and s0.shape[0] == 4 and np.array_equal(s0, s1)
    assert c0 == c1
    assert len(w0) == len(w1) and all(np.array_equal(a, b) for a, b in zip(w0, w1))
    assert r0[0] == r1[0] and np.array_equal(r0[1], r1[1]) and r0[2:] == r1[2:]


@pytest.mark.gpu
def test_feature_parallel_engine_is_refused(gpu):
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from test_rank_rowres_gpu import _NoComm
    e = Engine(200, [64], 128, compute_dtype="float16", seed=1, shard=(0, 200, 800), comm=_NoComm())
    codes = torch.zeros(128, 128, device=e.dev, dtype=torch.float16)
    with pytest.raises(ValueError, match="feature-parallel"):
        e.topk_columns(codes, 100, 10)
    with pytest.raises(ValueError, match="feature-parallel"):
        e.encode_rows(None)
