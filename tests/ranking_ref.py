"""NumPy references for the top-k selection (ocf_topk) and the ranking metrics (metrics.ranking_from_rows)."""
import numpy as np


def select(scores, k, excluded=None, n_real=None):
    """(idx [B, k] int32, val [B, k] of scores' dtype): per row the k largest eligible scores, descending, equal
    scores by ascending column; excluded ([B, N] bool) and columns >= n_real are not eligible; rows with fewer
    than k eligible columns end in (-1, -inf)."""
    s = np.array(scores, copy=True)
    B, N = s.shape
    out = np.zeros((B, N), bool) if excluded is None else np.asarray(excluded, bool).copy()
    if n_real is not None:
        out[:, n_real:] = True
    s[out] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")          # stable: equal scores keep ascending column
    idx = np.full((B, k), -1, np.int32)
    val = np.full((B, k), -np.inf, s.dtype)
    kk = min(k, N)
    top = order[:, :kk]
    v = np.take_along_axis(s, top, 1)
    ok = ~np.take_along_axis(out, top, 1)
    idx[:, :kk] = np.where(ok, top, -1)
    val[:, :kk] = np.where(ok, v, -np.inf)
    return idx, val


def csr_excluded(csr, rows, N):
    """[len(rows), N] bool: the (row, column) pairs a CSR lists for dataset rows `rows` (-1: none)"""
    out = np.zeros((len(rows), N), bool)
    for b, r in enumerate(rows):
        if r >= 0:
            out[b, csr.col[csr.row_ptr[r]:csr.row_ptr[r + 1]]] = True
    return out


def row_rank(items, rel_cols):
    """fp64 (hits, dcg, n_relevant) of one returned list against the set of relevant columns"""
    rel = set(int(c) for c in rel_cols)
    hit = np.array([int(c) >= 0 and int(c) in rel for c in items], bool)
    dcg = float(np.sum(hit / np.log2(np.arange(len(items), dtype=np.float64) + 2.0)))
    return int(hit.sum()), dcg, len(rel)


def ranking_metrics(hits, dcg, n_relevant, k):
    """the closed forms in fp64, row by row, over the rows with a relevant column"""
    hr, rec, nd, rows = [], [], [], 0
    for h, d, n in zip(hits, dcg, n_relevant):
        if n <= 0:
            continue
        rows += 1
        hr.append(1.0 if h > 0 else 0.0)
        rec.append(float(h) / float(n))
        ideal = sum(1.0 / np.log2(j + 2.0) for j in range(int(min(n, k))))
        nd.append(float(d) / ideal)
    return {"hit_rate@%d" % k: float(np.mean(hr)), "recall@%d" % k: float(np.mean(rec)),
            "ndcg@%d" % k: float(np.mean(nd)), "rows": rows}
