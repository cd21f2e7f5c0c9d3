"""CPU: the top-k entry points of the C ABI (declared, mirrored, laid out as gcc lays them out), their argument
checks (every refusal has its own message and happens before any launch), the workspace bound, the host closed
forms of the ranking metrics, and the Model surface.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ranking_ref
from omnidirectional_collaborative_filtering_amd import _lib, metrics
from test_abi import HDR, declared_functions


def test_header_declares_topk():
    fns = declared_functions()
    for name in ("ocf_topk", "ocf_topk_workspace"):
        assert name in fns and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["ocf_topk"][0] is ctypes.c_int and _lib.SIGNATURES["ocf_topk_workspace"][0] is ctypes.c_int64
    assert "#define OCF_TOPK_MAX_K 128" in open(HDR).read() and _lib.TOPK_MAX_K == 128


def test_topk_args_layout_matches_c():
    fields = [f for f, _ in _lib.OcfTopkArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void) {",
             'printf("size %zu\\n", sizeof(OcfTopkArgs));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(OcfTopkArgs, %s));' % (f, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert ctypes.sizeof(_lib.OcfTopkArgs) == got["size"]
    for f in fields:
        assert getattr(_lib.OcfTopkArgs, f).offset == got[f], f


def _good(B=256, N=20096, K=512, k=10, groups=0):
    a = _lib.OcfTopkArgs()
    a.compute_dtype, a.w_dtype = _lib.DT_F16, _lib.DT_F16
    a.h = a.W = a.bias = a.out_idx = a.out_val = a.work = 1      # never dereferenced: every call below is refused
    a.ldh = a.ldw = K
    a.M, a.N, a.K, a.m_real, a.n_real = B, N, K, B, N - 96
    a.k, a.groups, a.ld_out = k, groups, k
    a.work_bytes = 1 << 40
    return a


def _set(a, **kw):
    for key, v in kw.items():
        setattr(a, key, v)
    return a


@pytest.mark.parametrize("change, message", [
    (dict(k=0), "k must be in 1"),
    (dict(k=129), "k must be in 1"),
    (dict(M=100), "multiples of 128"),
    (dict(N=20000), "multiples of 128"),
    (dict(K=500), "multiples of 128"),
    (dict(n_real=20097), "n_real > N"),
    (dict(ld_out=9), "ld_out < k"),
    (dict(h=None), "null h, W, bias, out_idx or out_val"),
    (dict(W=None), "null h, W, bias, out_idx or out_val"),
    (dict(bias=None), "null h, W, bias, out_idx or out_val"),
    (dict(out_idx=None), "null h, W, bias, out_idx or out_val"),
    (dict(out_val=None), "null h, W, bias, out_idx or out_val"),
    (dict(ex_rows=1, ex_rp=1, ex_tptr=1, ex_col=1, ex_ntiles=157, ex_mask=1, ld_ex=20096), "both exclusion forms"),
    (dict(w_dtype=_lib.DT_F32, w_blocked=1), "blocked flag needs a 16-bit weight"),
    (dict(work_bytes=1024), "work_bytes too small"),
    (dict(work=None), "work_bytes too small"),
    (dict(rel_rows=1, rel_rp=1, rel_col=1, rel_val=1), "relevance given without row_rank"),
])
def test_topk_refusals_have_their_own_message(change, message):
    a = _set(_good(), **change)
    with pytest.raises(_lib.OcfError, match=message):
        _lib.call("ocf_topk", a, None)


def test_topk_workspace_is_bounded():
    lib = _lib.load()
    B, N, k = 256, 20000, 10
    Np = -(-N // 128) * 128
    n_tiles = Np // 128
    for groups in (0, n_tiles):
        a = _good(B, Np, 512, k, groups)
        nb = lib.ocf_topk_workspace(ctypes.byref(a))
        assert 0 < nb <= B * N * 4 // 4
        assert nb <= B * n_tiles * min(k, 128) * 8 + 4096
    # more groups than tiles: as many as there are tiles
    assert lib.ocf_topk_workspace(ctypes.byref(_good(B, Np, 512, k, 10 * n_tiles))) == nb
    # and never a function of B x N: k = 128 at every tile its own group is the largest it gets
    assert lib.ocf_topk_workspace(ctypes.byref(_good(B, Np, 512, 128, n_tiles))) <= B * n_tiles * 128 * 8 + 4096
    bad = _good(k=0)
    assert lib.ocf_topk_workspace(ctypes.byref(bad)) == -1 and b"k must be in 1" in lib.ocf_last_error()
    assert lib.ocf_topk_workspace(None) == -1


def test_ranking_from_rows_closed_forms():
    k = 5
    disc = 1.0 / np.log2(np.arange(k) + 2.0)
    # (hits, dcg, n_relevant): no relevant column (left out), no hit, more relevant columns than k (all k hit),
    # a perfect list of 3, one hit at the last position
    rows = [(0, 0.0, 0), (0, 0.0, 4), (5, disc.sum(), 9), (3, disc[:3].sum(), 3), (1, disc[4], 2)]
    hits, dcg, nrel = (np.array(x) for x in zip(*rows))
    got = metrics.ranking_from_rows(hits, dcg, nrel, k)
    ref = ranking_ref.ranking_metrics(hits, dcg, nrel, k)
    assert got["rows"] == ref["rows"] == 4
    for key in ("hit_rate@5", "recall@5", "ndcg@5"):
        assert abs(got[key] - ref[key]) <= 1e-12, key
    assert abs(got["hit_rate@5"] - 0.75) <= 1e-12
    assert abs(got["recall@5"] - (0 + 5 / 9 + 1 + 0.5) / 4) <= 1e-12
    assert abs(got["ndcg@5"] - (0 + 1 + 1 + disc[4] / disc[:2].sum()) / 4) <= 1e-12
    # float32 inputs (the device rows) and no row at all
    got32 = metrics.ranking_from_rows(hits.astype(np.float32), dcg.astype(np.float32), nrel.astype(np.float32), k)
    assert abs(got32["ndcg@5"] - ref["ndcg@5"]) <= 1e-6
    assert metrics.ranking_from_rows([0], [0.0], [0], k)["rows"] == 0
    for name in ("hit_rate@5", "recall@5", "ndcg@5", "ranking_from_rows"):
        assert name not in metrics.KNOWN


def test_selection_reference_orders_ties_by_column():
    s = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    ex = np.zeros((2, 5), bool)
    ex[1, [0, 1, 3]] = True
    idx, val = ranking_ref.select(s, 3, ex, n_real=5)
    assert idx.tolist() == [[1, 2, 4], [2, 4, -1]]
    assert val[1].tolist() == [0.0, 0.0, -np.inf]


def test_model_has_the_recommendation_methods():
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from omnidirectional_collaborative_filtering_amd.model import Model
    for name in ("recommend_on_batch", "recommend_generator", "evaluate_ranking"):
        assert callable(getattr(Model, name))
    assert callable(Engine.topk)
