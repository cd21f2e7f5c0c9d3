"""NumPy fixtures, fp64 reference and bound for the encoder over column tiles (include/ocf.h OcfEncTileArgs,
csrc/ocf_tiles.hip: the per-row chain and the packed form), the small hand-built calls the GPU tests launch
(tests/test_tiles_direct_gpu.py), a float32 restatement that accumulates tile by tile (`twin`) and ten deliberately
wrong variants of it.  tests/test_tiles_ref.py shows on the CPU that the bound accepts the float32 restatement
and rejects every wrong variant.

    part[b][s][h] = sum over the list entries j of batch row b whose column lies in split s of
                    x_j W[col_j][h],     x_j = xval[lboff[b] + j] rounded to the compute dtype

Split s covers the 128-column tiles [s tiles_per, min(n_tiles, (s + 1) tiles_per)), tiles_per = ceil(n_tiles /
splits).  Rows b >= B, rows with rows[b] < 0 and empty splits are exactly 0.

Bound (nothing tuned): epilogue_ref.product_tol(K, mag) with K = max(nonzero products of the (row, split), 1) and
mag = sum |x||w|.  The product of two f16 or two bf16 values is exact in fp32 and an added zero is exact, so only
the fp32 additions of the nonzero products round; a (row, split) without a nonzero product has mag = 0, a bound
of 0, and must be exactly 0.

Values: half-integers in [-5, 5] (every value and every duplicate sum exact in f16 and bf16, so "add a run in
fp32, round once" and "add in the compute dtype" build the same X and one reference serves both forms); the
`rounding` case holds uniform reals and no doubly-nonzero duplicate, and its reference rounds xval to the
compute dtype (round to nearest even) before multiplying.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np

import epilogue_ref as R
from gather_ref import worst

BK, BM, EMAX, BUCKET, PK_CHUNK = 128, 256, 8, 1024, 1024      # ocf_tiles.hip: tile, row group, slow-path thresholds

# name -> tiles, splits, B, Bp, H, ldw; `heavy`: the tile where twelve rows hold 9 to 20 entries (and none in the
# tile after it); `fill`: every other free row of row group 0 holds 5 to 7 entries there (a bucket over 1,024 words)
CASES = {
    "one_tile":    dict(n_tiles=1, splits=1, B=256, Bp=256, H=128, ldw=128, heavy=0, fill=True),
    "deep7":       dict(n_tiles=7, splits=1, B=300, Bp=384, H=256, ldw=264, heavy=2, fill=True),
    "short_last":  dict(n_tiles=10, splits=3, B=200, Bp=256, H=128, ldw=136, heavy=5, fill=True),
    "empty_split": dict(n_tiles=5, splits=4, B=128, Bp=128, H=256, ldw=256, heavy=2),
    "xcd_round2":  dict(n_tiles=20, splits=10, B=64, Bp=128, H=128, ldw=128, heavy=16),
    "long_split":  dict(n_tiles=23, splits=2, B=37, Bp=128, H=512, ldw=512, heavy=5, long_row=1500),
    "h384":        dict(n_tiles=6, splits=1, B=128, Bp=128, H=384, ldw=392, heavy=3, scattered=True),
    "no_rows":     dict(n_tiles=3, splits=2, B=0, Bp=256, H=128, ldw=128, heavy=1),
    "rounding":    dict(n_tiles=7, splits=2, B=100, Bp=128, H=256, ldw=256, heavy=1, rounding=True),
}
NAMES = tuple(CASES)
EXACT_NAMES = tuple(n for n in NAMES if n != "rounding")        # the half-integer cases
DTYPES = ("f16", "bf16")

# batch rows with a fixed role (B >= 37 in every case with rows)
ROW_EDGE, ROW_ALLZERO, ROW_EMPTY, ROW_ONE, ROW_DUP, ROW_LONG = range(6)
ROWS_OVER = tuple(range(20, 32))
SCATTERED_NONE, SCATTERED_EMPTY = (7, 40, 41, 100), (6, 42, 99)
HALVES = np.array([v / 2.0 for v in range(-10, 11) if v], np.float32)


def tiles_per(c):
    return -(-c.n_tiles // c.splits)


def split_range(c, s):
    tp = tiles_per(c)
    return min(c.n_tiles, s * tp), min(c.n_tiles, (s + 1) * tp)


# ---- the fixture ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(name, seed=11):
    """Host arrays of one ocf_encoder_tiles call (read-only, cached): a small dataset CSR with rows the batch does
    not use, its column-sorted view, the batch (rows, lboff, xval) and W as float32 [n_tiles * 128][ldw]
    (weights_for rounds it to a compute dtype and sets the columns >= H to NaN)."""
    from omnidirectional_collaborative_filtering_amd.dataset import RatingsCSR
    p = CASES[name]
    rng = np.random.RandomState(seed + 7 * NAMES.index(name))
    n_tiles, B, heavy = p["n_tiles"], p["B"], p["heavy"]
    n_cols = BK if n_tiles == 1 else n_tiles * BK - 37
    rounding = bool(p.get("rounding"))
    none = set()
    empty = set()
    if B:
        none.add(B // 2)
        empty.add(ROW_EMPTY)
    if p.get("scattered"):
        none |= set(SCATTERED_NONE)
        empty |= set(SCATTERED_EMPTY)
    over = set(ROWS_OVER) if B else set()
    in_tile = lambda t: np.arange(t * BK, min((t + 1) * BK, n_cols))
    lists = []                                             # per batch row: (columns, values) in list order
    for b in range(B):
        if b in none or b in empty:
            lists.append((np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        fill = bool(p.get("fill")) and b < BM and b > ROW_LONG and b not in over
        allowed = np.ones(n_cols, bool)
        if b in over or fill:
            allowed[in_tile(heavy)] = False
        if b in over and heavy + 1 < n_tiles:
            allowed[in_tile(heavy + 1)] = False
        allowed = np.nonzero(allowed)[0]
        if b == ROW_EDGE:
            forced = [0, 127, 128, n_cols - 1] + [BK * k + d for k in range(1, n_tiles) for d in (-1, 0)]
            cols = np.unique([c for c in forced if c < n_cols])
        elif b == ROW_ONE:
            cols = rng.permutation(n_cols)[:1]
        elif b == ROW_LONG and p.get("long_row"):
            cols = rng.permutation(n_cols)[:p["long_row"]]
        else:
            n = min(int(rng.randint(2, 3 * n_tiles + 4)), len(allowed))
            cols = rng.permutation(allowed)[:n]
        if b in over:
            cols = np.concatenate([cols, rng.permutation(in_tile(heavy))[:rng.randint(9, 21)]])
        elif fill:
            cols = np.concatenate([cols, rng.permutation(in_tile(heavy))[:rng.randint(5, 8)]])
        cols = np.asarray(cols, np.int64)
        chain = []
        if b == ROW_DUP:                                   # runs of 2 and 3 equal columns, and the engine's chain of 3
            free = np.setdiff1d(np.arange(n_cols), cols)
            c1, c2, c3 = rng.permutation(free)[:3]
            cols = np.concatenate([cols, [c3] * 3] + ([] if rounding else [[c1] * 2, [c2] * 3]))
            chain = [int(c3)]
        cols = rng.permutation(cols)
        if rounding:
            x = rng.uniform(-5.0, 5.0, size=len(cols)).astype(np.float32)
        else:
            x = HALVES[rng.randint(0, len(HALVES), size=len(cols))]
        keep = rng.rand(len(cols)) >= 0.3
        if b == ROW_EDGE or b == ROW_DUP or b == ROW_ONE:
            keep[:] = True
        if b in over:
            keep[cols // BK == heavy] = True
        if b == ROW_ALLZERO:
            keep[:] = False
        x = np.where(keep, x, np.float32(0.0)).astype(np.float32)
        for c3 in chain:                                   # earlier entries zero, the last one live
            at = np.nonzero(cols == c3)[0]
            x[at[:-1]] = 0.0
        lists.append((cols, x))
    # the dataset: the batch's rows in shuffled order among five rows it does not use; its last row is batch row B - 1
    live = [b for b in range(B) if b not in none]
    n_ds = len(live) + 5
    rows = np.full(B, -1, np.int32)
    if live:
        where = rng.permutation(n_ds - 1)[:len(live) - 1]
        rows[live[:-1]] = where
        rows[live[-1]] = n_ds - 1
    ds_cols = [rng.permutation(n_cols)[:rng.randint(1, 10)].astype(np.int64) for _ in range(n_ds)]
    for b in live:
        ds_cols[rows[b]] = lists[b][0]
    ds_len = np.array([len(c) for c in ds_cols], np.int64)
    rp = np.zeros(n_ds + 1, np.int64)
    np.cumsum(ds_len, out=rp[1:])
    col = np.concatenate(ds_cols).astype(np.int32)
    val = HALVES[rng.randint(10, len(HALVES), size=len(col))].copy()       # the ratings themselves (not read)
    col_s, _, lidx_s, tptr = RatingsCSR(rp, col, val).tile_index(n_cols)
    lens = np.array([len(lists[b][0]) for b in range(B)], np.int64)
    lboff = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=lboff[1:])
    E = int(lboff[-1])
    xval = np.concatenate([lists[b][1] for b in range(B)] + [np.zeros(0 if E else 1, np.float32)]).astype(np.float32)
    W = (0.5 * rng.randn(n_tiles * BK, p["ldw"])).astype(np.float32)
    c = SimpleNamespace(name=name, n_tiles=n_tiles, splits=p["splits"], B=B, Bp=p["Bp"], H=p["H"], ldw=p["ldw"],
                        n_cols=n_cols, heavy=heavy, fill=bool(p.get("fill")), rounding=rounding, none=sorted(none),
                        empty=sorted(empty), over=sorted(over), rp=rp, col=col, val=val,
                        tcol=np.ascontiguousarray(col_s, np.int32), tlidx=np.ascontiguousarray(lidx_s, np.int32),
                        tptr=np.ascontiguousarray(tptr, np.int32), rows=rows, lboff=lboff, lens=lens, E=E, xval=xval,
                        W=W, nnz=len(col), n_entries=max(E, 1), max_row_len=max(int(lens.max()) if B else 0, 1))
    validate(c)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def variant(c, **kw):
    """a shallow copy of a case with some fields replaced (the CPU tests' broken fixtures)"""
    d = copy.copy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def entries(c):
    """per batch-local entry, in list order: batch row, position in its list, CSR position, column"""
    eb = np.repeat(np.arange(c.B), c.lens)
    ej = np.arange(c.E) - c.lboff[eb]
    src = c.rp[np.maximum(c.rows[eb], 0)] + ej
    return eb, ej, src, c.col[src].astype(np.int64)


def view_entries(c):
    """per entry of the batch rows' column-sorted views, rows in batch order: batch row, position p in the view,
    column, list index, tile, position in the (row, tile), word position in the (row group, tile) bucket"""
    vb = np.repeat(np.arange(c.B), c.lens)
    vp = np.arange(c.E) - c.lboff[vb]
    r = np.maximum(c.rows[vb], 0)
    at = c.rp[r] + vp
    vcol, vli = c.tcol[at].astype(np.int64), c.tlidx[at].astype(np.int64)
    vt = vcol // BK
    vk = vp - c.tptr[r, vt]
    key = (vb // BM) * c.n_tiles + vt                      # bucket; words in (row, view position) order
    order = np.argsort(key, kind="stable")
    first = np.zeros(len(key), np.int64)
    if len(key):
        ks = key[order]
        start = np.concatenate([[0], np.nonzero(np.diff(ks))[0] + 1])
        run = np.arange(len(ks)) - np.repeat(start, np.diff(np.concatenate([start, [len(ks)]])))
        first[order] = run
    return SimpleNamespace(b=vb, p=vp, col=vcol, li=vli, t=vt, k=vk, word=first)


def validate(c):
    """Everything the kernels rely on to stay in bounds, then the edges the fixture promises.  Every GPU test calls
    it before launching, so a fixture mistake is an assertion here and not an out-of-bounds read on the GPU."""
    n_ds = len(c.rp) - 1
    B, nt = c.B, c.n_tiles
    # -- ranges and shapes
    assert c.rp.dtype == np.int64 and c.lboff.dtype == np.int64 and c.rows.dtype == np.int32
    assert c.tcol.dtype == np.int32 and c.tlidx.dtype == np.int32 and c.tptr.dtype == np.int32
    assert c.xval.dtype == np.float32 and np.isfinite(c.xval).all()
    assert c.rp[0] == 0 and (np.diff(c.rp) >= 0).all() and c.rp[-1] == len(c.col) == len(c.tcol) == len(c.tlidx) == c.nnz
    assert c.nnz >= 1 and nt >= 1 and c.splits >= 1 and 0 <= B <= c.Bp and c.Bp % 128 == 0
    assert c.H % 128 == 0 and c.ldw >= c.H and c.ldw % 8 == 0 and tiles_per(c) <= 1024
    assert c.W.shape == (nt * BK, c.ldw) and nt == -(-c.n_cols // BK)
    assert len(c.rows) == B and ((c.rows >= -1) & (c.rows < n_ds)).all()
    assert ((c.col >= 0) & (c.col < c.n_cols)).all() and ((c.tcol >= 0) & (c.tcol < c.n_cols)).all()
    assert c.tptr.shape == (n_ds, nt + 1)
    ds_len = np.diff(c.rp)
    assert (c.tptr[:, 0] == 0).all() and (np.diff(c.tptr, axis=1) >= 0).all(), "tptr rows are not monotone"
    assert (c.tptr[:, -1] == ds_len).all(), "tptr rows do not end at the row length"
    for r in range(n_ds):
        s, e = int(c.rp[r]), int(c.rp[r + 1])
        li = c.tlidx[s:e]
        assert ((li >= 0) & (li < e - s)).all(), "tlidx out of range in row %d" % r
        assert np.array_equal(np.sort(li), np.arange(e - s)), "tlidx is no permutation of row %d" % r
        assert np.array_equal(c.tcol[s:e], c.col[s:e][li]) and (np.diff(c.tcol[s:e]) >= 0).all()
        # the tile pointers cut the sorted columns at the tile boundaries
        assert np.array_equal(c.tptr[r], np.searchsorted(c.tcol[s:e], np.arange(nt + 1) * BK))
    lens = np.where(c.rows >= 0, ds_len[np.maximum(c.rows, 0)], 0) if B else np.zeros(0, np.int64)
    assert len(c.lboff) == B + 1 and c.lboff[0] == 0 and np.array_equal(np.diff(c.lboff), lens)
    assert np.array_equal(lens, c.lens) and c.E == c.lboff[B]
    assert c.n_entries == max(int(c.lboff[B]), 1) == len(c.xval)
    assert c.max_row_len == max(int(lens.max()) if B else 0, 1)
    assert len(set(c.rows[c.rows >= 0].tolist())) == int((c.rows >= 0).sum())
    # -- the weights: finite and nonzero in every row, the rows at or beyond n_cols included
    assert np.isfinite(c.W).all() and (c.W != 0).all()
    if c.name != "one_tile":
        assert c.n_cols % BK != 0
    if B == 0:
        return
    # -- the promised edges
    eb, ej, src, ecol = entries(c)
    used = np.ones(n_ds, bool)
    used[c.rows[c.rows >= 0]] = False
    assert used.sum() == 5 and c.rows[B - 1] == n_ds - 1 and lens[B - 1] >= 1        # the clamps reach nnz - 1, E - 1
    assert list(c.rows[:-1][c.rows[:-1] >= 0]) != sorted(c.rows[:-1][c.rows[:-1] >= 0])   # shuffled
    at = lambda b: slice(int(c.lboff[b]), int(c.lboff[b + 1]))
    mid = B // 2
    assert c.rows[mid] == -1 and 0 < mid < B - 1 and all(c.rows[b] == -1 for b in c.none)
    assert all(c.rows[b] >= 0 and lens[b] == 0 for b in c.empty) and ROW_EMPTY in c.empty
    assert lens[ROW_ONE] == 1 and c.xval[at(ROW_ONE)][0] != 0
    assert lens[ROW_ALLZERO] >= 2 and not c.xval[at(ROW_ALLZERO)].any()
    free = np.ones(c.E, bool)
    for b in (ROW_EDGE, ROW_ALLZERO, ROW_ONE, ROW_DUP) + tuple(c.over):
        free[at(b)] = False
    assert 0.2 < (c.xval[free] == 0).mean() < 0.4
    # list order is not column order
    multi = [b for b in range(B) if lens[b] >= 3]
    assert np.mean([bool((np.diff(ecol[at(b)]) < 0).any()) for b in multi]) > 0.8
    # columns 0, 127, 128, the last real column, both sides of every tile boundary of one row, all live inputs
    edge = set(ecol[at(ROW_EDGE)].tolist())
    want = {0, 127, c.n_cols - 1} | {BK * k + d for k in range(1, nt) for d in (-1, 0) if BK * k + d < c.n_cols}
    assert want <= edge and (nt == 1 or 128 in edge) and c.xval[at(ROW_EDGE)].all() and ecol.max() == c.n_cols - 1
    # duplicates: runs of 2 and 3 with every value nonzero (not in the rounding case), the engine's chain
    cols_d, x_d = ecol[at(ROW_DUP)], c.xval[at(ROW_DUP)]
    u, n = np.unique(cols_d, return_counts=True)
    runs = sorted(n[n > 1].tolist())
    assert runs == ([3] if c.rounding else [2, 3, 3])
    full = sorted(int(k) for col_, k in zip(u, n) if k > 1 and x_d[cols_d == col_].all())
    chains = [col_ for col_, k in zip(u, n) if k > 1 and not x_d[cols_d == col_][:-1].any() and x_d[cols_d == col_][-1] != 0]
    assert full == ([] if c.rounding else [2, 3]) and len(chains) == 1
    for b in range(B):
        if b != ROW_DUP:
            assert len(np.unique(ecol[at(b)])) == lens[b]
    # values
    if c.rounding:
        assert (c.xval * 2 != np.round(c.xval * 2)).mean() > 0.6
    else:
        assert (c.xval * 2 == np.round(c.xval * 2)).all() and np.abs(c.xval).max() <= 5
    # the heavy tile: twelve rows over EMAX entries there and none in the tile after it
    h = c.heavy
    cnt = np.zeros((B, nt), np.int64)
    np.add.at(cnt, (eb, ecol // BK), 1)
    assert len(c.over) == 12 and all(9 <= cnt[b, h] <= 20 for b in c.over) and max(cnt[b, h] for b in c.over) > 12
    assert all(c.xval[at(b)][ecol[at(b)] // BK == h].all() for b in c.over)
    if h + 1 < nt:
        assert all(cnt[b, h + 1] == 0 for b in c.over)
    if c.fill:
        role = set(range(ROW_LONG + 1)) | set(c.over) | set(c.none) | set(c.empty)
        rest = [b for b in range(min(B, BM)) if b not in role]
        assert all(5 <= cnt[b, h] <= 7 for b in rest) and cnt[:BM, h].sum() > BUCKET
    if c.name == "long_split":
        assert lens[ROW_LONG] > PK_CHUNK and c.max_row_len == lens[ROW_LONG]
    assert c.E <= 6000


@functools.lru_cache(maxsize=None)
def weights_for(name, wt):
    """(the 16-bit patterns of W [n_tiles * 128][ldw] rounded to wt with NaN in the columns >= H, the rounded values
    [n_tiles * 128][H] as float64)"""
    import torch
    c = make_case(name)
    td = {"f16": torch.float16, "bf16": torch.bfloat16}[wt]
    t = torch.from_numpy(np.array(c.W)).to(td)
    Wr = t[:, :c.H].float().numpy().astype(np.float64)
    assert (Wr == 0).mean() < 1e-4 and (np.sign(Wr) > 0).mean() > 0.4 and (np.sign(Wr) < 0).mean() > 0.4   # mixed sign
    t[:, c.H:] = float("nan")
    bits = t.view(torch.int16).numpy().copy()
    bits.setflags(write=False)
    Wr.setflags(write=False)
    return bits, Wr


def x_rounded(c, wt):
    """xval as the MFMA operand: unchanged in the half-integer cases (asserted), rounded to nearest even otherwise"""
    xr = R.round_to(np.array(c.xval), wt)
    if not c.rounding:
        assert np.array_equal(xr, c.xval)
    return xr.astype(np.float64)


# ---- fp64 references ---------------------------------------------------------------------------------------------
def ref_partials(c, wt):
    """(ref [Bp][S][H], mag = sum |x||w|, nterms [Bp][S] = nonzero products' entries) from the raw list entries"""
    _, Wr = weights_for(c.name, wt)
    S, H = c.splits, c.H
    ref = np.zeros((c.Bp * S, H))
    mag = np.zeros((c.Bp * S, H))
    nterms = np.zeros(c.Bp * S, np.int64)
    if c.E:
        eb, _, _, ecol = entries(c)
        x = x_rounded(c, wt)[:c.E]
        key = eb * S + (ecol // BK) // tiles_per(c)
        terms = x[:, None] * Wr[ecol]
        np.add.at(ref, key, terms)
        np.add.at(mag, key, np.abs(terms))
        np.add.at(nterms, key, (x != 0).astype(np.int64))
    return ref.reshape(c.Bp, S, H), mag.reshape(c.Bp, S, H), nterms.reshape(c.Bp, S)


def ref_dense(c, wt):
    """the same partials from a dense X built from the column-sorted view: X[:, tiles of s] @ W[tiles of s]"""
    _, Wr = weights_for(c.name, wt)
    X = np.zeros((c.Bp, c.n_tiles * BK))
    if c.E:
        v = view_entries(c)
        np.add.at(X, (v.b, v.col), x_rounded(c, wt)[c.lboff[v.b] + v.li])
    out = np.zeros((c.Bp, c.splits, c.H))
    for s in range(c.splits):
        t0, t1 = split_range(c, s)
        out[:, s] = X[:, t0 * BK:t1 * BK] @ Wr[t0 * BK:t1 * BK]
    return out


def bound(c, wt):
    """(ref, tol) of part[:Bp, :S, :H]"""
    ref, mag, nterms = ref_partials(c, wt)
    return ref, R.product_tol(np.maximum(nterms, 1)[:, :, None], mag)


def zero_rows(c):
    """batch rows whose partials are exactly 0 in every split: b >= B, rows[b] < 0, zero-length rows"""
    z = np.ones(c.Bp, bool)
    z[:c.B] = (c.rows < 0) | (c.lens == 0)
    return z


def check(c, wt, got):
    """(worst |got - ref| / bound over every element of part[:Bp, :S, :H], its index); a NaN is infinite"""
    ref, tol = bound(c, wt)
    got = np.asarray(got)
    assert got.shape == ref.shape
    return worst(got, ref, tol)


# ---- float32 restatement, tile by tile, and its wrong variants ---------------------------------------------------
WRONG = {
    1: "entries past the 8th of a (row, tile) dropped",
    2: "X image not cleared after the heavy tile",
    3: "duplicates last-write-wins instead of added",
    4: "xval truncated instead of rounded to nearest even",
    5: "a split boundary one tile off",
    6: "rows >= B repeat row 0's result",
    7: "tlidx ignored (values taken in view order)",
    8: "in-tile columns of the wrong tile on the last tile of a split",
    9: "words past 1,024 of a bucket dropped",
    10: "entries past position 1,023 of a row dropped",
}
# the case that shows each (tests/test_tiles_ref.py asserts the rejection there)
WRONG_AT = {1: "deep7", 2: "deep7", 3: "short_last", 4: "rounding", 5: "short_last", 6: "deep7", 7: "h384",
            8: "xcd_round2", 9: "deep7", 10: "long_split"}


def truncate_to(x, wt):
    """float32 -> wt by dropping the low mantissa bits (toward zero)"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if wt == "bf16":
        return (bits & np.uint32(0xFFFF0000)).view(np.float32)
    return (bits & np.uint32(0xFFFFE000)).view(np.float32)      # f16: 10 of fp32's 23 mantissa bits (normal range)


def twin(c, wt, wrong=None):
    """part [Bp][S][H] in float32: a dense float32 X per tile from the view, one float32 product per tile, the
    tiles of a split accumulated in order; `wrong` (a key of WRONG): one deliberate bug"""
    f = np.float32
    _, Wr = weights_for(c.name, wt)
    W = Wr.astype(f)
    S, H, nt = c.splits, c.H, c.n_tiles
    X = np.zeros((c.Bp, nt * BK), f)
    if c.E:
        v = view_entries(c)
        src = c.lboff[v.b] + (v.p if wrong == 7 else v.li)
        xv = np.array(c.xval)[src]
        x = truncate_to(xv, wt) if wrong == 4 else R.round_to(xv, wt)
        keep = np.ones(len(x), bool)
        if wrong == 1:
            keep = v.k < EMAX
        if wrong == 9:
            keep = v.word < BUCKET
        if wrong == 10:
            keep = v.p < PK_CHUNK
        if wrong == 3:
            X[v.b[keep], v.col[keep]] = x[keep]            # (view order = list order within a run: the last wins)
        else:
            np.add.at(X, (v.b[keep], v.col[keep]), x[keep])
    out = np.zeros((c.Bp, S, H), f)
    for s in range(S):
        t0, t1 = split_range(c, s)
        if wrong == 5 and s > 0:
            t0 = min(nt, t0 + 1)
        if wrong == 5 and s + 1 < S and t1 < nt:
            t1 = t1 + 1
        acc = np.zeros((c.Bp, H), f)
        for t in range(t0, t1):
            tx = t - 1 if (wrong == 8 and t == t1 - 1 and t > 0) else t
            Xt = X[:, tx * BK:(tx + 1) * BK]
            if wrong == 2 and t == c.heavy + 1 and t > t0:
                Xt = Xt + X[:, (t - 1) * BK:t * BK]
            acc = acc + np.matmul(Xt, W[t * BK:(t + 1) * BK]).astype(f)
        out[:, s] = acc
    if wrong == 6 and c.B:
        out[c.B:] = out[0]
    return out
