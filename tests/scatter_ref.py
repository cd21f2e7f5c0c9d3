"""NumPy restatements of the batch scatter (include/ocf.h OcfScatterArgs / OcfEpochScatterArgs,
csrc/ocf_scatter.hip): the small hand-built batches the GPU tests launch it on (tests/test_scatter_direct_gpu.py),
a per-rating reference loop in the statement order of the reference reader (data_reader.py:158-169 train,
:234-268 eval), the device reciprocal split in float32 and float64, a second restatement that works the way the
kernel does (`twin`: per entry, through find_row, the duplicate chain and role1) and a list of deliberately wrong
variants of it.  tests/test_scatter_ref.py shows on the CPU that the fixtures hold the edges they are meant to hold,
that the twin equals the reference and that every wrong variant is rejected by an output the GPU test compares.

Everything the scatter writes is a copy of an input or a constant, so every comparison is exact; the only
arithmetic is the device split's row threshold (device_split), restated one float32 operation at a time.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from mlp_ref import philox_uniform

SC_THREADS = 1024                 # ocf_scatter.hip: entries per workgroup of scatter_flat_kernel / bucket_fill_kernel
SE_U = 4                          # entries per thread of scatter_epoch_kernel
SPLIT_GAP = 2.0 ** -22            # no draw this close to its row's threshold, no row share this close to 0 or 1

# duplicate chains planted into a row of >= 33 entries: list positions sharing one column, and which of them are
# kept (K: input) or dropped (D: target).  Lengths 2, 3 and 4.
CHAINS = [((0, 5), "KD"), ((1, 6), "DK"), ((2, 7), "KK"), ((3, 8), "DD"),
          ((10, 14, 18), "KDK"), ((11, 15, 19), "DKD"), ((12, 16, 20), "KKD"), ((13, 17, 21), "DDK"),
          ((22, 25, 28, 31), "KDDK"), ((23, 26, 29, 32), "DKKD")]
DUP_LEN = 40


# ---- building blocks ---------------------------------------------------------------------------------------
def dup_chain(rp, col):
    """next[i] = the next entry of the same row with the same column, else -1; None without duplicates"""
    nxt = np.full(len(col), -1, np.int32)
    found = False
    for r in range(len(rp) - 1):
        last = {}
        for i in range(int(rp[r + 1]) - 1, int(rp[r]) - 1, -1):
            c = int(col[i])
            if c in last:
                nxt[i] = last[c]
                found = True
            last[c] = i
    return nxt if found else None


def _ratings(rng, n):
    """half-star ratings + 1/3: no value is representable in 16 bits"""
    return (rng.randint(1, 11, size=n) / 2.0 + 1.0 / 3.0).astype(np.float32)


def _csr(rng, ds_len, N, forced=None):
    """a CSR of len(ds_len) rows, each a random set of distinct columns in random list order"""
    rp = np.zeros(len(ds_len) + 1, np.int64)
    np.cumsum(ds_len, out=rp[1:])
    col = np.zeros(rp[-1], np.int32)
    for r, n in enumerate(ds_len):
        if N > 4096:
            c = np.unique(rng.randint(0, N, size=2 * n + 16))
            c = rng.permutation(c)[:n]
        else:
            c = rng.permutation(N)[:n]
        if forced and r in forced:
            f = np.asarray(forced[r], np.int64)
            c = rng.permutation(np.concatenate([f, np.setdiff1d(c, f)[:n - len(f)]]))
        assert len(c) == n and len(np.unique(c)) == n
        col[rp[r]:rp[r + 1]] = c
    return rp, col, _ratings(rng, int(rp[-1]))


def _plant(col, val, start, chains=CHAINS):
    """make the listed positions of the row starting at CSR index `start` share their first position's column,
    with distinct ratings along each chain"""
    for pos, _ in chains:
        for k, p in enumerate(pos):
            col[start + p] = col[start + pos[0]]
            val[start + p] = np.float32(0.5 * (k + 1) + 0.5 * (pos[0] % 3) + 1.0 / 3.0)


def _entries(rp, rows, lboff):
    """batch row, list position and CSR index of every batch-local entry"""
    lens = np.diff(lboff)
    eb = np.repeat(np.arange(len(rows)), lens)
    ej = np.arange(int(lboff[-1])) - lboff[eb]
    ei = rp[np.maximum(rows[eb], 0)] + ej
    return eb, ej, ei


def _offsets(rp, rows):
    lens = np.where(rows >= 0, rp[np.maximum(rows, 0) + 1] - rp[np.maximum(rows, 0)], 0)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _freeze(c):
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def replace(c, **kw):
    d = dict(vars(c))
    d.update(kw)
    return SimpleNamespace(**d)


def _train_case(name, rng, B, B_pad, N, ld, lens, neg_rows=(), dup_rows=(), pre=37, zeros=6, forced=None, extra=6,
                p_keep=0.6):
    """a train-mode batch (mode 0) over a dataset CSR of B + extra rows, the batch rows a shuffled subset; host
    keep flags in keep1 at boff1 = pre + the local offsets"""
    lens = np.asarray(lens, np.int64)
    n_ds = B + extra
    ds_of = rng.permutation(n_ds)[:B]
    ds_len = rng.randint(1, 30, size=n_ds)
    ds_len[ds_of] = lens
    for b in neg_rows:
        ds_len[ds_of[b]] = 9                      # the dataset row has entries; rows1 = -1 is what empties it
    rp, col, val = _csr(rng, ds_len, N, {int(ds_of[b]): f for b, f in (forced or {}).items()})
    for b in dup_rows:
        assert lens[b] >= 33
        _plant(col, val, int(rp[ds_of[b]]))
    rows = ds_of.astype(np.int32)
    for b in neg_rows:
        rows[b] = -1
    lboff = _offsets(rp, rows)
    E = int(lboff[-1])
    eb, ej, ei = _entries(rp, rows, lboff)
    keep = (rng.rand(E) < p_keep)
    chain_e = np.zeros(E, bool)
    for b in dup_rows:
        for pos, pat in CHAINS:
            for p, k in zip(pos, pat):
                keep[lboff[b] + p] = k == "K"
                chain_e[lboff[b] + p] = True
    free = np.nonzero(~chain_e)[0]
    if zeros:
        val[ei[rng.permutation(free)[:zeros]]] = 0.0
    keep1 = (rng.rand(pre + E + 50) < 0.5).astype(np.uint8)
    keep1[pre:pre + E] = keep
    return SimpleNamespace(
        name=name, mode=0, pass_through=1, B=B, B_pad=B_pad, N=N, ld=ld, aux=-1.0, rp1=rp, col1=col, val1=val,
        dup1=dup_chain(rp, col), rows1=rows, lboff1=lboff, boff1=lboff + pre, pos1=None, keep1=keep1, s0=1.0, s1=1.0,
        seed=0, stream=0, E1=E, E2=0, rp2=None, col2=None, val2=None, dup2=None, rows2=None, lboff2=None,
        n_tiles=(N + 127) // 128, tb_nk=(B + 63) // 64, eb=eb, epos=ej, ei=ei, keep_ref=keep.astype(np.uint8),
        dup_rows=tuple(dup_rows))


# ---- fixtures ----------------------------------------------------------------------------------------------
T_EMPTY = (0, 30, 31, 69)         # train: empty rows first, two in a row in the middle (31 is rows1 = -1), last
T_ONE, T_TWO, T_LONG, T_DUP = 3, 4, 33, 40


@functools.lru_cache(maxsize=None)
def train(pass_through=1):
    rng = np.random.RandomState(11)
    B = 70
    lens = rng.randint(20, 56, size=B)
    lens[list(T_EMPTY)] = 0
    lens[T_ONE], lens[T_TWO], lens[T_LONG], lens[T_DUP] = 1, 2, 290, DUP_LEN
    c = _train_case("train", rng, B, 72, 300, 304, lens, neg_rows=(31,), dup_rows=(T_DUP,),
                    forced={T_LONG: [0, 127, 128, 255, 256, 299]})
    return _freeze(replace(c, pass_through=pass_through, name="train-pt%d" % pass_through))


E_NOIN, E_NOTGT, E_NONE, E_DUP2, E_DUP1 = 5, 9, 17, 20, 22


@functools.lru_cache(maxsize=None)
def eval_case():
    """mode 1: two CSRs over the same dataset rows (inputs, targets), rows1 = -1 where the input is None"""
    rng = np.random.RandomState(12)
    B, N = 40, 300
    n_ds = B + 6
    ds_of = rng.permutation(n_ds)[:B]
    len1, len2 = rng.randint(1, 30, size=n_ds), rng.randint(1, 30, size=n_ds)
    len1[ds_of], len2[ds_of] = rng.randint(30, 48, size=B), rng.randint(30, 48, size=B)
    len2[ds_of[[E_NOTGT, E_NONE]]] = 0
    len2[ds_of[E_DUP2]], len1[ds_of[E_DUP1]] = DUP_LEN, DUP_LEN
    rp1, rp2 = np.zeros(n_ds + 1, np.int64), np.zeros(n_ds + 1, np.int64)
    np.cumsum(len1, out=rp1[1:])
    np.cumsum(len2, out=rp2[1:])
    col1, col2 = np.zeros(rp1[-1], np.int32), np.zeros(rp2[-1], np.int32)
    for r in range(n_ds):
        perm = rng.permutation(N)
        col1[rp1[r]:rp1[r + 1]] = perm[:len1[r]]
        lo = max(len1[r] - 3, 0)                  # the sources overlap in three cells of the row
        col2[rp2[r]:rp2[r + 1]] = rng.permutation(perm[lo:lo + len2[r]])
    val1, val2 = _ratings(rng, len(col1)), _ratings(rng, len(col2))
    _plant(col2, val2, int(rp2[ds_of[E_DUP2]]), CHAINS[:1] + CHAINS[4:5] + CHAINS[8:9])
    _plant(col1, val1, int(rp1[ds_of[E_DUP1]]), CHAINS[1:2] + CHAINS[5:6])
    val1[rp1[ds_of[0]] + 1] = 0.0
    val2[rp2[ds_of[0]] + 2] = 0.0
    rows2 = ds_of.astype(np.int32)
    rows1 = rows2.copy()
    rows1[[E_NOIN, E_NONE]] = -1
    lboff1, lboff2 = _offsets(rp1, rows1), _offsets(rp2, rows2)
    eb, ej, ei = _entries(rp1, rows1, lboff1)
    return _freeze(SimpleNamespace(
        name="eval", mode=1, pass_through=0, B=B, B_pad=B, N=N, ld=304, aux=2.5, rp1=rp1, col1=col1, val1=val1,
        dup1=dup_chain(rp1, col1), rows1=rows1, lboff1=lboff1, boff1=lboff1, pos1=None, keep1=None, s0=1.0, s1=1.0,
        seed=0, stream=0, E1=int(lboff1[-1]), E2=int(lboff2[-1]), rp2=rp2, col2=col2, val2=val2,
        dup2=dup_chain(rp2, col2), rows2=rows2, lboff2=lboff2, n_tiles=3, tb_nk=1, eb=eb, epos=ej, ei=ei,
        keep_ref=np.ones(int(lboff1[-1]), np.uint8), dup_rows=()))


SHARD_CUTS = ((0, 140), (140, 300))


@functools.lru_cache(maxsize=None)
def shards(pass_through=1):
    """the train fixture cut into two column shards: the columns of [lo, hi) with local index c - lo, pos1 = the
    entry's position in the full row, lboff1 = shard-local offsets, boff1 = the full rows' keep offsets; src_e =
    each shard entry's index in the full batch"""
    full = train(pass_through)
    out = []
    for lo, hi in SHARD_CUTS:
        n_ds = len(full.rp1) - 1
        sel = np.nonzero((full.col1 >= lo) & (full.col1 < hi))[0]
        ds_row = np.repeat(np.arange(n_ds), np.diff(full.rp1))
        rp = np.zeros(n_ds + 1, np.int64)
        np.cumsum(np.bincount(ds_row[sel], minlength=n_ds), out=rp[1:])
        col = (full.col1[sel] - lo).astype(np.int32)
        pos = (sel - full.rp1[ds_row[sel]]).astype(np.int32)
        lboff = _offsets(rp, full.rows1)
        eb, ej, ei = _entries(rp, full.rows1, lboff)
        src_e = full.lboff1[eb] + pos[ei]
        N = hi - lo
        out.append(_freeze(replace(
            full, name="shard[%d,%d)-pt%d" % (lo, hi, pass_through), N=N, ld=(N + 3) // 4 * 4, rp1=rp, col1=col,
            val1=full.val1[sel].copy(), dup1=dup_chain(rp, col), lboff1=lboff, pos1=pos, E1=int(lboff[-1]),
            n_tiles=(N + 127) // 128, eb=eb, epos=pos[ei].astype(np.int64), ei=ei, keep_ref=full.keep_ref[src_e].copy(),
            src_e=src_e, col_lo=lo)))
    return tuple(out)


W_N = 131072 + 128 + 5


@functools.lru_cache(maxsize=None)
def wide():
    rng = np.random.RandomState(13)
    edge = [0, 127, 128, 131071, 131072, 131199, 131200, W_N - 1]
    c = _train_case("wide", rng, 4, 4, W_N, (W_N + 3) // 4 * 4, [700, 0, 800, 1500], dup_rows=(3,), forced={0: edge})
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def many_rows(B=8192):
    """B = 8,192: the first offset table past 64 KB; B = 16,384: the largest batch the entry point admits"""
    rng = np.random.RandomState(14)
    c = _train_case("many_rows" if B == 8192 else "many_rows-%d" % B, rng, B, B, 64, 64,
                    (rng.rand(B) < 3000.0 / B).astype(np.int64), pre=5, zeros=3, extra=40)
    return _freeze(c)


EP_B, EP_SEL, EP_EBASE0, EP_STREAM_MUL, EP_SEED = 48, (2, 0, 1), 1000, 2, 77


@functools.lru_cache(maxsize=None)
def epoch(pass_through=1):
    """three batches of one plan over one dataset CSR: the per-batch cases (what the reference reads) and the
    plan-wide tables ocf_epoch_scatter takes"""
    rng = np.random.RandomState(15)
    B, N, nb = EP_B, 300, 3
    lens = [rng.randint(92, 112, size=B), rng.randint(5, 25, size=B), rng.randint(30, 50, size=B)]
    n_ds = nb * B + 5
    order = rng.permutation(n_ds)
    ds_len = rng.randint(1, 30, size=n_ds)
    dup_b, neg_b = 7, B - 1
    for k in range(nb):
        lens[k][dup_b] = DUP_LEN
        lens[k][[0, 20]] = 0
        ds_len[order[k * B:(k + 1) * B]] = lens[k]
    rp, col, val = _csr(rng, ds_len, N)
    for k in range(nb):
        _plant(col, val, int(rp[order[k * B + dup_b]]))
    dup = dup_chain(rp, col)
    rows = order[:nb * B].astype(np.int32).reshape(nb, B).copy()
    rows[:, neg_b] = -1                            # the padding row
    lboff = np.stack([_offsets(rp, rows[k]) for k in range(nb)])
    E = lboff[:, -1]
    pre = np.array([11, 3, 29], np.int64)
    keep_off = np.zeros(nb, np.int64)
    keep_off[1:] = np.cumsum(pre + E + 13)[:-1]
    keep1 = (rng.rand(int(keep_off[-1] + pre[-1] + E[-1] + 64)) < 0.5).astype(np.uint8)
    cases = []
    for k in range(nb):
        eb, ej, ei = _entries(rp, rows[k], lboff[k])
        keep = rng.rand(int(E[k])) < 0.6
        for pos, pat in CHAINS:
            for p, kk in zip(pos, pat):
                keep[lboff[k, dup_b] + p] = kk == "K"
        keep1[keep_off[k] + pre[k]:keep_off[k] + pre[k] + E[k]] = keep
        cases.append(SimpleNamespace(
            name="epoch-b%d-pt%d" % (k, pass_through), mode=0, pass_through=pass_through, B=B, B_pad=B, N=N, ld=304,
            aux=-1.0, rp1=rp, col1=col, val1=val, dup1=dup, rows1=rows[k], lboff1=lboff[k], boff1=lboff[k] + pre[k],
            pos1=None, keep1=None, s0=1.0, s1=1.0, seed=0, stream=0, E1=int(E[k]), E2=0, rp2=None, col2=None, val2=None,
            dup2=None, rows2=None, lboff2=None, n_tiles=3, tb_nk=1, eb=eb, epos=ej, ei=ei,
            keep_ref=keep.astype(np.uint8), dup_rows=(dup_b,)))
    for k in range(nb):
        cases[k].keep1 = keep1[keep_off[k]:]
        _freeze(cases[k])
    sel = np.array(EP_SEL, np.int32)
    ebase = np.zeros(len(sel) + 1, np.int64)
    ebase[0] = EP_EBASE0
    ebase[1:] = EP_EBASE0 + np.cumsum(E[sel])
    return _freeze(SimpleNamespace(
        name="epoch-pt%d" % pass_through, cases=tuple(cases), B=B, N=N, nb=nb, pass_through=pass_through, rp1=rp,
        col1=col, val1=val, dup1=dup, rows1=rows.reshape(-1), lboff1=lboff.reshape(-1),
        boff1=(lboff + pre[:, None]).reshape(-1), keep1=keep1, keep_off=keep_off, sel=sel, ebase=ebase,
        ebase0=EP_EBASE0, max_e=int(E.max()), total=int(E[sel].sum())))


# ---- the device split ----------------------------------------------------------------------------------------
DEV_SEED, DEV_STREAM = 2024, 6    # the GPU tests' device split (a seed violating test_scatter_ref's conditions is replaced)
DEV_RANGES = ((0.3, 0.7), (0.5, 0.5))


def row_cut(seed, stream, s0, s1, B, dtype=np.float32):
    """ocf_scatter.hip row_cut: (the row's uniform, its share s, its threshold), one operation at a time in `dtype`
    (the library is built with -ffp-contract=off).  s0 / s1 are the struct's floats in either case."""
    f = dtype
    u = philox_uniform(seed, stream, np.arange(B, dtype=np.uint64)).astype(f)
    lo, hi = f(np.float32(s0)), f(np.float32(s1))
    d = f(hi - lo)
    s = (lo + (d * u).astype(f)).astype(f)
    om = (f(1.0) - s).astype(f)
    den = (om + s).astype(f)
    return u, s, (om / den).astype(f)


def device_split(c, s0, s1, seed, stream, entry_stream=None):
    """the keep flag of every batch-local entry under the device RNG (keep1 == NULL): keep = u_e >= cut_b with
    u_e = philox(seed, stream + 1, boff1[b] + position in the full row); all kept when s0 >= 1.  Returns the flags
    from the float32 thresholds, those from the float64 thresholds, the entries' draws and the float64 rows"""
    if np.float32(s0) >= np.float32(1.0):
        one = np.ones(c.E1, np.uint8)
        return SimpleNamespace(keep=one, keep64=one, u=None, s64=None, cut64=None)
    _, _, cut32 = row_cut(seed, stream, s0, s1, c.B, np.float32)
    _, s64, cut64 = row_cut(seed, stream, s0, s1, c.B, np.float64)
    idx = (c.boff1[c.eb] + c.epos).astype(np.uint64)
    u = philox_uniform(seed, stream + 1 if entry_stream is None else entry_stream, idx)
    return SimpleNamespace(keep=(u >= cut32[c.eb]).astype(np.uint8),
                           keep64=(u.astype(np.float64) >= cut64[c.eb]).astype(np.uint8), u=u, s64=s64, cut64=cut64)


def with_device_split(c, s0, s1, seed, stream):
    """the case with keep1 == NULL and the device split's flags as the reference's keep flags"""
    return replace(c, name="%s-dev(%g,%g)" % (c.name, s0, s1), keep1=None, s0=float(s0), s1=float(s1), seed=seed,
                   stream=stream, keep_ref=device_split(c, s0, s1, seed, stream).keep)


def kept_count_bound(s, lens):
    """|kept - sum_b s_b len_b| of the reference's choice([0, 1], p=[1 - s, s]) law, row shares s given: 6 standard
    deviations of the sum of independent Bernoulli(s_b) draws (two-sided tail 2e-9) + the 2^-24 grid of the
    24-bit uniform per entry"""
    s, lens = np.asarray(s, np.float64), np.asarray(lens, np.float64)
    return 6.0 * np.sqrt(float((s * (1.0 - s) * lens).sum())) + 2.0 ** -24 * float(lens.sum())


# ---- the reference: a per-rating loop in the reference reader's statement order ----------------------------------
def reference(c, keep=None):
    """data_reader.py:158-169 (mode 0) / :234-268 (mode 1) over a CSR plus rows (-1: an empty row), explicit keep
    flags per batch-local source-1 entry"""
    keep = c.keep_ref if keep is None else keep
    B, N, aux = c.B, c.N, float(np.float32(c.aux))
    X, Min, Mout, T, Mmiss = (np.zeros((B, N)) for _ in range(5))
    lastX, lastT = np.full((B, N), -1, np.int64), np.full((B, N), -1, np.int64)
    e1b, e1c, e1v = [], [], []
    e2b, e2c = [], []
    e = 0
    for b in range(B):
        r = int(c.rows1[b])
        if r >= 0:
            for i in range(int(c.rp1[r]), int(c.rp1[r + 1])):
                item, rating = int(c.col1[i]), float(c.val1[i])
                if c.mode == 0:
                    if keep[e]:
                        Min[b, item] = aux
                        X[b, item] = rating
                        lastX[b, item] = e
                        if c.pass_through:
                            Mout[b, item] = aux
                            T[b, item] = rating
                            lastT[b, item] = e
                    else:
                        Mout[b, item] = aux
                        T[b, item] = rating
                        lastT[b, item] = e
                    Mmiss[b, item] = aux
                else:
                    Min[b, item] = aux
                    X[b, item] = rating
                    lastX[b, item] = e
                    Mmiss[b, item] = aux
                e1b.append(b)
                e1c.append(item)
                e1v.append(rating)
                e += 1
    assert e == c.E1
    e = 0
    if c.mode == 1:
        for b in range(B):
            r = int(c.rows2[b])
            if r < 0:
                continue
            for i in range(int(c.rp2[r]), int(c.rp2[r + 1])):
                item, rating = int(c.col2[i]), float(c.val2[i])
                Mout[b, item] = aux
                T[b, item] = rating
                lastT[b, item] = e
                Mmiss[b, item] = aux
                e2b.append(b)
                e2c.append(item)
                e += 1
        assert e == c.E2
    e1b, e1c = np.array(e1b, np.int64), np.array(e1c, np.int64)
    e2b, e2c = np.array(e2b, np.int64), np.array(e2c, np.int64)
    ids1, ids2 = np.arange(len(e1b)), np.arange(len(e2b))
    o = SimpleNamespace(X=X, Min=Min, Mout=Mout, T=T, Mmiss=Mmiss, lastX=lastX, lastT=lastT)
    live_x = lastX[e1b, e1c] == ids1
    o.xval1 = np.where(live_x, np.array(e1v, np.float32), np.float32(0.0)).astype(np.float32)
    if c.mode == 0:
        live_t = lastT[e1b, e1c] == ids1
        o.tflag1, o.tflag2 = live_t.astype(np.uint8), np.zeros(0, np.uint8)
    else:
        o.tflag1 = np.zeros(len(e1b), np.uint8)
        o.tflag2 = (lastT[e2b, e2c] == ids2).astype(np.uint8)
    o.live_in = np.zeros(N, bool)
    o.live_in[e1c[live_x]] = True
    o.live_out = np.zeros(N, bool)
    if c.mode == 0:
        o.live_out[e1c[live_t]] = True
    o.ecb = (e1c | (e1b << 19)).astype(np.int32) if B <= 4096 else np.zeros(len(e1b), np.int32)
    o.col_cnt = (np.bincount(e1c, minlength=N) if B <= 4096 else np.zeros(N)).astype(np.int32)
    o.tb_cnt = np.bincount((e1c >> 7) * c.tb_nk + (e1b >> 6), minlength=c.n_tiles * c.tb_nk).astype(np.int32)
    tb, tc = np.nonzero(lastT >= 0)
    o.bk = _buckets(c.n_tiles, tc >> 7, (tb << 7) | (tc & 127), T[tb, tc], aux)
    return o


def _buckets(n_tiles, tile, rc, t, aux):
    """(bk_ptr [n_tiles + 1], the triples (rc, t, aux) sorted within each tile)"""
    tile, rc, t = np.asarray(tile, np.int64), np.asarray(rc, np.int64), np.asarray(t, np.float32)
    ptr = np.zeros(n_tiles + 1, np.int64)
    np.cumsum(np.bincount(tile, minlength=n_tiles)[:n_tiles], out=ptr[1:])
    order = np.lexsort((t, rc, tile))
    tri = np.stack([rc[order].astype(np.float64), t[order].astype(np.float64), np.full(len(order), float(aux))], 1)
    return SimpleNamespace(ptr=ptr.astype(np.int32), tri=tri)


def sort_buckets(n_tiles, bk_ptr, bk_rc, bk_t, bk_m):
    """device bucket arrays -> the triples sorted within each tile (the order inside a tile comes from atomics)"""
    ptr = np.asarray(bk_ptr, np.int64)
    n = int(ptr[n_tiles])
    tile = np.searchsorted(ptr[1:n_tiles + 1], np.arange(n), side="right")
    order = np.lexsort((np.asarray(bk_t[:n], np.float32), np.asarray(bk_rc[:n], np.int64), tile))
    return np.stack([np.asarray(bk_rc[:n], np.float64)[order], np.asarray(bk_t[:n], np.float64)[order],
                     np.asarray(bk_m[:n], np.float64)[order]], 1)


def xin_blocks(feed, both):
    """blocks of the layer-0 input the kernel addresses: ratings, block 1 under any feed, block 2 under `both`"""
    return 3 if both else (2 if feed else 1)


def xin_image(x, m_in, m_miss, feed, both, xb):
    """the layer-0 input [B][k * xb] as fp32: block 0 the ratings, block 1 M_in (feed 1) / M_miss (feed 2) / zeros
    (feed 3), block 2 M_miss (both)"""
    B, N = x.shape
    img = np.zeros((B, xin_blocks(feed, both) * xb), np.float32)
    img[:, :N] = x
    if feed == 1:
        img[:, xb:xb + N] = m_in
    if feed == 2:
        img[:, xb:xb + N] = m_miss
    if both:
        img[:, 2 * xb:2 * xb + N] = m_miss
    return img


# ---- the twin: per entry, the way the kernel works, and its wrong variants -----------------------------------------
WRONG = {
    1: "the duplicate chain is ignored: every duplicate writes",
    2: "the first duplicate wins instead of the last",
    3: "later_in used where later_tg belongs",
    4: "pass_through ignored for kept entries",
    5: "a later duplicate's role taken at the current entry's position",
    6: "keep flag indexed by the shard-local j instead of pos1",
    7: "keep offset taken from lboff1 instead of boff1",
    8: "find_row compares with < where <= belongs",
    9: "the source-2 block index is not rebased by nblk1",
    10: "a dead source-2 duplicate is still bucketed and flagged",
    11: "bucket packing with a 6-bit shift for b",
    12: "M_miss and the feed = 2 / both blocks skipped for entries that are only targets",
    13: "device split: stream reused for the entry draws instead of stream + 1",
    14: "bucket packing with c & 127 dropped",
}


def find_row(off, B, e, strict=False):
    lo, hi = 0, B
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if (off[mid] < e) if strict else (off[mid] <= e):
            lo = mid
        else:
            hi = mid
    return lo


def twin(c, wrong=None):
    """ocf_scatter.hip scatter_entry + the bucket kernels, entry by entry in entry order: find_row over the local
    offsets, the keep flag at boff1[b] + pos1 (host flags or the device draw), the duplicate chain's later roles.
    `wrong`: a key of WRONG.  Indices a wrong variant sends out of range wrap around (garbage either way)."""
    B, N, aux = c.B, c.N, float(np.float32(c.aux))
    o = SimpleNamespace()
    o.X, o.Min, o.Mout, o.T, o.Mmiss = (np.zeros((B, N)) for _ in range(5))
    o.xX, o.xMin, o.xMiss = (np.zeros((B, N)) for _ in range(3))      # what the xin stores hold, per block source
    o.xval1, o.tflag1 = np.zeros(c.E1, np.float32), np.zeros(c.E1, np.uint8)
    o.tflag2 = np.zeros(c.E2, np.uint8)
    o.live_in, o.live_out = np.zeros(N, bool), np.zeros(N, bool)
    o.ecb, o.col_cnt = np.zeros(c.E1, np.int32), np.zeros(N, np.int32)
    o.tb_cnt = np.zeros(c.n_tiles * c.tb_nk, np.int32)
    bt, brc, bv = [], [], []
    n1 = len(c.col1)
    off = c.lboff1 if c.lboff1 is not None else c.boff1
    boff = c.lboff1 if wrong == 7 else c.boff1
    device = c.keep1 is None and c.mode == 0 and not np.float32(c.s0) >= np.float32(1.0)
    if device:
        cut = row_cut(c.seed, c.stream, c.s0, c.s1, B)[2]
        draws = philox_uniform(c.seed, c.stream + (0 if wrong == 13 else 1),
                               np.arange(int(c.boff1[-1]) + 1024, dtype=np.uint64))

    def role1(b, pos, bo):
        if c.mode == 1:
            return 1
        if c.keep1 is not None:
            k = c.keep1[(bo + pos) % len(c.keep1)] != 0
        elif not device:
            k = True
        else:
            k = draws[(bo + pos) % len(draws)] >= cut[b]
        tg = not k if wrong == 4 else (not k or c.pass_through)
        return (1 if k else 0) | (2 if tg else 0)

    prev = None
    if wrong == 2 and c.dup1 is not None:
        prev = np.full(n1, -1, np.int64)
        src = np.nonzero(c.dup1 >= 0)[0]
        prev[c.dup1[src]] = src
    for e in range(c.E1):
        b = find_row(off, B, e, wrong == 8)
        j = e - int(off[b])
        s = int(c.rp1[c.rows1[b]])
        i = (s + j) % n1
        bo = int(boff[b])
        pos_of = (lambda k: k - s) if (c.pos1 is None or wrong == 6) else (lambda k: int(c.pos1[k]))
        col, v = int(c.col1[i]), float(c.val1[i])
        role = role1(b, pos_of(i), bo)
        later_in = later_tg = False
        if c.dup1 is not None and wrong != 1:
            chain = prev if wrong == 2 else c.dup1
            f = int(chain[i])
            while f >= 0:
                rf = role1(b, pos_of(i if wrong == 5 else f), bo)
                later_in |= bool(rf & 1)
                later_tg |= bool(rf & 2)
                f = int(chain[f])
        if wrong == 3:
            later_tg = later_in
        if role & 1:
            o.Min[b, col] = aux
            if not later_in:
                o.X[b, col] = v
                o.xX[b, col] = v
            o.xMin[b, col] = aux
        o.xval1[e] = v if (role & 1) and not later_in else 0.0
        o.tb_cnt[(col >> 7) * c.tb_nk + (b >> 6)] += 1
        if c.mode == 0 and B <= 4096:                 # (col_cnt / ecb: the entry point takes them up to B = 4,096)
            o.col_cnt[col] += 1
            o.ecb[e] = col | (b << 19)
        live_tg = bool(role & 2) and not later_tg
        if role & 2:
            o.Mout[b, col] = aux
            if live_tg:
                o.T[b, col] = v
                bt.append(col >> 7)
                brc.append(((b << 6) if wrong == 11 else (b << 7)) | (0 if wrong == 14 else col & 127))
                bv.append(v)
        o.tflag1[e] = 1 if live_tg else 0
        if (role & 1) and not later_in:
            o.live_in[col] = True
        if live_tg:
            o.live_out[col] = True
        if not (wrong == 12 and role == 2):
            o.Mmiss[b, col] = aux
            o.xMiss[b, col] = aux
    nblk1 = (c.E1 + SC_THREADS - 1) // SC_THREADS
    nblk2 = (c.E2 + SC_THREADS - 1) // SC_THREADS
    for blk in range(nblk2):
        for tid in range(SC_THREADS):
            e = ((blk + nblk1) if wrong == 9 else blk) * SC_THREADS + tid
            if e >= c.E2:
                continue
            b = find_row(c.lboff2, B, e, wrong == 8)
            j = e - int(c.lboff2[b])
            i = (int(c.rp2[c.rows2[b]]) + j) % len(c.col2)
            col, v = int(c.col2[i]), float(c.val2[i])
            dead = c.dup2 is not None and c.dup2[i] >= 0
            o.Mout[b, col] = aux
            if not dead:
                o.T[b, col] = v
            if not dead or wrong == 10:
                bt.append(col >> 7)
                brc.append(((b << 6) if wrong == 11 else (b << 7)) | (0 if wrong == 14 else col & 127))
                bv.append(v)
                o.tflag2[e] = 1
            o.Mmiss[b, col] = aux
            o.xMiss[b, col] = aux
    o.bk = _buckets(c.n_tiles, bt, brc, bv, aux)
    return o


def twin_epoch(ep, wrong=None, device=None):
    """ocf_scatter.hip scatter_epoch_kernel: slot s takes batch sel[s]'s slices of the plan-wide tables, keep1 +
    keep_off, stream = stream_mul * (sel[s] + 1), and writes at ebase[s] - ebase0.  device: (s0, s1) for the device
    split, None for the host flags.  Returns (xval, tflag) over [0, total)"""
    B = ep.B
    xval, tflag = np.zeros(ep.total, np.float32), np.zeros(ep.total, np.uint8)
    for s, bi in enumerate(ep.sel):
        bi = int(bi)
        n = int(ep.ebase[s + 1] - ep.ebase[s])
        a = replace(ep.cases[bi], rows1=ep.rows1[bi * B:(bi + 1) * B], lboff1=ep.lboff1[bi * (B + 1):(bi + 1) * (B + 1)],
                    boff1=ep.boff1[bi * (B + 1):(bi + 1) * (B + 1)], keep1=ep.keep1[ep.keep_off[bi]:], E1=n)
        if device is not None:
            a = replace(a, keep1=None, s0=device[0], s1=device[1], seed=EP_SEED, stream=EP_STREAM_MUL * (bi + 1))
        o = twin(a, wrong)
        at = int(ep.ebase[s] - ep.ebase0)
        xval[at:at + n], tflag[at:at + n] = o.xval1, o.tflag1
    return xval, tflag


def reference_epoch(ep, device=None):
    """the reference loop per selected batch, laid out at ebase[s] - ebase0"""
    xval, tflag = np.zeros(ep.total, np.float32), np.zeros(ep.total, np.uint8)
    for s, bi in enumerate(ep.sel):
        c = ep.cases[int(bi)]
        if device is not None:
            c = with_device_split(c, device[0], device[1], EP_SEED, EP_STREAM_MUL * (int(bi) + 1))
        o = reference(c)
        at = int(ep.ebase[s] - ep.ebase0)
        xval[at:at + c.E1], tflag[at:at + c.E1] = o.xval1, o.tflag1
    return xval, tflag


# ---- what the GPU test compares --------------------------------------------------------------------------------
XIN_MODES = [(feed, both) for feed in range(4) for both in (0, 1)]
XB = 384                          # xin_block of the GPU tests


DENSE_OUT = ("X", "Min", "Mout", "T", "Mmiss")
ENTRY_OUT = ("xval1", "tflag1")
# what tests/test_scatter_direct_gpu.py compares on each fixture (by the start of the case's name; the first match)
GPU_COMPARES = (
    ("train-pt0-dev", DENSE_OUT + ENTRY_OUT + ("col_cnt", "ecb")),                       # test_device_split
    ("train-pt1-dev", DENSE_OUT + ENTRY_OUT + ("col_cnt", "ecb")),
    ("train-pt0", DENSE_OUT + ENTRY_OUT + ("tb_cnt", "col_cnt", "ecb", "live_in", "live_out", "buckets", "xin")),
    ("train-pt1", DENSE_OUT + ENTRY_OUT + ("tb_cnt", "col_cnt", "ecb", "live_in", "live_out", "buckets")),
    ("eval", DENSE_OUT + ENTRY_OUT + ("tflag2", "tb_cnt", "live_in", "buckets", "xin")),
    ("shard", DENSE_OUT + ENTRY_OUT + ("col_cnt", "ecb")),                               # host flags and device split
    ("wide", ENTRY_OUT + ("tb_cnt", "live_in", "live_out", "buckets")),
    ("many_rows", ENTRY_OUT + ("tb_cnt", "buckets")),
    ("epoch", ENTRY_OUT),                                                                # through ocf_epoch_scatter
)


def gpu_compares(c):
    return next(outs for head, outs in GPU_COMPARES if c.name.startswith(head))


def compared(c, o, from_twin=False, everything=False):
    """name -> array of the outputs the GPU test compares on this fixture (everything: of every output), from a
    reference or a twin result"""
    every = DENSE_OUT + ENTRY_OUT + ("tflag2", "tb_cnt", "live_in", "buckets") + (
        ("live_out", "ecb", "col_cnt") if c.mode == 0 else ()) + (("xin",) if c.N <= XB and c.B <= 128 else ())
    d = {}
    for k in (every if everything else gpu_compares(c)):
        if k == "buckets":
            d["bk_ptr"], d["bk_triples"] = o.bk.ptr, o.bk.tri
        elif k == "xin":
            blocks = (o.xX, o.xMin, o.xMiss) if from_twin else (o.X, o.Min, o.Mmiss)
            for feed, both in XIN_MODES:
                d["xin(feed=%d,both=%d)" % (feed, both)] = xin_image(*blocks, feed, both, XB)
        else:
            d[k] = getattr(o, k)
    return d


def first_difference(c, ref, tw, everything=False):
    """the first compared output in which a twin result differs from the reference's (None: equal in all)"""
    a, b = compared(c, ref, everything=everything), compared(c, tw, from_twin=True, everything=everything)
    for k in a:
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            return k
    return None
