"""CPU checks of tests/scatter_ref.py: every fixture holds the edges it is meant to hold, the per-rating reference
loop agrees with oracle.batch_oracle.scatter_rows_numpy, the kernel-shaped twin equals the reference on every
output of every fixture, every wrong variant of the twin is rejected by an output the GPU test compares, the two
column shards add up to the unsharded batch, and the device split's seed meets the conditions under which its
float32 restatement is unambiguous."""
import functools

import numpy as np
import pytest

import scatter_ref as S
from oracle.batch_oracle import scatter_rows_numpy


def device_cases():
    out = [S.with_device_split(S.train(pt), s0, s1, S.DEV_SEED, S.DEV_STREAM) for pt in (1, 0) for s0, s1 in S.DEV_RANGES]
    out += [S.with_device_split(sh, 0.3, 0.7, S.DEV_SEED, S.DEV_STREAM) for sh in S.shards(1)]
    return out


def all_cases():
    return ([S.train(1), S.train(0), S.eval_case()] + list(S.shards(1)) + list(S.shards(0)) + [S.wide(), S.many_rows()] +
            list(S.epoch(1).cases) + list(S.epoch(0).cases) + device_cases())


@functools.lru_cache(maxsize=None)
def ref_of(i):
    return S.reference(all_cases()[i])


def chain_combos(c):
    """{(a later input exists, a later target exists)} over the entries of the case's duplicate chains"""
    seen = set()
    members = set(np.nonzero(c.dup1 >= 0)[0].tolist()) | set(c.dup1[c.dup1 >= 0].tolist())
    for e in range(c.E1):
        i = int(c.ei[e])
        if i not in members:
            continue
        later_in = later_tg = False
        f = int(c.dup1[i])
        while f >= 0:
            k = bool(c.keep_ref[e + f - i])
            later_in |= k
            later_tg |= (not k) or bool(c.pass_through)
            f = int(c.dup1[f])
        seen.add((later_in, later_tg))
    return seen


def chain_lengths(rp, dup):
    heads = set(np.nonzero(dup >= 0)[0].tolist()) - set(dup[dup >= 0].tolist())
    out = set()
    for h in heads:
        n, f = 1, int(dup[h])
        while f >= 0:
            n, f = n + 1, int(dup[f])
        out.add(n)
    return out


def inside_a_row(off, e):
    """entry index e lies strictly inside a row (neither its first entry nor past the end)"""
    b = int(np.searchsorted(off, e, side="right")) - 1
    return off[b] < e < off[b + 1]


# ---- the fixtures hold their edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [1, 0])
def test_train_fixture_edges(pt):
    c = S.train(pt)
    lens = np.diff(c.lboff1)
    assert (c.B, c.B_pad, c.N, c.ld, c.n_tiles, c.tb_nk) == (70, 72, 300, 304, 3, 2)
    assert c.N % 128 != 0                                              # the last tile is partial
    assert 2 * S.SC_THREADS < c.E1 < 3 * S.SC_THREADS                  # three workgroups, the last partial
    assert inside_a_row(c.lboff1, S.SC_THREADS) and inside_a_row(c.lboff1, 2 * S.SC_THREADS)
    assert all(lens[b] == 0 for b in S.T_EMPTY) and S.T_EMPTY[0] == 0 and S.T_EMPTY[-1] == c.B - 1
    assert S.T_EMPTY[2] == S.T_EMPTY[1] + 1 and c.rows1[31] == -1 and (c.rows1 >= 0).sum() == c.B - 1
    r = c.rows1[30]
    assert c.rp1[r + 1] == c.rp1[r]                                     # empty in the dataset itself
    assert (lens[S.T_ONE], lens[S.T_TWO], lens[S.T_LONG]) == (1, 2, 290)
    assert chain_lengths(c.rp1, c.dup1) == {2, 3, 4}
    every = {(False, False), (False, True), (True, False), (True, True)}
    # with pass-through a kept entry is a target as well, so "a later input but no later target" cannot occur
    assert chain_combos(c) == (every - {(True, False)} if pt else every)
    # list order is not column order; the dataset has more rows than the batch, the batch rows are shuffled
    s = int(c.rp1[c.rows1[S.T_LONG]])
    assert (np.diff(c.col1[s:s + 290]) < 0).any()
    assert len(c.rp1) - 1 > c.B and (np.diff(c.rows1[c.rows1 >= 0]) < 0).any()
    assert {0, 127, 128, 255, 256, 299} <= set(c.col1[c.ei].tolist())
    # ratings: an exact 0.0 at a live input and at a live target; no other value is representable in 16 bits
    ref = S.reference(c)
    v = c.val1[c.ei]
    assert ((v == 0) & (ref.lastX[c.eb, c.col1[c.ei]] == np.arange(c.E1))).any()
    assert ((v == 0) & (ref.tflag1 == 1)).any()
    import torch
    nz = torch.from_numpy(v[v != 0].copy())
    assert (nz.half().float() != nz).all() and (nz.bfloat16().float() != nz).all()
    # host flags at an offset into a longer array
    assert c.boff1[0] > 0 and len(c.keep1) > c.boff1[-1] and not np.array_equal(c.boff1, c.lboff1)
    assert 0.3 < c.keep_ref.mean() < 0.8


def test_eval_fixture_edges():
    c = S.eval_case()
    assert c.mode == 1
    assert S.SC_THREADS < c.E1 < 2 * S.SC_THREADS and S.SC_THREADS < c.E2 < 2 * S.SC_THREADS    # nblk1 = nblk2 = 2
    l1, l2 = np.diff(c.lboff1), np.diff(c.lboff2)
    assert l1[S.E_NOIN] == 0 and l2[S.E_NOIN] > 0 and c.rows1[S.E_NOIN] == -1
    assert l1[S.E_NOTGT] > 0 and l2[S.E_NOTGT] == 0
    assert l1[S.E_NONE] == 0 and l2[S.E_NONE] == 0
    assert chain_lengths(c.rp2, c.dup2) == {2, 3, 4} and c.dup1 is not None
    ref = S.reference(c)
    assert ((ref.lastX >= 0) & (ref.lastT >= 0)).sum() >= c.B           # cells held by both sources
    assert (ref.tflag2 == 0).sum() == 1 + 2 + 3 and not ref.tflag1.any()


def test_shards_fixture():
    full = S.train(1)
    a, b = S.shards(1)
    assert a.E1 + b.E1 == full.E1 and a.N + b.N == full.N and a.E1 > 0 and b.E1 > 0
    for sh in (a, b):
        assert sh.pos1 is not None and not np.array_equal(sh.lboff1, full.lboff1)
        assert np.array_equal(sh.boff1, full.boff1) and sh.keep1 is full.keep1
        assert (sh.epos != np.arange(sh.E1) - sh.lboff1[sh.eb]).any()   # a shard-local j is not the full position
        assert np.array_equal(full.col1[full.ei[sh.src_e]] - sh.col_lo, sh.col1[sh.ei])
        assert sh.dup1 is not None                                       # both shards hold chains
    assert sorted(np.concatenate([a.src_e, b.src_e]).tolist()) == list(range(full.E1))


def test_wide_fixture():
    c = S.wide()
    assert c.B == 4 and c.N == 131072 + 128 + 5 and c.n_tiles == 1026
    assert (c.n_tiles + 1023) // 1024 == 2                              # bucket_scan_kernel: two tiles per thread
    assert 2 * S.SC_THREADS < c.E1 < 3 * S.SC_THREADS + 200
    tiles = set((c.col1[c.ei] >> 7).tolist())
    assert {0, 1, 1023, 1024, 1025} <= tiles and c.col1[c.ei].max() == c.N - 1
    assert chain_lengths(c.rp1, c.dup1) == {2, 3, 4}


def test_many_rows_fixture():
    c = S.many_rows()
    assert c.B == 8192 and (c.B + 1) * 8 > 65536 and 8192 * 8 <= 65536   # the first offset table past 64 KB
    assert set(np.diff(c.lboff1).tolist()) == {0, 1} and 2500 < c.E1 < 3500
    assert c.tb_nk == 128
    c = S.many_rows(16384)                                               # the largest batch ocf_scatter_batch admits
    assert c.B == 16384 and set(np.diff(c.lboff1).tolist()) == {0, 1} and 2500 < c.E1 < 3500
    assert S.first_difference(c, S.reference(c), S.twin(c), everything=True) is None


@pytest.mark.parametrize("pt", [1, 0])
def test_epoch_fixture(pt):
    ep = S.epoch(pt)
    E = [c.E1 for c in ep.cases]
    assert len(E) == 3 and len(set(E)) == 3
    assert max(E) > S.SC_THREADS * S.SE_U and min(E) < S.SC_THREADS     # two workgroups in x; less than one
    assert list(ep.sel) != sorted(ep.sel) and ep.ebase0 != 0 and ep.ebase[0] == ep.ebase0
    assert len(set(ep.keep_off.tolist())) == 3 and ep.max_e == max(E)
    every = {(False, False), (False, True), (True, False), (True, True)}
    for c in ep.cases:
        assert c.rows1[-1] == -1 and chain_lengths(c.rp1, c.dup1) == {2, 3, 4}
        assert chain_combos(c) == (every - {(True, False)} if pt else every)


# ---- reference, oracle, twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [1, 0])
def test_reference_matches_batch_oracle(pt):
    c = S.train(pt)
    rows = c.rows1.astype(np.int64)
    rows[rows < 0] = c.rows1[30]                                        # the -1 row as a row empty in the dataset
    m_in, m_out, x, t, m_miss = scatter_rows_numpy(c.rp1, c.col1, c.val1, rows, c.N, keep=c.keep_ref != 0, aux=c.aux,
                                                   pass_through=bool(pt))
    ref = S.reference(c)
    for name, want in (("Min", m_in), ("Mout", m_out), ("X", x), ("T", t), ("Mmiss", m_miss)):
        np.testing.assert_array_equal(getattr(ref, name), want, err_msg=name)


CASE_IDS = [c.name for c in all_cases()]


@pytest.mark.parametrize("i", range(len(CASE_IDS)), ids=CASE_IDS)
def test_twin_equals_reference(i):
    c = all_cases()[i]
    assert S.first_difference(c, ref_of(i), S.twin(c), everything=True) is None


@pytest.mark.parametrize("pt", [1, 0])
@pytest.mark.parametrize("device", [None, (0.3, 0.7)])
def test_epoch_twin_equals_reference(pt, device):
    ep = S.epoch(pt)
    want, got = S.reference_epoch(ep, device), S.twin_epoch(ep, None, device)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("wrong", sorted(S.WRONG))
def test_wrong_variant_is_rejected(wrong):
    """by an output the GPU test compares, on at least one fixture"""
    cases = all_cases()
    for i, c in enumerate(cases):
        if c.name.startswith("epoch") or c.name == "many_rows":
            continue                                                     # (compared through ocf_epoch_scatter below)
        what = S.first_difference(c, ref_of(i), S.twin(c, wrong))
        if what is not None:
            print("WRONG %2d (%s): rejected on '%s' by %s" % (wrong, S.WRONG[wrong], c.name, what))
            return
    ep = S.epoch(0)
    for device in (None, (0.3, 0.7)):
        want, got = S.reference_epoch(ep, device), S.twin_epoch(ep, wrong, device)
        for k, name in enumerate(("xval", "tflag")):
            if not np.array_equal(want[k], got[k]):
                print("WRONG %2d (%s): rejected on '%s' by %s" % (wrong, S.WRONG[wrong], ep.name, name))
                return
    pytest.fail("wrong variant %d (%s) is rejected by no fixture" % (wrong, S.WRONG[wrong]))


@pytest.mark.parametrize("wrong", [1, 2, 3, 4, 5, 7, 8])
def test_epoch_rejects(wrong):
    """the epoch fixture alone rejects the variants its kernel shares with the per-batch scatter"""
    bad = False
    for pt in (1, 0):
        ep = S.epoch(pt)
        want, got = S.reference_epoch(ep), S.twin_epoch(ep, wrong)
        bad |= not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
    assert bad


@pytest.mark.parametrize("pt", [1, 0])
def test_shard_union(pt):
    full = S.train(pt)
    ref = S.reference(full)
    parts = [(sh, S.reference(sh)) for sh in S.shards(pt)]
    for name in ("X", "Min", "Mout", "T", "Mmiss"):
        np.testing.assert_array_equal(np.concatenate([getattr(o, name) for _, o in parts], axis=1), getattr(ref, name))
    for name in ("live_in", "live_out", "col_cnt"):
        np.testing.assert_array_equal(np.concatenate([getattr(o, name) for _, o in parts]), getattr(ref, name))
    for name in ("xval1", "tflag1"):
        got = np.full(full.E1, 99, getattr(ref, name).dtype)
        for sh, o in parts:
            got[sh.src_e] = getattr(o, name)
        np.testing.assert_array_equal(got, getattr(ref, name))
    np.testing.assert_array_equal(union_targets(parts), full_targets(ref))


def full_targets(ref):
    """(b, column, t) of every live target, sorted"""
    rc, t = ref.bk.tri[:, 0].astype(np.int64), ref.bk.tri[:, 1]
    tile = np.searchsorted(ref.bk.ptr[1:], np.arange(len(rc)), side="right")
    out = np.stack([rc >> 7, tile * 128 + (rc & 127), t], 1)
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]


def union_targets(parts):
    out = []
    for sh, o in parts:
        t = full_targets(o)
        t[:, 1] += sh.col_lo
        out.append(t)
    out = np.concatenate(out)
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]


# ---- the device split ------------------------------------------------------------------------------------------------
def split_cases():
    out = [(c, c.s0, c.s1, c.seed, c.stream) for c in device_cases()]
    for pt in (1, 0):
        for bi, c in enumerate(S.epoch(pt).cases):
            out.append((c, 0.3, 0.7, S.EP_SEED, S.EP_STREAM_MUL * (bi + 1)))
    return out


@pytest.mark.parametrize("k", range(len(split_cases())), ids=[t[0].name for t in split_cases()])
def test_device_split_conditions(k):
    """the conditions under which the float32 restatement of row_cut cannot disagree with the kernel's by a
    rounding: none of them is loosened for the GPU test; a seed that violates one is replaced"""
    c, s0, s1, seed, stream = split_cases()[k]
    d = S.device_split(c, s0, s1, seed, stream)
    assert np.abs(d.u.astype(np.float64) - d.cut64[c.eb]).min() > S.SPLIT_GAP
    assert d.s64.min() > S.SPLIT_GAP and d.s64.max() < 1.0 - S.SPLIT_GAP
    np.testing.assert_array_equal(d.keep, d.keep64)
    lens = np.bincount(c.eb, minlength=c.B)
    want = float((d.s64 * lens).sum())
    assert abs(float(d.keep.sum()) - want) <= S.kept_count_bound(d.s64, lens), (d.keep.sum(), want)
    assert S.device_split(c, 1.0, 1.0, seed, stream).keep.all()
