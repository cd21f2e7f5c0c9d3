"""CPU: the data side of the per-column ranking -- RatingsCSR.transposed against a dense NumPy transpose (with
and without duplicate ratings) and FixedSplit.catalogue's keys, inputs and per-column views.  No GPU."""
import numpy as np
import pytest

import parity


def _dense_counts(csr, n_cols):
    """[rows, n_cols] number of entries and sum of values per cell"""
    cnt = np.zeros((csr.n_rows, n_cols), np.int64)
    tot = np.zeros((csr.n_rows, n_cols), np.float64)
    rows = np.repeat(np.arange(csr.n_rows), csr.row_lengths())
    np.add.at(cnt, (rows, csr.col), 1)
    np.add.at(tot, (rows, csr.col), csr.val)
    return cnt, tot


def _row_multiset(csr, r):
    sl = slice(csr.row_ptr[r], csr.row_ptr[r + 1])
    return sorted(zip(csr.col[sl].tolist(), csr.val[sl].tolist()))


def _check_transposed(csr, n_cols):
    t = csr.transposed(n_cols)
    assert t.n_rows == n_cols and t.nnz == csr.nnz and t.col.dtype == np.int32 and t.val.dtype == np.float32
    assert t.row_ptr.dtype == np.int64 and t.row_ptr[0] == 0
    cnt, tot = _dense_counts(csr, n_cols)
    cnt_t, tot_t = _dense_counts(t, csr.n_rows)
    assert np.array_equal(cnt_t, cnt.T) and np.array_equal(tot_t, tot.T)
    for c in range(n_cols):                                    # ascending columns; duplicates in source order
        sl = slice(t.row_ptr[c], t.row_ptr[c + 1])
        assert (np.diff(t.col[sl]) >= 0).all()
        for r in np.unique(t.col[sl]):
            src = csr.val[csr.row_ptr[r]:csr.row_ptr[r + 1]][csr.col[csr.row_ptr[r]:csr.row_ptr[r + 1]] == c]
            assert np.array_equal(t.val[sl][t.col[sl] == r], src)
    # twice: the same multiset per row
    tt = t.transposed(csr.n_rows)
    assert tt.n_rows == csr.n_rows and np.array_equal(tt.row_ptr, csr.row_ptr)
    for r in range(csr.n_rows):
        assert _row_multiset(tt, r) == _row_multiset(csr, r)
    # and the tile index works on it
    col_s, val_s, lidx_s, tptr = t.tile_index(csr.n_rows)
    assert np.array_equal(col_s, t.col) and np.array_equal(val_s, t.val)        # already column-sorted
    assert tptr.shape == (n_cols, -(-csr.n_rows // 128) + 1) and np.array_equal(tptr[:, -1], t.row_lengths())
    return t


def test_transposed_matches_dense_transpose():
    data = parity.dataset()
    assert data.train.n_rows == 700 and data.num_cols == 333
    t = _check_transposed(data.train, 333)
    assert t.dup is None
    _check_transposed(data.valid_tgt, 333)


def test_transposed_keeps_duplicates():
    data = parity.with_duplicates(300, 150, 6000, seed=4)
    assert data.train.dup is not None
    t = _check_transposed(data.train, 150)
    assert t.dup is not None and (t.dup >= 0).sum() == (data.train.dup >= 0).sum()


def test_transposed_refuses_a_column_out_of_range():
    with pytest.raises(ValueError, match="outside"):
        parity.dataset().train.transposed(100)
    from omnidirectional_collaborative_filtering_amd.dataset import RatingsCSR
    empty = RatingsCSR(np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)).transposed(5)
    assert empty.n_rows == 5 and empty.nnz == 0


def _rows_equal(a, ra, b, rb):
    sa, sb = slice(a.row_ptr[ra], a.row_ptr[ra + 1]), slice(b.row_ptr[rb], b.row_ptr[rb + 1])
    return np.array_equal(a.col[sa], b.col[sb]) and np.array_equal(a.val[sa], b.val[sb])


def test_catalogue_valid_and_train():
    data = parity.dataset()
    keys, inputs, seen, held = data.catalogue("valid")
    assert len(keys) == 700 and keys == list(data.train.keys)
    assert inputs.n_rows == 700 and all(_rows_equal(inputs, r, data.train, r) for r in range(700))
    assert seen.n_rows == 333 and seen.nnz == data.train.nnz
    assert held.n_rows == 333 and held.nnz == data.valid_tgt.nnz
    lens = held.row_lengths()
    assert int((lens == 0).sum()) == 6 and int((lens > 0).sum()) == 327
    # held_by_col[c] lists (position in keys, rating) of every valid target in column c
    pos = {k: i for i, k in enumerate(keys)}
    want = sorted((int(c), pos[data.valid_tgt.keys[r]], float(v)) for r in range(data.valid_tgt.n_rows)
                  for c, v in zip(data.valid_tgt.col[data.valid_tgt.row_ptr[r]:data.valid_tgt.row_ptr[r + 1]],
                                  data.valid_tgt.val[data.valid_tgt.row_ptr[r]:data.valid_tgt.row_ptr[r + 1]]))
    got = sorted((c, int(i), float(v)) for c in range(333)
                 for i, v in zip(held.col[held.row_ptr[c]:held.row_ptr[c + 1]], held.val[held.row_ptr[c]:held.row_ptr[c + 1]]))
    assert got == want
    k2, in2, seen2, held2 = data.catalogue("train")
    assert k2 == keys and held2 is None and np.array_equal(seen2.col, seen.col) and in2.nnz == inputs.nnz
    with pytest.raises(ValueError, match="split must be"):
        data.catalogue("all")


def test_catalogue_test():
    data = parity.dataset()
    keys, inputs, seen, held = data.catalogue("test")
    n_tr = len(data.train.keys)
    assert keys[:n_tr] == list(data.train.keys)
    extra = [k for k in data.valid_tgt.keys if k not in set(data.train.keys)]
    assert keys[n_tr:] == extra and len(set(keys)) == len(keys)
    pos = {k: i for i, k in enumerate(keys)}
    in_test = set(data.test_tgt.keys)
    assert len(in_test) > 0
    for r, key in enumerate(data.test_tgt.keys):               # the test_in row, entry for entry
        assert _rows_equal(inputs, pos[key], data.test_in, r), key
    tr_pos = {k: i for i, k in enumerate(data.train.keys)}
    va_pos = {k: i for i, k in enumerate(data.valid_tgt.keys)}
    others = [k for k in keys if k not in in_test]
    for key in others:                                         # train entries, then valid targets
        i = pos[key]
        cols = inputs.col[inputs.row_ptr[i]:inputs.row_ptr[i + 1]]
        parts = [c.col[c.row_ptr[p[key]]:c.row_ptr[p[key] + 1]] for c, p in ((data.train, tr_pos), (data.valid_tgt, va_pos))
                 if key in p]
        assert np.array_equal(cols, np.concatenate(parts)), key
    assert np.array_equal(seen.col, inputs.transposed(333).col) and seen.nnz == inputs.nnz
    assert held.nnz == data.test_tgt.nnz and held.n_rows == 333


def test_catalogue_raises_on_a_held_out_row_outside_the_candidates():
    data = parity.dataset()
    data.test_tgt.keys = list(data.test_tgt.keys)
    data.test_tgt.keys[0] = "nobody"
    data.test_in.keys = list(data.test_tgt.keys)
    with pytest.raises(ValueError, match="not among the candidate rows"):
        data.catalogue("test")
