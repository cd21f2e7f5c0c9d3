"""CPU: the fixtures, reference and bound of tests/tiles_ref.py, which tests/test_tiles_direct_gpu.py applies to
ocf_encoder_tiles.  For every case the GPU tests launch: the fixture holds its edges (validate), the two fp64
references agree, a float32 restatement that accumulates tile by tile is inside the bound, and each of ten
deliberately wrong restatements is outside it on the case named for it."""
import numpy as np
import pytest

import tiles_ref as T


@pytest.mark.parametrize("name", T.NAMES)
def test_fixture_edges_and_shapes(name):
    c = T.make_case(name)
    T.validate(c)
    p = T.CASES[name]
    assert (c.n_tiles, c.splits, c.B, c.Bp, c.H, c.ldw) == (p["n_tiles"], p["splits"], p["B"], p["Bp"], p["H"], p["ldw"])
    assert c.n_tiles <= 23 and c.Bp <= 384
    print("%s: %d entries, %d dataset rows, tiles per split %d" % (name, c.E, len(c.rp) - 1, T.tiles_per(c)))


def test_the_cases_reach_what_they_are_for():
    tp = {n: T.tiles_per(T.make_case(n)) for n in T.NAMES}
    assert tp == {"one_tile": 1, "deep7": 7, "short_last": 4, "empty_split": 2, "xcd_round2": 2, "long_split": 12,
                  "h384": 6, "no_rows": 2, "rounding": 4}
    assert T.split_range(T.make_case("short_last"), 2) == (8, 10)
    c = T.make_case("empty_split")
    assert T.split_range(c, 2) == (4, 5) and T.split_range(c, 3) == (5, 5)
    c = T.make_case("deep7")
    assert c.heavy == 2 and c.Bp - c.B == 84 and c.Bp % 256 == 128
    v = T.view_entries(c)
    assert v.word[(v.b < T.BM) & (v.t == c.heavy)].max() >= T.BUCKET         # a bucket over 1,024 words ...
    assert v.word[(v.b < T.BM) & (v.t != c.heavy)].max() < T.BUCKET          # ... and only that one
    assert v.k.max() >= T.EMAX
    c = T.make_case("long_split")
    assert T.view_entries(c).p.max() >= T.PK_CHUNK and c.max_row_len > T.PK_CHUNK
    assert T.make_case("xcd_round2").splits > 8


@pytest.mark.parametrize("wt", T.DTYPES)
@pytest.mark.parametrize("name", T.NAMES)
def test_the_two_references_agree(name, wt):
    c = T.make_case(name)
    ref, mag, nterms = T.ref_partials(c, wt)
    dense = T.ref_dense(c, wt)
    assert (np.abs(ref - dense) <= 1e-12 * np.maximum(mag, 1e-300)).all() and (dense[mag == 0] == 0).all()
    z = T.zero_rows(c)
    assert not ref[z].any() and not mag[z].any() and not nterms[z].any()
    for s in range(c.splits):
        t0, t1 = T.split_range(c, s)
        if t0 == t1:
            assert not mag[:, s].any()
    if c.B:
        assert (nterms[~z].sum(1) > 0).mean() > 0.9 and nterms[T.ROW_EDGE].sum() == c.lens[T.ROW_EDGE]
        assert not mag[T.ROW_ALLZERO].any()


@pytest.mark.parametrize("wt", T.DTYPES)
@pytest.mark.parametrize("name", T.NAMES)
def test_float32_restatement_is_inside_the_bound(name, wt):
    c = T.make_case(name)
    r, i = T.check(c, wt, T.twin(c, wt))
    print("%s %s: worst error / bound %.3g at %s" % (name, wt, r, i))
    assert r <= 1.0, (name, wt, r, i)


@pytest.mark.parametrize("wt", T.DTYPES)
@pytest.mark.parametrize("k", sorted(T.WRONG))
def test_wrong_variant_is_outside_the_bound(k, wt):
    name = T.WRONG_AT[k]
    c = T.make_case(name)
    r, i = T.check(c, wt, T.twin(c, wt, wrong=k))
    print("variant %d (%s) on %s %s: worst error / bound %.3g at %s" % (k, T.WRONG[k], name, wt, r, i))
    assert r > 1.0, (k, T.WRONG[k], name, "NOT REJECTED")


def test_a_nan_is_an_error():
    c = T.make_case("one_tile")
    got = T.twin(c, "f16")
    got[c.Bp - 1, 0, c.H - 1] = np.nan
    assert T.check(c, "f16", got)[0] == np.inf


def test_validate_rejects_broken_fixtures():
    c = T.make_case("short_last")
    r = int(c.rows[T.ROWS_OVER[0]])
    tptr = np.array(c.tptr)
    tptr[r, 3] += 1                                        # one entry moved across a tile boundary
    with pytest.raises(AssertionError):
        T.validate(T.variant(c, tptr=tptr))
    tptr = np.array(c.tptr)
    tptr[r, -1] += 1                                       # a row that ends past its length
    with pytest.raises(AssertionError):
        T.validate(T.variant(c, tptr=tptr))
    tlidx = np.array(c.tlidx)
    tlidx[c.rp[r]] = c.rp[r + 1] - c.rp[r]                 # one past the row's list
    with pytest.raises(AssertionError):
        T.validate(T.variant(c, tlidx=tlidx))
    lboff = np.array(c.lboff)
    lboff[5:] += 1
    with pytest.raises(AssertionError):
        T.validate(T.variant(c, lboff=lboff))
