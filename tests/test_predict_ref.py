"""CPU: the references and bounds of tests/predict_ref.py, which tests/test_predict_direct_gpu.py applies to
ocf_predict_entries.  The fixture holds its edges at every hidden width the kernel takes, the clip range cuts the
predictions on both sides with next to none of them at an edge, a float32 restatement in the kernel's order is inside
every bound, and each deliberately wrong variant is outside at least one."""
import numpy as np
import pytest

import gather_ref as G
import predict_ref as P


def configs():
    """(aux, clip, use_flag): the GPU test's launches"""
    return [(aux, clip, fl) for aux in (1.0, -1.0) for clip in (None, P.CLIP) for fl in (True, False)]


@pytest.mark.parametrize("H", P.ALL_H)
def test_fixture_at_every_width(H):
    fx = G.make_batch(H)
    G.check_batch(fx)
    for chunk in (P.CHUNK, P.CHUNK_ALT):
        ct = G.chunks_for(H, chunk)
        ln = ct.ch_j1 - ct.ch_j0
        assert (ln > 0).all() and ln.max() <= chunk and (np.diff(ct.ch_row) >= 0).all()
    assert G.chunks_for(H, P.CHUNK).n_chunks < G.chunks_for(H, P.CHUNK_ALT).n_chunks
    # aux = 1: a good third of the predictions lie inside the clip range, most of the rest below it (above it: a few
    # at some widths, test_clip_range_cuts_on_both_sides), and so few lie within their own bound of an edge that none
    # has to be left out of the comparison
    _, hr = P.hidden(fx, "f32")
    ref = P.reference(fx, G.chunks_for(H, P.CHUNK), hr, G.weights_for("f32", H, 0)[3], 1.0, None, True)
    inside = ((ref.y >= P.CLIP[0]) & (ref.y <= P.CLIP[1])).mean()
    assert 0.2 < inside < 0.5 and (ref.y < P.CLIP[0]).mean() > 0.4, inside
    near = np.minimum(np.abs(ref.y - P.CLIP[0]), np.abs(ref.y - P.CLIP[1])) <= ref.by
    assert near.mean() <= 0.001, near.mean()
    # aux = -1 changes the sign of every prediction
    neg = P.reference(fx, G.chunks_for(H, P.CHUNK), hr, G.weights_for("f32", H, 0)[3], -1.0, None, True)
    assert np.array_equal(neg.y, -ref.y)


def test_clip_range_cuts_on_both_sides():
    """both edges of the clip range cut in the GPU grid's launches: in the register form at either aux (H = 128), in
    the slab form at aux = 1 (H = 1024)"""
    for H, auxes in ((128, (1.0, -1.0)), (1024, (1.0,))):
        fx = G.make_batch(H)
        y1 = P.reference(fx, G.chunks_for(H, P.CHUNK), P.hidden(fx, "f32")[1], G.weights_for("f32", H, 0)[3], 1.0, None,
                         True).y
        for aux in auxes:
            assert (aux * y1 > P.CLIP[1]).any() and (aux * y1 < P.CLIP[0]).any(), (H, aux)


def test_shapes_follow_the_kernel():
    assert [P.shape("f16", H) for H in (128, 256, 384, 512)] == [(16, 1, False), (32, 1, False), (16, 3, False),
                                                                  (32, 2, False)]
    assert [P.shape("f32", H) for H in (128, 256, 384, 512)] == [(32, 1, False), (32, 2, False), (32, 3, False),
                                                                  (32, 4, False)]
    assert P.shape("bf16", 640) == (32, 2, True) and P.shape("f32", 2048) == (32, 4, True)
    assert set(G.GRID) < set(P.GRID) and {H for _, H, _ in P.GRID if H > 512} == {640, 1024}


@pytest.mark.parametrize("wt,H,bl", P.GRID, ids=P.GRID_IDS)
def test_float32_restatement_is_inside_every_bound(wt, H, bl):
    fx = G.make_batch(H)
    _, hr = P.hidden(fx, wt)
    Wr = G.weights_for(wt, H, bl)[3]
    for chunk in (P.CHUNK, P.CHUNK_ALT):
        ct = G.chunks_for(H, chunk)
        for aux, clip, fl in configs():
            ref = P.reference(fx, ct, hr, Wr, aux, clip, fl)
            o = P.twin(fx, ct, wt, bl, aux, clip, fl)
            rep = G.Report()
            P.check(rep, fx, ref, o.y, o.row_stats, o.total)
            what, r, i = rep.worst()
            print("%s H=%d bl=%d chunk=%d aux=%g clip=%s flag=%d: worst %s %.3g at %s" % (wt, H, bl, chunk, aux, clip, fl,
                                                                                            what, r, i))
            assert not rep.failures(), rep.failures()
            assert ref.ent.ambiguous.sum() <= 0.01 * fx.E


# where each wrong variant is shown: a blocked point, a PPL > 1 point, fp32, and both slab points
WRONG_AT = [("f16", 512, 1), ("bf16", 384, 1), ("f32", 256, 0), ("f16", 640, 1), ("f32", 1024, 0)]


@pytest.mark.parametrize("k", sorted(P.WRONG))
def test_wrong_variant_is_outside_a_bound(k):
    caught, tried = [], 0
    for wt, H, bl in WRONG_AT:
        fx, ct = G.make_batch(H), G.chunks_for(H, P.CHUNK)
        _, hr = P.hidden(fx, wt)
        Wr = G.weights_for(wt, H, bl)[3]
        for aux, clip, fl in configs():
            if not P.wrong_applies(k, wt, H, bl, aux, clip, fl):
                continue
            tried += 1
            ref = P.reference(fx, ct, hr, Wr, aux, clip, fl)
            o = P.twin(fx, ct, wt, bl, aux, clip, fl, wrong=k)
            rep = G.Report()
            P.check(rep, fx, ref, o.y, o.row_stats, o.total)
            bad = rep.failures()
            print("variant %d (%s) at %s H=%d bl=%d aux=%g clip=%s flag=%d: %s" % (
                k, P.WRONG[k], wt, H, bl, aux, clip, fl, [(w, "%.3g" % r) for w, r, _ in bad] or "NOT REJECTED"))
            caught.append(bool(bad))
    assert tried and all(caught), (k, P.WRONG[k], caught)
