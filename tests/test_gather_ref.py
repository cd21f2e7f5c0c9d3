"""CPU: the fixtures, references and bounds of tests/gather_ref.py, which tests/test_gathers_gpu.py applies to the
row-gather kernels.  For every fixture the GPU tests use: the batch holds its edge rows, at most 1 % of the live
targets sit at a kink of rho', a float32 restatement of every stage (summed in the kernels' order, not the
reference's) is inside every bound, and each deliberately wrong variant is outside at least one."""
import numpy as np
import pytest

import gather_ref as G


def cases_of(wt, H, bl):
    """(m, loss, activation, h_given) per grid point: the GPU tests' decoder cases"""
    out = [(-1.0, "mse", "sigmoid", False), (0.5, "mse", "sigmoid", True)]
    out += [(-1.0, ls, "sigmoid", True) for ls, w, h, b in G.LOSS_CASES if (w, h, b) == (wt, H, bl)]
    if (wt, H, bl) == G.ALL_ACTS_AT:
        out += [(0.5, "mse", a, False) for a in ("tanh", "relu", "linear")]
    return out


@pytest.mark.parametrize("H", sorted(G.CHUNK_OF))
def test_batch_edges(H):
    fx = G.make_batch(H)
    G.check_batch(fx)
    for chunk in (G.CHUNK_OF[H], 64, 1024):
        ct = G.chunks_for(H, chunk)
        ln = ct.ch_j1 - ct.ch_j0
        assert (ln > 0).all() and ln.max() <= chunk and ct.row_cptr[-1] == ct.n_chunks
        assert np.array_equal(np.bincount(ct.ch_row, weights=ln, minlength=fx.B), fx.lens)
        # equal-length chunks of a row, in order
        for b in range(fx.B):
            c0, c1 = ct.row_cptr[b], ct.row_cptr[b + 1]
            assert c1 - c0 == -(-fx.lens[b] // chunk)
            if c1 > c0:
                assert ct.ch_j0[c0] == 0 and ct.ch_j1[c1 - 1] == fx.lens[b]
                assert (ct.ch_j0[c0 + 1:c1] == ct.ch_j1[c0:c1 - 1]).all() and ln[c0:c1].max() - ln[c0:c1].min() <= 1
    ct = G.chunks_for(H)
    ln = ct.ch_j1 - ct.ch_j0
    for wt in ("f16", "f32"):
        ng = 256 // G.gather_shape(wt, H)[0]
        assert (ln < ng).any() and (ln % (ng * 4) != 0).any()         # chunks below the group count, ragged strides
    assert np.diff(G.chunks_for(H, 64).row_cptr).max() == 11            # more chunks than the reduce loop holds in flight


def test_blocked_layout_round_trip():
    fx = G.make_batch(128)
    for wt in ("f16", "bf16"):
        p, Wr = G.pack_weights(fx.W1, wt, 1)
        n = np.array([0, 1, 63, 64, 65, 999, 1023])
        assert np.array_equal(G.unpack_rows(p, wt, 1, n).astype(np.float64), Wr[n])
        q, Wr2 = G.pack_weights(fx.W1, wt, 0)
        assert np.array_equal(Wr, Wr2) and np.array_equal(G.unpack_rows(q, wt, 0, n).astype(np.float64), Wr[n])
        assert not np.array_equal(p, q)
        # ocf.h: blocks of 64 rows x 64 columns, 8 KB each, row-major inside, blocks row-major
        assert np.array_equal(p.reshape(-1)[4096 * 3 + 64 * 5:4096 * 3 + 64 * 5 + 64], q[64 + 5, 64:128])


@pytest.mark.parametrize("wt,H,bl", G.GRID, ids=G.GRID_IDS)
def test_float32_restatement_is_inside_every_bound(wt, H, bl):
    fx, ct = G.make_batch(H), G.chunks_for(H)
    for m, loss, act, h_given in cases_of(wt, H, bl):
        for keep in ((G.KEEP, 1.0) if loss == "mse" and not h_given else (G.KEEP,)):
            o = G.twin(fx, ct, wt, bl, act=act, keep=keep, m=m, loss=loss, h_given=h_given)
            rep, share = G.check_twin(fx, ct, wt, bl, o, act=act, keep=keep, m=m, loss=loss)
            what, r, i = rep.worst()
            print("%s H=%d bl=%d m=%g %s %s keep=%g: worst %s %.3g at %s; kink share %.4f" %
                  (wt, H, bl, m, loss, act, keep, what, r, i, share))
            assert share <= 0.01, (loss, share)
            assert not rep.failures(), rep.failures()


# where each wrong variant is shown: grid points with PPL > 1 / blocked weights among them, a loss other than MSE
# for variant 12, the plain decoder's zero hidden row (h_given) for variant 8
WRONG_AT = [("f16", 512, 1, "mse"), ("bf16", 384, 1, "huber"), ("f32", 256, 0, "mse"), ("f16", 128, 0, "logcosh")]


@pytest.mark.parametrize("k", sorted(G.WRONG))
def test_wrong_variant_is_outside_a_bound(k):
    caught, tried = [], 0
    for wt, H, bl, loss in WRONG_AT:
        if not G.wrong_applies(k, wt, H, bl, loss):
            continue
        tried += 1
        fx, ct = G.make_batch(H), G.chunks_for(H)
        o = G.twin(fx, ct, wt, bl, m=-1.0 if tried % 2 else 0.5, loss=loss, h_given=True, wrong=k)
        rep, _ = G.check_twin(fx, ct, wt, bl, o, m=-1.0 if tried % 2 else 0.5, loss=loss)
        bad = rep.failures()
        print("variant %d (%s) at %s H=%d bl=%d %s: %s" % (k, G.WRONG[k], wt, H, bl, loss,
                                                          [(w, "%.3g" % r) for w, r, _ in bad] or "NOT REJECTED"))
        caught.append(bool(bad))
    assert tried and all(caught), (k, G.WRONG[k], caught)


@pytest.mark.parametrize("wt,bl", [("f16", 1), ("f32", 0)])
@pytest.mark.parametrize("chunk", [1024, 64])
def test_rank_step_fixtures(wt, bl, chunk):
    """the chunk tables of the rank-step GPU test (one chunk per row; chunk 64) and the from-the-entries hidden check
    of the launches that run the encoder themselves"""
    from types import SimpleNamespace
    fx, ct = G.make_batch(256), G.chunks_for(256, chunk)
    assert (ct.n_chunks <= 2 * fx.B) == (chunk == 1024)
    o = G.twin(fx, ct, wt, bl)
    rep, share = G.check_twin(fx, ct, wt, bl, o)
    _, W1r, _, _ = G.weights_for(wt, 256, bl)
    G.check_hidden_scratch(rep, "scratch", fx, ct, wt, W1r, "sigmoid", G.KEEP, fx.bias_h,
                           SimpleNamespace(a_out=o.a_out, mask_out=o.mask_out, h=o.h), None)
    assert share <= 0.01 and not rep.failures(), rep.failures()
