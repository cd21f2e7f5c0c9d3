"""CPU checks of tests/mlp_ref.py, the reference behind tests/test_mlp_direct_gpu.py: on every case and compute dtype
the float32 restatement of ocf_mlp_step lies inside every bound (gradients, statistics, the four optimizers' updates,
the shadows, the exact count), every deliberately wrong variant of it lies outside one on at least one case, the
input conditions the GPU tests rely on hold with no exclusion, and the host-side validation refuses a case the
kernel could not be trusted with."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import epilogue_ref as R
import mlp_ref as M


@functools.lru_cache(maxsize=None)
def ref_of(name, cd):
    return M.reference(M.make_case(name), cd)


def verdict(name, cd, variant=None, opts=("probe",) + R.OPTS):
    """(worst gradient ratio, worst stats ratio, worst update ratio, list of failed exact checks) of the twin"""
    c, ref = M.make_case(name), ref_of(name, cd)
    g = s = u = 0.0
    failed = []
    for k, opt in enumerate(opts):
        blocked = k % 2
        out = M.twin(c, cd, opt, variant, blocked)
        st = M.init_state(c, opt)
        if opt == "probe":
            g = M.check_grads(c, ref, out)
            s, count_ok = M.check_stats(c, ref, out.stats)
            if not count_ok:
                failed.append("count")
            # what the GPU test relies on: Adam with beta_1 = 0.5 from zero slots leaves exactly g / 2
            for i in range(c.L + 1):
                assert np.array_equal(2.0 * out.sW1[i], np.where(M.live_w(c, i), out.gW[i], 0))
                assert np.array_equal(2.0 * out.sb1[i], out.gb[i])
        w, pad_ok = M.check_update(c, opt, st, out.gW, out.gb, out)
        u = max(u, w)
        if not pad_ok:
            failed.append("padding (%s)" % opt)
        if cd != "f32" and not M.check_shadows(c, cd, out, blocked):
            failed.append("shadow (%s)" % opt)
    return g, s, u, failed


@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_twin_lies_inside_every_bound(name, cd):
    g, s, u, failed = verdict(name, cd)
    print("MLP_TWIN %s %s grad %.3g stats %.3g update %.3g" % (name, cd, g, s, u))
    assert not failed, failed
    assert g <= 1.0 and s <= 1.0 and u <= 1.0, (g, s, u)


# where each wrong variant is expected to show first (every other case is tried after these)
FIRST = {"row_sse_8_blocks": ("ktail", "f32"), "totals_2048_slots": ("wide", "f32"), "k_tail_dropped": ("ktail", "f32"),
         "act_grad_post_dropout": ("base_drop", "f32"), "no_dropout_scale_backward": ("base_drop", "f32"),
         "shared_philox_stream": ("base_drop", "f32"), "shadow_pre_update": ("k64", "bf16"),
         "shadow_row_major": ("base", "f16"), "loss_grad_unmasked": ("k64_mae", "f32")}


@pytest.mark.parametrize("variant", M.WRONG)
def test_wrong_twin_lies_outside_a_bound(variant):
    order = [FIRST.get(variant, ("base", "f32"))] + M.COMBOS
    for name, cd in order:
        g, s, u, failed = verdict(name, cd, variant, opts=("probe", "rmsprop"))
        if failed or max(g, s, u) > 1.0:
            print("MLP_WRONG %s rejected on %s %s: grad %.3g stats %.3g update %.3g %s" % (variant, name, cd, g, s, u, failed))
            return
    pytest.fail("%s lies inside every bound on every case" % variant)


@pytest.mark.parametrize("variant", ["shadow_row_major", "loss_grad_unmasked", "count_from_t", "db_last_block"])
def test_wrong_twin_is_rejected_in_16_bit_too(variant):
    """the bugs whose size does not shrink with the compute dtype's bound show on the 16-bit cases as well"""
    g, s, u, failed = verdict("base", "bf16", variant, opts=("probe", "rmsprop"))
    assert failed or max(g, s, u) > 1.0


@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_input_conditions_hold_without_exclusion(name, cd):
    c, ref = M.make_case(name), ref_of(name, cd)
    cond = M.conditions(c, cd, ref)
    assert cond["count"].size > 0
    for key, ok in cond.items():
        assert ok.all(), "%s %s: %s fails at %d of %d elements" % (name, cd, key, int((~ok).sum()), ok.size)
    if c.loss in ("mae", "huber"):
        assert c.loss in cond
    if c.loss == "huber":                                  # both branches are taken
        a = np.abs(ref.e[ref.e != 0])
        assert (a < c.delta).sum() > 10 and (a > c.delta).sum() > 10
    if c.act == "relu":                                    # both sides of 0
        z = ref.f.z[0][ref.f.live[0]]
        assert 0.2 < (z > 0).mean() < 0.8
    # the layout every case uses: a non-monotone selection with repeats from taller arrays, ld_x != ld_t, both > N
    assert c.n_src > c.B and c.ld_x > c.N and c.ld_t > c.N and c.ld_x != c.ld_t
    if c.B >= 3:
        assert len(set(c.rows.tolist())) < c.B and (np.diff(c.rows) < 0).any() and (np.diff(c.rows) > 0).any()
    # entries of every kind: m = 1 with and without a target, a target without m
    rows = c.rows[:c.B]
    m, t = c.om[rows, :c.N], c.tg[rows, :c.N]
    if c.B > 1:
        assert ((m != 0) & (t != 0)).any() and ((m != 0) & (t == 0)).any() and ((m == 0) & (t != 0)).any()
    if c.keep < 1.0:
        for mk in c.masks:
            assert abs(mk.mean() - c.keep) <= M.mask_share_bound(mk.size, c.keep)


def test_table_reaches_the_edges_it_claims():
    c = {n: M.make_case(n) for n in M.NAMES}
    assert all(w == 64 for w in (c["k64"].Np, *c["k64"].hidden_p)) and c["k64"].k == 1 and c["k64_b1"].B == 1
    assert c["ktail"].Np == 320 and c["ktail"].Np // 32 > 8
    assert c["rows16"].Bp // 32 == 16 and c["rows16"].B % 32 and c["rows16"].B % 4 == 0 and c["base"].B % 4
    assert c["deep8"].L == M.MAX_HIDDEN and c["deep8"].B == c["deep8"].Bp and 1 + 2 * (2 * 8 + 1) + 1 > M.TRACE_WORDS
    w = c["wide"]
    assert (w.Bp // 32) * (w.Np // 32) == 544 and 544 * 4 > 2048
    assert c["base_drop"].keep == 0.8 and c["deep3_drop"].keep == 0.5 and c["deep3_drop"].L == 3


def sizes_of(c):
    d, _ = M.dims(c)
    s = {"rows": c.B, "out_mask": c.om.size, "targets": c.tg.size, "stats": 4 + c.Bp, "barrier": 2,
         "work": 4 * M.workspace_floats(c)}
    for j in range(c.k):
        s["x%d" % j] = c.x[j].size
    for i in range(c.L + 1):
        s["W%d" % i], s["b%d" % i] = d[i] * d[i + 1], d[i + 1]
    for i in range(c.L):
        s["mask%d" % i] = c.Bp * d[i + 1]
    return s


def test_validation_refuses_what_the_kernel_would_trust():
    c = M.make_case("base_drop")
    s = sizes_of(c)
    M.validate(c, s, cus=256, wgs=256)
    bad_rows = c.rows.copy()
    bad_rows[5] = c.n_src
    cases = [
        (SimpleNamespace(**dict(vars(c), rows=bad_rows)), s, dict(cus=256)),
        (c, dict(s, stats=3 + c.Bp), dict(cus=256)),
        (c, dict(s, W1=s["W1"] - 1), dict(cus=256)),
        (c, dict(s, mask0=s["mask0"] - 1), dict(cus=256)),
        (c, dict(s, x1=s["x1"] - c.ld_x), dict(cus=256)),
        (c, dict(s, work=s["work"] - 4), dict(cus=256)),
        (c, s, dict(cus=256, wgs=257)),
        (c, s, dict(cus=256, work_bytes=s["work"] + 256)),
        (SimpleNamespace(**dict(vars(c), Bp=576)), s, dict(cus=256)),
    ]
    for cc, ss, kw in cases:
        with pytest.raises(ValueError):
            M.validate(cc, ss, **kw)
