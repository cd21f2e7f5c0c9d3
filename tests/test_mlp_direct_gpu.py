"""ocf_mlp_step called directly through the library's C entry point, one launch at a time, on the table of
tests/mlp_ref.py (the smallest shapes that reach each edge of csrc/ocf_mlp.hip: every K = 64, K = 320 tails, ten
column blocks, 16 row blocks, eight hidden layers, 544 output tiles / 2,176 stats slots, B = 1, dropout at two keep
rates, the four losses), against its NumPy fp64 reference under the bounds derived there.

The gradient is observed exactly: a launch with Adam, beta_1 = 0.5 and zero slots leaves sW1 = sb1 = g / 2, so
2 * slot is the kernel's fp32 gradient of every element; it is compared element by element, nothing excluded.  The
four optimizers then run from nonzero slots and are compared with epilogue_ref.opt_update in fp64 applied to that
recovered gradient (opt_limit).  Without tolerance: the count, the shadows (RNE of the updated weight at shadow_index,
row-major and blocked), every padding and every word after every buffer, the inputs, the barrier words (zero after
every launch), ocf_check_async, the dropout masks (against ocf_splitk_bias_act's for (seed, stream + i) and the NumPy
Philox), results across wgs in {1, 4, default, the CU count}, and a second launch on a dirty workspace after a first
on a NaN-filled one.  Every host-side argument check must raise before any launch.
Every buffer is validated on the host (mlp_ref.validate) before its first launch.  tests/test_mlp_ref.py shows on the
CPU that the bounds accept a float32 restatement of the kernel and reject fourteen plausible bugs.

Worst observed |err| / bound over all cases (MI355X, this file's own run; recorded, not used to set a bound):

    dtype    gradients            updates (opt_limit)    statistics
    f32      0.012  (k64_mae)     0.011  (deep8, Adam)   0.010  (k64_mae)
    f16      0.50   (k64)         0.0096 (base_mae)      0.071  (k64)
    bf16     0.77   (k64_b1)      0.010  (ktail)         0.13   (k64_huber)
    Bit-for-bit comparisons (grids, dirty workspace, paddings, tails, masks, shadows, counts): no mismatch.
    222 tests in 3.7 s.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import epilogue_ref as R
import mlp_ref as M
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

TORCH16 = {"f16": torch.float16, "bf16": torch.bfloat16}
TAIL = 64                                # canary elements after every buffer
SENTINEL = 123.0                         # a shadow's live elements before the launch
OPT_KIND = {"probe": _lib.OPT_ADAM, "sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "rmsprop": _lib.OPT_RMSPROP,
            "adam": _lib.OPT_ADAM}


def cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Buf:
    """a device buffer of n elements followed by TAIL canary elements (bytes 0xEE), with its host image"""

    def __init__(self, host, dtype16=None):
        h = np.ascontiguousarray(host).ravel()
        self.n = h.size
        if dtype16 is not None:          # float32 values stored in a 16-bit type
            full = np.concatenate([h.astype(np.float32), np.full(TAIL, SENTINEL, np.float32)])
            self.t = torch.from_numpy(full).to(dtype16).cuda()
            self.image = self.t.float().cpu().numpy()
        else:
            full = np.empty(self.n + TAIL, h.dtype)
            full[:self.n] = h
            full[self.n:].view(np.uint8)[:] = 0xEE
            self.t = torch.from_numpy(full).cuda()
            self.image = full
        self.dtype16 = dtype16

    def ptr(self):
        return self.t.data_ptr()

    def restore(self):
        src = torch.from_numpy(self.image)
        self.t.copy_(src.to(self.dtype16) if self.dtype16 is not None else src)

    def read(self):
        """(the n elements, the tail still as it was)"""
        got = (self.t.float() if self.dtype16 is not None else self.t).cpu().numpy()
        tail_ok = np.array_equal(got[self.n:].view(np.uint8), self.image[self.n:].view(np.uint8))
        return got[:self.n], tail_ok

    def unchanged(self):
        got, tail_ok = self.read()
        return tail_ok and np.array_equal(got.view(np.uint8), self.image[:self.n].view(np.uint8))


class Rig:
    """one case's device buffers for one (compute dtype, optimizer, shadow layout), validated before any launch"""

    def __init__(self, name, cd, opt, blocked=0, trace=False):
        c = self.c = M.make_case(name)
        self.cd, self.opt, self.blocked = cd, opt, blocked
        d, _ = M.dims(c)
        st = self.st = M.init_state(c, opt)
        self.inputs = dict(rows=Buf(c.rows), out_mask=Buf(c.om), targets=Buf(c.tg))
        for j in range(c.k):
            self.inputs["x%d" % j] = Buf(c.x[j])
        self.state = {}
        for i in range(c.L + 1):
            for key, arr in (("W", st.W), ("b", st.b), ("sW1", st.sW1), ("sW2", st.sW2), ("sb1", st.sb1), ("sb2", st.sb2)):
                if arr[i] is not None:
                    self.state["%s%d" % (key, i)] = Buf(arr[i])
            if cd != "f32":
                # the padding already holds the weight's rounding (the update rewrites every element), the live part a sentinel
                sh = M.shadow_of(np.where(M.live_w(c, i), SENTINEL, st.W[i]).astype(np.float32), cd, blocked)
                self.state["shadow%d" % i] = Buf(sh, TORCH16[cd])
        self.masks = [Buf(np.full(c.Bp * d[i + 1], 0xEE, np.uint8)) for i in range(c.L)] if c.keep < 1.0 else []
        self.stats = Buf(np.full(4 + c.Bp, np.nan, np.float32))
        self.barrier = Buf(np.zeros(2, np.int32))
        self.trace = Buf(np.zeros(M.TRACE_WORDS, np.int64)) if trace else None
        a = self.args = _lib.OcfMlpStepArgs()
        a.n_hidden, a.B, a.Bp, a.N, a.Np, a.k_blocks = c.L, c.B, c.Bp, c.N, c.Np, c.k
        for i in range(c.L):
            a.hidden[i], a.hidden_p[i] = c.hidden[i], c.hidden_p[i]
        for j in range(c.k):
            a.x[j] = self.inputs["x%d" % j].ptr()
        a.ld_x, a.rows, a.ld_t = c.ld_x, self.inputs["rows"].ptr(), c.ld_t
        a.out_mask, a.targets = self.inputs["out_mask"].ptr(), self.inputs["targets"].ptr()
        for i in range(c.L + 1):
            for key in ("W", "b", "sW1", "sW2", "sb1", "sb2", "shadow"):
                buf = self.state.get("%s%d" % (key, i))
                getattr(a, key)[i] = buf.ptr() if buf is not None else None
        a.shadow_blocked, a.act, a.compute_dtype = blocked, M.ACT_CODE[c.act], M.DT_CODE[cd]
        kind, h = M.hyper_of(opt)
        a.opt = _lib.OcfOptParams(OPT_KIND[opt], h["lr"], h["eps"], h["rho"], h["beta2"], 0.0, c.gscale)
        a.keep, a.seed, a.stream = c.keep, M.SEED, M.STREAM
        for i, mk in enumerate(self.masks):
            a.mask[i] = mk.ptr()
        a.loss, a.loss_param = M.LOSS_CODE[c.loss], c.delta
        a.stats, a.barrier = self.stats.ptr(), self.barrier.ptr()
        a.trace = self.trace.ptr() if trace else None
        need = int(_lib.load().ocf_mlp_step_workspace(ctypes.byref(a)))
        assert need > 0, _lib.load().ocf_last_error()
        self.work_bytes = need
        self.work = torch.full((need // 4 + 1024,), float("nan"), device="cuda")
        self.work[need // 4:] = -1.0
        a.work, a.work_bytes = self.work.data_ptr(), need
        sizes = {k: b.n for k, b in {**self.inputs, **self.state}.items()}
        sizes.update({"mask%d" % i: b.n for i, b in enumerate(self.masks)})
        sizes.update(stats=self.stats.n, barrier=self.barrier.n, work=need)
        if trace:
            sizes["trace"] = self.trace.n
        self.sizes = sizes
        M.validate(c, sizes, cu_count(), 0, need)

    def restore(self):
        """the launch's starting state again; the workspace is left as the last launch left it"""
        for b in (*self.state.values(), *self.masks, self.stats):
            b.restore()

    def launch(self, wgs=0):
        c = self.c
        M.validate(c, self.sizes, cu_count(), wgs, self.work_bytes)
        self.args.wgs = wgs
        _lib.call("ocf_mlp_step", ctypes.byref(self.args), cur_stream())
        torch.cuda.synchronize()
        _lib.call("ocf_check_async")
        bar, bar_tail = self.barrier.read()
        assert not bar.any() and bar_tail, "barrier words %s after the launch" % bar.tolist()
        assert bool((self.work[self.work_bytes // 4:] == -1.0).all()), "a write past the workspace"
        for key, b in self.inputs.items():
            assert b.unchanged(), "input %s was written" % key
        out = SimpleNamespace(shadow=[None] * (c.L + 1), masks=[])
        for key in ("W", "b", "sW1", "sW2", "sb1", "sb2", "shadow"):
            vals = []
            for i in range(c.L + 1):
                b = self.state.get("%s%d" % (key, i))
                if b is None:
                    vals.append(None)
                    continue
                got, tail_ok = b.read()
                assert tail_ok, "a write past %s%d" % (key, i)
                vals.append(got.reshape(M.w_shape(c, i)) if key in ("W", "sW1", "sW2") else got)
            setattr(out, key, vals)
        d, _ = M.dims(c)
        for i, mk in enumerate(self.masks):
            got, tail_ok = mk.read()
            assert tail_ok, "a write past mask %d" % i
            out.masks.append(got.reshape(c.Bp, d[i + 1]))
        out.stats, tail_ok = self.stats.read()
        assert tail_ok, "a write past the 4 + Bp floats of the stats row"
        if self.trace is not None:
            out.trace, tail_ok = self.trace.read()
            assert tail_ok, "a write past the 24 trace words"
        return out


def same_bits(a, b):
    """every output of two launches, bit for bit -> the list of those that differ"""
    bad = []
    for key in ("W", "b", "sW1", "sW2", "sb1", "sb2", "shadow", "masks"):
        for i, (x, y) in enumerate(zip(getattr(a, key), getattr(b, key))):
            if x is not None and not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
                bad.append("%s%d (%d elements)" % (key, i, int((x.view(np.uint8) != y.view(np.uint8)).sum())))
    if not np.array_equal(a.stats.view(np.int32), b.stats.view(np.int32)):
        bad.append("stats %s" % np.flatnonzero(a.stats.view(np.int32) != b.stats.view(np.int32))[:8].tolist())
    return bad


@functools.lru_cache(maxsize=None)
def probe(name, cd):
    """the gradient-exposing launch (Adam, beta_1 = 0.5, zero slots; default grid, row-major shadows, NaN-filled
    workspace): (rig, outputs with gW / gb recovered, the fp64 reference on the device's masks)"""
    rig = Rig(name, cd, "probe", 0, trace=name == "deep8")
    out = rig.launch()
    c = rig.c
    out.gW = [2.0 * s for s in out.sW1]
    out.gb = [2.0 * s for s in out.sb1]
    ref = M.reference(c, cd, masks=out.masks if c.keep < 1.0 else None)
    return rig, out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_gradient_and_statistics_against_fp64(gpu, name, cd):
    rig, out, ref = probe(name, cd)
    c = rig.c
    for key, ok in M.conditions(c, cd, ref).items():
        assert ok.all(), (key, int((~ok).sum()))
    g = M.check_grads(c, ref, out)
    s, count_ok = M.check_stats(c, ref, out.stats)
    print("MLP_RATIO grad %s %s %.4g" % (cd, name, g))
    print("MLP_RATIO stats %s %s %.4g" % (cd, name, s))
    assert g <= 1.0, "%s %s: worst gradient |err| / bound %.4g" % (name, cd, g)
    assert s <= 1.0, "%s %s: worst statistics |err| / bound %.4g" % (name, cd, s)
    assert count_ok, "count %r, reference %d" % (out.stats[2], ref.count)
    # the probe's own update (Adam from zero slots), its padding and its row-major shadows
    u, pad_ok = M.check_update(c, "probe", rig.st, out.gW, out.gb, out)
    assert u <= 1.0 and pad_ok, (u, pad_ok)
    if cd != "f32":
        assert M.check_shadows(c, cd, out, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", R.OPTS)
@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_update_against_fp64(gpu, name, cd, opt):
    """nonzero slots (their padding zero), epilogue_ref.HYPER with l2 = 0; blocked shadows"""
    _, g, _ = probe(name, cd)
    rig = Rig(name, cd, opt, blocked=1)
    out = rig.launch()
    c = rig.c
    u, pad_ok = M.check_update(c, opt, rig.st, g.gW, g.gb, out)
    print("MLP_RATIO update %s %s %s %.4g" % (cd, name, opt, u))
    assert u <= 1.0, "%s %s %s: worst |err| / opt_limit %.4g" % (name, cd, opt, u)
    assert pad_ok, "padding of W, b or a slot changed"
    if cd != "f32":
        assert M.check_shadows(c, cd, out, 1), "a blocked shadow is not the rounding of its updated weight"
    assert np.array_equal(out.stats.view(np.int32), g.stats.view(np.int32))       # (the optimizer does not reach the stats)


@pytest.mark.gpu
@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_results_do_not_depend_on_the_grid(gpu, name, cd):
    """wgs = 1 (every phase's side work after the tiles), 4, the CU count (idle workgroups take the side work)
    against the default grid, bit for bit: every sum has a fixed order"""
    rig, base, _ = probe(name, cd)
    for wgs in (1, 4, cu_count()):
        rig.restore()
        out = rig.launch(wgs)
        bad = same_bits(base, out)
        assert not bad, "wgs = %d differs from the default grid in %s" % (wgs, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name,cd", M.COMBOS, ids=M.COMBO_IDS)
def test_no_stale_scratch_and_reproducible(gpu, name, cd):
    """the probe ran on a NaN-filled workspace; the same launch from the restored state on the workspace it left gives
    the same bits (run-to-run reproducible, nothing read that the launch did not write first)"""
    rig, base, _ = probe(name, cd)
    assert all(np.isfinite(x).all() for x in (*base.W, *base.b, *base.sW1, *base.sW2, base.stats[:4 + rig.c.Bp]))
    rig.restore()
    bad = same_bits(base, rig.launch())
    assert not bad, "the second launch differs in %s" % bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base_drop", "deep3_drop"])
def test_dropout_masks(gpu, name):
    """mask[i] = ocf_splitk_bias_act's mask for (seed, stream + i) at M = Bp, N = ld = hidden_p[i], bit for bit (and the
    NumPy Philox of mlp_ref); its share of ones within 6 binomial standard deviations of keep; all Bp x hidden_p[i]
    elements written"""
    c = M.make_case(name)
    _, out, _ = probe(name, c.dtypes[0])
    _, out2, _ = probe(name, c.dtypes[1])
    for i, w in enumerate(c.hidden_p):
        slab = torch.zeros(c.Bp * w, device="cuda")
        bias = torch.zeros(w, device="cuda")
        mk = torch.full((c.Bp * w,), 0xEE, dtype=torch.uint8, device="cuda")
        _lib.call("ocf_splitk_bias_act", slab.data_ptr(), 1, c.Bp * w, c.Bp, w, w, bias.data_ptr(), 0, c.keep, M.SEED,
                  M.STREAM + i, None, mk.data_ptr(), None, None, 0, c.Bp, w, cur_stream())
        torch.cuda.synchronize()
        want = mk.cpu().numpy().reshape(c.Bp, w)
        assert set(np.unique(want).tolist()) <= {0, 1}
        assert np.array_equal(out.masks[i], want) and np.array_equal(out2.masks[i], want)
        assert np.array_equal(want, c.masks[i])
        assert abs(want.mean() - c.keep) <= M.mask_share_bound(want.size, c.keep)


@pytest.mark.gpu
def test_trace_stays_inside_its_24_words(gpu):
    """eight hidden layers make 36 phase marks: the first 24 are recorded, non-decreasing; nothing after them is written
    (Rig.launch checks the canary words)"""
    _, out, _ = probe("deep8", "f32")
    assert (out.trace > 0).all() and (np.diff(out.trace) >= 0).all(), out.trace.tolist()


BAD_ARGS = {
    "Bp = 576": ("probe", dict(Bp=576)),
    "Bp = 96": ("probe", dict(Bp=96)),
    "B = 0": ("probe", dict(B=0)),
    "B > Bp": ("probe", dict(B=65)),
    "ld_x < N": ("probe", dict(ld_x=39)),
    "ld_t < N": ("probe", dict(ld_t=39)),
    "adagrad without sW1": ("adagrad", ("sW1", 0)),
    "rmsprop without sb1": ("rmsprop", ("sb1", 1)),
    "adam without sW2": ("adam", ("sW2", 1)),
    "adam without sb2": ("adam", ("sb2", 0)),
    "keep < 1 without a mask": ("probe", dict(keep=0.8)),
    "keep = 0": ("probe", dict(keep=0.0)),
    "keep < 0": ("probe", dict(keep=-0.25)),
    "keep > 1": ("probe", dict(keep=1.5)),
    "workspace one byte short": ("probe", "short"),
    "wgs above the CU count": ("probe", "wgs"),
    "l2 != 0": ("probe", "l2"),
    "compute dtype 7": ("probe", dict(compute_dtype=7)),
    "loss code 9": ("probe", dict(loss=9)),
    "Huber without delta": ("probe", dict(loss=2, loss_param=0.0)),
    "no hidden layer": ("probe", dict(n_hidden=0)),
    "nine hidden layers": ("probe", dict(n_hidden=9)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_argument_checks_raise_before_any_launch(gpu, what):
    """host-side only: _lib.OcfError, and the parameters, slots, stats row and barrier words as they were"""
    opt, kw = BAD_ARGS[what]
    rig = Rig("k64", "f32", opt)
    a = rig.args
    if kw == "short":
        a.work_bytes = rig.work_bytes - 1
    elif kw == "wgs":
        a.wgs = cu_count() + 1
    elif kw == "l2":
        a.opt.l2 = 0.01
    elif isinstance(kw, tuple):
        getattr(a, kw[0])[kw[1]] = None
    else:
        for k, v in kw.items():
            setattr(a, k, v)
    with pytest.raises(_lib.OcfError):
        _lib.call("ocf_mlp_step", ctypes.byref(a), cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")
    for key, b in {**rig.state, "stats": rig.stats, "barrier": rig.barrier}.items():
        assert b.unchanged(), key
    assert bool(torch.isnan(rig.work[:rig.work_bytes // 4]).all())


@pytest.mark.gpu
def test_workspace_size_is_the_documented_layout(gpu):
    for name in M.NAMES:
        c = M.make_case(name)
        a = _lib.OcfMlpStepArgs()
        a.n_hidden, a.B, a.Bp, a.N, a.Np, a.k_blocks, a.keep = c.L, c.B, c.Bp, c.N, c.Np, c.k, c.keep
        for i in range(c.L):
            a.hidden[i], a.hidden_p[i] = c.hidden[i], c.hidden_p[i]
        assert int(_lib.load().ocf_mlp_step_workspace(ctypes.byref(a))) == 4 * M.workspace_floats(c)
    assert int(_lib.load().ocf_mlp_step_workspace(None)) == -1
