"""NumPy restatements of ocf_mlp_step (include/ocf.h OcfMlpStepArgs, csrc/ocf_mlp.hip): the table of direct calls
tests/test_mlp_direct_gpu.py launches, the host-side validation of everything the kernel trusts, an fp64 reference
of one whole step with a running error bound for every value it produces, a float32 restatement in the kernel's
operation order (`twin`) and a list of deliberately wrong variants of it.  tests/test_mlp_ref.py shows on the CPU
that the bounds accept the float32 restatement and reject every wrong variant, and that the input conditions hold.

The reference reads the same buffers as the kernel: the caller's source arrays through `rows`, the padded weights,
the dropout masks the caller supplies.  The operands that are INPUTS of the launch (x, W) are rounded to the compute
dtype exactly as the kernel stages them (a deterministic rounding of a known float32 value, so the reference mirrors
it); every value the kernel computes itself (h, delta) stays fp64 in the reference and its staging is bounded.

Bounds (u = 2^-24, uc = the compute dtype's unit roundoff, 0 for f32; nothing tuned; E_q bounds |q - q_ref|):
  * staging an fp32 value q of bound E_q to the compute dtype: S_q = E_q + uc (|q_ref| + E_q) (+ 2^-25 for f16, the
    subnormal grid: epilogue_ref.round_tol); this is what lets an operand land on the other side of a rounding
    boundary: the kernel's q may differ from the reference's by E_q before it is rounded;
  * a product sum over K terms of staged operands, accumulated in fp32 by the MFMAs and the wave-order sum:
    S_A |B| + |A| S_B + S_A S_B for the operands, plus epilogue_ref.product_tol(K, (|A| + S_A)(|B| + S_B)) = 4 K u mag
    for the accumulation (any order of K terms is within (K - 1) u mag);
  * a sum or difference: the terms' bounds plus u |result|; a product a b: |a| E_b + |b| E_a + E_a E_b plus
    u (|a b| + that); an fp32 sum of n terms that are not products: the terms' bounds + 1.01 (n + 2) u sum|terms|
    (gather_ref's form);
  * an activation: its Lipschitz constant (1/4 sigmoid, else 1) times the input's bound plus 4 fp32 ulp of the
    output (product_tol's term for __expf / tanhf); act' from the activation a: |d act'/da| E_a + E_a^2 + 2 u (the
    two roundings of 1 - a a or a (1 - a), absolute: near saturation the result is far below its terms); relu' has
    no error because the input conditions keep every pre-activation 16 bounds away from 0;
  * dropout: h = (a / keep) mask: E_a / keep + 2 u |h|; mask / keep: u mask / keep;
  * the loss: y = m (v + b), e = y - t by the sum / product rules; rho' is 1-Lipschitz for Huber and log-cosh (+ 8 u
    for expm1f and the division), exact for MAE (the input conditions keep |e| 16 bounds away from 0) and the
    identity for MSE; rho is |rho'|-Lipschitz plus its evaluation: 4 u rho, for log-cosh 8 u (|e| + 1) (a + log1p
    (exp(-2 a)) - ln 2 has terms of that size; the polynomial's truncation 2e-8 lies inside it);
  * gradients: the column sums of delta (n = Bp terms) and the dW product sums (K = Bp), times gscale (+ u |g|).
The optimizer is compared with epilogue_ref.opt_update in fp64 on the kernel's OWN fp32 gradient (recovered exactly
from an Adam launch with beta_1 = 0.5 and zero slots: m = 0.5 g) under epilogue_ref.opt_limit, so no update inherits
the gradient's bound.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import epilogue_ref as R
import loss_ref as LR

U = 2.0 ** -24
ULP4 = 4.0 * 2.0 ** -23
LIP = {"sigmoid": 0.25, "tanh": 1.0, "relu": 1.0, "linear": 1.0}
ACT_CODE = {"linear": 0, "sigmoid": 1, "tanh": 2, "relu": 3}            # ocf.h OCF_ACT_*
LOSS_CODE = {"mse": 0, "mae": 1, "huber": 2, "logcosh": 3}               # ocf.h OCF_LOSS_*
DT_CODE = {"f32": 0, "f16": 1, "bf16": 2}                                # ocf.h OCF_F32 / F16 / BF16
KC = {"f32": 32, "f16": 64, "bf16": 64}                                  # ocf_mlp.hip Geo<CT>::KC
TT, WAVES, MAX_HIDDEN, MAX_BP, TRACE_WORDS = 32, 4, 8, 512, 24
SEED, STREAM = 0x1234ABCD5678, 48                                        # the dropout cases' Philox seed / stream
HUBER_DELTA = 1.25                                                       # (no half-star target lies on it)
MARGIN = 0.3                                                             # the targets keep |T + y|, |e|, ||e| - d| above it
COND = 16.0                                                              # ... which must be COND bounds
PROBE = dict(R.HYPER, rho=0.5, l2=0.0)                                   # the Adam launch that exposes the gradient


def _case(hidden, hidden_p, k, N, Np, B, Bp, act, dtypes, keep=1.0, loss="mse", s_out=0.02, amp=2.5, seed=1):
    return SimpleNamespace(hidden=tuple(hidden), hidden_p=tuple(hidden_p), k=k, N=N, Np=Np, B=B, Bp=Bp, act=act,
                           dtypes=tuple(dtypes), keep=keep, loss=loss, s_out=s_out, amp=amp, seed=seed)


DEEP = (17, 64, 33, 50, 21, 64, 40, 29)
_BASE = dict(hidden=(200, 96), hidden_p=(256, 128), k=2, N=100, Np=128, B=118, Bp=128, act="tanh")
_K64 = dict(hidden=(33,), hidden_p=(64,), k=1, N=40, Np=64, B=37, Bp=64, act="sigmoid")
# the issue's table: the smallest shapes that reach each edge of the kernel
TABLE = {
    "base": _case(dtypes=("f32", "f16", "bf16"), **_BASE),
    "k64": _case(dtypes=("f32", "f16", "bf16"), s_out=0.05, **_K64),                  # every K = 64: one short chunk
    "k64_b1": _case(dtypes=("f32", "bf16"), s_out=0.05, **dict(_K64, B=1)),
    "ktail": _case((300,), (320,), 1, 300, 320, 200, 256, "relu", ("f32", "bf16"), s_out=0.004),   # K = 320 tails; 10 column blocks
    "rows16": _case((64,), (64,), 3, 50, 64, 500, 512, "tanh", ("f32", "f16")),       # 16 row blocks; dW K = 512
    "deep8": _case(DEEP, (64,) * 8, 1, 30, 64, 64, 64, "tanh", ("f32",)),             # 17 barriers, a full batch
    "wide": _case((20,), (64,), 1, 1030, 1088, 512, 512, "sigmoid", ("f32", "f16"), s_out=0.05),   # 544 tiles, 2,176 slots
    "base_drop": _case(dtypes=("f32", "bf16"), keep=0.8, **_BASE),
    "deep3_drop": _case(DEEP[:3], (64,) * 3, 1, 30, 64, 64, 64, "tanh", ("f32", "f16"), keep=0.5),
}
for _l in ("mae", "huber", "logcosh"):
    TABLE["k64_" + _l] = _case(dtypes=("f32", "bf16"), loss=_l, s_out=0.05, **_K64)
    TABLE["base_" + _l] = _case(dtypes=("f16",), loss=_l, **_BASE)
NAMES = tuple(TABLE)
COMBOS = [(n, cd) for n in NAMES for cd in TABLE[n].dtypes]
COMBO_IDS = ["%s-%s" % nc for nc in COMBOS]


def dims(c):
    """(padded, real) widths: [k Np, hidden_p.., Np] / [k N, hidden.., N]  (ocf_mlp.hip dims_of)"""
    return [c.k * c.Np, *c.hidden_p, c.Np], [c.k * c.N, *c.hidden, c.N]


def w_shape(c, i):
    """weight i in the engine's padded layout: [in][out], the output layer transposed [Np][in]"""
    d, _ = dims(c)
    return (d[i + 1], d[i]) if i == len(c.hidden) else (d[i], d[i + 1])


def live_w(c, i):
    """the real elements of weight i (input block j's column n at row j Np + n)"""
    d, r = dims(c)
    rin = ((np.arange(d[0]) % c.Np) < c.N) if i == 0 else (np.arange(d[i]) < r[i])
    m = np.outer(rin, np.arange(d[i + 1]) < r[i + 1])
    return m.T if i == len(c.hidden) else m


def gscale(c):
    return float(np.float32((1.0 if c.loss != "mse" else 2.0) / (c.B * c.N)))


# ---- Philox4x32-10 (ocf_common.h philox_uniform) and the dropout masks ------------------------------------------
def philox_uniform(seed, stream, idx):
    M32 = np.uint64(0xFFFFFFFF)
    idx = np.asarray(idx, np.uint64)
    c0, c1 = idx & M32, idx >> np.uint64(32)
    c2 = np.full_like(idx, np.uint64(stream) & M32)
    c3 = np.full_like(idx, np.uint64(stream) >> np.uint64(32))
    k0, k1 = np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return (c0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_masks(c, shared_stream=False):
    """mask[i] u8 [Bp][hidden_p[i]] = floor(keep + U(seed, stream + i, m hidden_p[i] + n)) in float32"""
    out = []
    for i, w in enumerate(c.hidden_p):
        u = philox_uniform(SEED, STREAM + (0 if shared_stream else i), np.arange(c.Bp * w, dtype=np.uint64))
        out.append(np.floor(np.float32(c.keep) + u).astype(np.uint8).reshape(c.Bp, w))
    return out


def mask_share_bound(n, keep):
    """|share of ones - keep| of n Bernoulli(keep) draws: 6 standard deviations (two-sided tail 2e-9) + the 2^-24
    grid of the 24-bit uniform"""
    return 6.0 * np.sqrt(keep * (1.0 - keep) / n) + 2.0 ** -24


# ---- the cases' data ------------------------------------------------------------------------------------------
def _weights(c, rng):
    d, r = dims(c)
    L = len(c.hidden)
    W, b = [], []
    for i in range(L + 1):
        lw = live_w(c, i)
        if c.act == "relu" and i == 0:
            # dyadic: x in half-stars, W_0 in sixteenths, b_0 an odd multiple of 1/64: every pre-activation is exact
            # in every compute dtype and at least 1/64 from 0
            w = rng.randint(-2, 3, size=lw.shape) * (rng.rand(*lw.shape) < 0.5) / 16.0
            bb = (2 * rng.randint(0, 8, size=d[1]) + 1) * rng.choice([-1.0, 1.0], size=d[1]) / 64.0
        elif i == L:
            w = c.s_out * rng.randn(*lw.shape)
            bb = rng.uniform(-0.6, 0.6, size=d[i + 1])
        else:
            fan = r[i] * (0.15 if i == 0 else 0.4)
            s = 1.0 / np.sqrt(fan)
            if i > 0:
                s = min(s, c.amp / (0.8 * r[i]))          # sum_k |W[k][n]| ~ amp: the bound's growth per layer
            w = s * rng.randn(*lw.shape)
            bb = 0.3 * rng.randn(d[i + 1])
        w = np.where(lw, w, 0.37).astype(np.float32)       # padding: finite, never part of a result
        bb = np.where(np.arange(d[i + 1]) < r[i + 1], bb, -7.5).astype(np.float32)
        W.append(w)
        b.append(bb)
    return W, b


@functools.lru_cache(maxsize=None)
def make_case(name):
    """the case's host buffers (read-only, cached): source arrays taller than the batch with NaN beyond column N,
    a non-monotone row selection with repeats, ld_x != ld_t, both > N; targets placed MARGIN away from every
    decision the kernel takes on them (asserted per dtype by `conditions`)"""
    c = SimpleNamespace(**vars(TABLE[name]), name=name)
    rng = np.random.RandomState(1000 + c.seed + len(name) * 7 + c.N)
    c.L = len(c.hidden)
    c.n_src, c.ld_x, c.ld_t = c.B + 9, c.N + 5, c.N + 11
    rows = rng.randint(0, c.n_src, size=c.B)
    if c.B >= 3:
        rows[0], rows[1], rows[2] = c.n_src - 1, c.n_src - 1, 0      # a repeat, then a step down
    c.rows = rows.astype(np.int64)
    c.x = []
    for j in range(c.k):
        on = rng.rand(c.n_src, c.N) < (0.1 if c.act == "relu" else 0.3)
        stars = rng.randint(1, 11, size=on.shape) / 2.0
        v = (stars if c.act == "relu" else stars * 0.2) if j == 0 else (1.0 if j == 1 else 0.5 * rng.randn(*on.shape))
        xa = np.full((c.n_src, c.ld_x), np.nan, np.float32)
        xa[:, :c.N] = np.where(on, v, 0.0)
        c.x.append(xa)
    c.W, c.b = _weights(c, rng)
    c.masks = philox_masks(c) if c.keep < 1.0 else None
    c.delta = HUBER_DELTA if c.loss == "huber" else 0.0
    c.gscale = gscale(c)
    # output mask / targets: m = 1 on a quarter of the entries (a seventh of them with t = 0), t != 0 under m = 0 on a few
    m = (rng.rand(c.n_src, c.N) < 0.25)
    t = np.where(m, rng.randint(1, 11, size=m.shape) / 2.0, 0.0)
    zero_t = m & (rng.rand(*m.shape) < 0.15)
    stray = ~m & (rng.rand(*m.shape) < 0.03)
    t = np.where(stray, rng.randint(1, 11, size=m.shape) / 2.0, t)
    # the predictions the targets must keep clear of (fp64, f32 operands; the other dtypes move them far less than MARGIN)
    c.om = np.full((c.n_src, c.ld_t), np.nan, np.float32)
    c.tg = np.full((c.n_src, c.ld_t), np.nan, np.float32)
    c.om[:, :c.N], c.tg[:, :c.N] = 0.0, 0.0
    s = _forward(c, "f32", c.masks).s[:c.B, :c.N]

    def clear(tt):
        e, ty = s - tt[c.rows], s + tt[c.rows]
        good = (np.abs(ty) >= MARGIN)
        if c.loss in ("mae", "huber"):
            good &= np.abs(e) >= MARGIN
        if c.loss == "huber":
            good &= np.abs(np.abs(e) - c.delta) >= MARGIN
        ok = np.ones((c.n_src, c.N), bool)
        np.logical_and.at(ok, c.rows, good)
        return ok
    t = np.where(zero_t & clear(np.zeros_like(t)), 0.0, t)          # t = 0 under m = 1 only where y itself is clear
    for _ in range(16):
        bad = m & (t != 0) & ~clear(t)
        if not bad.any():
            break
        t = np.where(bad, np.where(t >= 7.0, 0.5, t + 0.5), t)
    c.om[:, :c.N], c.tg[:, :c.N] = m, t
    for a in (c.rows, c.om, c.tg, *c.x, *c.W, *c.b):
        a.setflags(write=False)
    return c


def init_state(c, opt):
    """the parameters and slots a launch starts from: zero slots for the probe, else epilogue_ref.opt_inputs' (their
    padding zero, as ocf.h asks); slots an optimizer does not have are None"""
    st = SimpleNamespace(W=[w.copy() for w in c.W], b=[x.copy() for x in c.b], sW1=[], sW2=[], sb1=[], sb2=[])
    d, r = dims(c)
    for i in range(c.L + 1):
        _, s1, s2 = R.opt_inputs(w_shape(c, i), 50 + i)
        _, t1, t2 = R.opt_inputs((d[i + 1],), 70 + i)
        lw, lb = live_w(c, i), np.arange(d[i + 1]) < r[i + 1]
        zero = opt == "probe"
        has1, has2 = opt in ("probe", "adagrad", "rmsprop", "adam"), opt in ("probe", "adam")
        st.sW1.append(np.where(lw & (not zero), s1, 0).astype(np.float32) if has1 else None)
        st.sW2.append(np.where(lw & (not zero), s2, 0).astype(np.float32) if has2 else None)
        st.sb1.append(np.where(lb & (not zero), t1, 0).astype(np.float32) if has1 else None)
        st.sb2.append(np.where(lb & (not zero), t2, 0).astype(np.float32) if has2 else None)
    return st


def hyper_of(opt):
    """(kind name, opt_update keywords) of a launch: the probe is Adam with beta_1 = 0.5"""
    h = dict(PROBE if opt == "probe" else dict(R.HYPER, l2=0.0), gscale=1.0)
    return ("adam" if opt == "probe" else opt), h


def workspace_floats(c):
    """ocf_mlp.hip layout(): every region rounded up to 256 bytes"""
    d, _ = dims(c)
    take = lambda n: (n * 4 + 255) // 256 * 256
    L, Bp = c.L, c.Bp
    n = sum(take(Bp * d[i + 1]) for i in range(L)) + sum(take(Bp * d[i + 1]) for i in range(L + 1))
    n += sum(take(d[i] * d[i + 1]) for i in range(1, L + 1)) + sum(take(Bp // TT * d[i + 1]) for i in range(L + 1))
    n += sum(2 * take(Bp * d[i + 1] if c.keep < 1.0 else 0) for i in range(L))
    n += take(c.Np // TT * Bp) + take(Bp // TT * (c.Np // TT) * WAVES * 3) + take(Bp // TT * (c.Np // TT) * WAVES)
    return n // 4


def validate(c, sizes, cus, wgs=0, work_bytes=None):
    """everything the kernel trusts, checked on the host before any launch; `sizes` holds the element counts of the
    buffers the caller allocated.  Raises ValueError: a case that fails is a test error, never a launch."""
    d, _ = dims(c)

    def need(key, n):
        if sizes.get(key, -1) < n:
            raise ValueError("%s: %s holds %s elements, the kernel needs %d" % (c.name, key, sizes.get(key), n))
    if not (1 <= c.L <= MAX_HIDDEN and 1 <= c.B <= c.Bp <= MAX_BP and c.Bp % 64 == 0 and c.Np % 64 == 0 and 1 <= c.k <= 3):
        raise ValueError("%s: shape outside ocf_mlp_step's limits" % c.name)
    if any(hp % 64 or not 1 <= h <= hp for h, hp in zip(c.hidden, c.hidden_p)) or not 1 <= c.N <= c.Np:
        raise ValueError("%s: widths" % c.name)
    if len(c.rows) < c.B or c.rows[:c.B].min() < 0 or c.rows[:c.B].max() >= c.n_src:
        raise ValueError("%s: rows outside the source arrays" % c.name)
    if c.ld_x < c.N or c.ld_t < c.N:
        raise ValueError("%s: ld < N" % c.name)
    need("rows", c.B)
    for j in range(c.k):
        need("x%d" % j, (c.n_src - 1) * c.ld_x + c.N)
    need("out_mask", (c.n_src - 1) * c.ld_t + c.N)
    need("targets", (c.n_src - 1) * c.ld_t + c.N)
    for i in range(c.L + 1):
        n = d[i] * d[i + 1]
        for key, m in (("W", n), ("sW1", n), ("sW2", n), ("shadow", n), ("b", d[i + 1]), ("sb1", d[i + 1]), ("sb2", d[i + 1])):
            if "%s%d" % (key, i) in sizes:
                need("%s%d" % (key, i), m)
        need("W%d" % i, n)
        need("b%d" % i, d[i + 1])
    if c.keep < 1.0:
        for i in range(c.L):
            need("mask%d" % i, c.Bp * d[i + 1])
    need("stats", 4 + c.Bp)
    need("barrier", 2)
    if "trace" in sizes:
        need("trace", TRACE_WORDS)
    wb = 4 * workspace_floats(c)
    if work_bytes is not None and work_bytes != wb:
        raise ValueError("%s: ocf_mlp_step_workspace says %d bytes, the layout %d" % (c.name, work_bytes, wb))
    need("work", wb)
    if not 0 <= wgs <= cus:
        raise ValueError("%s: wgs %d above the device's %d CUs" % (c.name, wgs, cus))


def shadow_index(rows, cols, blocked):
    """ocf_mlp.hip shadow_index over a whole [rows][cols] weight: the flat position of every element"""
    r, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    if not blocked:
        return r * cols + cc
    return ((r >> 6) * (cols >> 6) + (cc >> 6)) * 4096 + (r & 63) * 64 + (cc & 63)


def shadow_of(w, cd, blocked):
    """the flat compute-dtype shadow (as float32 values) of weight w: RNE of every element at shadow_index"""
    out = np.empty(w.size, np.float32)
    out[shadow_index(*w.shape, blocked).ravel()] = _round(w, cd).ravel()
    return out


# ---- the batch as the kernel sees it ---------------------------------------------------------------------------
def _batch(c, pad_live=False):
    """X [Bp][k Np], M, T [Bp][Np] gathered through rows, zero in every padding; live rows [Bp]"""
    rows = c.rows[:c.B]
    nb = c.B
    if pad_live:                                          # (wrong twin) the padded rows are copies of row B - 1
        rows = np.concatenate([rows, np.full(c.Bp - c.B, rows[-1])])
        nb = c.Bp
    X = np.zeros((c.Bp, c.k * c.Np), np.float32)
    for j in range(c.k):
        X[:nb, j * c.Np:j * c.Np + c.N] = c.x[j][rows, :c.N]
    M = np.zeros((c.Bp, c.Np), np.float32)
    T = np.zeros((c.Bp, c.Np), np.float32)
    M[:nb, :c.N], T[:nb, :c.N] = c.om[rows, :c.N], c.tg[rows, :c.N]
    return X, M, T, np.arange(c.Bp) < nb


def _stage(v, E, cd):
    """S_q of the docstring"""
    if cd == "f32":
        return E
    mag = np.abs(v) + E
    return E + np.where(mag > 0, R.round_tol(cd, mag), 0.0)


def _gemm(A, SA, B, SB, K):
    aA, aB = np.abs(A), np.abs(B)
    E = SA @ aB + aA @ SB + SA @ SB + R.product_tol(K, (aA + SA) @ (aB + SB))
    return A @ B, E


def _mul(a, Ea, b, Eb):
    v = a * b
    E = np.abs(a) * Eb + np.abs(b) * Ea + Ea * Eb
    return v, E + U * (np.abs(v) + E)


def _act_grad(act, a, Ea):
    if act in ("relu", "linear"):
        return R.act_grad(act, a), np.zeros_like(a)
    slope = 2.0 * np.abs(a) if act == "tanh" else np.abs(1.0 - 2.0 * a)
    return R.act_grad(act, a), slope * Ea + Ea * Ea + 2.0 * U


def _forward(c, cd, masks):
    """the forward pass in fp64 with its bounds, up to s = h W_L + b_L (before the output mask)"""
    d, r = dims(c)
    X, M, T, rows_live = _batch(c)
    Wr = [np.where(live_w(c, i), _round(c.W[i], cd), 0.0).astype(np.float64) for i in range(c.L + 1)]
    keep = float(np.float32(c.keep))
    f = SimpleNamespace(A=[_round(X, cd).astype(np.float64)], SA=[np.zeros(X.shape)], a=[], Ea=[], z=[], Ez=[], dm=[],
                        Edm=[], Wr=Wr, M=M.astype(np.float64), T=T.astype(np.float64), live=[], rows_live=rows_live)
    for i in range(c.L):
        live = np.outer(rows_live, np.arange(d[i + 1]) < r[i + 1])
        v, Ev = _gemm(f.A[i], f.SA[i], Wr[i], np.zeros(Wr[i].shape), d[i])
        z = np.where(live, v + c.b[i].astype(np.float64), 0.0)
        Ez = np.where(live, Ev + U * (np.abs(z) + Ev), 0.0)
        a = np.where(live, R.act(c.act, z), 0.0)
        Ea = np.where(live, LIP[c.act] * Ez + ULP4 * np.abs(a), 0.0)
        h, Eh = a, Ea
        if c.keep < 1.0:
            mk = masks[i].astype(np.float64)
            h = (a / keep) * mk
            Eh = (Ea / keep + 2.0 * U * np.abs(h)) * mk
            f.dm.append(mk / keep)
            f.Edm.append(U * mk / keep)
        f.z.append(z), f.Ez.append(Ez), f.a.append(a), f.Ea.append(Ea), f.live.append(live)
        f.A.append(h), f.SA.append(_stage(h, Eh, cd))
    live = np.outer(rows_live, np.arange(c.Np) < c.N)
    v, Ev = _gemm(f.A[c.L], f.SA[c.L], Wr[c.L].T, np.zeros(Wr[c.L].T.shape), d[c.L])
    f.s = np.where(live, v + c.b[c.L].astype(np.float64), 0.0)
    f.Es = np.where(live, Ev + U * (np.abs(f.s) + Ev), 0.0)
    f.live.append(live)
    return f


def _sum_bound(E, terms, n, axis=None):
    return E.sum(axis) + 1.01 * (n + 2) * U * np.abs(terms).sum(axis)


def reference(c, cd, masks=None):
    """fp64 reference of one step from the case's buffers with the bound of every value (module docstring);
    masks: the dropout masks the launch drew (default: the case's Philox masks)"""
    masks = masks if masks is not None else c.masks
    d, r = dims(c)
    L, gs = c.L, c.gscale
    f = _forward(c, cd, masks)
    live, M, T = f.live[L], f.M, f.T
    y = M * f.s
    Ey = np.abs(M) * f.Es + U * np.abs(y)
    e = np.where(live, y - T, 0.0)
    Ee = np.where(live & ((M != 0) | (T != 0)), Ey + U * np.abs(e), 0.0)      # (0 - 0 is exact)
    se = e * e
    Ese = 2.0 * np.abs(e) * Ee + Ee * Ee + U * se
    n = c.B * c.N
    ref = SimpleNamespace(f=f, y=y, Ey=Ey, e=e, Ee=Ee, count=int(np.count_nonzero(np.where(live, T + y, 0.0))))
    ref.stats = dict(sse=se.sum(), sae=np.abs(e).sum(), row_sse=se.sum(1), rho=0.0)
    ref.Estats = dict(sse=_sum_bound(Ese, se, n), sae=_sum_bound(Ee, e, n), row_sse=_sum_bound(Ese, se, c.N, 1), rho=0.0)
    if c.loss == "mse":
        D = e * M
        ED = np.abs(M) * Ee + U * np.abs(D)
    else:
        rho, dr = LR.rho(c.loss, e, c.delta), LR.drho(c.loss, e, c.delta)
        slope = np.minimum(np.abs(e) + Ee, c.delta) if c.loss == "huber" else 1.0
        Erho = slope * Ee + (8.0 * U * (np.abs(e) + 1.0) if c.loss == "logcosh" else 4.0 * U * rho)
        Erho = np.where(e != 0, Erho, 0.0)
        ref.stats["rho"], ref.Estats["rho"] = rho.sum(), _sum_bound(Erho, rho, n)
        Edr = {"mae": 0.0 * Ee, "huber": Ee, "logcosh": np.where(e != 0, Ee + 8.0 * U, 0.0)}[c.loss]
        D, ED = _mul(dr, Edr, M, np.zeros_like(M))
    ref.gW, ref.gb, ref.EgW, ref.Egb = [None] * (L + 1), [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
    for i in range(L, -1, -1):
        SD = _stage(D, ED, cd)
        gb = gs * D.sum(0)
        ref.gb[i], ref.Egb[i] = gb, gs * _sum_bound(ED, D, c.Bp, 0) * (1.0 + U) + 2.0 * U * np.abs(gb)
        G, EG = _gemm(f.A[i].T, f.SA[i].T, D, SD, c.Bp)
        if i == L:
            G, EG = G.T, EG.T
        ref.gW[i], ref.EgW[i] = gs * G, gs * EG * (1.0 + U) + U * np.abs(gs * G)
        if i > 0:
            Wb = f.Wr[i] if i == L else f.Wr[i].T
            v, Ev = _gemm(D, SD, Wb, np.zeros(Wb.shape), d[i + 1])
            gp, Egp = _act_grad(c.act, f.a[i - 1], f.Ea[i - 1])
            if c.keep < 1.0:
                v, Ev = _mul(v, Ev, f.dm[i - 1], f.Edm[i - 1])
            D, ED = _mul(v, Ev, gp, Egp)
            D, ED = np.where(f.live[i - 1], D, 0.0), np.where(f.live[i - 1], ED, 0.0)
    return ref


def conditions(c, cd, ref):
    """the input conditions of the GPU tests, each an array of booleans that must hold with no exclusion"""
    f, live = ref.f, ref.f.live[c.L]
    out = {"count": (np.abs(f.T + ref.y) >= COND * ref.Ey)[live & (f.M != 0)]}
    if c.loss == "mae":
        out["mae"] = (np.abs(ref.e) >= COND * ref.Ee)[live]
    if c.loss == "huber":
        out["huber"] = (np.abs(np.abs(ref.e) - c.delta) >= COND * ref.Ee)[live]
    if c.act == "relu":
        for i in range(c.L):
            out["relu%d" % i] = (np.abs(f.z[i]) >= COND * f.Ez[i])[f.live[i]]
    return out


# ---- comparisons ----------------------------------------------------------------------------------------------
def ratio(got, ref, E):
    """worst |got - ref| / E; where E is 0 the values must be equal (else inf)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    E = np.broadcast_to(np.asarray(E, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(E > 0, err / E, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


def check_grads(c, ref, out):
    """worst ratio over every element of every dW and db (out.gW / out.gb in the kernel's padded layouts)"""
    w = 0.0
    for i in range(c.L + 1):
        w = max(w, ratio(out.gW[i], ref.gW[i], ref.EgW[i]), ratio(out.gb[i], ref.gb[i][:len(out.gb[i])], ref.Egb[i][:len(out.gb[i])]))
    return w


def check_stats(c, ref, stats):
    """(worst ratio of sse / sae / sum rho / row sse, the count is exact); stats: the row {sse, sae, count, rho, row sse}"""
    s, E = ref.stats, ref.Estats
    w = max(ratio(stats[0], s["sse"], E["sse"]), ratio(stats[1], s["sae"], E["sae"]), ratio(stats[3], s["rho"], E["rho"]),
            ratio(stats[4:4 + c.Bp], s["row_sse"], E["row_sse"]))
    return w, float(stats[2]) == float(ref.count)


def expected_update(c, opt, st, gW, gb):
    """epilogue_ref.opt_update in fp64 on the given fp32 gradients from state st -> lists of (p, s1, s2) per weight
    and per bias (live elements; the padding must stay as it was)"""
    kind, h = hyper_of(opt)
    z = lambda s: None if s is None else s.astype(np.float64)
    ws = [R.opt_update(kind, st.W[i], gW[i], z(st.sW1[i]), z(st.sW2[i]), **h) for i in range(c.L + 1)]
    bs = [R.opt_update(kind, st.b[i], gb[i], z(st.sb1[i]), z(st.sb2[i]), **h) for i in range(c.L + 1)]
    return ws, bs


def check_update(c, opt, st, gW, gb, out):
    """worst |got - fp64| / opt_limit over the live elements of W, b and the slots; padding bit-unchanged (bool)"""
    d, r = dims(c)
    ws, bs = expected_update(c, opt, st, gW, gb)
    w, pad_ok = 0.0, True
    for i in range(c.L + 1):
        lw, lb = live_w(c, i), np.arange(d[i + 1]) < r[i + 1]
        for got, want, was, lv in ((out.W[i], ws[i][0], st.W[i], lw), (out.sW1[i], ws[i][1], st.sW1[i], lw),
                                   (out.sW2[i], ws[i][2], st.sW2[i], lw), (out.b[i], bs[i][0], st.b[i], lb),
                                   (out.sb1[i], bs[i][1], st.sb1[i], lb), (out.sb2[i], bs[i][2], st.sb2[i], lb)):
            if was is None:
                continue
            w = max(w, R.opt_worst([got[lv]], [want[lv]]))
            pad_ok &= bool(np.array_equal(got[~lv].view(np.int32), was[~lv].view(np.int32)))
    return w, pad_ok


def check_shadows(c, cd, out, blocked):
    """every shadow equals the RNE rounding of the updated weight at shadow_index, exactly"""
    return all(np.array_equal(out.shadow[i], shadow_of(out.W[i], cd, blocked)) for i in range(c.L + 1))


# ---- the float32 twin -------------------------------------------------------------------------------------------
WRONG = (
    "pad_rows_live",            # a padded batch row is row rows[B - 1] again (its data read, its guards missing), not zero
    "backprop_updated_w",       # delta_{i-1} through the already-updated W_i
    "act_grad_post_dropout",    # act' taken from the post-dropout h
    "no_dropout_scale_backward",    # mask without 1 / keep in the backward pass
    "shared_philox_stream",     # one Philox stream for every layer's mask
    "db_last_block",            # db without its last 32-row block
    "row_sse_8_blocks",         # row SSE without the column blocks beyond 8
    "totals_2048_slots",        # sse / sae / count without the slots beyond 2,048
    "gscale_bp",                # the mean taken over Bp rows, not B
    "loss_grad_unmasked",       # rho'(e) without the output mask
    "count_from_t",             # count_nonzero(T)
    "shadow_pre_update",        # the shadow of the weight before the update
    "shadow_row_major",         # a row-major shadow where the blocked layout was asked for
    "k_tail_dropped",           # a GEMM's short last K chunk skipped
)


def _round(x, cd):
    """epilogue_ref.round_to on a writable copy (the cases' arrays are read-only)"""
    return R.round_to(np.array(x, np.float32), cd)


def _r32(x, cd):
    return _round(x, cd)


def _tgemm(A, B, cd, drop_tail=False):
    """tile_s: A [M][K], B [K][N] staged to cd; K split over the four waves, each walking chunks of KC; the four
    partials summed in wave order; float32 throughout"""
    A, B = _r32(A, cd), _r32(B, cd)
    K = A.shape[1]
    kw, kc = K // WAVES, KC[cd]
    part = []
    for w in range(WAVES):
        acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
        for k0 in range(0, kw, kc):
            k1 = min(k0 + kc, kw)
            if drop_tail and k1 - k0 < kc and k0 > 0:
                continue
            acc = acc + A[:, w * kw + k0:w * kw + k1] @ B[w * kw + k0:w * kw + k1]
        part.append(acc)
    return ((part[0] + part[1]) + part[2]) + part[3]


def _blocks32(v, axis):
    """float32 sums over consecutive blocks of 32 along axis -> the axis becomes the block index"""
    sh = list(v.shape)
    sh[axis:axis + 1] = [sh[axis] // TT, TT]
    return v.reshape(sh).sum(axis + 1, dtype=np.float32)


def _seq_sum(v, n=None):
    acc = np.zeros(v.shape[1:], np.float32)
    for j in range(v.shape[0] if n is None else n):
        acc = acc + v[j]
    return acc


def _f32_update(kind, h, p, g, s1, s2):
    return R.opt_update(kind, p, g, s1, s2, dtype=np.float32, **h)


def twin(c, cd, opt="probe", variant=None, blocked=0):
    """ocf_mlp_step in NumPy float32 with the kernel's rounding points and reduction structure (the order inside an
    MFMA and inside a float32 np.sum differs, which the bounds cover); variant: one of WRONG.
    Returns the launch's outputs: W, b, slots, shadow (flat, as float32 values), stats [4 + Bp], masks, and gW / gb."""
    f32 = np.float32
    d, r = dims(c)
    L, kind = c.L, hyper_of(opt)[0]
    h_opt = hyper_of(opt)[1]
    st = init_state(c, opt)
    pad_live = variant == "pad_rows_live"
    X, M, T, rows_live = _batch(c, pad_live)
    drop = variant == "k_tail_dropped"
    keep = f32(c.keep)
    masks = None
    if c.keep < 1.0:
        masks = philox_masks(c, shared_stream=variant == "shared_philox_stream")
    gs = f32(c.gscale * (c.B / c.Bp if variant == "gscale_bp" else 1.0))
    hs, acts, dms = [X], [], []
    for i in range(L):
        live = np.outer(rows_live, np.arange(d[i + 1]) < r[i + 1])
        v = _tgemm(hs[i], st.W[i], cd, drop)
        with np.errstate(over="ignore"):
            a = np.where(live, R.act(c.act, (v + st.b[i]).astype(f32)), 0.0).astype(f32)
        h = a
        if c.keep < 1.0:
            mk = masks[i].astype(f32)
            h = (a / keep) * mk
            dms.append(mk if variant == "no_dropout_scale_backward" else mk / keep)
        acts.append(h if variant == "act_grad_post_dropout" else a)
        hs.append(h)
    live = np.outer(rows_live, np.arange(c.Np) < c.N)
    v = _tgemm(hs[L], st.W[L].T, cd, drop)
    y = np.where(live, M * (v + st.b[L]), 0.0).astype(f32)
    e = np.where(live, y - T, 0.0).astype(f32)
    se = e * e
    cnt = np.where(live, (T if variant == "count_from_t" else T + y) != 0, False).astype(f32)
    rho = np.zeros_like(e)
    if c.loss == "mse":
        D = e * (1.0 if variant == "loss_grad_unmasked" else M)
    else:
        rho = LR.rho(c.loss, e, c.delta).astype(f32)
        D = (LR.drho(c.loss, e, c.delta).astype(f32) * (1.0 if variant == "loss_grad_unmasked" else M)).astype(f32)
    D = D.astype(f32)
    # statistics: per (tile, wave) partials (a wave holds rows 2 w, 2 w + 1 (+ 8 j) of its tile), then the slots;
    # per-row SSE per 32-column block, then the blocks
    Bt, nt = c.Bp // TT, c.Np // TT

    def slots(v):
        p = v.reshape(Bt, 4, WAVES, 2, nt, TT).sum((1, 3, 5), dtype=f32)          # [Bt][wave][nt]
        p = p.transpose(0, 2, 1).reshape(-1)                                       # slot = (bt nt + ct) 4 + wave
        return p[:2048] if variant == "totals_2048_slots" else p
    stats = np.zeros(4 + c.Bp, f32)
    stats[0], stats[1], stats[2] = (slots(q).sum(dtype=f32) for q in (se, np.abs(e), cnt))
    if c.loss != "mse":
        stats[3] = rho.reshape(-1).sum(dtype=f32)
    rowp = _blocks32(se, 1)                                                        # [Bp][nt]
    stats[4:] = _seq_sum(rowp.T, 8 if variant == "row_sse_8_blocks" and nt > 8 else None)
    out = SimpleNamespace(W=[None] * (L + 1), b=[None] * (L + 1), sW1=[None] * (L + 1), sW2=[None] * (L + 1),
                          sb1=[None] * (L + 1), sb2=[None] * (L + 1), shadow=[None] * (L + 1), gW=[None] * (L + 1),
                          gb=[None] * (L + 1), stats=stats, masks=masks)
    for i in range(L, -1, -1):
        colp = _blocks32(D, 0)                                                     # [Bt][width]
        out.gb[i] = (_seq_sum(colp, Bt - 1 if variant == "db_last_block" else None) * gs).astype(f32)
        G = _tgemm(hs[i].T, D, cd, drop)
        out.gW[i] = ((G.T if i == L else G) * gs).astype(f32)
        lw = live_w(c, i)
        nw = _f32_update(kind, h_opt, st.W[i], np.where(lw, out.gW[i], 0), st.sW1[i], st.sW2[i])
        out.W[i], out.sW1[i], out.sW2[i] = (None if q is None else q.astype(f32) for q in nw)
        lb = np.arange(d[i + 1]) < r[i + 1]
        nb = _f32_update(kind, h_opt, st.b[i], out.gb[i], st.sb1[i], st.sb2[i])
        out.b[i], out.sb1[i], out.sb2[i] = (None if q is None else np.where(lb, q, was).astype(f32)
                                            for q, was in zip(nb, (st.b[i], st.sb1[i], st.sb2[i])))
        if cd != "f32":
            src = st.W[i] if variant == "shadow_pre_update" else out.W[i]
            out.shadow[i] = shadow_of(src, cd, blocked and variant != "shadow_row_major")
        if i > 0:
            Wb = out.W[i] if variant == "backprop_updated_w" else st.W[i]
            v = _tgemm(D, Wb if i == L else Wb.T, cd, drop)
            if c.keep < 1.0:
                v = v * dms[i - 1]
            lv = np.outer(rows_live, np.arange(d[i]) < r[i])
            D = np.where(lv, v * R.act_grad(c.act, acts[i - 1]).astype(f32), 0.0).astype(f32)
    return out
