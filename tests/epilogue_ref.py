"""NumPy fp64 restatements of the dense epilogue / elementwise arithmetic (include/ocf.h, the comments of
csrc/ocf_epilogues.h), the shared inputs, hyper-parameters and tolerances of tests/test_epilogues_gpu.py and
tests/test_elem_gpu.py, a float32 restatement of the optimizer update in the kernel's operation order
(opt_update_k) and a set of deliberately wrong variants.  tests/test_epilogue_ref.py shows on the CPU that
the GPU tests' tolerances hold for a correct float32 kernel and reject every wrong variant.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import numpy as np

ACTS = ("linear", "sigmoid", "tanh", "relu")
OPTS = ("sgd", "adagrad", "rmsprop", "adam")
OPT_KIND = {"sgd": 0, "adagrad": 1, "rmsprop": 2, "adam": 3}      # ocf.h OCF_OPTK_*

# hyper-parameters at which every term of every update is visible (lr * g, eps against sqrt(slot), the
# (1 - rho) / (1 - beta2) factors, the l2 term against g)
HYPER = dict(lr=0.05, eps=1e-2, rho=0.9, beta2=0.99, l2=1e-2)
GSCALE = 3e-3
# optimizer state against fp64: the bar of test_rows_dw_gpu.py::test_rows_kernel_vs_torch
OPT_RTOL, OPT_ATOL = 1e-5, 2e-6

U16 = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}


def round_tol(name, ref):
    """error of one rounding of an fp32 value to f16 / bf16 (0 for f32: no rounding happens): the unit roundoff
    times |ref|, and for f16 half the subnormal spacing 2^-24 (values under 6.1e-5 round on a fixed grid and
    underflow to 0; bf16 keeps fp32's exponent range)"""
    if name == "f32":
        return np.zeros_like(np.asarray(ref, np.float64))
    return U16[name] * np.abs(ref) + (2.0 ** -25 if name == "f16" else 0.0)


# ---- activations (ocf_common.h act_apply / act_grad) ---------------------------------------------------
def act(name, z):
    z = np.asarray(z, np.float64)
    if name == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.where(z > 0, z, 0.0)
    if name == "linear":
        return z
    raise ValueError(name)


def act_grad(name, a, variant=None):
    """the derivative taken from the activation's OUTPUT a (the relu derivative is a > 0)"""
    a = np.asarray(a, np.float64)
    if name == "sigmoid":
        return 1.0 - a * a if variant == "sigmoid_grad_as_tanh" else a * (1.0 - a)
    if name == "tanh":
        return 1.0 - a * a
    if name == "relu":
        return (a > 0).astype(np.float64)
    if name == "linear":
        return np.ones_like(a)
    raise ValueError(name)


def dropout_fwd(a, mask, keep):
    """h = (a / keep) * mask"""
    return (np.asarray(a, np.float64) / float(keep)) * np.asarray(mask, np.float64)


def grad_act(name, d, a, mask=None, keep=1.0, variant=None):
    """d * mask / keep * act'(a)  (no mask, or keep = 1: d * act'(a))"""
    d = np.asarray(d, np.float64)
    if mask is not None and keep < 1.0:
        mk = np.asarray(mask, np.float64)
        d = d * (mk if variant == "mask_without_keep" else mk / float(keep))
    return d * act_grad(name, a, variant)


# ---- Keras 2.0.4 get_updates: g * gscale, then + 2 * l2 * p, then the update ------------------------------
# wrong variants -> the optimizers each applies to
WRONG_OPT = {
    "l2_dropped": OPTS,
    "l2_without_factor_2": OPTS,
    "eps_inside_sqrt": ("adagrad", "rmsprop", "adam"),
    "one_minus_decay_missing": ("rmsprop", "adam"),       # (1 - rho) of RMSprop, (1 - beta2) of Adam
    "adam_divides_g": ("adam",),
    "gscale_after_l2": OPTS,
}
WRONG_ACT = ("sigmoid_grad_as_tanh", "mask_without_keep")


def opt_update(kind, p, g, s1=None, s2=None, lr=0.01, eps=1e-8, rho=0.9, beta2=0.999, l2=0.0, gscale=1.0,
               variant=None, dtype=np.float64):
    """One step of the update in `dtype` (float64: the reference; float32: opt_update_k's operation order,
    every intermediate rounded to float32).  rho is Adam's beta_1; lr is Adam's lr_t.  Returns (p, s1, s2)
    (slots the optimizer does not have come back unchanged)."""
    f = dtype
    p, g = np.asarray(p, f), np.asarray(g, f)
    s1 = None if s1 is None else np.asarray(s1, f)
    s2 = None if s2 is None else np.asarray(s2, f)
    lr, eps, rho, beta2, l2, gscale = (f(np.float32(x)) for x in (lr, eps, rho, beta2, l2, gscale))
    one, two = f(1.0), f(2.0)
    if variant == "gscale_after_l2":
        g = (g + two * l2 * p) * gscale if l2 != 0 else g * gscale
    else:
        g = g * gscale
        if l2 != 0 and variant != "l2_dropped":
            g = g + (l2 * p if variant == "l2_without_factor_2" else two * l2 * p)

    def denom(a):
        return np.sqrt(a + eps) if variant == "eps_inside_sqrt" else np.sqrt(a) + eps

    if kind == "sgd":
        return p - lr * g, s1, s2
    if kind == "adagrad":
        a = s1 + g * g
        return p - (lr * g) / denom(a), a, s2
    if kind == "rmsprop":
        w = one if variant == "one_minus_decay_missing" else one - rho
        a = rho * s1 + w * (g * g)
        return p - (lr * g) / denom(a), a, s2
    if kind == "adam":
        w = one if variant == "one_minus_decay_missing" else one - beta2
        m = rho * s1 + (one - rho) * g
        v = beta2 * s2 + w * (g * g)
        num = g if variant == "adam_divides_g" else m
        return p - (lr * num) / denom(v), m, v
    raise ValueError(kind)


def opt_inputs(shape, seed, g_std=None):
    """the optimizer tests' state: p ~ 0.05 randn, slots uniform in [0.25, 1.25); with g_std also a raw
    gradient ~ g_std randn (the elementwise kernels; the GEMM tests form theirs from the operands)"""
    rng = np.random.RandomState(seed)
    p = (0.05 * rng.randn(*shape)).astype(np.float32)
    s1 = (0.25 + rng.rand(*shape)).astype(np.float32)
    s2 = (0.25 + rng.rand(*shape)).astype(np.float32)
    if g_std is None:
        return p, s1, s2
    return p, s1, s2, (g_std * rng.randn(*shape)).astype(np.float32)


def hyper(kind, l2=True, gscale=GSCALE):
    """keyword arguments of opt_update for the tests' hyper-parameters"""
    h = dict(HYPER, gscale=gscale)
    if not l2:
        h["l2"] = 0.0
    return h


def opt_limit(ref):
    return OPT_ATOL + OPT_RTOL * np.abs(ref)


def opt_worst(got, ref):
    """worst |got - ref| / (atol + rtol |ref|) over the arrays a test compares (p and the slots present)"""
    w = 0.0
    for x, r in zip(got, ref):
        if r is None:
            continue
        w = max(w, float((np.abs(np.asarray(x, np.float64) - r) / opt_limit(r)).max()))
    return w


# ---- products -----------------------------------------------------------------------------------------
def round_to(x, name):
    """float32 array rounded once (RNE) to f32 / f16 / bf16, returned as float32"""
    import torch
    td = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[name]
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(td).float().numpy()


def product_tol(K, mag, out=None):
    """|got - ref| bound of an fp32-accumulated product of operands already rounded to the compute dtype:
    K * 2^-24 for the fp32 summation, times 4 for MFMA's internal ordering, on mag = sum |a||b| (+ |bias|);
    plus 4 fp32 ulp of the output for __expf / tanhf (the activations are 1-Lipschitz).
    Measured on an MI355X at K = 192 (worst |err| / bound): the plain product through EPI_PREDICT 0.0054 (f32),
    0.0018 (f16), 0.0020 (bf16); over every product check with an fp32 output 0.18 in all three -- the 16-bit
    MFMA paths meet the derived bound, so no dtype needs the looser per-dtype TOL of test_gemm_gpu.py."""
    t = 4.0 * K * 2.0 ** -24 * np.asarray(mag, np.float64)
    if out is not None:
        t = t + 4.0 * 2.0 ** -23 * np.abs(out)
    return t


# ---- masked MSE (EpiMaskedMSE: train.py:49, model.py:86) --------------------------------------------------
def masked_mse(y_full, t, m):
    """entry arithmetic on dense [B][N] arrays, an entry wherever t != 0 or m != 0:
    yhat = m * y, err = yhat - t, d = err * m; SSE, SAE, count_nonzero(t + yhat), per-row SSE"""
    y_full, t, m = (np.asarray(x, np.float64) for x in (y_full, t, m))
    on = (t != 0) | (m != 0)
    yhat = np.where(on, m * y_full, 0.0)
    err = np.where(on, yhat - t, 0.0)
    d = err * m
    return dict(on=on, yhat=yhat, err=err, d=d, sse=float((err * err).sum()), sae=float(np.abs(err).sum()),
                count=int(np.count_nonzero(np.where(on, t + yhat, 0.0))), row_sse=(err * err).sum(1))


def bucket_layout(T, M, n_tiles, rows=None, B=None, N=None):
    """the buckets ocf_dense_targets documents: an entry wherever T != 0 or M != 0, per 128-column tile in
    (row, column) order; bk_rc = (b << 7) | (n & 127); batch row b reads source row rows[b]"""
    T, M = np.asarray(T), np.asarray(M)
    B = T.shape[0] if B is None else B
    N = T.shape[1] if N is None else N
    src = np.arange(B) if rows is None else np.asarray(rows)[:B]
    Tb, Mb = T[src][:, :N], M[src][:, :N]
    ptr, rc, bt, bm = [0], [], [], []
    for t in range(n_tiles):
        c0, c1 = 128 * t, min(128 * t + 128, N)
        if c0 < c1:
            b, n = np.nonzero((Tb[:, c0:c1] != 0) | (Mb[:, c0:c1] != 0))        # row-major = (row, column) order
            rc.append((b.astype(np.int64) << 7) | n)
            bt.append(Tb[b, c0 + n])
            bm.append(Mb[b, c0 + n])
        ptr.append(ptr[-1] + (len(rc[-1]) if c0 < c1 else 0))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return np.asarray(ptr, np.int32), cat(rc, np.int32), cat(bt, np.float32), cat(bm, np.float32)


# ---- the GPU tests' shapes and inputs (shared with the CPU test of the tolerances) ------------------------
M, N, K = 256, 256, 192          # two row tiles, two column tiles, three K-steps (six in fp32)
M_REAL, N_REAL = 200, 130        # last row tile part padding; two real columns in the second column tile
G_STD = 15.0                     # raw gradient of the elementwise tests: |g * GSCALE| ~ 0.05


def optim_operands(cd, seed=21):
    """EPI_OPTIM's operands: A [K][M] (delta^T), B [K][N] (activations), randn rounded to the compute dtype;
    the raw gradient A^T B has |g| ~ sqrt(K) ~ 14, so |g * GSCALE| ~ 0.04"""
    rng = np.random.RandomState(seed)
    return round_to(rng.randn(K, M), cd), round_to(rng.randn(K, N), cd)


def a_in_for(name, shape, rng):
    """forward activations a GRAD_ACT test feeds back: in the activation's range, with exact 0.0 and 1.0
    entries (relu' (0) = 0, sigmoid' (1) = 0, tanh' (1) = 0)"""
    a = rng.rand(*shape)
    if name == "tanh":
        a = 2.0 * a - 1.0
    elif name == "relu":
        a = np.where(rng.rand(*shape) < 0.4, 0.0, 3.0 * a)
    elif name == "linear":
        a = 4.0 * a - 2.0
    a = a.astype(np.float32)
    a[rng.rand(*shape) < 0.02] = 0.0
    a[rng.rand(*shape) < 0.02] = 1.0
    return a
