"""NumPy restatements of the Adadelta / Adamax updates (Keras 2.0.4 get_updates; csrc/ocf_epilogues.h
opt_update_k): the fp64 reference, a float32 restatement in the kernel's operation order, deliberately wrong
variants, the shared inputs of tests/test_optim_ref.py and tests/test_optimizers_gpu.py, and oracle optimizers
with the step(params, grads) interface of oracle.model_oracle.AdagradOracle.

The bar is the project's own (tests/epilogue_ref.py OPT_RTOL / OPT_ATOL), imported, not copied.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import numpy as np

from tests.epilogue_ref import GSCALE, HYPER, OPT_ATOL, OPT_RTOL, opt_limit, opt_worst  # noqa: F401

KINDS = ("adadelta", "adamax")
OPT_KIND2 = {"adadelta": 4, "adamax": 5}                 # ocf.h OCF_OPTK_ADADELTA / OCF_OPTK_ADAMAX
G_STD = 16.0                                             # raw gradient ~ a K = 256 product of unit operands

WRONG2 = {
    "adadelta": ("update_from_old_a", "eps_outside_sqrt", "d_from_g2", "lr_folded_into_d"),
    "adamax": ("max_dropped", "g_without_abs", "u_not_decayed", "adam_second_moment", "sqrt_u"),
}


def opt_update2(kind, p, g, s1, s2, lr=0.01, eps=1e-8, rho=0.9, beta2=0.999, l2=0.0, gscale=1.0, variant=None,
                dtype=np.float64):
    """One step in `dtype` (float64: the reference; float32: opt_update_k's operation order, every intermediate
    rounded to float32).  Adadelta: s1 = a, s2 = d, rho.  Adamax: s1 = m, s2 = u, rho = beta_1, lr = lr_t.
    Returns (p, s1, s2)."""
    f = dtype
    p, g, s1, s2 = (np.asarray(x, f) for x in (p, g, s1, s2))
    lr, eps, rho, beta2, l2, gscale = (f(np.float32(x)) for x in (lr, eps, rho, beta2, l2, gscale))
    one, two = f(1.0), f(2.0)
    g = g * gscale
    if l2 != 0:
        g = g + two * l2 * p
    if kind == "adadelta":
        a = rho * s1 + (one - rho) * (g * g)
        if variant == "eps_outside_sqrt":
            u = (g * (np.sqrt(s2) + eps)) / (np.sqrt(a) + eps)
        else:
            u = (g * np.sqrt(s2 + eps)) / np.sqrt((s1 if variant == "update_from_old_a" else a) + eps)
        acc = g if variant == "d_from_g2" else (lr * u if variant == "lr_folded_into_d" else u)
        return p - lr * u, a, rho * s2 + (one - rho) * (acc * acc)
    if kind == "adamax":
        m = rho * s1 + (one - rho) * g
        ag = g if variant == "g_without_abs" else np.abs(g)
        if variant == "max_dropped":
            u = beta2 * s2
        elif variant == "u_not_decayed":
            u = np.maximum(s2, ag)
        elif variant == "adam_second_moment":
            u = beta2 * s2 + (one - beta2) * (g * g)
        else:
            u = np.maximum(beta2 * s2, ag)
        den = (np.sqrt(u) if variant == "sqrt_u" else u) + eps
        return p - (lr * m) / den, m, u
    raise ValueError(kind)


def inputs2(kind, shape, seed, g_std=G_STD):
    """p ~ 0.05 randn; s1 signed with magnitude in [0.25, 1.25) (Adadelta's a must not be negative: its sign
    is dropped there); s2 = Adadelta's d in [0.25, 1.25) or Adamax's u in [0.02, 0.12), around |g * GSCALE| ~ 0.05,
    so both branches of the max are taken; raw gradient ~ g_std randn (None: no gradient returned)"""
    rng = np.random.RandomState(seed)
    p = (0.05 * rng.randn(*shape)).astype(np.float32)
    s1 = (0.25 + rng.rand(*shape)).astype(np.float32)
    if kind == "adamax":
        s1 = (s1 * np.where(rng.rand(*shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    s2 = ((0.25 if kind == "adadelta" else 0.02) + (1.0 if kind == "adadelta" else 0.1) * rng.rand(*shape))
    s2 = s2.astype(np.float32)
    if g_std is None:
        return p, s1, s2
    return p, s1, s2, (g_std * rng.randn(*shape)).astype(np.float32)


def hyper2(l2=True, gscale=GSCALE):
    h = dict(HYPER, gscale=gscale)
    if not l2:
        h["l2"] = 0.0
    return h


def max_branches(g_eff, u, beta2):
    """fractions of the elements where Adamax's max takes the decayed u / takes |g| (g_eff: the gradient after
    gscale and l2, fp64)"""
    took_g = np.abs(np.asarray(g_eff, np.float64)) > np.float64(np.float32(beta2)) * np.asarray(u, np.float64)
    return float(1.0 - took_g.mean()), float(took_g.mean())


def assert_max_branches(g_eff, u, beta2):
    lo, hi = max_branches(g_eff, u, beta2)
    assert lo >= 0.1 and hi >= 0.1, "Adamax: each branch of the max needs >= 10 %% of the elements (%.3f / %.3f)" % (lo, hi)


def eff_grad(g, p, gscale, l2):
    """the gradient the update sees, fp64 (scalars as the float32 values the kernel receives)"""
    g = np.asarray(g, np.float64) * np.float64(np.float32(gscale))
    if l2:
        g = g + 2.0 * np.float64(np.float32(l2)) * np.asarray(p, np.float64)
    return g


# ---- oracle optimizers (Keras 2.0.4 get_updates; accumulators start at 0) ---------------------------------
class AdadeltaOracle:
    def __init__(self, lr=1.0, rho=0.95, epsilon=1e-8, decay=0.0):
        self.lr, self.rho, self.eps, self.decay = lr, rho, epsilon, decay
        self.a = self.d = None
        self.iterations = 0

    def step(self, params, grads):
        if self.a is None:
            self.a = [np.zeros_like(p) for p in params]
            self.d = [np.zeros_like(p) for p in params]
        dt = params[0].dtype.type
        lr = self.lr
        if self.decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * self.iterations))
        lr, rho, eps = dt(lr), dt(self.rho), dt(self.eps)
        out = []
        for i, (p, g) in enumerate(zip(params, grads)):
            a = rho * self.a[i] + (dt(1.0) - rho) * g * g
            u = g * np.sqrt(self.d[i] + eps) / np.sqrt(a + eps)
            self.a[i] = a
            self.d[i] = rho * self.d[i] + (dt(1.0) - rho) * u * u
            out.append(p - lr * u)
        self.iterations += 1
        return out


class AdamaxOracle:
    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0):
        self.lr, self.b1, self.b2, self.eps, self.decay = lr, beta_1, beta_2, epsilon, decay
        self.m = self.u = None
        self.iterations = 0
        self.n_dec = self.n_g = 0          # elements whose max took the decayed u / took |g|, steps 2..

    def branch_fractions(self):
        n = float(self.n_dec + self.n_g)
        return self.n_dec / n, self.n_g / n

    def step(self, params, grads):
        if self.m is None:
            self.m = [np.zeros_like(p) for p in params]
            self.u = [np.zeros_like(p) for p in params]
        dt = params[0].dtype.type
        lr = self.lr
        if self.decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * self.iterations))
        t = self.iterations + 1
        lr_t = dt(lr / (1.0 - self.b1 ** t))
        b1, b2, eps = dt(self.b1), dt(self.b2), dt(self.eps)
        out = []
        for i, (p, g) in enumerate(zip(params, grads)):
            m = b1 * self.m[i] + (dt(1.0) - b1) * g
            u = np.maximum(b2 * self.u[i], np.abs(g))
            if self.iterations > 0:
                took_g = int((np.abs(g) > b2 * self.u[i]).sum())
                self.n_g += took_g
                self.n_dec += g.size - took_g
            self.m[i], self.u[i] = m, u
            out.append(p - lr_t * m / (u + eps))
        self.iterations += 1
        return out


def oracle_opt2(name, lr=None):
    return {"adadelta": lambda: AdadeltaOracle(lr=lr or 1.0), "adamax": lambda: AdamaxOracle(lr=lr or 0.002)}[name]()


def our_opt2(name, lr=None):
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    return {"adadelta": lambda: O.Adadelta(lr=lr or 1.0), "adamax": lambda: O.Adamax(lr=lr or 0.002)}[name]()
