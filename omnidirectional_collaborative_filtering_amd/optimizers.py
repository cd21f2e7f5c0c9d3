"""Keras 2.0.4 optimizer surface (train.py:12,50-51; train_jester.py:61).

Only the hyper-parameters live here; the update itself runs on the GPU inside the weight-gradient
GEMM epilogue (``OCF_EPI_OPTIM``) or ``ocf_opt_step``.  ``step_params()`` turns the Keras
schedule (decay, Adam bias correction) into the per-step scalars the kernels take.
"""
from __future__ import annotations

import math

from . import _lib


class Optimizer:
    kind = _lib.OPT_SGD
    n_slots = 0
    name = "optimizer"          # the get() identifier; Model.save stores it with the slots
    # True where step_params() changes with `iterations` even without decay (a bias correction): the
    # engine's one-call step then refreshes the optimizer scalars every step instead of freezing them
    step_dependent = False

    @property
    def scalars_change(self):
        """the per-step scalars depend on the step (decay, or a bias correction)"""
        return self.step_dependent or bool(self.decay)

    def __init__(self, lr=0.01, decay=0.0, **kw):
        self.lr = float(lr)
        self.decay = float(decay)
        self.iterations = 0
        self.extra = kw

    def _lr(self):
        lr = self.lr
        if self.decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * self.iterations))
        return lr

    def step_params(self, gscale=1.0, l2=0.0):
        o = _lib.OcfOptParams()
        o.kind = self.kind
        o.lr = self._lr()
        o.eps = getattr(self, "epsilon", 1e-8)
        o.rho = 0.0
        o.beta2 = 0.0
        o.l2 = float(l2 or 0.0)
        o.gscale = float(gscale)
        return o

    def get_config(self):
        return {"lr": self.lr, "decay": self.decay}


class SGD(Optimizer):
    """p -= lr*g   (Keras 2.0.4 SGD.get_updates with momentum = 0, nesterov = False).

    Keras' SGD also has momentum and Nesterov momentum; this library implements neither, so asking for
    one raises instead of training silently without it."""
    kind = _lib.OPT_SGD
    name = "sgd"

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False):
        if float(momentum) != 0.0 or nesterov:
            raise ValueError("SGD: momentum / nesterov are not implemented (got momentum=%r, nesterov=%r)"
                             % (momentum, nesterov))
        super().__init__(lr, decay)


class Adagrad(Optimizer):
    """a += g^2; p -= lr*g/(sqrt(a)+eps)   (Keras 2.0.4 Adagrad.get_updates)."""
    kind = _lib.OPT_ADAGRAD
    n_slots = 1
    name = "adagrad"

    def __init__(self, lr=0.01, epsilon=1e-8, decay=0.0):
        super().__init__(lr, decay)
        self.epsilon = float(epsilon)


class RMSprop(Optimizer):
    """a = rho*a + (1-rho)*g^2; p -= lr*g/(sqrt(a)+eps)."""
    kind = _lib.OPT_RMSPROP
    n_slots = 1
    name = "rmsprop"

    def __init__(self, lr=0.001, rho=0.9, epsilon=1e-8, decay=0.0):
        super().__init__(lr, decay)
        self.rho = float(rho)
        self.epsilon = float(epsilon)

    def step_params(self, gscale=1.0, l2=0.0):
        o = super().step_params(gscale, l2)
        o.rho = self.rho
        return o


class Adam(Optimizer):
    """lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMAs; p -= lr_t*m/(sqrt(v)+eps)."""
    kind = _lib.OPT_ADAM
    n_slots = 2
    name = "adam"
    step_dependent = True

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0):
        super().__init__(lr, decay)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)

    def step_params(self, gscale=1.0, l2=0.0):
        o = super().step_params(gscale, l2)
        t = self.iterations + 1
        o.lr = self._lr() * (math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t))
        o.rho = self.beta_1
        o.beta2 = self.beta_2
        return o


class Adadelta(Optimizer):
    """a = rho*a + (1-rho)*g^2; u = g*sqrt(d+eps)/sqrt(a+eps); p -= lr*u; d = rho*d + (1-rho)*u^2
    (Keras 2.0.4 Adadelta.get_updates; slots: a, d)."""
    kind = _lib.OPT_ADADELTA
    n_slots = 2
    name = "adadelta"

    def __init__(self, lr=1.0, rho=0.95, epsilon=1e-8, decay=0.0):
        super().__init__(lr, decay)
        self.rho = float(rho)
        self.epsilon = float(epsilon)

    def step_params(self, gscale=1.0, l2=0.0):
        o = super().step_params(gscale, l2)
        o.rho = self.rho
        return o

    def get_config(self):
        return {"lr": self.lr, "rho": self.rho, "epsilon": self.epsilon, "decay": self.decay}


class Adamax(Optimizer):
    """lr_t = lr/(1-b1^t); m = b1*m + (1-b1)*g; u = max(b2*u, |g|); p -= lr_t*m/(u+eps)
    (Keras 2.0.4 Adamax.get_updates; slots: m, u)."""
    kind = _lib.OPT_ADAMAX
    n_slots = 2
    name = "adamax"
    step_dependent = True

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0):
        super().__init__(lr, decay)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)

    def step_params(self, gscale=1.0, l2=0.0):
        o = super().step_params(gscale, l2)
        t = self.iterations + 1
        o.lr = self._lr() / (1.0 - self.beta_1 ** t)
        o.rho = self.beta_1
        o.beta2 = self.beta_2
        return o

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "decay": self.decay}


def check_single_gpu(opt, layout):
    """Adadelta / Adamax run on one GPU only: nothing of the multi-GPU layouts is verified for them."""
    if isinstance(opt, (Adadelta, Adamax)):
        raise NotImplementedError("optimizer %r is not implemented under %s (sgd, adagrad, rmsprop and adam are)"
                                  % (opt.name, layout))


def get(identifier):
    """Keras string identifiers ('adagrad', 'rmsprop', 'adam', 'adadelta', 'adamax', 'sgd') or an instance."""
    if isinstance(identifier, Optimizer):
        return identifier
    table = {"sgd": SGD, "adagrad": Adagrad, "rmsprop": RMSprop, "adam": Adam, "adadelta": Adadelta,
             "adamax": Adamax}
    key = str(identifier).lower()
    if key not in table:
        raise ValueError("unknown optimizer %r" % (identifier,))
    return table[key]()
