"""Training losses of ``Model.compile(loss=...)``: a function rho of the masked residual e = m * y - t with
rho(0) = 0, so the Keras mean over all B * N elements is a sum over the batch's live target entries.

    name                               rho(e)                                    rho'(e)
    mean_squared_error / mse           e^2                                       2 e          (train.py:49)
    mean_absolute_error / mae          |e|                                       sign(e), 0 at e = 0
    huber (delta d > 0, default 1)     e^2 / 2 if |e| <= d, else d (|e| - d / 2) clamp(e, -d, d)
    logcosh                            log cosh e                                tanh e

The kernels specialise on ``code`` (ocf.h OCF_LOSS_*) and take ``param`` (Huber's delta).  ``grad_num`` is the
numerator of the gradient scale the engine folds into the weight / bias updates: 2 / (B N) for MSE, whose kernels
carry delta = e * m, and 1 / (B N) for the others, whose kernels carry delta = rho'(e) * m.
"""
import math

from . import _lib


class Loss(object):
    name = None
    code = _lib.LOSS_MSE
    param = 0.0
    grad_num = 1.0

    def params(self):
        """what a checkpoint stores besides the name"""
        return {}

    def __eq__(self, other):
        return isinstance(other, Loss) and (self.name, self.param) == (other.name, other.param)

    def __hash__(self):
        return hash((self.name, self.param))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % kv for kv in sorted(self.params().items())))


class MeanSquaredError(Loss):
    name = "mean_squared_error"
    code = _lib.LOSS_MSE
    grad_num = 2.0


class MeanAbsoluteError(Loss):
    name = "mean_absolute_error"
    code = _lib.LOSS_MAE


class Huber(Loss):
    name = "huber"
    code = _lib.LOSS_HUBER

    def __init__(self, delta=1.0):
        try:
            delta = float(delta)
        except (TypeError, ValueError):
            raise ValueError("huber: delta must be a number > 0, got %r" % (delta,))
        if not (delta > 0.0) or math.isinf(delta) or math.isnan(delta):
            raise ValueError("huber: delta must be a finite number > 0, got %r" % (delta,))
        self.param = delta

    def params(self):
        return {"delta": self.param}


class LogCosh(Loss):
    name = "logcosh"
    code = _lib.LOSS_LOGCOSH


_TABLE = {"mean_squared_error": MeanSquaredError, "mse": MeanSquaredError,
          "mean_absolute_error": MeanAbsoluteError, "mae": MeanAbsoluteError,
          "huber": Huber, "logcosh": LogCosh}
# Keras losses that exist but are not built here (they touch unobserved entries or squash the output)
_KNOWN_UNBUILT = ("mean_absolute_percentage_error", "mape", "mean_squared_logarithmic_error", "msle", "squared_hinge",
                  "hinge", "categorical_hinge", "categorical_crossentropy", "sparse_categorical_crossentropy",
                  "binary_crossentropy", "kullback_leibler_divergence", "kld", "poisson", "cosine_proximity", "cosine")


def get(identifier, loss_params=None):
    """A Keras loss name (with ``loss_params``, e.g. {"delta": 2.5} for "huber") or a Loss instance.
    ValueError: an unknown name, a parameter the loss does not take, a bad delta.  NotImplementedError: a Keras
    loss this package does not build."""
    if isinstance(identifier, Loss):
        if loss_params:
            raise ValueError("loss_params goes with a loss name, not with a Loss instance")
        return identifier
    if not isinstance(identifier, str):
        raise ValueError("loss must be a name or a losses.Loss instance, got %r" % (identifier,))
    key = identifier.lower()
    if key in _KNOWN_UNBUILT:
        raise NotImplementedError("loss %r is not implemented: the masked losses built are %s"
                                  % (identifier, ", ".join(sorted(_TABLE))))
    if key not in _TABLE:
        raise ValueError("unknown loss %r (known: %s)" % (identifier, ", ".join(sorted(_TABLE))))
    cls = _TABLE[key]
    kw = dict(loss_params or {})
    if cls is Huber:
        extra = set(kw) - {"delta"}
        if extra:
            raise ValueError("huber takes loss_params {'delta': d}, got %r" % (sorted(extra),))
        return Huber(**kw)
    if kw:
        raise ValueError("loss %r takes no loss_params, got %r" % (identifier, sorted(kw)))
    return cls()
