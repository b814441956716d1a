"""Keras optimizers (reference keras/optimizers.py) -> fused HIP SGD / Adam / AdamW / LAMB of flexflow_amd.core.

global_clipnorm=C clips the global gradient norm of all trainable weights to C (the core optimizers'
clip_norm). Keras' clipnorm (per variable) and clipvalue (per element) are not implemented: they
are accepted and ignored, like every other unknown keyword."""
from __future__ import annotations

from ..core.optimizers import AdamOptimizer, AdamWOptimizer, LAMBOptimizer, SGDOptimizer


class Optimizer:
    ffhandle = None

    def create_ffhandle(self, ffmodel):
        raise NotImplementedError

    def set_learning_rate(self, lr):
        self.learning_rate = float(lr)
        if self.ffhandle is not None:
            self.ffhandle.set_learning_rate(lr)


class SGD(Optimizer):
    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, weight_decay=0.0, global_clipnorm=None, **kw):
        self.learning_rate = float(kw.pop("lr", learning_rate))
        self.momentum, self.nesterov, self.weight_decay = float(momentum), bool(nesterov), float(weight_decay)
        self.global_clipnorm = global_clipnorm

    def create_ffhandle(self, ffmodel):
        self.ffhandle = SGDOptimizer(ffmodel, self.learning_rate, self.momentum, self.nesterov, self.weight_decay,
                                     clip_norm=self.global_clipnorm)
        return self.ffhandle


class Adam(Optimizer):
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-8, weight_decay=0.0,
                 global_clipnorm=None, **kw):
        self.learning_rate = float(kw.pop("lr", learning_rate))
        self.beta_1, self.beta_2, self.epsilon, self.weight_decay = beta_1, beta_2, epsilon, weight_decay
        self.global_clipnorm = global_clipnorm

    def create_ffhandle(self, ffmodel):
        self.ffhandle = AdamOptimizer(ffmodel, self.learning_rate, self.beta_1, self.beta_2, self.weight_decay,
                                      self.epsilon, clip_norm=self.global_clipnorm)
        return self.ffhandle


class Lamb(Optimizer):
    """LAMB with decoupled weight decay (core LAMBOptimizer); exclude_1d leaves biases and
    LayerNorm vectors out of the decay and the trust ratio."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-6, weight_decay=0.01,
                 bias_correction=True, exclude_1d=True, global_clipnorm=None, **kw):
        self.learning_rate = float(kw.pop("lr", learning_rate))
        self.beta_1, self.beta_2, self.epsilon, self.weight_decay = beta_1, beta_2, epsilon, weight_decay
        self.bias_correction, self.exclude_1d = bias_correction, exclude_1d
        self.global_clipnorm = global_clipnorm

    def create_ffhandle(self, ffmodel):
        self.ffhandle = LAMBOptimizer(ffmodel, self.learning_rate, self.beta_1, self.beta_2, self.weight_decay,
                                      self.epsilon, self.bias_correction, self.exclude_1d,
                                      clip_norm=self.global_clipnorm)
        return self.ffhandle


class AdamW(Optimizer):
    """AdamW (core AdamWOptimizer) with Keras' defaults: decoupled weight_decay=0.004 on every
    variable; exclude_1d=True leaves biases and LayerNorm vectors out of the decay."""

    def __init__(self, learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 exclude_1d=False, global_clipnorm=None, **kw):
        self.learning_rate = float(kw.pop("lr", learning_rate))
        self.beta_1, self.beta_2, self.epsilon, self.weight_decay = beta_1, beta_2, epsilon, weight_decay
        self.exclude_1d = exclude_1d
        self.global_clipnorm = global_clipnorm

    def create_ffhandle(self, ffmodel):
        self.ffhandle = AdamWOptimizer(ffmodel, self.learning_rate, self.beta_1, self.beta_2, self.weight_decay,
                                       self.epsilon, self.exclude_1d, clip_norm=self.global_clipnorm)
        return self.ffhandle


def get(spec):
    if isinstance(spec, Optimizer):
        return spec
    return {"sgd": SGD, "adam": Adam, "adamw": AdamW, "lamb": Lamb}[str(spec).lower()]()
