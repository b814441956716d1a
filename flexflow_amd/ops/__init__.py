"""Operator library. Importing this package registers every op in `OPS`."""
from .base import OPS, OpCtx, OpImpl, WeightSpec, register, torch_dtype  # noqa: F401
from . import attention, conv, elementwise, embedding, glu, linear, misc, norm, parallel_ops, rnn, rope, sdpa, shape, softmax  # noqa: F401
