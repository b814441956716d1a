"""Gated linear unit (extension: no reference counterpart; the FFN gate of LLaMA / Mistral / Qwen
(SwiGLU), of T5 v1.1 / mt5 / Gemma (GeGLU), and the original GLU).

y = act(gate) * up with act one of silu, gelu (erf), gelu_tanh, relu, sigmoid (attribute `activation`).
Two inputs (gate, up: same shape and dtype; the output has that shape), or one packed input
(attribute `packed`) whose last dim 2F holds the gate in [..., :F] and the up in [..., F:], the output
of one GEMM of 2F columns; the output's last dim is F. No weights. One launch of kernels.glu_fwd
(glu.hip) forward and one of kernels.glu_bwd backward, which recomputes act(gate) and act'(gate): only
the inputs are saved. The packed backward writes both halves of one [..., 2F] gradient in its launch.

Parallel axes: every output dim for the two-input form (identity input maps, like a same-shape binary
op: column-parallel gate / up GEMMs feed it shard by shard). The packed form offers all but the last
dim: a split of the 2F columns would separate a gate from its up.
"""
from __future__ import annotations

import math

import torch

from .. import kernels as K
from ..type import OperatorType
from .base import OpImpl, register


@register(OperatorType.OP_GLU)
class GatedLinearUnit(OpImpl):
    op_type = OperatorType.OP_GLU

    @classmethod
    def infer(cls, attrs, in_dims, in_dtypes):
        K.glu_act_code("glu", attrs.get("activation", "silu"))
        if attrs.get("packed"):
            if len(in_dims) != 1:
                raise ValueError(f"glu: the packed form takes one input, got {len(in_dims)}")
            x = tuple(in_dims[0])
            if not x or x[-1] % 2:
                raise ValueError(f"glu: the packed input's last dim must be even (gate | up), got {list(x)}")
            return [x[:-1] + (x[-1] // 2,)], [in_dtypes[0]], []
        if len(in_dims) != 2:
            raise ValueError(f"glu takes gate and up, got {len(in_dims)} inputs")
        if tuple(in_dims[0]) != tuple(in_dims[1]):
            raise ValueError(f"glu: gate and up must have one shape, got {list(in_dims[0])} and {list(in_dims[1])}")
        if in_dtypes[0] != in_dtypes[1]:
            raise ValueError(f"glu: gate and up must have one dtype, got {in_dtypes[0]} and {in_dtypes[1]}")
        return [tuple(in_dims[0])], [in_dtypes[0]], []

    @property
    def act(self):
        return self.attrs.get("activation", "silu")

    def supports_axis(self, axis):
        return not (self.attrs.get("packed") and axis == len(self.layer.outputs[0].dims) - 1)

    def _halves(self, x):
        F = x.shape[-1] // 2
        return x[..., :F], x[..., F:]

    def forward(self, ctx, xs, ws):
        g, u = self._halves(xs[0]) if self.attrs.get("packed") else xs
        if ctx.training:
            ctx.saved["x"] = list(xs)
        return [K.glu_fwd(g, u, self.act)]

    def backward(self, ctx, douts):
        xs = ctx.saved.pop("x")
        dy = douts[0]
        if self.attrs.get("packed"):
            x = xs[0]
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            g, u = self._halves(x)
            dg, du = self._halves(dx)
            K.glu_bwd(g, u, dy, self.act, dg=dg, du=du)
            return [dx]
        dg, du = K.glu_bwd(xs[0], xs[1], dy, self.act)
        return [dg, du]

    def saves_output(self):
        return False

    def flops(self, in_shapes, out_shapes, w_shapes):
        return 8.0 * math.prod(out_shapes[0])  # the activation (exp, reciprocal, a few FMAs) and the product

    def uses_mfma(self):
        return False
