"""Rotary position embedding of projected heads (extension: no reference counterpart; the rotation
HuggingFace decoders apply to q and k in front of scaled_dot_product_attention).

y = rope(x) for x [B, H, S, D] (attribute `seq_dim=2`) or [B, S, H, D] (`seq_dim=1`): the first
`rope_dim` columns of every head row rotate by the angle of the row's position p, theta[p][i] =
(p / rope_scale) * inv_freq[i] with inv_freq[i] = rope_base^(-2i / rope_dim) (or the explicit
`rope_inv_freq`); pairs (i, i + rope_dim/2) (HF / NeoX rotate_half) or, `rope_interleaved`, (2i, 2i + 1)
(GPT-J); columns behind `rope_dim` pass through. p is the row index s, or position_ids[b, s] (second
input, int32 [B, S], attribute `rope_positions=True`), clamped to [0, rope_max_positions - 1] on the
device. Same shape and dtype, out of place, no weights; one launch of kernels.rope (rope.hip) through
the input's strides, the (cos, sin) table built on the host in float64 (kernels.rope_table). The
backward is the inverse rotation of dy (the Jacobian is orthogonal: nothing is saved but the ids);
the ids take no gradient.

Parallel axes: batch and heads (every part owns whole head rows and its rows of the ids).
"""
from __future__ import annotations

import math

import torch

from .. import kernels as K
from ..type import OperatorType
from .attention import check_rope_ids_dims, rope_attrs, rope_table_of
from .base import OpImpl, register


@register(OperatorType.OP_ROPE)
class RotaryEmbedding(OpImpl):
    op_type = OperatorType.OP_ROPE

    @classmethod
    def infer(cls, attrs, in_dims, in_dtypes):
        nr = 1 if attrs.get("rope_positions") else 0
        if len(in_dims) != 1 + nr:
            raise ValueError(f"rotary_embedding takes x[, position_ids]; got {len(in_dims)} inputs for "
                             f"rope_positions={bool(nr)}")
        x = tuple(in_dims[0])
        sd = attrs.get("seq_dim", 2)
        if len(x) != 4 or sd not in (1, 2):
            raise ValueError(f"rotary_embedding: x must be [B, H, S, D] (seq_dim=2) or [B, S, H, D] (seq_dim=1), got "
                             f"{list(x)} with seq_dim={sd}")
        rd, _, _, _, inv, maxp = rope_attrs(attrs)
        if rd < 2 or rd % 2 or rd > x[3]:
            raise ValueError(f"rotary_embedding: the rotary dim must be even and in [2, {x[3]}], got {rd}")
        if inv is not None and len(inv) != rd // 2:
            raise ValueError(f"rotary_embedding: inv_freq must hold {rd // 2} values, got {len(inv)}")
        if nr:
            check_rope_ids_dims("rotary_embedding", in_dims[1], in_dtypes[1], x[0], x[sd], x[sd])
        elif maxp < x[sd]:
            raise ValueError(f"rotary_embedding: max_positions ({maxp}) is below the sequence length ({x[sd]})")
        return [x], [in_dtypes[0]], []

    def _h_axis(self):
        return 3 - self.attrs.get("seq_dim", 2)

    def axis_kinds(self):
        kinds = ["sample", "none", "none", "none"]
        kinds[self._h_axis()] = "parameter"
        return kinds

    def supports_axis(self, axis):
        return axis in (0, self._h_axis())

    def input_maps(self):
        m = [None] * 4
        m[0], m[self._h_axis()] = 0, self._h_axis()
        maps = [tuple(m)]
        if self.attrs.get("rope_positions"):
            maps.append((0, None))
        return maps

    def needs_input_grad(self, i):
        return i == 0

    def setup_device(self, device):
        rope_table_of(rope_attrs(self.attrs), device)

    def _rotate(self, x, pos, inverse):
        x = x.contiguous()
        y = torch.empty_like(x)
        B, D = x.shape[0], x.shape[3]
        if self.attrs.get("seq_dim", 2) == 2:
            H, S = x.shape[1], x.shape[2]
            st = [H * S * D, S * D, D]
        else:
            S, H = x.shape[1], x.shape[2]
            st = [S * H * D, D, H * D]
        rope = rope_attrs(self.attrs)
        K.rope(x.view(-1), st, None, None, B, H, 0, S, 0, D, rope[0], rope_table_of(rope, x.device), pos=pos,
               interleaved=rope[2], inverse=inverse, q_out=y.view(-1))
        return y

    def forward(self, ctx, xs, ws):
        pos = xs[1] if self.attrs.get("rope_positions") else None
        if pos is not None and (pos.dtype != torch.int32 or pos.device != xs[0].device or not pos.is_contiguous()):
            pos = pos.to(device=xs[0].device, dtype=torch.int32).contiguous()
        if ctx.training:
            ctx.saved["pos"] = pos
        return [self._rotate(xs[0], pos, False)]

    def backward(self, ctx, douts):
        dx = self._rotate(douts[0], ctx.saved.get("pos"), True)
        ctx.saved.clear()
        return [dx] + [None] * (len(self.layer.inputs) - 1)

    def saves_output(self):
        return False

    def flops(self, in_shapes, out_shapes, w_shapes):
        x = in_shapes[0]
        return 3.0 * math.prod(x[:3]) * self.attrs["rope_dim"]

    def uses_mfma(self):
        return False
