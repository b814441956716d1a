"""Scaled dot-product attention on already projected heads (extension: no reference counterpart;
torch.nn.functional.scaled_dot_product_attention, met by the HuggingFace import path).

out[b, h] = softmax(scale * q[b, h] . k[b, h]^T + attn_bias[b, h], masks) . v[b, h] for q [B, H, Sq, D],
k [B, H, Sk, D], v [B, H, Sk, Dv] -> [B, H, Sq, Dv]. No weights. Inputs after q, k, v: `key_lengths`
(attribute `key_lengths=True`; int32 [B] or [B, 1]) and then `attn_bias` (attribute `attn_bias=True`;
float [1|B, 1|H, Sq, Sk]), with the semantics of ops/attention.py: a -inf (or overflowing) bias element
removes a key, a query row with no key left gives zeros, the bias and the lengths take no gradient.
`segment_ids` (attribute `segment_ids=True`; int32 [B, S], the 4th input, for Sq == Sk == S) packs several
sequences into a row as in ops/attention.py; not combined with `key_lengths` or `attn_bias`.
`scale` defaults to 1 / sqrt(D); `causal` and `dropout` are those of multihead_attention (the same
counter-based mask, drawn from global batch / head indices).
`enable_gqa` (attribute; torch's): k [B, Hkv, Sk, D] and v [B, Hkv, Sk, Dv] with Hkv dividing H, query head
h reading KV head h // (H // Hkv); dk / dv come back in those shapes. Without it mismatched head counts
are a ValueError. The heads axis then takes the degrees that divide Hkv.

Parallel axes: batch (sample) and heads (dim 1; a parameter-style split without a reduction: every
part owns whole heads of q, k, v and of the output). The kernels read q / k / v and write the output
through their [H*S*D, S*D, D] strides, so nothing is permuted or copied; the path (flash kernels, head
dims zero-padded to 64 / 128, fp32 device kernels, reference / CPU) is attention.attn_core_fwd's.
"""
from __future__ import annotations

import math

import torch

from .. import kernels as K
from ..type import DataType, OperatorType
from .attention import (attn_bias_map, attn_core_bwd, attn_core_fwd, attn_drop_args, attn_keep_ref,
                        check_attn_bias_dims, check_segment_ids_dims, check_window_dims, setup_window, window_attrs,
                        window_pairs)
from .base import OpImpl, register


@register(OperatorType.OP_SDPA)
class ScaledDotProductAttention(OpImpl):
    op_type = OperatorType.OP_SDPA
    H_AXIS = 1

    @classmethod
    def infer(cls, attrs, in_dims, in_dtypes):
        nk, nb = (1 if attrs.get("key_lengths") else 0), (1 if attrs.get("attn_bias") else 0)
        ns = 1 if attrs.get("segment_ids") else 0
        if ns and nk:
            raise ValueError("scaled_dot_product_attention: segment_ids cannot be combined with key_lengths")
        if len(in_dims) != 3 + nk + nb + ns:
            raise ValueError("scaled_dot_product_attention takes q, k, v[, key_lengths][, attn_bias]; got "
                             f"{len(in_dims)} inputs for key_lengths={bool(nk)}, attn_bias={bool(nb)}")
        q, k, v = (tuple(d) for d in in_dims[:3])
        if not (len(q) == len(k) == len(v) == 4):
            raise ValueError(f"scaled_dot_product_attention: q, k, v must be [B, H, S, D], got {q}, {k}, {v}")
        if attrs.get("enable_gqa"):
            if q[0] != k[0] or q[0] != v[0] or q[3] != k[3] or k[2] != v[2] or k[1] != v[1] or k[1] <= 0 or q[1] % k[1]:
                raise ValueError(f"scaled_dot_product_attention: mismatched q {q}, k {k}, v {v} (enable_gqa: k and v "
                                 "have equal head counts that divide q's)")
        elif q[:2] != k[:2] or q[:2] != v[:2] or q[3] != k[3] or k[2] != v[2]:
            raise ValueError(f"scaled_dot_product_attention: mismatched q {q}, k {k}, v {v} (GQA / MQA head "
                             "broadcasting needs enable_gqa=True)")
        B, H, Sq, _ = q
        if ns:
            check_segment_ids_dims("scaled_dot_product_attention", in_dims, nb, B, Sq, k[2])
        if window_attrs(attrs) is not None:
            check_window_dims("scaled_dot_product_attention", attrs, nk, nb, Sq, k[2])
        if nk:
            kl = tuple(in_dims[3])
            if kl not in ((B,), (B, 1)):
                raise ValueError(f"key_lengths must have shape [{B}] or [{B}, 1], got {list(kl)}")
        if nb:
            check_attn_bias_dims("scaled_dot_product_attention", in_dims[-1], B, H, Sq, k[2])
            if in_dtypes[-1] not in (DataType.DT_FLOAT, DataType.DT_BF16, DataType.DT_HALF, DataType.DT_DOUBLE):
                raise ValueError(f"scaled_dot_product_attention: attn_bias must be a float tensor, got {in_dtypes[-1]}")
        K.attn_dropout_thr(attrs.get("dropout", 0.0))  # ValueError outside [0, 1)
        sc = attrs.get("scale")
        if sc is not None and not math.isfinite(float(sc)):
            raise ValueError(f"scaled_dot_product_attention: scale must be finite, got {sc}")
        return [(B, H, Sq, v[3])], [in_dtypes[0]], []

    # axes: 0 batch, 1 heads, 2 query rows, 3 head dim
    def axis_kinds(self):
        return ["sample", "parameter", "none", "none"]

    def supports_axis(self, axis):
        return axis in (0, 1)

    def input_maps(self):
        maps = [(0, 1, None, None)] * 3
        q = self.layer.inputs[0].dims
        if self.attrs.get("key_lengths") or self.attrs.get("segment_ids"):
            maps.append((0,) + (None,) * (len(self.layer.inputs[3].dims) - 1))
        if self.attrs.get("attn_bias"):
            maps.append(attn_bias_map(self.layer.inputs[-1].dims, q[0], q[1], 0, self.H_AXIS))
        return maps

    def needs_input_grad(self, i):
        return i < 3

    def setup_device(self, device):
        """Called once by the executor, outside any captured region: a sliding window's bound arrays."""
        q = self.layer.inputs[0].dims
        setup_window(self.attrs, q[0], q[2], device)

    def drops_attention(self) -> bool:
        return K.attn_dropout_thr(self.attrs.get("dropout", 0.0)) > 0

    def forward(self, ctx, xs, ws):
        q, k, v = (t.contiguous() for t in xs[:3])
        B, Hl, Sq, kd = q.shape
        Hkv, Sk, vd = k.shape[1], k.shape[2], v.shape[3]  # Hkv < Hl: enable_gqa (this part's heads of both)
        has_kl, has_bias = bool(self.attrs.get("key_lengths")), bool(self.attrs.get("attn_bias"))
        kl = K.attn_key_lens(xs[3], B, q.device) if has_kl else None
        bias = K.attn_score_bias(xs[-1], B, Hl, Sq, Sk, q.device) if has_bias else None
        has_seg, win = bool(self.attrs.get("segment_ids")), window_attrs(self.attrs)
        seg = K.attn_segments(xs[3] if has_seg else None, B, Sq, q.device, window=win) if has_seg or win else None
        sc = self.attrs.get("scale")
        scale = 1.0 / math.sqrt(kd) if sc is None else float(sc)
        causal = bool(self.attrs.get("causal", False))
        H_total = self.layer.inputs[0].dims[1]
        drop = attn_drop_args(self, ctx, B, Hl, self.H_AXIS, H_total, q.device)
        s = ctx.saved if ctx.training else {}
        qs, ks, vs = [Hl * Sq * kd, Sq * kd, kd], [Hkv * Sk * kd, Sk * kd, kd], [Hkv * Sk * vd, Sk * vd, vd]
        os_ = [Hl * Sq * vd, Sq * vd, vd]
        o = torch.empty(B, Hl, Sq, vd, device=q.device, dtype=q.dtype)
        attn_core_fwd(s, self.layer.name, q.view(-1), qs, k.view(-1), ks, v.view(-1), vs, o, os_, B, Hl, Sq, Sk, kd, vd,
                      scale, causal, kl, drop, bias, lambda: attn_keep_ref(self, ctx, drop, B, Hl, Sq, Sk, q.device), seg=seg,
                      Hkv=Hkv)
        if ctx.training:
            s.update(q=q, k=k, v=v, o=o, shape=(B, Hl, Sq, Sk, kd, vd), st=(qs, ks, vs, os_), scale=scale,
                     causal=causal, key_lens=kl, drop=drop, sbias=bias, seg=seg, Hkv=Hkv)
        return [o]

    def backward(self, ctx, douts):
        s = ctx.saved
        B, Hl, Sq, Sk, kd, vd = s["shape"]
        qs, ks, vs, os_ = s["st"]
        q, k, v, o = s["q"], s["k"], s["v"], s["o"]
        do = douts[0].contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        attn_core_bwd(s, q.view(-1), qs, k.view(-1), ks, v.view(-1), vs, o, os_, do, os_, dq, dk, dv, B, Hl, Sq, Sk, kd,
                      vd, s["scale"], s["causal"], s["key_lens"], s["drop"], s["sbias"], seg=s.get("seg"), Hkv=s.get("Hkv"))
        ctx.saved.clear()
        return [dq, dk, dv] + [None] * (len(self.layer.inputs) - 3)

    def flops(self, in_shapes, out_shapes, w_shapes):
        B, H, Sq, D = in_shapes[0]
        Sk, Dv = in_shapes[2][2], in_shapes[2][3]
        win = window_attrs(self.attrs)
        if win is not None:  # the band's pairs only
            return 2.0 * B * H * window_pairs(Sq, win, bool(self.attrs.get("causal"))) * (D + Dv)
        return 2.0 * B * H * Sq * Sk * (D + Dv)

    def uses_mfma(self):
        return True
