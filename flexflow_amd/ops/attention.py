"""Multi-head attention (reference src/ops/attention.cc / attention.cu, cuDNN MHA; the reference HIP
build compiles it to a no-op, attention.cpp:33-43).

Semantics follow the reference API: `kdim`/`vdim` are per-head projection sizes, output size is
`embed_dim`. Parallel axes: batch (sample), sequence (query side only; kept at 1), and a *heads*
axis (parameter parallelism): each part owns H/deg heads — its slice of the Q/K/V and output
projections — and emits a partial sum of the output projection (reduced on the consumer edge).

GPU path (bf16): for self-attention ONE fused QKV GEMM ([T,E] x [3*H*D,E]^T) whose output is read
in place by the flash-attention kernel through strides (no permute copies), then the output
projection GEMM; the backward mirrors it (flash bwd writes dQ/dK/dV straight into the fused
[T, 3, H, D] gradient buffer that feeds one dgrad and one split-K wgrad GEMM).

Optional 4th input `key_lengths` (int32 [B] or [B, 1], on the activations' device): sample b of a
right-padded batch has L_b = clamp(key_lengths[b], 0, Sk) real keys; key j takes part in the softmax
iff j < L_b (and j <= q with `causal`). Every query row is still computed (as with torch's
key_padding_mask); L_b = 0 gives zero output rows and zero gradients. The lengths are read on the
device only, by every path (flash, zero-padded head dims, fp32 device, reference, CPU), so a step
that takes them still captures into a graph. The pad positions' labels are left out of the loss by
`FFModel.compile(ignore_index=...)`. Query-side skipping comes with packing (`segment_ids`, below).

Optional last input `attn_bias` (attribute `attn_bias=True`; after `key_lengths` when both are given):
a float tensor [1|B, 1|H, Sq, Sk] added to the scaled scores before the softmax, in every path — ALiBi,
relative-position biases, sliding windows, left padding or block masks as 0 / -inf. The flash kernels
read it as fp32 (cast once per forward when it is not) while they compute the scores, so no [B, H,
Sq, Sk] tensor is built. An element of -inf, or one so negative that bias * log2(e) overflows fp32
(HuggingFace's finfo.min masks), removes that key; a query row with no key left gives a zero output
row and zero gradients (the key-length convention; torch gives NaN). +inf and NaN are the caller's
problem. The bias takes no gradient, and with it the flash backward leaves the QKV bias gradient to
the projection's own backward. It is sharded with the batch where its first extent is B and with the
heads where its second is H, replicated elsewhere. The same core (attn_core_fwd / attn_core_bwd) serves
`scaled_dot_product_attention` (ops/sdpa.py).

Packed sequences (attribute `segment_ids=True`; the 4th input, where the key lengths would sit): an
int32 tensor [B, S] with one id per token of rows that hold several sequences back to back. A
position is padding iff its id is negative; a segment is a maximal run of equal ids >= 0 (two runs
that reuse an id are two segments; ids need not be sorted; pad runs may sit anywhere). Query i sees key
j iff both lie in the same run (and j <= i with `causal`), so it needs Sq == Sk. A padding position
gives a zero attention row (the output row is the output bias) and zero gradients, as a query and as
a key. The ids are read on the device only, by every path: a bounds kernel (kernels.attn_seg_bounds)
turns them into the run [lo, hi) of every position once per layer forward, and the flash kernels'
SEG forms bound their mask tests and their tile loops by it, so tiles outside a workgroup's runs are
never fetched. Not combined with `key_lengths` (a pad id of -1 says the same) or `attn_bias`. It takes
no gradient, is sharded with the batch and replicated over the heads axis.

Sliding window (attributes `window_left` / `window_right`, set by the builder's `window=`; -1 is an
unbounded side; absent for a window that bounds nothing, and then the graph and every launch are what
they were): query i sees key j iff i - left <= j <= i + right, and j <= i with `causal`, and both lie in
one run with `segment_ids` (flash-attention's window_size convention). It needs Sq == Sk and goes with
neither `key_lengths` nor `attn_bias`, the rule of `segment_ids`; padding is said with negative segment
ids. A small kernel (kernels.attn_band_bounds) writes the key interval of every query and, for the
backward, the query interval of every key; the flash kernels' SEG forms bound their mask tests and their
tile loops by them, so the tiles outside the band are never fetched. Without segment ids the arrays are
a constant of the layer, built when the executor sets it up; with ids they follow the run bounds once
per layer forward. `flops()` counts the band.

Attention dropout (`dropout` = p in [0, 1), torch's `dropout_p`): in a training forward every
attention probability is dropped with the effective rate p_eff = round(256 p) / 256 and the kept ones
are scaled by 1 / (1 - p_eff); evaluation forwards apply nothing, and p_eff = 0 runs exactly the
kernels of a layer without dropout. Whether element (b, h, q, k) is kept is a pure function of
(seed, layer id, step, b, h, q, k) with GLOBAL batch and head indices (csrc/kernels/attn_dropout.h,
mirrored by kernels.attn_dropout_keep_ref), so every path (flash kernels, zero-padded head dims,
fp32 device, reference, CPU) and every shard draws the mask a 1-GPU run draws. The layer id is the
CRC-32 of the layer name; the step is the executor's device-side counter (`ctx.rng_step`, read by
the kernels on the device, so a captured step draws a new mask at every replay; step 0 without an
executor). The flash kernels generate the mask themselves, forward and backward, from the same
counters: P is never materialised.

Grouped-query / multi-query attention (attribute `num_kv_heads` = Hkv < H, dividing H; absent for plain
multi-head attention, whose graph and launches are unchanged): the K / V projections produce Hkv heads
(`k_weight` (Hkv, kd, Ek), `v_weight` (Hkv, vd, Ev), always the unfused form) and query head h reads KV
head h // (H // Hkv), torch's `enable_gqa` / `repeat_interleave` convention. K and V are never
repeated: the flash kernels index them by the KV head, and in the backward each query head's dK / dV
contribution is summed per group in fp32 by one kernel (kernels.flash_attn_bwd). The heads axis splits
dim 0 of every projection weight, so it takes the degrees that divide Hkv. The score bias's head extent
stays 1 or H (query heads); the QKV bias gradient is summed by the projections' own backward.

Rotary position embeddings (attributes `rope_dim`, `rope_base`, `rope_interleaved`, `rope_scale`,
`rope_inv_freq`, `rope_max_positions`, set by the builder's `rotary=`; absent otherwise, and then the graph
and every launch are what they were): after the projection GEMMs ONE launch (kernels.rope, rope.hip)
rotates the Q and K head rows in place, inside the fused [T, 3, H, D] buffer or in the separate q / k
buffers, so every path below (flash, zero-padded head dims, fp32 device, reference / CPU) sees rotated
heads and the tensors saved for the backward are the rotated ones. Query i and key j take positions i
and j (also for Sq != Sk), or, with the int32 [B, S] input `rope_position_ids` (attribute
`rope_positions=True`; after key_lengths / segment_ids and before attn_bias; Sq == Sk), the ids of a
packed row (utils/packing.py), read and clamped to [0, max_positions - 1] on the device. The backward
rotates dq / dk back with one inverse launch (the Jacobian is orthogonal, nothing is saved for it) before
the projections' backward; the flash kernel's fused QKV bias gradient is off with rotary, since it would
sum dq / dk columns before they are rotated back, and linear_bwd sums it instead. The ids take no
gradient, are sharded with the batch and replicated over the heads axis; the rotation is per head row,
so a shard needs nothing but its rows. The (cos, sin) table is built on the host in float64
(kernels.rope_table) when the executor sets the layer up, outside any captured region.
"""
from __future__ import annotations

import math
import os
import zlib

import torch

from .. import kernels as K
from ..type import OperatorType
from .base import OpImpl, WeightSpec, register


def _pad_heads(t, st, B, S, H, d, Dp):
    """[B, S, H, Dp] zero-padded copy of the strided per-head view (batch, head, row strides st)."""
    out = torch.zeros(B, S, H, Dp, device=t.device, dtype=t.dtype)
    out[..., :d].copy_(t.as_strided((B, H, S, d), (st[0], st[1], st[2], 1)).permute(0, 2, 1, 3))
    return out


def _attn_ref(q, k, v, scale, causal, key_lens=None, keep=None, keep_scale=1.0, bias=None, segments=None, window=None):
    """window: optional sliding window (left, right) with -1 for an unbounded side (Sq == Sk): the mask is
    kernels.band_mask_ref's, built from the definition, with the runs of `segments` when those are given.
    segments: optional segment ids [B, S] of packed rows (Sq == Sk == S): query i sees key j iff both
    lie in one run of equal ids >= 0; the mask is built on the tensor's device from the run boundaries
    (kernels.segment_mask_ref), and a padding row gets P = 0. keep: optional bool [B, H, Sq, Sk] attention dropout mask (kernels.attn_dropout_keep_ref), the
    kept probabilities scaled by keep_scale = 1 / (1 - p_eff). bias: optional score bias [1|B, 1|H, Sq,
    Sk], added to the scaled scores; a query row it leaves no key gets P = 0 (not the softmax's NaN)."""
    def drop(p):
        return p if keep is None else torch.where(keep, p * keep_scale, torch.zeros_like(p))

    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    Sq, Sk = s.shape[-2:]
    if bias is not None:
        s = s + bias.to(device=s.device, dtype=s.dtype)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    if segments is not None or window is not None:
        if key_lens is not None or bias is not None:
            raise ValueError("attention: segment_ids / window cannot be combined with key_lengths or attn_bias")
        if window is not None:  # [B|1, 1, S, S]; the causal bound is in s already
            if Sq != Sk:
                raise ValueError(f"attention: window needs Sq == Sk, got Sq {Sq}, Sk {Sk}")
            ids = segments.to(s.device) if segments is not None else None
            see = K.band_mask_ref(Sq, window[0], window[1], False, ids).to(s.device)[:, None]
        else:
            see = K.segment_mask_ref(segments.to(s.device))[:, None]  # [B, 1, S, S]
        dead = ~see.any(-1, keepdim=True)  # padding rows: finite scores first, then P = 0
        s = torch.where(dead, torch.zeros_like(s), s.masked_fill(~see, float("-inf")))
        p = torch.where(dead, torch.zeros_like(s), torch.softmax(s, -1))
        return torch.einsum("bhqk,bhkd->bhqd", drop(p), v)
    if bias is not None:
        # the kernels' convention for every removed key and every row without keys, lengths included
        if key_lens is not None:
            L = key_lens.reshape(-1).to(s.device).clamp(0, Sk)
            s = s.masked_fill((torch.arange(Sk, device=s.device)[None, :] >= L[:, None])[:, None, None, :], float("-inf"))
        dead = (s == float("-inf")).all(-1, keepdim=True)
        s = torch.where(dead, torch.zeros_like(s), s)
        p = torch.where(dead, torch.zeros_like(s), torch.softmax(s, -1))
        return torch.einsum("bhqk,bhkd->bhqd", drop(p), v)
    if key_lens is None:
        return torch.einsum("bhqk,bhkd->bhqd", drop(torch.softmax(s, -1)), v)
    # keys at or past the sample's length leave the softmax; a sample without keys gets P = 0 (its
    # scores are made finite first, so neither the softmax nor its gradient sees a NaN). All on the
    # tensor's device: the lengths are never read on the host.
    L = key_lens.reshape(-1).to(s.device).clamp(0, Sk)
    pad = torch.arange(Sk, device=s.device)[None, :] >= L[:, None]
    empty = (L == 0)[:, None, None, None]
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    s = torch.where(empty, torch.zeros_like(s), s)
    p = torch.where(empty, torch.zeros_like(s), torch.softmax(s, -1))
    return torch.einsum("bhqk,bhkd->bhqd", drop(p), v)


def _view4(t, st, B, H, S, d):
    """[B, H, S, d] view of a flat / strided buffer with (batch, head, row) element strides st."""
    return t.as_strided((B, H, S, d), (st[0], st[1], st[2], 1))


def _repeat_kv(t, G):
    """[B, Hkv, S, d] -> [B, Hkv * G, S, d], head h a copy of KV head h // G (grouped-query attention);
    autograd sums a group's gradients back into its KV head."""
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def attn_core_fwd(s, name, qv, qs, kv, ks, vv, vs, o, os_, B, Hl, Sq, Sk, kd, vd, scale, causal, kl, drop, bias, keep_ref,
                  seg=None, Hkv=None):
    """softmax(scale q.k + bias, masks) v of MultiHeadAttention and ScaledDotProductAttention: q / k / v
    / o are buffers read and written through their (batch, head, row) element strides qs / ks / vs /
    os_ with contiguous head dims. Picks the path (flash kernels, head dims zero-padded to 64 / 128,
    fp32 device kernels, fp32 PyTorch reference / CPU) and leaves in `s` what attn_core_bwd needs of
    it. kl: key lengths (kernels.attn_key_lens) or None; drop: attention dropout as the kernels take it
    or None; bias: score bias (kernels.attn_score_bias) or None; keep_ref(): the dropout mask for the
    reference path; seg: packed-sequence runs (kernels.attn_segments) or None; Hkv: the KV head count
    of grouped-query attention (k / v and ks / vs hold Hkv heads, query head h reads KV head
    h // (Hl // Hkv)) or None for Hl."""
    Hkv = K.attn_kv_heads(Hl, Hkv)
    if K.attn_supported(qv, kd) and kd == vd:
        s["lse"] = K.flash_attn_fwd(qv, qs, kv, ks, vv, vs, o, os_, B, Hl, Sq, Sk, kd, scale, causal, key_lens=kl,
                                    drop=drop, bias=bias, segments=seg, Hkv=Hkv)
    elif K.attn_padded_dim(qv, kd, vd):
        # head dims the MFMA kernels have no instance for (e.g. 16, 32, 80, 96): zero-pad Q, K,
        # V to the next instance (64 / 128). Zero columns add nothing to Q.K^T and give zero
        # output columns, so the softmax and the sliced output are exact; the scale is the caller's
        Dp = K.attn_padded_dim(qv, kd, vd)
        pq, pk, pv = (_pad_heads(t, st, B, S_, H_, kd, Dp) for t, st, S_, H_ in
                      ((qv, qs, Sq, Hl), (kv, ks, Sk, Hkv), (vv, vs, Sk, Hkv)))
        po = torch.empty(B, Sq, Hl, Dp, device=qv.device, dtype=qv.dtype)
        pst = [Sq * Hl * Dp, Dp, Hl * Dp]
        kst = [Sk * Hkv * Dp, Dp, Hkv * Dp]
        lse = K.flash_attn_fwd(pq, pst, pk, kst, pv, kst, po, pst, B, Hl, Sq, Sk, Dp, scale, causal, key_lens=kl,
                               drop=drop, bias=bias, segments=seg, Hkv=Hkv)
        _view4(o, os_, B, Hl, Sq, vd).copy_(po[..., :vd].permute(0, 2, 1, 3))
        s.update(lse=lse, pad=(Dp, pq, pk, pv, po))
    elif K.attn_f32_supported(qv) and os.environ.get("FF_ATTN_REF_FALLBACK") != "1":
        # --dtype fp32 on the device: f32 MFMA GEMMs + causal mask + row softmax, our kernels
        s["P"] = K.attn_f32_fwd(qv, qs, kv, ks, vv, vs, o.view(-1), os_, B, Hl, Sq, Sk, kd, vd, scale, causal,
                                key_lens=kl, drop=drop, bias=bias, segments=seg, Hkv=Hkv)
    else:
        if K.native(qv) and qv.dtype == torch.bfloat16 and os.environ.get("FF_ATTN_REF_FALLBACK") != "1":
            raise NotImplementedError(
                f"{name}: no MFMA attention kernel for head dims q/k {kd}, v {vd} (supported: equal "
                "q/k/v head dims up to 128; FF_ATTN_REF_FALLBACK=1 runs the fp32 PyTorch reference instead)")
        q4 = _view4(qv, qs, B, Hl, Sq, kd).float()
        k4 = _repeat_kv(_view4(kv, ks, B, Hkv, Sk, kd).float(), Hl // Hkv)
        v4 = _repeat_kv(_view4(vv, vs, B, Hkv, Sk, vd).float(), Hl // Hkv)
        keep = keep_ref() if drop else None
        if keep is not None:
            s["keep"] = keep
        _view4(o, os_, B, Hl, Sq, vd).copy_(
            _attn_ref(q4, k4, v4, scale, causal, kl, keep, 256.0 / (256 - drop[0]) if drop else 1.0, bias,
                      seg[0] if seg is not None else None, seg.window if seg is not None else None))


def attn_core_bwd(s, qv, qs, kv, ks, vv, vs, o, os_, do, dos, dq, dk, dv, B, Hl, Sq, Sk, kd, vd, scale, causal, kl, drop,
                  bias, dbq=None, seg=None, Hkv=None):
    """Backward of attn_core_fwd on the path it took: dq / dk / dv (buffers with q / k / v's strides)
    from do (strides dos) and what the forward left in `s`. dbq: the fp32 [3*H*D] bias gradient of a fused
    QKV projection the flash kernel may add into; returns whether it did. Hkv: as in attn_core_fwd; dk /
    dv hold Hkv heads, each the sum over its group of query heads."""
    Hkv = K.attn_kv_heads(Hl, Hkv)
    if "pad" in s:
        Dp, pq, pk, pv, po = s["pad"]
        pdo = torch.zeros_like(po)
        pdo[..., :vd] = _view4(do, dos, B, Hl, Sq, vd).permute(0, 2, 1, 3)
        pdq, pdk, pdv = torch.empty_like(pq), torch.empty_like(pk), torch.empty_like(pv)
        pst = [Sq * Hl * Dp, Dp, Hl * Dp]
        kst = [Sk * Hkv * Dp, Dp, Hkv * Dp]
        K.flash_attn_bwd(pq, pst, pk, kst, pv, kst, po, pst, pdo, pst, s["lse"], pdq, pst, pdk, kst, pdv, kst,
                         B, Hl, Sq, Sk, Dp, scale, causal, key_lens=kl, drop=drop, bias=bias, segments=seg, Hkv=Hkv)
        for g, st, pg, S_, d, H_ in ((dq, qs, pdq, Sq, kd, Hl), (dk, ks, pdk, Sk, kd, Hkv), (dv, vs, pdv, Sk, vd, Hkv)):
            _view4(g, st, B, H_, S_, d).copy_(pg[..., :d].permute(0, 2, 1, 3))
    elif "lse" in s:
        if dbq is not None and Hkv == Hl:
            return K.flash_attn_bwd(qv, qs, kv, ks, vv, vs, o, os_, do, dos, s["lse"], dq, qs, dk, ks, dv, vs,
                                    B, Hl, Sq, Sk, kd, scale, causal, dbias=dbq, key_lens=kl, drop=drop, bias=bias,
                                    segments=seg)
        K.flash_attn_bwd(qv, qs, kv, ks, vv, vs, o, os_, do, dos, s["lse"], dq, qs, dk, ks, dv, vs,
                         B, Hl, Sq, Sk, kd, scale, causal, key_lens=kl, drop=drop, bias=bias, segments=seg, Hkv=Hkv)
    elif "P" in s:
        K.attn_f32_bwd(qv, qs, kv, ks, vv, vs, do.contiguous().view(-1), dos, s["P"], dq.view(-1), dk.view(-1),
                       dv.view(-1), B, Hl, Sq, Sk, kd, vd, scale, key_lens=kl, drop=drop, bias=bias, segments=seg,
                       Hkv=Hkv)
    else:
        q4 = _view4(qv, qs, B, Hl, Sq, kd).detach().float().requires_grad_()
        k4 = _view4(kv, ks, B, Hkv, Sk, kd).detach().float().requires_grad_()
        v4 = _view4(vv, vs, B, Hkv, Sk, vd).detach().float().requires_grad_()
        with torch.enable_grad():
            out = _attn_ref(q4, _repeat_kv(k4, Hl // Hkv), _repeat_kv(v4, Hl // Hkv), scale, causal, kl, s.get("keep"),
                            256.0 / (256 - drop[0]) if drop else 1.0, bias, seg[0] if seg is not None else None,
                            seg.window if seg is not None else None)
        g4 = _view4(do, dos, B, Hl, Sq, vd).float()
        gq, gk, gv = torch.autograd.grad(out, (q4, k4, v4), g4)
        _view4(dq, qs, B, Hl, Sq, kd).copy_(gq)
        _view4(dk, ks, B, Hkv, Sk, kd).copy_(gk)
        _view4(dv, vs, B, Hkv, Sk, vd).copy_(gv)
    return False


def attn_drop_args(impl, ctx, B, Hl, h_axis, H_total, device):
    """Attention dropout of this training forward as the kernels take it: (thr, rng_step, rng_seed,
    b0, h0, H_total) with the shard's first global batch / head index, or None."""
    thr = K.attn_dropout_thr(impl.attrs.get("dropout", 0.0))
    if not (ctx.training and thr):
        return None
    step = ctx.rng_step
    if step is None or step.device != device:  # no executor (cost model, op-level tests): step 0
        step = ctx.extra.get("rng_step0")
        if step is None or step.device != device:
            step = ctx.extra["rng_step0"] = torch.zeros(1, dtype=torch.int64, device=device)
    seed = K.attn_dropout_seed(ctx.seed, zlib.crc32(impl.layer.name.encode()))
    return (thr, step, seed, ctx.coord(0) * B, ctx.coord(h_axis) * Hl, int(H_total))


def attn_keep_ref(impl, ctx, drop, B, Hl, Sq, Sk, device):
    """The mirror's mask for the reference / CPU path (the same one the kernels draw)."""
    thr, step, _, b0, h0, H_total = drop
    return K.attn_dropout_keep_ref(ctx.seed, zlib.crc32(impl.layer.name.encode()), step, B, Hl, Sq, Sk,
                                   thr / 256.0, b0=b0, h0=h0, H_total=H_total, device=device)


def check_attn_bias_dims(what, dims, B, H, Sq, Sk):
    d = tuple(dims)
    if len(d) != 4 or d[0] not in (1, B) or d[1] not in (1, H) or d[2:] != (Sq, Sk):
        raise ValueError(f"{what}: attn_bias must have shape [1|{B}, 1|{H}, {Sq}, {Sk}], got {list(d)}")


def check_segment_ids_dims(what, in_dims, nb, B, Sq, Sk):
    """infer-time checks of an attention layer built with segment_ids=True: the ids are the 4th input,
    [B, S] for Sq == Sk == S, and there is neither a score bias nor (the builder's check) key lengths."""
    if nb:
        raise ValueError(f"{what}: segment_ids cannot be combined with attn_bias")
    if len(in_dims) != 4:
        raise ValueError(f"{what}: segment_ids=True takes query, key, value, segment_ids; got {len(in_dims)} inputs")
    if Sq != Sk:
        raise ValueError(f"{what}: segment_ids needs Sq == Sk (one segmentation for queries and keys), "
                         f"got Sq {Sq}, Sk {Sk}")
    if tuple(in_dims[3]) != (B, Sq):
        raise ValueError(f"{what}: segment_ids must have shape [{B}, {Sq}], got {list(in_dims[3])}")


def window_attrs(attrs):
    """(left, right) of a layer built with a sliding window (-1: that side unbounded), or None."""
    if "window_left" not in attrs and "window_right" not in attrs:
        return None
    return int(attrs.get("window_left", -1)), int(attrs.get("window_right", -1))


def check_window_dims(what, attrs, has_kl, nb, Sq, Sk):
    """infer-time checks of an attention layer built with window_left / window_right: the rule of
    segment_ids (Sq == Sk, neither key lengths nor a score bias), and sizes >= 0 or -1."""
    left, right = window_attrs(attrs)
    if min(left, right) < -1 or max(left, right) < 0:
        raise ValueError(f"{what}: window sizes must be >= 0 (-1: unbounded) with one side bounded, got {(left, right)}")
    if has_kl:
        raise ValueError(f"{what}: window cannot be combined with key_lengths (mark padding with a negative segment id)")
    if nb:
        raise ValueError(f"{what}: window cannot be combined with attn_bias")
    if Sq != Sk:
        raise ValueError(f"{what}: window needs Sq == Sk (positions are row indices), got Sq {Sq}, Sk {Sk}")


def window_pairs(S, window, causal):
    """The (query, key) pairs a window leaves in an S x S score matrix: per row min(i, left) +
    min(S - 1 - i, right) + 1 keys, nothing to the right with causal."""
    def side(w):  # sum over i of min(i, w): 0 + 1 + .. + w, then w for each of the S - 1 - w rows behind
        w = S - 1 if w < 0 else min(w, S - 1)
        return w * (w + 1) // 2 + (S - 1 - w) * w

    left, right = window
    return S + side(left) + (0 if causal else side(right))


def setup_window(attrs, B, S, device):
    """The bound arrays of a window without segment ids are a constant of the layer: built here, when
    the executor sets the layer up, outside any captured region (kernels.attn_band_bounds_const)."""
    win = window_attrs(attrs)
    if win is not None and not attrs.get("segment_ids") and K.native_device(device):
        K.attn_band_bounds_const(B, S, win[0], win[1], device)


def rope_attrs(attrs):
    """(dim, base, interleaved, scale, inv_freq, max_positions) of a layer built with rotary, or None."""
    if not attrs.get("rope_dim"):
        return None
    return (attrs["rope_dim"], attrs.get("rope_base", 10000.0), bool(attrs.get("rope_interleaved", False)),
            attrs.get("rope_scale", 1.0), attrs.get("rope_inv_freq"), attrs["rope_max_positions"])


def rope_table_of(rope, device):
    rd, base, _, scale, inv, maxp = rope
    return K.rope_table(rd, maxp, base, scale, inv, device)


def check_rope_ids_dims(what, dims, dtype, B, Sq, Sk):
    from ..type import DataType
    if Sq != Sk:
        raise ValueError(f"{what}: rope_position_ids needs Sq == Sk (one id per token), got Sq {Sq}, Sk {Sk}")
    if tuple(dims) != (B, Sq):
        raise ValueError(f"{what}: rope_position_ids must have shape [{B}, {Sq}], got {list(dims)}")
    if dtype != DataType.DT_INT32:
        raise ValueError(f"{what}: rope_position_ids must be an int32 tensor, got {dtype}")


def attn_bias_map(dims, B, H, batch_axis, heads_axis):
    """input_maps entry of a score bias: with the batch where its first extent is B, with the heads
    where its second is H, replicated elsewhere."""
    return (batch_axis if dims[0] == B else None, heads_axis if dims[1] == H else None, None, None)


@register(OperatorType.OP_MULTIHEAD_ATTENTION)
class MultiHeadAttention(OpImpl):
    op_type = OperatorType.OP_MULTIHEAD_ATTENTION

    @classmethod
    def infer(cls, attrs, in_dims, in_dtypes):
        nb = 1 if attrs.get("attn_bias") else 0
        nr = 1 if attrs.get("rope_positions") else 0
        if len(in_dims) - nb - nr not in (3, 4):
            raise ValueError("multihead_attention takes query, key, value[, key_lengths][, rope_position_ids]"
                             f"[, attn_bias]; got {len(in_dims)} inputs" + (" with attn_bias=True" if nb else "")
                             + (" with rope_positions=True" if nr else ""))
        q, k, v = in_dims[:3]
        if nr:  # behind the key lengths / segment ids, in front of the score bias
            ri = len(in_dims) - nb - 1
            if not attrs.get("rope_dim"):
                raise ValueError("multihead_attention: rope_position_ids needs rotary")
            check_rope_ids_dims("multihead_attention", in_dims[ri], in_dtypes[ri], q[0], q[1], k[1])
            in_dims = [d for i, d in enumerate(in_dims) if i != ri]
        if attrs.get("segment_ids"):
            check_segment_ids_dims("multihead_attention", in_dims, nb, q[0], q[1], k[1])
        elif len(in_dims) - nb == 4:
            kl = tuple(in_dims[3])
            if kl not in ((q[0],), (q[0], 1)):
                raise ValueError(f"key_lengths must have shape [{q[0]}] or [{q[0]}, 1], got {list(kl)}")
        if window_attrs(attrs) is not None:
            check_window_dims("multihead_attention", attrs, not attrs.get("segment_ids") and len(in_dims) - nb == 4,
                              nb, q[1], k[1])
        if nb:
            from ..type import DataType
            check_attn_bias_dims("multihead_attention", in_dims[-1], q[0], attrs["num_heads"], q[1], k[1])
            if in_dtypes[-1] not in (DataType.DT_FLOAT, DataType.DT_BF16, DataType.DT_HALF, DataType.DT_DOUBLE):
                raise ValueError(f"multihead_attention: attn_bias must be a float tensor, got {in_dtypes[-1]}")
        K.attn_dropout_thr(attrs.get("dropout", 0.0))  # ValueError outside [0, 1)
        H = attrs["num_heads"]
        Hkv = attrs.get("num_kv_heads") or H
        if Hkv <= 0 or H % Hkv:
            raise ValueError(f"multihead_attention: num_kv_heads ({Hkv}) must divide num_heads ({H})")
        E = attrs["embed_dim"]
        kd = attrs.get("kdim") or E // H
        vd = attrs.get("vdim") or E // H
        attrs["kdim"], attrs["vdim"] = kd, vd
        if attrs.get("rope_dim"):
            rd, maxp = attrs["rope_dim"], attrs["rope_max_positions"]
            if rd < 2 or rd % 2 or rd > kd:
                raise ValueError(f"multihead_attention: the rotary dim must be even and in [2, {kd}], got {rd}")
            if attrs.get("rope_inv_freq") is not None and len(attrs["rope_inv_freq"]) != rd // 2:
                raise ValueError(f"multihead_attention: rotary inv_freq must hold {rd // 2} values")
            if not nr and maxp < max(q[1], k[1]):
                raise ValueError(f"multihead_attention: rotary max_positions ({maxp}) is below the sequence length")
        dt = in_dtypes[0]
        kinit = attrs.get("kernel_init")
        from ..core.initializers import ZeroInitializer
        ws = []
        if Hkv == H and attrs.get("self_attn") and kd == vd and q[-1] == k[-1] == v[-1]:
            attrs["fused_qkv"] = True
            ws.append(WeightSpec("qkv_weight", (3, H, kd, q[-1]), dt, kinit))
            if attrs.get("bias", True):
                ws.append(WeightSpec("qkv_bias", (3, H, kd), dt, ZeroInitializer()))
        else:
            attrs["fused_qkv"] = False
            # grouped-query attention (Hkv < H): the K / V projections produce Hkv heads; the heads axis
            # splits dim 0 of every weight (weight_maps), so its degrees are those that divide Hkv
            ws += [WeightSpec("q_weight", (H, kd, q[-1]), dt, kinit), WeightSpec("k_weight", (Hkv, kd, k[-1]), dt, kinit),
                   WeightSpec("v_weight", (Hkv, vd, v[-1]), dt, kinit)]
            if attrs.get("bias", True):
                ws += [WeightSpec("q_bias", (H, kd), dt, ZeroInitializer()),
                       WeightSpec("k_bias", (Hkv, kd), dt, ZeroInitializer()),
                       WeightSpec("v_bias", (Hkv, vd), dt, ZeroInitializer())]
        ws.append(WeightSpec("o_weight", (E, H, vd), dt, kinit))
        if attrs.get("bias", True):
            ws.append(WeightSpec("o_bias", (E,), dt, ZeroInitializer()))
        return [tuple(q[:-1]) + (E,)], [dt], ws

    # axes: 0 batch, 1 seq, 2 embed, 3 heads
    H_AXIS = 3

    def extra_axis_sizes(self):
        return [self.attrs["num_heads"]]

    def axis_kinds(self):
        return ["sample", "none", "none", "parameter"]

    def supports_axis(self, axis):
        return axis in (0, 3)

    def input_maps(self):
        maps = [(0, 1, None), (0, None, None), (0, None, None)]
        if self._has_key_lens():  # key lengths: sharded with the batch, replicated over the heads axis
            maps.append((0,) + (None,) * (len(self.layer.inputs[3].dims) - 1))
        if self.attrs.get("rope_positions"):  # the key lengths' map
            maps.append((0, None))
        if self.attrs.get("attn_bias"):
            maps.append(attn_bias_map(self.layer.inputs[-1].dims, self.layer.inputs[0].dims[0],
                                      self.attrs["num_heads"], 0, self.H_AXIS))
        return maps

    def _has_key_lens(self):  # or segment ids: the same place and the same sharding
        return len(self.layer.inputs) - (1 if self.attrs.get("attn_bias") else 0) - \
            (1 if self.attrs.get("rope_positions") else 0) > 3

    def setup_device(self, device):
        """Called once by the executor, outside any captured region: uploads the rotary table and builds
        a sliding window's bound arrays."""
        rope = rope_attrs(self.attrs)
        if rope is not None:
            rope_table_of(rope, device)
        setup_window(self.attrs, *self.layer.inputs[0].dims[:2], device)

    def _rope(self, pos, inverse, qb, kb, B, Hl, Hkv, Sq, Sk, kd, qs, ks):
        """One launch that rotates the Q and K head rows in place (inverse: dq / dk back)."""
        rope = rope_attrs(self.attrs)
        K.rope(qb, qs, kb, ks, B, Hl, Hkv, Sq, Sk, kd, rope[0], rope_table_of(rope, qb.device), pos=pos,
               interleaved=rope[2], inverse=inverse)

    def needs_input_grad(self, i):
        return i < 3

    def weight_maps(self):
        out = []
        for w in self.layer.weights:
            n = w.short_name
            if n == "qkv_weight":
                out.append((None, 3, None, None))
            elif n == "qkv_bias":
                out.append((None, 3, None))
            elif n in ("q_weight", "k_weight", "v_weight"):
                out.append((3, None, None))
            elif n in ("q_bias", "k_bias", "v_bias"):
                out.append((3, None))
            elif n == "o_weight":
                out.append((None, 3, None))
            else:  # o_bias
                out.append((None,))
        return out

    def _w(self, ws):
        return {w.short_name: t for w, t in zip(self.layer.weights, ws)}

    def drops_attention(self) -> bool:
        """Whether training forwards of this layer drop attention probabilities (p_eff > 0): the
        executor then keeps a device-side step counter (ctx.rng_step)."""
        return K.attn_dropout_thr(self.attrs.get("dropout", 0.0)) > 0

    def _drop(self, ctx, B, Hl, device):
        return attn_drop_args(self, ctx, B, Hl, self.H_AXIS, self.attrs["num_heads"], device)

    def _keep_ref(self, ctx, drop, B, Hl, Sq, Sk, device):
        return attn_keep_ref(self, ctx, drop, B, Hl, Sq, Sk, device)

    def forward(self, ctx, xs, ws):
        q_in, k_in, v_in = xs[:3]
        W = self._w(ws)
        B, Sq, _ = q_in.shape
        has_bias = bool(self.attrs.get("attn_bias"))
        has_seg = bool(self.attrs.get("segment_ids"))
        has_pos = bool(self.attrs.get("rope_positions"))
        kl = K.attn_key_lens(xs[3], B, q_in.device) if len(xs) - has_bias - has_pos > 3 and not has_seg else None
        rope = rope_attrs(self.attrs)
        pos = xs[len(xs) - has_bias - 1] if has_pos else None
        if pos is not None and (pos.dtype != torch.int32 or pos.device != q_in.device or not pos.is_contiguous()):
            pos = pos.to(device=q_in.device, dtype=torch.int32).contiguous()
        win = window_attrs(self.attrs)
        seg = K.attn_segments(xs[3] if has_seg else None, B, Sq, q_in.device, window=win) if has_seg or win else None
        Sk = k_in.shape[1]
        kd, vd = self.attrs["kdim"], self.attrs["vdim"]
        Hl = W["o_weight"].shape[1]
        E = W["o_weight"].shape[0]
        scale = 1.0 / math.sqrt(kd)
        causal = bool(self.attrs.get("causal", False))
        bo = W.get("o_bias")
        if bo is not None and ctx.degree(self.H_AXIS) > 1 and ctx.coord(self.H_AXIS) != 0:
            bo = None
        fused = self.attrs["fused_qkv"] and (q_in is k_in is v_in or (q_in.data_ptr() == k_in.data_ptr() == v_in.data_ptr()))
        s = ctx.saved if ctx.training else {}
        drop = self._drop(ctx, B, Hl, q_in.device)
        if fused:
            x2 = q_in.reshape(B * Sq, -1)
            wq = W["qkv_weight"].reshape(3 * Hl * kd, -1)
            bq = W["qkv_bias"].reshape(-1) if "qkv_bias" in W else None
            qkv, _ = K.linear_fwd(x2, wq, bq, K.ACT_NONE, False)  # [T, 3, Hl, D]
            st = [Sq * 3 * Hl * kd, kd, 3 * Hl * kd]
            qv, kv, vv = qkv.view(-1), qkv.view(-1)[Hl * kd:], qkv.view(-1)[2 * Hl * kd:]
            qs = ks = vs = st
            Hkv = Hl
            s.update(x2=x2, wqkv=wq, qkv=qkv)
            if ctx.training and ctx.extra.get("need_dx0", True):  # TN dgrad (kernels.weight_t)
                s["wqkv_t"] = K.weight_t(ctx.extra.setdefault("wt_store_qkv", {}), wq)
        else:
            outs = []
            Hkv = W["k_weight"].shape[0]  # this part's KV heads: Hl, or fewer with num_kv_heads
            for name, t, d, H_ in (("q", q_in, kd, Hl), ("k", k_in, kd, Hkv), ("v", v_in, vd, Hkv)):
                x2 = t.reshape(-1, t.shape[-1])
                w2 = W[f"{name}_weight"].reshape(H_ * d, -1)
                b2 = W[f"{name}_bias"].reshape(-1) if f"{name}_bias" in W else None
                y, _ = K.linear_fwd(x2, w2, b2, K.ACT_NONE, False)
                outs.append(y)
                s[f"x_{name}"], s[f"w_{name}"] = x2, w2
            qv, kv, vv = outs
            qs = [Sq * Hl * kd, kd, Hl * kd]
            ks = [Sk * Hkv * kd, kd, Hkv * kd]
            vs = [Sk * Hkv * vd, vd, Hkv * vd]
            s.update(q=qv, k=kv, v=vv)
        if rope is not None:  # q and k are rotated where they lie; what is saved above is the rotated heads
            self._rope(pos, False, qv, kv, B, Hl, Hkv, Sq, Sk, kd, qs, ks)
        o = torch.empty(B, Sq, Hl, vd, device=q_in.device, dtype=q_in.dtype)
        os_ = [Sq * Hl * vd, vd, Hl * vd]
        bias = K.attn_score_bias(xs[-1], B, Hl, Sq, Sk, q_in.device) if has_bias else None
        attn_core_fwd(s, self.layer.name, qv, qs, kv, ks, vv, vs, o, os_, B, Hl, Sq, Sk, kd, vd, scale, causal, kl, drop,
                      bias, lambda: self._keep_ref(ctx, drop, B, Hl, Sq, Sk, q_in.device), seg=seg, Hkv=Hkv)
        o2 = o.view(B * Sq, Hl * vd)
        wo = W["o_weight"].reshape(E, Hl * vd)
        if ctx.training:
            s["wo_t"] = K.weight_t(ctx.extra.setdefault("wt_store_o", {}), wo)
        y, _ = K.linear_fwd(o2, wo, bo, K.ACT_NONE, False)
        if ctx.training:
            s.update(o=o, wo=wo, has_bo=bo is not None, shape=(B, Sq, Sk, Hl, kd, vd, E), fused=fused,
                     qs=qs, ks=ks, vs=vs, os=os_, scale=scale, causal=causal, key_lens=kl, drop=drop, sbias=bias,
                     seg=seg, Hkv=Hkv, rope_pos=pos)
        return [y.view(B, Sq, E)]

    def overwrites_wgrad(self, i):
        return not self.layer.weights[i].short_name.endswith("bias")  # projection GEMMs use dw_beta = wb

    def _grad_index(self):
        return {w.short_name: i for i, w in enumerate(self.layer.weights)}

    def backward(self, ctx, douts):
        s = ctx.saved
        B, Sq, Sk, Hl, kd, vd, E = s["shape"]
        gi = self._grad_index()
        gw = lambda n: (ctx.wgrads[gi[n]] if (ctx.wgrads and n in gi) else None)  # noqa: E731
        dy2 = douts[0].reshape(B * Sq, E).contiguous()
        o = s["o"]
        o2 = o.view(B * Sq, Hl * vd)
        dwo = gw("o_weight")
        dbo = gw("o_bias") if (s["has_bo"] and not ctx.extra.get("bias_grad_fused")) else None
        wb = 0.0 if ctx.extra.get("wgrad_overwrite") else 1.0
        do2 = K.linear_bwd(dy2, o2, s["wo"], None, K.ACT_NONE,
                           dwo.view(E, Hl * vd) if dwo is not None else None, dbo, dw_beta=wb, wt=s.get("wo_t"))
        do = do2.view(B, Sq, Hl, vd)
        scale, causal = s["scale"], s["causal"]
        qs, ks, vs, os_ = s["qs"], s["ks"], s["vs"], s["os"]
        fused = s["fused"]
        kl = s["key_lens"]
        drop = s["drop"]  # the counter is read on the device again: the next forward advances it, not this backward
        no_kl_grad = [None] * (len(self.layer.inputs) - 3)  # the lengths and the score bias take no gradient
        if fused:
            qkv = s["qkv"]
            qv, kv, vv = qkv.view(-1), qkv.view(-1)[Hl * kd:], qkv.view(-1)[2 * Hl * kd:]
            dqkv = torch.empty_like(qkv)
            dq, dk, dv = dqkv.view(-1), dqkv.view(-1)[Hl * kd:], dqkv.view(-1)[2 * Hl * kd:]
        else:
            qv, kv, vv = s["q"], s["k"], s["v"]
            dq, dk, dv = torch.empty_like(qv), torch.empty_like(kv), torch.empty_like(vv)
        # fused projection: the flash kernel can add the QKV bias gradient (column sums of dq / dk / dv)
        # itself, sparing linear_bwd a pass over dqkv (bias_act_bwd + fold); never with a score bias
        # nor with rotary: the kernel would sum dq / dk columns before they are rotated back
        rope = rope_attrs(self.attrs)
        dbq = gw("qkv_bias") if (fused and rope is None and os.environ.get("FF_ATTN_BIAS_FUSION", "1") == "1") else None
        if dbq is not None and not (dbq.dtype == torch.float32 and dbq.is_contiguous()):
            dbq = None
        bias_done = attn_core_bwd(s, qv, qs, kv, ks, vv, vs, o, os_, do, os_, dq, dk, dv, B, Hl, Sq, Sk, kd, vd, scale,
                                  causal, kl, drop, s.get("sbias"), dbq.view(-1) if dbq is not None else None,
                                  seg=s.get("seg"), Hkv=s.get("Hkv"))
        if rope is not None:  # the rotation's backward: dq / dk rotated by the negated angle, in place
            self._rope(s.get("rope_pos"), True, dq, dk, B, Hl, s.get("Hkv") or Hl, Sq, Sk, kd, qs, ks)
        if fused:
            dw = gw("qkv_weight")
            db = None if bias_done else gw("qkv_bias")
            acc = (ctx.extra.get("dx_accum") or {}).get(0)
            dx2 = K.linear_bwd(dqkv, s["x2"], s["wqkv"], None, K.ACT_NONE,
                               dw.view(3 * Hl * kd, -1) if dw is not None else None,
                               db.view(-1) if db is not None else None, dw_beta=wb,
                               dx_out=acc.view(B * Sq, -1) if acc is not None else None, wt=s.get("wqkv_t"))
            dx = acc if acc is not None else dx2.view(B, Sq, -1)
            ctx.saved.clear()
            return [dx, None, None] + no_kl_grad  # all three inputs are the same tensor: gradient once
        grads = []
        accs = ctx.extra.get("dx_accum") or {}
        Hkv = s.get("Hkv") or Hl
        for slot, (name, g, d, S_, H_) in enumerate((("q", dq, kd, Sq, Hl), ("k", dk, kd, Sk, Hkv), ("v", dv, vd, Sk, Hkv))):
            acc = accs.get(slot)
            dw = gw(f"{name}_weight")
            db = gw(f"{name}_bias")
            x2 = s[f"x_{name}"]
            dx2 = K.linear_bwd(g.view(B * S_, H_ * d), x2, s[f"w_{name}"], None, K.ACT_NONE,
                               dw.view(H_ * d, -1) if dw is not None else None,
                               db.view(-1) if db is not None else None, dw_beta=wb,
                               dx_out=acc.view(B * S_, -1) if acc is not None else None)
            grads.append(acc if acc is not None else dx2.view(B, S_, -1))
        ctx.saved.clear()
        return grads + no_kl_grad

    def accumulates_dx(self):
        return True

    def accum_may_alias_douts(self):
        return True  # dy is consumed by the output projection before the QKV dgrad writes

    def flops(self, in_shapes, out_shapes, w_shapes):
        B, Sq, Eq = in_shapes[0]
        Sk = in_shapes[1][1]
        kd, vd = self.attrs["kdim"], self.attrs["vdim"]
        Hl = w_shapes[-2][1] if len(w_shapes[-1]) == 1 else w_shapes[-1][1]
        E = self.attrs["embed_dim"]
        H = self.attrs["num_heads"]
        Hkv = Hl * (self.attrs.get("num_kv_heads") or H) // H  # this part's KV heads: the smaller K / V projections
        proj = 2.0 * B * (Sq * Hl * kd * Eq + Sk * Hkv * kd * Eq + Sk * Hkv * vd * Eq + Sq * Hl * vd * E)
        att = 2.0 * B * Hl * Sq * Sk * (kd + vd)
        win = window_attrs(self.attrs)
        if win is not None:  # the band's pairs only (the flash kernels skip the tiles outside it)
            att = 2.0 * B * Hl * window_pairs(Sq, win, bool(self.attrs.get("causal"))) * (kd + vd)
        return proj + att

    def uses_mfma(self):
        return True
