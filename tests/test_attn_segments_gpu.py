"""Packed sequences (AttnArgs.seg_lo / seg_hi) in the flash-attention kernels, the bounds kernel, the
attention ops and a captured bert-tiny training step, on the GPU.

The layout follows tests/test_attn_key_lengths_gpu.py: inputs are seeded on the CPU, every output
buffer starts as NaN (an element a kernel leaves unwritten fails the comparison), a guard band sits
behind the backward workspace, and the tolerances are that file's (relative Frobenius error against
fp32 torch with the block-diagonal mask: o < 2e-2, lse < 1e-3, gradients < 3e-2), every element
compared. A padding position has a NaN torch reference, so the reference holds what the semantics
promise there: exact zeros, lse = +inf.

A case's rows are lists of run lengths; ("p", n) is a padding run. Neighbouring segments get
different ids, ids are reused further along the row, and padding runs use -1 and -2. The reference
mask comes from the run lists themselves (tests/attn_segments_common.py), not from the bounds code.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from attn_segments_common import bounds_loop, ids_of, live_of, mask_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
TOL_O, TOL_LSE, TOL_G = 2e-2, 1e-3, 3e-2


def p(n):
    return ("p", n)


S1 = [[70, 58, 40, p(24)], [192]]  # cuts inside a 32-block, across a 64-key tile and the 128-row workgroup
S2 = [[100, 156, 64], [p(10), 120, p(30), 160]]  # a cut on the 256-key block edge, a segment wholly in block 1
# s5: the four D = 64 layouts above at S = 320 (those of s1 with their tail as padding) and an all-padding row
S5 = [[70, 58, 40, p(152)], [192, p(128)], S2[0], S2[1], [p(320)]]
# name: H, S, D, causal, rows
CASES = {
    "s1": (2, 192, 64, False, S1),
    "s2": (2, 320, 64, True, S2),
    "s3": (2, 256, 128, False, [[129, 127], [1, 1, 254]]),
    "s4": (2, 576, 64, False, [[p(576)], [300, 276]]),  # Sq >= 512: the generic forward; three key blocks
    "s5": (16, 320, 64, False, [S5[i % 5] for i in range(16)]),  # B*H = 256: the chained backward, two key blocks
}


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ref_attn(q, k, v, see, scale, keep=None, keep_scale=1.0):
    """fp32 torch attention of [B, H, S, D] tensors under the bool mask see [B, S, S]: (o, lse); a row
    without keys has o = 0 and lse = +inf (differentiable in q, k, v)."""
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    m = see[:, None]
    dead = ~m.any(-1, keepdim=True)
    s = torch.where(dead, torch.zeros_like(s), s.masked_fill(~m, -INF))
    pr = torch.where(dead, torch.zeros_like(s), torch.softmax(s, -1))
    lse = torch.where(dead[..., 0], torch.full_like(s[..., 0], INF), torch.logsumexp(s, -1)).detach()
    if keep is not None:
        pr = torch.where(keep, pr * keep_scale, torch.zeros_like(pr))
    return torch.einsum("bhqk,bhkd->bhqd", pr, v), lse


_cache = {}


def _case(name):
    """Inputs (bf16, on the device), segment ids, bounds and the fp32 reference of a case, computed once."""
    if name not in _cache:
        H, S, D, causal, rows = CASES[name]
        B = len(rows)
        g = torch.Generator().manual_seed(2000 + int(name[1:]))
        q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(4))
        ids = torch.tensor(np.stack([ids_of(r, S) for r in rows]), dtype=torch.int32, device=DEV)
        see = torch.tensor(np.stack([mask_of(r, S, causal) for r in rows]), device=DEV)
        live = torch.tensor(np.stack([live_of(r, S) for r in rows]), device=DEV)
        scale = 1.0 / math.sqrt(D)
        qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
        o, lse = _ref_attn(qf, kf, vf, see, scale)
        o.backward(do.float())
        ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
        _cache[name] = (q, k, v, do, ids, live, scale, ref)
    return _cache[name]


def _bounds(ffC, ids):
    lo, hi = torch.full_like(ids, -7), torch.full_like(ids, -7)
    ffC.attn_seg_bounds(ids, lo, hi)
    return lo, hi


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _fwd(ffC, q, k, v, seg, scale, causal, variant=None, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    o, lse = _nan_like(q), torch.full((B * H * Sq,), float("nan"), device=DEV)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    prev = ffC.attn_fwd_variant()
    if variant is not None:
        ffC.attn_set_fwd_variant(variant)
    try:
        if seg is not None:
            kw = dict(kw, seg_lo=seg[0], seg_hi=seg[1])
        ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, causal, **kw)
    finally:
        ffC.attn_set_fwd_variant(prev)
    return o, lse


def _bwd(ffC, q, k, v, o, lse, do, seg, scale, causal, variant, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    dq, dk, dv = _nan_like(q), _nan_like(k), _nan_like(v)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    n = ffC.attn_bwd_ws(B, H, Sq, Sk, D)
    ws = torch.full((n + 4096,), 7.0, device=DEV)  # a guard band after the workspace
    prev = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    try:
        if seg is not None:
            kw = dict(kw, seg_lo=seg[0], seg_hi=seg[1])
        done = ffC.attn_bwd(q, sq, k, sk, v, sk, o, sq, do, sq, lse, dq, sq, dk, sk, dv, sk, ws[:n], B, H, Sq, Sk, D,
                            scale, causal, **kw)
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    assert seg is None or not done  # the segment kernels leave the fused bias gradient to the caller
    return dq, dk, dv


def _check_against_ref(name, got, ref, live):
    """got / ref: dicts of o, lse [B, H, S], dq, dk, dv in [B, H, S, D]; live: bool [B, S]. Tolerances,
    then finiteness and the exact zeros / lse = +inf of the padding positions."""
    H = got["o"].shape[1]
    lv = live[:, None, :].expand(-1, H, -1)
    errs = {key: _rel(got[key], ref[key]) for key in ("o", "dq", "dk", "dv")}
    errs["lse"] = _rel(got["lse"][lv], ref["lse"][lv])
    print(name, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs["o"] < TOL_O and errs["lse"] < TOL_LSE, errs
    assert errs["dq"] < TOL_G and errs["dk"] < TOL_G and errs["dv"] < TOL_G, errs
    for key in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[key]).all(), key
        assert (got[key][~lv] == 0).all(), key
    assert torch.isfinite(got["lse"][lv]).all()
    assert (got["lse"][~lv] == INF).all()


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_segments_vs_fp32(ffC, name, variant):
    """Forward structures 0, 1, 3 (bitwise equal to each other) and backward structures 2 and 10 against
    the fp32 reference with the block-diagonal mask, plus the exact zeros of the padding positions."""
    H, S, D, causal, rows = CASES[name]
    q, k, v, do, ids, live, scale, ref = _case(name)
    seg = _bounds(ffC, ids)
    o, lse = _fwd(ffC, q, k, v, seg, scale, causal)
    for fv in (0, 1, 3):
        o2, lse2 = _fwd(ffC, q, k, v, seg, scale, causal, fv)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, seg, scale, causal, variant)
    got = dict(o=o, lse=lse.view(len(rows), H, S), dq=dq, dk=dk, dv=dv)
    _check_against_ref(f"case {name} bwd {variant}", got, ref, live)


@pytest.mark.parametrize("name,variant", [("s2", 10), ("s2", 2), ("s5", 10), ("s5", 2)])
def test_segments_are_isolated(ffC, name, variant):
    """q / k / v / dO of one segment per row (the second run that is one) and of every padding run
    overwritten with 1e3 * randn: every output of the other segments is bitwise equal. The first run
    repeated is bitwise equal everywhere (no atomics anywhere)."""
    H, S, D, causal, rows = CASES[name]
    B = len(rows)
    q, k, v, do, ids, live, scale, _ = _case(name)
    seg = _bounds(ffC, ids)
    hit = np.zeros((B, S), dtype=bool)
    for b, row in enumerate(rows):
        at, nseg = 0, 0
        for r in row:
            n = r[1] if isinstance(r, tuple) else r
            if isinstance(r, tuple):
                hit[b, at:at + n] = True
            else:
                nseg += 1
                if nseg == 2:
                    hit[b, at:at + n] = True
            at += n
    hit_t = torch.tensor(hit, device=DEV)[:, None, :, None]
    g = torch.Generator().manual_seed(78)
    noise = [(1e3 * torch.randn(B, H, S, D, generator=g)).bfloat16().to(DEV) for _ in range(4)]
    runs = []
    for fill in (0, 0, 1):
        q2, k2, v2, do2 = (torch.where(hit_t, nz, t) if fill else t for t, nz in zip((q, k, v, do), noise))
        o, lse = _fwd(ffC, q2, k2, v2, seg, scale, causal)
        dq, dk, dv = _bwd(ffC, q2, k2, v2, o, lse, do2, seg, scale, causal, variant)
        runs.append(dict(o=o, lse=lse.view(B, H, S), dq=dq, dk=dk, dv=dv))
    first, again, noisy = runs
    for key in first:
        assert torch.equal(first[key], again[key]), key
    keep = ~torch.tensor(hit, device=DEV)[:, None, :].expand(-1, H, -1)
    assert keep.any()
    for key in first:
        assert torch.equal(first[key][keep], noisy[key][keep]), key


@pytest.mark.parametrize("S,causal", [(512, False), (384, True)])
@pytest.mark.parametrize("variant", [2, 10])
def test_one_full_segment_changes_nothing(ffC, S, causal, variant):
    """One segment over the whole row: o and lse bitwise equal to the call without segments in every
    forward structure, gradients within tolerance."""
    B, H, D = 2, 3, 64
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(4))
    ids = torch.full((B, S), 3, dtype=torch.int32, device=DEV)
    seg = _bounds(ffC, ids)
    scale = 1.0 / math.sqrt(D)
    for fv in (0, 1, 3):
        o0, lse0 = _fwd(ffC, q, k, v, None, scale, causal, fv)
        o1, lse1 = _fwd(ffC, q, k, v, seg, scale, causal, fv)
        assert torch.equal(o0, o1) and torch.equal(lse0, lse1), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o1, lse1, do, seg, scale, causal, variant)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    see = torch.tensor(np.stack([mask_of([S], S, causal)] * B), device=DEV)
    o, lse = _ref_attn(qf, kf, vf, see, scale)
    o.backward(do.float())
    ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    _check_against_ref(f"one segment S{S} bwd {variant}", dict(o=o1, lse=lse1.view(B, H, S), dq=dq, dk=dk, dv=dv),
                       ref, torch.ones(B, S, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("variant", [2, 10])
def test_segments_with_dropout(ffC, variant):
    """s1 with p = 0.25 against the fp32 reference under the mask attn_dropout_mask draws: q, k are
    the positions in the packed row."""
    from flexflow_amd import kernels as K
    H, S, D, causal, rows = CASES["s1"]
    B = len(rows)
    q, k, v, do, ids, live, scale, _ = _case("s1")
    seg = _bounds(ffC, ids)
    thr = K.attn_dropout_thr(0.25)
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    seed = K.attn_dropout_seed(11, 5)
    kw = K._drop_kw((thr, step, seed, 0, 0, H))
    keep = K.attn_dropout_mask(B, H, S, S, thr, step, seed, device=DEV)
    o, lse = _fwd(ffC, q, k, v, seg, scale, causal, **kw)
    for fv in (0, 1):
        o2, lse2 = _fwd(ffC, q, k, v, seg, scale, causal, fv, **kw)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, seg, scale, causal, variant, **kw)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    see = torch.tensor(np.stack([mask_of(r, S, causal) for r in rows]), device=DEV)
    orf, lrf = _ref_attn(qf, kf, vf, see, scale, keep, 256.0 / (256 - thr))
    orf.backward(do.float())
    ref = dict(o=orf.detach(), lse=lrf, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    _check_against_ref(f"s1 dropout bwd {variant}", dict(o=o, lse=lse.view(B, H, S), dq=dq, dk=dk, dv=dv), ref, live)


@pytest.mark.parametrize("S", [1, 77, 320, 4099])
def test_attn_seg_bounds_kernel(ffC, S):
    """attn_seg_bounds against the plain loop: all-equal ids, alternating ids, negatives in runs and
    alone, a reused id, random short runs; lo / hi start as -7, so every element must be written."""
    rng = np.random.default_rng(S)
    i = np.arange(S)
    rows = [np.full(S, 4), i % 2, -1 - (i % 2), np.where((i // 5) % 3 == 1, -1, (i // 5) % 2),
            np.where(i < S // 2, 7, np.where(i < S // 2 + 3, -3, 7)), rng.integers(-1, 2, S), np.full(S, -1)]
    ids = np.stack(rows).astype(np.int32)
    lo, hi = _bounds(ffC, torch.tensor(ids, device=DEV))
    want_lo, want_hi = bounds_loop(ids)
    assert np.array_equal(lo.cpu().numpy(), want_lo)
    assert np.array_equal(hi.cpu().numpy(), want_hi)


def test_segment_arguments_are_checked(ffC):
    H, S, D, causal, rows = CASES["s1"]
    q, k, v, do, ids, live, scale, _ = _case("s1")
    lo, hi = _bounds(ffC, ids)
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, (lo.long(), hi.long()), scale, False)  # not int32
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, (lo[:1], hi[:1]), scale, False)  # numel != B * Sq
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k[:, :, :128].contiguous(), v[:, :, :128].contiguous(), (lo, hi), scale, False)  # Sq != Sk
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, (lo, hi), scale, False, sbias=torch.zeros(1, 1, S, S, device=DEV))
    o, lse = _fwd(ffC, q, k, v, (lo, hi), scale, False)
    with pytest.raises(RuntimeError):
        _bwd(ffC, q, k, v, o, lse, do, (lo, hi), scale, False, 2, sbias=torch.zeros(1, 1, S, S, device=DEV))
    with pytest.raises(RuntimeError):
        _bwd(ffC, q, k, v, o, lse, do, (lo.long(), hi.long()), scale, False, 2)


# ------------------------------------------------------------------------------------- op level
OP_ROWS = [[50, 46, p(32)], [128], [p(5), 33, 90], [1, 64, p(62), 1]]


def _run_mha(dtype, E, H, S, rows, causal=False):
    """MultiHeadAttention with a segment_ids input through OpCtx on the device, and fp32 torch on the
    same weights: relative errors of the output, the input gradient and every weight / bias gradient."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B = len(rows)
    g = torch.Generator().manual_seed(9)
    ff = FFModel(FFConfig([]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    ts = ff.create_tensor([B, S], DataType.DT_INT32)
    L = ff.multihead_attention(tx, tx, tx, E, H, causal=causal, segment_ids=ts).owner_layer
    assert L.attrs["fused_qkv"] and L.attrs["segment_ids"]
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    x = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    ws = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).to(DEV, dtype) for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims, device=DEV) for w in L.weights]
    ids = torch.tensor(np.stack([ids_of(r, S) for r in rows]), dtype=torch.int32, device=DEV)
    y = L.impl.forward(ctx, [x, x, x, ids], ws)[0]
    dy = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == 4 and dxs[1] is None and dxs[2] is None and dxs[3] is None
    torch.cuda.synchronize()
    xf = x.float().requires_grad_()
    wf = [w.float().requires_grad_() for w in ws]
    D = E // H
    W, bb = wf[0].reshape(3, H * D, E), wf[1].reshape(3, H * D)
    qq, kk, vv = ((xf @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    see = torch.tensor(np.stack([mask_of(r, S, causal) for r in rows]), device=DEV)
    o, _ = _ref_attn(qq, kk, vv, see, 1.0 / math.sqrt(D))
    yr = o.transpose(1, 2).reshape(B, S, H * D) @ wf[2].reshape(E, -1).t() + wf[3]
    yr.backward(dy.float())
    errs = {"y": _rel(y, yr), "dx": _rel(dxs[0], xf.grad)}
    for w, gw, r in zip(L.weights, ctx.wgrads, wf):
        errs["d" + w.short_name] = _rel(gw, r.grad)
    for t in [y, dxs[0]] + ctx.wgrads:
        assert torch.isfinite(t).all()
    print(dtype, E // H, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    return y, yr, errs, ws


@pytest.mark.parametrize("H", [2, 4])
def test_mha_op_bf16_segments(ffC, H):
    """bf16 fused self-attention, E = 128, S = 128, B = 4: head dim 64 (the flash kernels on the fused
    QKV buffer) and head dim 32 (zero-padded to 64)."""
    _, _, errs, _ = _run_mha(torch.bfloat16, 128, H, 128, OP_ROWS)
    assert errs.pop("y") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


def test_mha_op_fp32_device_segments(ffC):
    """--dtype fp32 on the device (f32 MFMA GEMMs + segment mask + row softmax) with an all-padding row,
    at the bound of test_mha_op_fp32_device_key_lengths. The padding row's output rows are the output bias."""
    y, yr, errs, ws = _run_mha(torch.float32, 128, 2, 128, OP_ROWS[:1] + [[p(128)]] + OP_ROWS[2:])
    assert all(e < 1e-4 for e in errs.values()), errs
    assert torch.equal(y[1], ws[3].expand(128, 128))


def test_sdpa_op_bf16_segments(ffC):
    """ScaledDotProductAttention with segment_ids, bf16, [4, 2, 128, 64], causal."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B, H, S, D = 4, 2, 128, 64
    g = torch.Generator().manual_seed(10)
    ff = FFModel(FFConfig([]))
    tq, tk, tv = (ff.create_tensor([B, H, S, D], DataType.DT_FLOAT) for _ in range(3))
    ts = ff.create_tensor([B, S], DataType.DT_INT32)
    L = ff.scaled_dot_product_attention(tq, tk, tv, causal=True, segment_ids=ts).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(4))
    ids = torch.tensor(np.stack([ids_of(r, S) for r in OP_ROWS]), dtype=torch.int32, device=DEV)
    o = L.impl.forward(ctx, [q, k, v, ids], [])[0]
    dxs = L.impl.backward(ctx, [do])
    assert len(dxs) == 4 and dxs[3] is None
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    see = torch.tensor(np.stack([mask_of(r, S, True) for r in OP_ROWS]), device=DEV)
    orf, _ = _ref_attn(qf, kf, vf, see, 1.0 / math.sqrt(D))
    orf.backward(do.float())
    errs = dict(o=_rel(o, orf), dq=_rel(dxs[0], qf.grad), dk=_rel(dxs[1], kf.grad), dv=_rel(dxs[2], vf.grad))
    print("sdpa segments relative errors", errs)
    assert errs.pop("o") < TOL_O and all(e < TOL_G for e in errs.values()), errs


# --------------------------------------------------------------------------------- step capture
def _train_bert(flags, with_seg, steps=6):
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(0)
    B, bc = 4, BertConfig.tiny(64)
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    sg = ff.create_tensor([B, bc.seq], DataType.DT_INT32, name="segment_ids") if with_seg else None
    ids, pos, _ = build_bert(ff, B, bc, segment_ids=sg)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    tok = rng.integers(1, bc.vocab, (N, bc.seq)).astype(np.int32)
    cut = rng.integers(1, bc.seq - 8, N)  # two segments and a tail of up to 8 pads per row
    tail = rng.integers(0, 9, N)
    j = np.arange(bc.seq)[None, :]
    seg = np.where(j < cut[:, None], 0, np.where(j < (bc.seq - tail)[:, None], 1, -1)).astype(np.int32)
    loaders = [ff.create_data_loader(ids, tok),
               ff.create_data_loader(pos, np.tile(np.arange(bc.seq, dtype=np.int32), (N, 1))),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, bc.vocab, (N, bc.seq, 1)).astype(np.int32))]
    if with_seg:
        loaders.append(ff.create_data_loader(sg, seg))
    losses = []
    for _ in range(steps):
        for dl in loaders:
            dl.next_batch(ff)
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    torch.cuda.synchronize()
    weights = [np.asarray(w.get_weights(ff)) for L in ff.layers for w in L.weights]
    return ff, np.asarray(losses, dtype=np.float64), weights


def test_bert_segments_train_under_step_capture():
    """bert-tiny (BertConfig.tiny(64), batch 4) with segment ids fed by a data loader, hipGraph step
    capture on and off, with the assertions of test_bert_key_lengths_train_under_step_capture: the
    graph exists, losses and weights agree (rtol 1e-5, atol 1e-6), and the replayed steps differ from a
    run without segments, so the input reaches the kernels inside the graph."""
    ffg, lg, wg = _train_bert(["--hip-graphs"], True)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    _, le, we = _train_bert(["--no-hip-graphs"], True)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
    ffd, ld, _ = _train_bert(["--hip-graphs"], False)
    assert ffd._step_graph.graph is not None
    print("losses without segments", ld)
    assert np.abs(ld[3:] - lg[3:]).max() > 1e-6, (ld, lg)  # the replayed steps see the segments
