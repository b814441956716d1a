"""Attention dropout on the GPU: the mask the flash kernels really draw (recovered exactly through
probe inputs), their numerics against fp32 torch using the mirror's mask
(kernels.attn_dropout_keep_ref), the fp32 device path, a zero-padded head dim and a captured bert-tiny
training step.

Tolerances are those of tests/test_kernels_gpu.py::test_flash_attention (relative Frobenius error:
o < 2e-2, lse < 1e-3, gradients < 3e-2). Inputs are seeded on the CPU; every output buffer starts as
NaN, so an element a kernel leaves unwritten fails the comparison."""
import math
import zlib

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
TOL_O, TOL_LSE, TOL_G = 2e-2, 1e-3, 3e-2
SEED, LAYER, P, THR = 1234, 77, 0.1, 26
RNG = K.attn_dropout_seed(SEED, LAYER)
KEEP_SCALE = 256.0 / (256 - THR)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _step(n):
    return torch.tensor([n], dtype=torch.int64, device=DEV)


def _kw(step, b0=0, h0=0, H_total=0, thr=THR):
    return K._drop_kw((thr, step, RNG, b0, h0, H_total)) if thr else {}


def _mirror(step, B, H, Sq, Sk, **kw):
    return K.attn_dropout_keep_ref(SEED, LAYER, step, B, H, Sq, Sk, P, device=DEV, **kw)


def _fwd(ffC, q, k, v, scale, causal, kl=None, variant=None, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    o, lse = _nan_like(q), torch.full((B * H * Sq,), float("nan"), device=DEV)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    prev = ffC.attn_fwd_variant()
    if variant is not None:
        ffC.attn_set_fwd_variant(variant)
    try:
        ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, causal, kl, **kw)
    finally:
        ffC.attn_set_fwd_variant(prev)
    return o, lse


def _bwd(ffC, q, k, v, o, lse, do, scale, causal, variant, kl=None, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    dq, dk, dv = _nan_like(q), _nan_like(k), _nan_like(v)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    n = ffC.attn_bwd_ws(B, H, Sq, Sk, D)
    ws = torch.full((n + 4096,), 7.0, device=DEV)  # a guard band after the workspace
    prev = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    try:
        ffC.attn_bwd(q, sq, k, sk, v, sk, o, sq, do, sq, lse, dq, sq, dk, sk, dv, sk, ws[:n], B, H, Sq, Sk, D, scale,
                     causal, None, kl, **kw)
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    return dq, dk, dv


# ------------------------------------------------------------------------- the device function
def test_device_mask_function_equals_the_mirror(ffC):
    """attn_dropout_keep (attn_dropout.h) evaluated per element by attn_dropout_mask_kernel: odd
    extents, a shard offset, steps 0 and 2^40 + 3."""
    for step in (0, (1 << 40) + 3):
        got = K.attn_dropout_mask(3, 2, 37, 50, THR, _step(step), RNG, b0=2, h0=3, H_total=5)
        assert torch.equal(got, _mirror(step, 3, 2, 37, 50, b0=2, h0=3, H_total=5)), step
    got = K.attn_dropout_mask(1, 1, 8, 8, 128, None, RNG, device=DEV)  # no counter: step 0
    assert torch.equal(got, K.attn_dropout_keep_ref(SEED, LAYER, 0, 1, 1, 8, 8, 0.5, device=DEV))


# --------------------------------------------------------------------------- exact mask probes
def _probe_fwd(ffC, B, H, Sq, Sk, D, step, variant=None, **kw):
    """With Q = 0 every P is exactly 1 / Sk; with V the identity over the 64-key window w,
    o[q][d] != 0 iff (q, 64 w + d) was kept. Sweeps the windows: bool [B, H, Sq, Sk]."""
    q = torch.zeros(B, H, Sq, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, H, Sk, D, generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV)
    kept = torch.zeros(B, H, Sq, Sk, dtype=torch.bool, device=DEV)
    d = torch.arange(64, device=DEV)
    for w in range(Sk // 64):
        v = torch.zeros(B, H, Sk, D, device=DEV, dtype=torch.bfloat16)
        v[:, :, 64 * w + d, d] = 1
        o, _ = _fwd(ffC, q, k, v, 1.0, False, None, variant, **kw)
        assert torch.isfinite(o).all()
        kept[..., 64 * w:64 * w + 64] = o[..., :64] != 0
        assert (o[..., 64:] == 0).all()
    return kept


def _probe_bwd(ffC, B, H, Sq, Sk, D, step, variant, **kw):
    """With dO the identity over the 64-query window w, dv[k][d] != 0 iff (64 w + d, k) was kept."""
    g = torch.Generator().manual_seed(2)
    q = torch.zeros(B, H, Sq, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
    v = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
    o, lse = _fwd(ffC, q, k, v, 1.0, False, None, None, **kw)
    kept = torch.zeros(B, H, Sq, Sk, dtype=torch.bool, device=DEV)
    d = torch.arange(64, device=DEV)
    for w in range(Sq // 64):
        do = torch.zeros(B, H, Sq, D, device=DEV, dtype=torch.bfloat16)
        do[:, :, 64 * w + d, d] = 1
        dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, 1.0, False, variant, None, **kw)
        assert torch.isfinite(dv).all() and torch.isfinite(dq).all() and torch.isfinite(dk).all()
        kept[:, :, 64 * w:64 * w + 64, :] = (dv[..., :64] != 0).transpose(-1, -2)
        assert (dv[..., 64:] == 0).all()
    return kept


PROBES = {"d64_s128": (2, 2, 128, 128, 64), "d64_s512": (1, 2, 512, 512, 64), "d128_s256": (2, 2, 256, 256, 128)}


@pytest.mark.parametrize("name", list(PROBES))
def test_forward_mask_is_the_mirrors(ffC, name):
    B, H, Sq, Sk, D = PROBES[name]
    want = _mirror(7, B, H, Sq, Sk)
    for fv in (0, 1, 3):
        got = _probe_fwd(ffC, B, H, Sq, Sk, D, 7, fv, **_kw(_step(7)))
        assert torch.equal(got, want), (fv, (got != want).sum().item())


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(PROBES))
def test_backward_mask_is_the_mirrors(ffC, name, variant):
    B, H, Sq, Sk, D = PROBES[name]
    want = _mirror(7, B, H, Sq, Sk)
    got = _probe_bwd(ffC, B, H, Sq, Sk, D, 7, variant, **_kw(_step(7)))
    assert torch.equal(got, want), (got != want).sum().item()


def test_chained_backward_mask_is_the_mirrors(ffC):
    """B * H = 256 workgroups: one launch per key block with the dQ sum carried between them."""
    B, H, S, D = 16, 16, 128, 64
    want = _mirror(3, B, H, S, 512)
    for variant in (2, 10):
        got = _probe_bwd(ffC, B, H, S, 512, D, 3, variant, **_kw(_step(3)))
        assert torch.equal(got, want), (variant, (got != want).sum().item())


def test_shard_offsets_select_the_slice_of_the_full_mask(ffC):
    """One (batch, head) shard run with b0 = 1, h0 = 1 of a B = 2, H = 2 problem: its masks, forward
    and backward, are the [1, 1] slice of the full run's."""
    full_f = _probe_fwd(ffC, 2, 2, 128, 128, 64, 9, None, **_kw(_step(9)))
    full_b = _probe_bwd(ffC, 2, 2, 128, 128, 64, 9, 10, **_kw(_step(9)))
    kw = _kw(_step(9), b0=1, h0=1, H_total=2)
    assert torch.equal(_probe_fwd(ffC, 1, 1, 128, 128, 64, 9, None, **kw), full_f[1:, 1:])
    assert torch.equal(_probe_bwd(ffC, 1, 1, 128, 128, 64, 9, 10, **kw), full_b[1:, 1:])
    assert not torch.equal(full_f[1:, 1:], full_f[:1, :1])


# ----------------------------------------------------------------- numerics against the reference
def _ref_attn(q, k, v, keep, lens, scale, causal):
    """fp32 torch attention of [B, H, S, D] tensors with the keep-mask applied to P (kept elements
    scaled by 1 / (1 - p_eff)); lens: per-sample key lengths or None (a sample without keys: o = 0,
    lse = +inf). Returns (o, lse of the undropped softmax)."""
    Sq, Sk = q.shape[2], k.shape[2]
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), -INF)
    empty = torch.zeros(q.shape[0], dtype=torch.bool, device=q.device)
    if lens is not None:
        L = lens.long().clamp(0, Sk)
        s = s.masked_fill((torch.arange(Sk, device=q.device)[None, :] >= L[:, None])[:, None, None, :], -INF)
        empty = L == 0
    e4 = empty[:, None, None, None]
    s = torch.where(e4, torch.zeros_like(s), s)
    p = torch.where(e4, torch.zeros_like(s), torch.softmax(s, -1))
    lse = torch.where(empty[:, None, None], torch.full_like(s[..., 0], INF), torch.logsumexp(s, -1)).detach()
    if keep is not None:
        p = torch.where(keep, p * KEEP_SCALE, torch.zeros_like(p))
    return torch.einsum("bhqk,bhkd->bhqd", p, v), lse


# name: B, H, Sq, Sk, D, causal, lengths
CASES = {
    "small": (2, 2, 128, 128, 64, False, None),
    "slab": (1, 2, 512, 512, 64, False, None),        # slab backward + finish kernel
    "d128": (1, 2, 256, 256, 128, False, None),
    "ragged": (2, 3, 200, 200, 64, True, None),       # ragged tiles, causal
    "cross": (2, 2, 128, 320, 64, False, None),
    "lens": (4, 2, 512, 512, 64, False, [512, 300, 64, 0]),
    "chain": (16, 16, 128, 512, 64, False, None),     # B * H = 256: the chained backward
}
STEP = 5
_cache = {}


def _case(name):
    """Inputs (bf16, on the device), the mirror's mask and the fp32 reference of a case, computed once."""
    if name not in _cache:
        B, H, Sq, Sk, D, causal, lens = CASES[name]
        g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
        q = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        k = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        v = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        do = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
        scale = 1.0 / math.sqrt(D)
        keep = _mirror(STEP, B, H, Sq, Sk)
        qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
        o, lse = _ref_attn(qf, kf, vf, keep, kl, scale, causal)
        o.backward(do.float())
        ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
        _cache[name] = (q, k, v, do, kl, scale, ref)
    return _cache[name]


def _check(name, got, ref, lens, Sk):
    live = torch.tensor([True] * got["o"].shape[0] if lens is None else [n > 0 for n in lens], device=DEV)
    errs = {key: _rel(got[key], ref[key]) for key in ("o", "dq", "dk", "dv")}
    errs["lse"] = _rel(got["lse"][live], ref["lse"][live])
    print(name, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs["o"] < TOL_O and errs["lse"] < TOL_LSE, errs
    assert errs["dq"] < TOL_G and errs["dk"] < TOL_G and errs["dv"] < TOL_G, errs
    for key in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[key]).all(), key
    for b, n in enumerate(lens or []):  # the exact zeros the key lengths promise
        n = min(max(n, 0), Sk)
        for key in ("dk", "dv"):
            assert (got[key][b, :, n:] == 0).all(), (key, b)
        if n == 0:
            assert (got["lse"][b] == INF).all(), b
            for key in ("o", "dq", "dk", "dv"):
                assert (got[key][b] == 0).all(), (key, b)


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", [n for n in CASES if n != "chain"])
def test_dropout_vs_fp32(ffC, name, variant):
    B, H, Sq, Sk, D, causal, lens = CASES[name]
    q, k, v, do, kl, scale, ref = _case(name)
    kw = _kw(_step(STEP))
    o, lse = _fwd(ffC, q, k, v, scale, causal, kl, None, **kw)
    for fv in (0, 1, 3):  # the forward structures agree bitwise
        o2, lse2 = _fwd(ffC, q, k, v, scale, causal, kl, fv, **kw)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    # lse is that of the undropped softmax, bitwise
    o0, lse0 = _fwd(ffC, q, k, v, scale, causal, kl, 1)
    assert torch.equal(lse, lse0) and not torch.equal(o, o0)
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, scale, causal, variant, kl, **kw)
    _check(f"{name} bwd {variant}", dict(o=o, lse=lse.view(B, H, Sq), dq=dq, dk=dk, dv=dv), ref, lens, Sk)
    # the same counter value: the same bits; the next one: another mask
    o3, _ = _fwd(ffC, q, k, v, scale, causal, kl, None, **_kw(_step(STEP)))
    dq3, dk3, dv3 = _bwd(ffC, q, k, v, o, lse, do, scale, causal, variant, kl, **_kw(_step(STEP)))
    assert torch.equal(o, o3) and torch.equal(dq, dq3) and torch.equal(dk, dk3) and torch.equal(dv, dv3)
    o4, lse4 = _fwd(ffC, q, k, v, scale, causal, kl, None, **_kw(_step(STEP + 1)))
    assert torch.equal(lse, lse4) and not torch.equal(o, o4)


@pytest.mark.parametrize("variant", [2, 10])
def test_dropout_chained_fused_qkv_layout_and_bias_grad(ffC, variant):
    """B * H = 256 through the fused [B, S, 3, H, D] projection layout (the queries are the first
    128 rows of each sample), bias gradient requested. The dropout kernels leave the fused bias
    gradient to the caller (attn_bwd returns False and does not touch dbias): the column sums of
    what they wrote must match the reference's."""
    B, H, Sq, Sk, D, causal, _ = CASES["chain"]
    q, k, v, do, _, scale, ref = _case("chain")
    qkv = torch.zeros(B, Sk, 3, H, D, device=DEV, dtype=torch.bfloat16)
    qkv[:, :Sq, 0] = q.permute(0, 2, 1, 3)
    qkv[:, :, 1] = k.permute(0, 2, 1, 3)
    qkv[:, :, 2] = v.permute(0, 2, 1, 3)
    o = torch.full((B, Sq, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B * H * Sq,), float("nan"), device=DEV)
    sq, so = [Sk * 3 * H * D, D, 3 * H * D], [Sq * H * D, D, H * D]
    base = qkv.view(-1)
    kw = _kw(_step(STEP))
    ffC.attn_fwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, lse, B, H, Sq, Sk, D, scale, causal, None, **kw)
    dqkv = _nan_like(qkv)
    g = dqkv.view(-1)
    dob = do.permute(0, 2, 1, 3).contiguous()
    n = ffC.attn_bwd_ws(B, H, Sq, Sk, D)
    ws = torch.full((n + 65536,), 7.0, device=DEV)
    dbias = torch.full((3 * H * D,), 0.5, device=DEV)
    prev = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    try:
        done = ffC.attn_bwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, dob, so, lse, g, sq, g[H * D:], sq,
                            g[2 * H * D:], sq, ws[:n], B, H, Sq, Sk, D, scale, causal, dbias, None, **kw)
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    got = dict(o=o.permute(0, 2, 1, 3), lse=lse.view(B, H, Sq), dq=dqkv[:, :Sq, 0].permute(0, 2, 1, 3),
               dk=dqkv[:, :, 1].permute(0, 2, 1, 3), dv=dqkv[:, :, 2].permute(0, 2, 1, 3))
    _check(f"chain fused layout bwd {variant}", got, ref, None, Sk)
    assert torch.isnan(dqkv[:, Sq:, 0].float()).all()  # rows that are no query stay untouched
    want = torch.stack([ref[key].sum(dim=(0, 2)) for key in ("dq", "dk", "dv")]).reshape(-1)  # [3][H][D]
    if done:
        have = dbias - 0.5
    else:  # the caller's sum (linear_bwd's bias gradient over the dqkv rows)
        assert torch.equal(dbias, torch.full_like(dbias, 0.5))
        have = torch.stack([got[key].float().sum(dim=(0, 2)) for key in ("dq", "dk", "dv")]).reshape(-1)
    err = _rel(have, want)
    print("QKV bias gradient relative error", f"{err:.2e}", "fused" if done else "summed by the caller")
    assert err < TOL_G, err


def test_dropout_arguments_are_checked(ffC):
    q, k, v, do, _, scale, _ = _case("small")
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, scale, False, None, None, **_kw(_step(0).int()))  # not int64
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, scale, False, None, None, **_kw(torch.zeros(1, dtype=torch.int64)))  # not on the device
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, scale, False, None, None, **_kw(_step(0), thr=256))
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, scale, False, None, None, **_kw(_step(0), h0=1, H_total=2))  # 2 heads from head 1 of 2


# ------------------------------------------------------------------------------------- op level
def _run_mha(dtype, E, H, S, B=2, step=4):
    """MultiHeadAttention(dropout = 0.1) through OpCtx on the device, and fp32 torch on the same
    weights with the mirror's mask: relative errors of the output and every gradient."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    g = torch.Generator().manual_seed(9)
    ff = FFModel(FFConfig([]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    L = ff.multihead_attention(tx, tx, tx, E, H, dropout=P, name="att").owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n, seed=SEED)
    ctx.rng_step = _step(step)
    x = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    ws = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).to(DEV, dtype) for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims, device=DEV) for w in L.weights]
    y = L.impl.forward(ctx, [x, x, x], ws)[0]
    dy = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    dxs = L.impl.backward(ctx, [dy])
    ctx.training = False
    y_eval = L.impl.forward(ctx, [x, x, x], ws)[0]
    torch.cuda.synchronize()
    xf = x.float().requires_grad_()
    wf = [w.float().requires_grad_() for w in ws]
    D = E // H
    W, bb = wf[0].reshape(3, H * D, E), wf[1].reshape(3, H * D)
    qq, kk, vv = ((xf @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    keep = K.attn_dropout_keep_ref(SEED, zlib.crc32(b"att"), step, B, H, S, S, P, device=DEV)
    o, _ = _ref_attn(qq, kk, vv, keep, None, 1.0 / math.sqrt(D), False)
    yr = o.transpose(1, 2).reshape(B, S, H * D) @ wf[2].reshape(E, -1).t() + wf[3]
    yr.backward(dy.float())
    o0, _ = _ref_attn(qq, kk, vv, None, None, 1.0 / math.sqrt(D), False)
    y0 = (o0.transpose(1, 2).reshape(B, S, H * D) @ wf[2].reshape(E, -1).t() + wf[3]).detach()
    errs = {"y": _rel(y, yr), "dx": _rel(dxs[0], xf.grad), "y_eval": _rel(y_eval, y0)}
    for w, gw, r in zip(L.weights, ctx.wgrads, wf):
        errs["d" + w.short_name] = _rel(gw, r.grad)
    for t in [y, dxs[0]] + ctx.wgrads:
        assert torch.isfinite(t).all()
    print(dtype, D, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert _rel(y0, yr) > 0.05  # the mask matters: an op that ignored the rate fails the bounds below
    return errs


def test_mha_op_bf16_padded_head_dim(ffC):
    """bf16, E = 128, 4 heads: head dim 32 zero-padded to 64, the same kernels and the same mask."""
    errs = _run_mha(torch.bfloat16, 128, 4, 128)
    assert errs.pop("y") < TOL_O and errs.pop("y_eval") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


def test_mha_op_fp32_device_path(ffC):
    """--dtype fp32 on the device (f32 MFMA GEMMs, row softmax, attn_dropout_f32 on P and dP): rounds
    like the fp32 reference, 1e-4 as in the key-length test of this path."""
    errs = _run_mha(torch.float32, 128, 2, 128)
    assert all(e < 1e-4 for e in errs.values()), errs


# --------------------------------------------------------------------------------- step capture
def _train_bert(flags, attn_dropout, steps=6):
    from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(0)
    B, bc = 4, BertConfig.tiny(64)
    bc.attn_dropout = attn_dropout
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    ids, pos, _ = build_bert(ff, B, bc)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    loaders = [ff.create_data_loader(ids, rng.integers(1, bc.vocab, (N, bc.seq)).astype(np.int32)),
               ff.create_data_loader(pos, np.tile(np.arange(bc.seq, dtype=np.int32), (N, 1))),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, bc.vocab, (N, bc.seq, 1)).astype(np.int32))]
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


def test_bert_attention_dropout_trains_under_step_capture():
    """bert-tiny with attn_dropout = 0.1, 6 steps (3 eager, the capture, 2 replays), hipGraph step
    capture on and off: losses and weights agree (rtol 1e-5, atol 1e-6, the key-length test's bound).
    The kernels read the step counter on the device, so the replays draw new masks; a counter baked
    into the graph would repeat the capture step's mask and leave the eager run. The losses differ
    from the run without dropout."""
    ffg, lg, wg = _train_bert(["--hip-graphs"], P)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    assert int(ffg.executor.rng_step.item()) == 6
    _, le, we = _train_bert(["--no-hip-graphs"], P)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
    ffd, ld, _ = _train_bert(["--hip-graphs"], 0.0)
    assert ffd._step_graph.graph is not None and ffd.executor.rng_step is None
    print("losses without attention dropout", ld)
    assert np.abs(ld - lg).max() > 1e-4, (ld, lg)
