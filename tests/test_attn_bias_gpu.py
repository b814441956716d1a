"""Additive score bias (AttnArgs.sbias) of the flash-attention kernels, the attention ops that take it
(multihead_attention(attn_bias=...), scaled_dot_product_attention), the fused HuggingFace import and a
captured training step, on the GPU.

Scores are s = scale q.k + bias[b, h, q, k] with an fp32 bias whose batch / head extents may be 1
(broadcast). Tolerances are those of tests/test_kernels_gpu.py::test_flash_attention (relative
Frobenius error against fp32 torch on the same bf16-rounded inputs: o < 2e-2, lse < 1e-3, gradients <
3e-2); an fp32 bias adds no rounding of its own, so they carry over. A query row whose every key is
removed has a NaN torch reference, so the reference is built with such rows made finite first and
holds exact zeros (lse: +inf) there. Inputs are seeded on the CPU; every output buffer starts as NaN,
so an element a kernel leaves unwritten fails the comparison."""
import math

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
TOL_O, TOL_LSE, TOL_G = 2e-2, 1e-3, 3e-2

# name: B, H, Sq, Sk, D, causal, bias shape, key lengths
CASES = {
    "a": (2, 2, 128, 128, 64, False, (2, 2, 128, 128), None),    # a wrong batch or head stride shows
    "b": (2, 3, 200, 137, 64, False, (1, 3, 200, 137), None),    # ragged Sk, rows not 16-B aligned, batch broadcast
    "c": (2, 2, 256, 256, 128, True, (1, 1, 256, 256), None),    # D = 128, both broadcasts, causal on top
    "d": (1, 2, 256, 256, 64, False, (1, 1, 256, 256), None),    # sliding window of 0 / -inf, row 5 all -inf
    "e": (2, 2, 128, 320, 64, False, (2, 1, 128, 320), [320, 65]),  # bias and key lengths together
    "f": (16, 16, 128, 512, 64, False, (1, 16, 128, 512), None),  # B*H = 256: the chained backward, two key blocks
    "g": (1, 2, 512, 512, 64, False, (1, 2, 512, 512), None),    # Sq >= 512: not attn_fwd2_kernel
}
DEAD_ROW = 5


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _bias_kw(bias, B, H):
    """The bindings' keyword arguments of a contiguous fp32 [Bb, Hb, Sq, Sk] bias."""
    if bias is None:
        return {}
    Bb, Hb, Sq, Sk = bias.shape
    return dict(sbias=bias, sbias_sb=Hb * Sq * Sk if Bb > 1 else 0, sbias_sh=Sq * Sk if Hb > 1 else 0)


def _ref_attn(q, k, v, bias, lens, scale, causal, keep=None, keep_scale=1.0):
    """fp32 torch attention of [B, H, S, D] tensors with an additive bias: (o, lse, live) where live
    [B, H, Sq] marks the query rows with a key left; the others get o = 0 and lse = +inf
    (differentiable in q, k, v). keep: optional dropout mask applied to P, kept ones scaled."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale + bias
    if lens is not None:
        L = lens.to(q.device).long().clamp(0, Sk)
        s = s.masked_fill((torch.arange(Sk, device=q.device)[None, :] >= L[:, None])[:, None, None, :], -INF)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), -INF)
    live = ~(s == -INF).all(-1)
    sf = torch.where(live[..., None], s, torch.zeros_like(s))
    p = torch.where(live[..., None], torch.softmax(sf, -1), torch.zeros_like(s))
    lse = torch.where(live, torch.logsumexp(sf, -1), torch.full_like(sf[..., 0], INF)).detach()
    if keep is not None:
        p = torch.where(keep, p * keep_scale, torch.zeros_like(p))
    return torch.einsum("bhqk,bhkd->bhqd", p, v), lse, live


def _make_bias(name, shape, g):
    if name == "d":  # 0 where |q - k| <= 40, else -inf; query row DEAD_ROW entirely -inf
        Sq, Sk = shape[2:]
        i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
        b = torch.where((i - j).abs() <= 40, 0.0, -INF)
        b[DEAD_ROW] = -INF
        return b.expand(shape).contiguous().float()
    return torch.randn(shape, generator=g)


_cache = {}


def _case(name):
    """Inputs (bf16, bias fp32, on the device) and the fp32 reference of a case, computed once."""
    if name not in _cache:
        B, H, Sq, Sk, D, causal, bshape, lens = CASES[name]
        g = torch.Generator().manual_seed(2000 + ord(name))
        q = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        k = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        v = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        do = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        bias = _make_bias(name, bshape, g).to(DEV)
        kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
        scale = 1.0 / math.sqrt(D)
        qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
        o, lse, live = _ref_attn(qf, kf, vf, bias, kl, scale, causal)
        o.backward(do.float())
        ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad, live=live)
        _cache[name] = (q, k, v, do, bias, kl, scale, ref)
    return _cache[name]


def _fwd(ffC, q, k, v, bias, kl, scale, causal, variant=None, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    o, lse = _nan_like(q), torch.full((B * H * Sq,), float("nan"), device=DEV)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    prev = ffC.attn_fwd_variant()
    if variant is not None:
        ffC.attn_set_fwd_variant(variant)
    try:
        ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, causal, kl, **kw, **_bias_kw(bias, B, H))
    finally:
        ffC.attn_set_fwd_variant(prev)
    return o, lse


def _bwd(ffC, q, k, v, o, lse, do, bias, kl, scale, causal, variant, **kw):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    dq, dk, dv = _nan_like(q), _nan_like(k), _nan_like(v)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    n = ffC.attn_bwd_ws(B, H, Sq, Sk, D)
    ws = torch.full((n + 4096,), 7.0, device=DEV)  # a guard band after the workspace
    prev = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    try:
        done = ffC.attn_bwd(q, sq, k, sk, v, sk, o, sq, do, sq, lse, dq, sq, dk, sk, dv, sk, ws[:n], B, H, Sq, Sk, D,
                            scale, causal, None, kl, **kw, **_bias_kw(bias, B, H))
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    assert not done or bias is None  # with a score bias the QKV bias gradient is the caller's
    return dq, dk, dv


def _check(name, got, ref):
    live = ref["live"]
    errs = {key: _rel(got[key], ref[key]) for key in ("o", "dq", "dk", "dv")}
    errs["lse"] = _rel(got["lse"][live], ref["lse"][live])
    print(name, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs["o"] < TOL_O and errs["lse"] < TOL_LSE, errs
    assert errs["dq"] < TOL_G and errs["dk"] < TOL_G and errs["dv"] < TOL_G, errs
    for key in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[key]).all(), key
    assert torch.isfinite(got["lse"][live]).all()
    assert (got["lse"][~live] == INF).all()
    assert (got["o"][~live] == 0).all() and (got["dq"][~live] == 0).all()


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_score_bias_vs_fp32(ffC, name, variant):
    """Forward structures 0, 1 and the default (bitwise equal to each other) and backward structures 2
    and 10 against the fp32 reference; exact zeros where the semantics promise them."""
    B, H, Sq, Sk, D, causal, _, lens = CASES[name]
    q, k, v, do, bias, kl, scale, ref = _case(name)
    o, lse = _fwd(ffC, q, k, v, bias, kl, scale, causal)
    for fv in (0, 1):
        o2, lse2 = _fwd(ffC, q, k, v, bias, kl, scale, causal, fv)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, bias, kl, scale, causal, variant)
    got = dict(o=o, lse=lse.view(B, H, Sq), dq=dq, dk=dk, dv=dv)
    _check(f"case {name} bwd {variant}", got, ref)
    if name == "d":
        assert (~ref["live"]).sum().item() == B * H  # row DEAD_ROW of every (batch, head)
        assert (o[:, :, DEAD_ROW] == 0).all() and (dq[:, :, DEAD_ROW] == 0).all()
        assert (lse.view(B, H, Sq)[:, :, DEAD_ROW] == INF).all()
    if lens is not None:
        for b, n in enumerate(lens):  # rows at or past the length: written, as exact zeros
            assert (dk[b, :, n:] == 0).all() and (dv[b, :, n:] == 0).all(), b


@pytest.mark.parametrize("name", ["a", "b", "c", "g"])
def test_zero_bias_agrees_with_no_bias(ffC, name):
    """A bias of zeros against the call without one, within the tolerances (not bitwise: the running
    max is formed in another order)."""
    B, H, Sq, Sk, D, causal, bshape, _ = CASES[name]
    q, k, v, do, _, _, scale, _ = _case(name)
    zero = torch.zeros(bshape, device=DEV)
    o0, lse0 = _fwd(ffC, q, k, v, None, None, scale, causal)
    o1, lse1 = _fwd(ffC, q, k, v, zero, None, scale, causal)
    assert _rel(o1, o0) < TOL_O and _rel(lse1, lse0) < TOL_LSE
    for variant in (2, 10):
        g0 = _bwd(ffC, q, k, v, o0, lse0, do, None, None, scale, causal, variant)
        g1 = _bwd(ffC, q, k, v, o1, lse1, do, zero, None, scale, causal, variant)
        for a, b in zip(g1, g0):
            assert torch.isfinite(a).all() and _rel(a, b) < TOL_G


@pytest.mark.parametrize("variant", [2, 10])
def test_score_bias_with_dropout(ffC, variant):
    """Case a with drop_thr = 64: the reference drops P with the mirror's mask."""
    B, H, Sq, Sk, D, causal, _, _ = CASES["a"]
    q, k, v, do, bias, _, scale, _ = _case("a")
    seed, layer, thr = 1234, 77, 64
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    kw = K._drop_kw((thr, step, K.attn_dropout_seed(seed, layer), 0, 0, H))
    keep = K.attn_dropout_keep_ref(seed, layer, 3, B, H, Sq, Sk, thr / 256.0, device=DEV)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    oref, lref, live = _ref_attn(qf, kf, vf, bias, None, scale, causal, keep, 256.0 / (256 - thr))
    oref.backward(do.float())
    ref = dict(o=oref.detach(), lse=lref, dq=qf.grad, dk=kf.grad, dv=vf.grad, live=live)
    o, lse = _fwd(ffC, q, k, v, bias, None, scale, causal, **kw)
    for fv in (0, 1):
        o2, lse2 = _fwd(ffC, q, k, v, bias, None, scale, causal, fv, **kw)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, bias, None, scale, causal, variant, **kw)
    _check(f"bias x dropout bwd {variant}", dict(o=o, lse=lse.view(B, H, Sq), dq=dq, dk=dk, dv=dv), ref)


def test_finfo_min_bias_removes_keys(ffC):
    """HuggingFace-style masks: finfo(float32).min times log2(e) overflows, which the kernels read as
    -inf; the result equals the -inf mask's bitwise."""
    B, H, Sq, Sk, D, causal, _, _ = CASES["d"]
    q, k, v, do, bias, _, scale, _ = _case("d")
    fmin = torch.where(bias == -INF, torch.finfo(torch.float32).min, 0.0).to(DEV)
    o0, lse0 = _fwd(ffC, q, k, v, bias, None, scale, causal)
    o1, lse1 = _fwd(ffC, q, k, v, fmin, None, scale, causal)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


def test_score_bias_arguments_are_checked(ffC):
    B, H, Sq, Sk, D, causal, _, _ = CASES["a"]
    q, k, v, do, bias, _, scale, _ = _case("a")
    o, lse = _nan_like(q), torch.empty(B * H * Sq, device=DEV)
    sq = [H * Sq * D, Sq * D, D]

    def call(b, sb, sh):
        ffC.attn_fwd(q, sq, k, sq, v, sq, o, sq, lse, B, H, Sq, Sk, D, scale, causal, sbias=b, sbias_sb=sb, sbias_sh=sh)

    with pytest.raises(RuntimeError):
        call(bias.bfloat16(), H * Sq * Sk, Sq * Sk)  # not fp32
    with pytest.raises(RuntimeError):
        call(bias[..., :64], H * Sq * Sk, Sq * Sk)  # rows not [Sq, Sk] / not contiguous
    with pytest.raises(RuntimeError):
        call(bias[:1], H * Sq * Sk, Sq * Sk)  # storage too short for a batch stride
    with pytest.raises(RuntimeError):
        call(bias.cpu(), H * Sq * Sk, Sq * Sk)  # wrong device
    with pytest.raises(ValueError):
        K.flash_attn_fwd(q, sq, k, sq, v, sq, o, sq, B, H, Sq, Sk, D, scale, causal, bias=bias[:, :1, :64])
    assert torch.isnan(o.float()).all()  # nothing was launched


# ------------------------------------------------------------------------------------- op level
def _ctx(L):
    from flexflow_amd.ops import OpCtx
    n = len(L.impl.axis_sizes())
    return OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)


def _run_sdpa(dtype, D, causal=False):
    """OP_SDPA through OpCtx on the device against torch's scaled_dot_product_attention in fp32 on the
    same (rounded) inputs: relative errors of the output and the q / k / v gradients."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    B, H, Sq, Sk = 2, 3, 128, 192
    g = torch.Generator().manual_seed(21)
    ff = FFModel(FFConfig([]))
    tq, tk, tv = (ff.create_tensor([B, H, s, D], DataType.DT_FLOAT) for s in (Sq, Sk, Sk))
    tb = ff.create_tensor([1, H, Sq, Sk], DataType.DT_FLOAT)
    L = ff.scaled_dot_product_attention(tq, tk, tv, attn_bias=tb, scale=0.2, causal=causal).owner_layer
    q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, dtype) for s in (Sq, Sk, Sk))
    bias = torch.randn(1, H, Sq, Sk, generator=g)
    bias[..., 100:140] = -INF
    bias = bias.to(DEV)
    ctx = _ctx(L)
    y = L.impl.forward(ctx, [q, k, v, bias], [])[0]
    dy = torch.randn(B, H, Sq, D, generator=g).to(DEV, dtype)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == 4 and dxs[3] is None
    torch.cuda.synchronize()
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    m = bias.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=DEV).triu(1), -INF) if causal else bias
    yr = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=m, scale=0.2)
    yr.backward(dy.float())
    errs = {"y": _rel(y, yr), "dq": _rel(dxs[0], qf.grad), "dk": _rel(dxs[1], kf.grad), "dv": _rel(dxs[2], vf.grad)}
    for t in [y] + list(dxs[:3]):
        assert torch.isfinite(t).all() and t.dtype == dtype
    print("sdpa", dtype, D, causal, {k_: f"{e:.2e}" for k_, e in errs.items()})
    return errs


@pytest.mark.parametrize("D,causal", [(64, False), (64, True), (32, False)])
def test_sdpa_op_bf16(ffC, D, causal):
    """Head dim 64 (the flash kernels through the [H*S*D, S*D, D] strides) and 32 (zero-padded to 64)."""
    errs = _run_sdpa(torch.bfloat16, D, causal)
    assert errs.pop("y") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


def test_sdpa_op_fp32_device(ffC):
    """--dtype fp32 on the device (f32 MFMA GEMMs + score_bias_f32 + row softmax): rounds like the fp32
    reference (~1e-6 relative); 1e-4 as tests/test_attn_key_lengths_gpu.py asks of this path."""
    errs = _run_sdpa(torch.float32, 64)
    assert all(e < 1e-4 for e in errs.values()), errs


@pytest.mark.parametrize("H", [2, 4])
def test_mha_op_bf16_alibi(ffC, H):
    """bf16 fused self-attention with an ALiBi bias [1, H, S, S], E = 128, S = 128: head dim 64 and 32
    (zero-padded), against an explicit fp32 composition from the layer's own weights. The flash
    backward leaves the QKV bias gradient to the projection (it is still right)."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    B, S, E = 4, 128, 128
    g = torch.Generator().manual_seed(9)
    ff = FFModel(FFConfig([]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    tb = ff.create_tensor([1, H, S, S], DataType.DT_FLOAT)
    L = ff.multihead_attention(tx, tx, tx, E, H, causal=True, attn_bias=tb).owner_layer
    assert L.attrs["fused_qkv"]
    ctx = _ctx(L)
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)])
    dist = (torch.arange(S)[:, None] - torch.arange(S)[None, :]).abs().float()
    bias = (-slopes[:, None, None] * dist)[None].contiguous().to(DEV)
    x = torch.randn(B, S, E, generator=g).to(DEV, torch.bfloat16)
    ws = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).to(DEV, torch.bfloat16) for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims, device=DEV) for w in L.weights]
    y = L.impl.forward(ctx, [x, x, x, bias], ws)[0]
    dy = torch.randn(B, S, E, generator=g).to(DEV, torch.bfloat16)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == 4 and all(d is None for d in dxs[1:])
    torch.cuda.synchronize()
    xf = x.float().requires_grad_()
    wf = [w.float().requires_grad_() for w in ws]
    D = E // H
    W, bb = wf[0].reshape(3, H * D, E), wf[1].reshape(3, H * D)
    qq, kk, vv = ((xf @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    o, _, _ = _ref_attn(qq, kk, vv, bias, None, 1.0 / math.sqrt(D), True)
    yr = o.transpose(1, 2).reshape(B, S, H * D) @ wf[2].reshape(E, -1).t() + wf[3]
    yr.backward(dy.float())
    errs = {"y": _rel(y, yr), "dx": _rel(dxs[0], xf.grad)}
    for w, gw, r in zip(L.weights, ctx.wgrads, wf):
        errs["d" + w.short_name] = _rel(gw, r.grad)
    print("mha alibi", D, {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs.pop("y") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


# ------------------------------------------------------------------------------ fused HF import
@pytest.mark.parametrize("d_kv", [32, 64])
def test_mt5_fused_sdpa_bf16_gpu(d_kv):
    """The MT5 of tests/test_hf_import_gpu.py (d_kv = 32: zero-padded heads) and one with d_kv = 64,
    imported with fuse_sdpa=True: logits within that test's 3e-2 of the fp32 torch model, the loss
    falls over 4 steps, and the graph holds OP_SDPA in place of the batched matmuls."""
    transformers = pytest.importorskip("transformers")
    from flexflow_amd.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexflow_amd.torch.model import PyTorchModel
    from flexflow_amd.type import DataType, OperatorType
    B, S, T, V = 4, 16, 12, 512
    torch.manual_seed(0)
    cfg = transformers.MT5Config(vocab_size=V, d_model=128, d_kv=d_kv, d_ff=256, num_layers=2, num_decoder_layers=2,
                                 num_heads=4, relative_attention_num_buckets=8, dropout_rate=0.0)
    m = transformers.MT5ForConditionalGeneration(cfg)
    fc = FFConfig(["--dtype", "bf16", "--no-hip-graphs"])
    fc.batch_size = B
    ff = FFModel(fc)
    ins = [ff.create_tensor([B, S], DataType.DT_INT64), ff.create_tensor([B, S], DataType.DT_INT64),
           ff.create_tensor([B, T], DataType.DT_INT64)]
    outs = PyTorchModel(m, is_hf_model=True, input_names=["input_ids", "attention_mask", "decoder_input_ids"],
                        batch_size=B, seq_length=(S, T), fuse_sdpa=True).torch_to_ff(ff, ins)
    kinds = [L.op_type for L in ff.layers]
    assert kinds.count(OperatorType.OP_SDPA) == 6 and OperatorType.OP_BATCHMATMUL not in kinds
    ff.optimizer = SGDOptimizer(ff, 0.05)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    src = rng.integers(1, V, (B, S))
    tgt = src[:, :T]
    dec = np.concatenate([np.zeros((B, 1), np.int64), tgt[:, :-1]], 1)
    ins[0].set_tensor(ff, src.astype(np.int64))
    ins[1].set_tensor(ff, np.ones((B, S), np.int64))
    ins[2].set_tensor(ff, dec.astype(np.int64))
    ff.label_tensor.set_tensor(ff, tgt.reshape(B, T, 1).astype(np.int32))
    ff.forward()
    got = np.asarray(outs[0].get_tensor(ff), dtype=np.float32)
    with torch.no_grad():
        ref = m.eval()(input_ids=torch.tensor(src), attention_mask=torch.ones(B, S, dtype=torch.long),
                       decoder_input_ids=torch.tensor(dec), use_cache=False).logits.numpy()
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("mt5 fused d_kv", d_kv, "relative error", rel)
    assert rel < 3e-2, rel
    losses = []
    for _ in range(4):
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# --------------------------------------------------------------------------------- step capture
def _train_biased(flags, steps):
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    torch.manual_seed(0)
    B, S, E, H, C = 4, 64, 128, 2, 16
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT, name="x")
    bias = ff.create_tensor([1, H, S, S], DataType.DT_FLOAT, create_grad=False, name="alibi")
    t = x
    for i in range(2):
        a = ff.multihead_attention(t, t, t, E, H, causal=True, attn_bias=bias, name=f"attn{i}")
        t = ff.layer_norm(ff.add(t, a), [2], name=f"ln{i}")
    ff.softmax(ff.dense(t, C, name="head"), name="sm")
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    slopes = np.array([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], np.float32)
    dist = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :]).astype(np.float32)
    bias.set_tensor(ff, (-slopes[:, None, None] * dist)[None])
    rng = np.random.default_rng(0)
    N = B * steps
    loaders = [ff.create_data_loader(x, rng.standard_normal((N, S, E)).astype(np.float32)),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, C, (N, S, 1)).astype(np.int32))]
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


def test_biased_causal_mha_trains_under_step_capture():
    """Two biased, causal attention layers, hipGraph step capture on and off. A step is captured only
    after three eager warm-up steps, so 6 steps run (3 eager, the capture, 2 replays: 3 captured
    steps) and the graph must exist; losses and weights agree with 6 eager steps at the rtol 1e-5 /
    atol 1e-6 of tests/test_attn_key_lengths_gpu.py::test_bert_key_lengths_train_under_step_capture."""
    ffg, lg, wg = _train_biased(["--hip-graphs"], 6)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    _, le, we = _train_biased(["--no-hip-graphs"], 6)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
