"""Per-sample key lengths (AttnArgs.key_lens) of the flash-attention kernels, the attention op and a
captured bert-tiny training step, on the GPU.

Tolerances are those of tests/test_kernels_gpu.py::test_flash_attention (relative Frobenius error
against fp32 torch with masked_fill(-inf): o < 2e-2, lse < 1e-3, gradients < 3e-2), every element
compared. A sample with L_b = 0 has a NaN torch reference, so the reference is built from the
samples with L_b > 0 and holds exact zeros (lse: +inf) for the others. Inputs are seeded on the CPU;
every output buffer starts as NaN, so an element a kernel leaves unwritten fails the comparison."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
TOL_O, TOL_LSE, TOL_G = 2e-2, 1e-3, 3e-2

F_LENS = [512, 257, 256, 255, 64, 1, 300, 0]  # case f: second 256-key block live / wholly padding / L = 0
# name: B, H, Sq, Sk, D, causal, lengths
CASES = {
    "a": (4, 2, 512, 512, 64, False, [512, 300, 64, 1]),       # attn_fwd2_kernel
    "b": (4, 2, 256, 256, 128, False, [256, 130, 128, 7]),
    "c": (2, 3, 200, 200, 64, False, [200, 77]),               # ragged Sk plus lengths
    "d": (2, 3, 384, 384, 64, True, [384, 100]),
    "e": (2, 2, 128, 320, 64, False, [320, 65]),               # cross attention
    "f": (16, 16, 512, 512, 64, False, F_LENS * 2),            # B*H = 256: the chained backward
}


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ref_attn(q, k, v, lens, scale, causal):
    """fp32 torch attention of [B, H, S, D] tensors over each sample's first clamp(lens[b], 0, Sk)
    keys: (o, lse), o = 0 and lse = +inf for a sample without keys (differentiable in q, k, v)."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    L = lens.to(q.device).long().clamp(0, Sk)
    live = (L > 0).nonzero().flatten()
    s = torch.einsum("bhqd,bhkd->bhqk", q[live], k[live]) * scale
    pad = torch.arange(Sk, device=q.device)[None, :] >= L[live][:, None]
    s = s.masked_fill(pad[:, None, None, :], -INF)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), -INF)
    o_live = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), v[live])
    o = torch.zeros(B, H, Sq, v.shape[-1], device=q.device).index_copy(0, live, o_live)
    lse = torch.full((B, H, Sq), INF, device=q.device).index_copy(0, live, torch.logsumexp(s, -1).detach())
    return o, lse


_cache = {}


def _case(name):
    """Inputs (bf16, on the device) and the fp32 reference of a case, computed once."""
    if name not in _cache:
        B, H, Sq, Sk, D, causal, lens = CASES[name]
        g = torch.Generator().manual_seed(1000 + ord(name))
        q = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        k = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        v = torch.randn(B, H, Sk, D, generator=g).bfloat16().to(DEV)
        do = torch.randn(B, H, Sq, D, generator=g).bfloat16().to(DEV)
        kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        scale = 1.0 / math.sqrt(D)
        qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
        o, lse = _ref_attn(qf, kf, vf, kl, scale, causal)
        o.backward(do.float())
        ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
        _cache[name] = (q, k, v, do, kl, scale, ref)
    return _cache[name]


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _fwd(ffC, q, k, v, kl, scale, causal, variant=None):
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    o, lse = _nan_like(q), torch.full((B * H * Sq,), float("nan"), device=DEV)
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    prev = ffC.attn_fwd_variant()
    if variant is not None:
        ffC.attn_set_fwd_variant(variant)
    try:
        if kl is None:
            ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, causal)
        else:
            ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, causal, kl)
    finally:
        ffC.attn_set_fwd_variant(prev)
    return o, lse


def _bwd(ffC, q, k, v, o, lse, do, kl, scale, causal, variant):
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
                     causal, None, kl)
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    return dq, dk, dv


def _check_against_ref(name, got, ref, lens, Sk):
    """got / ref: dicts of o, lse [B, H, Sq], dq, dk, dv in [B, H, S, D]. Tolerances, then the exact
    zeros and finiteness the semantics promise."""
    L = torch.tensor(lens).clamp(0, Sk)
    live = (L > 0).to(DEV)
    errs = {key: _rel(got[key], ref[key]) for key in ("o", "dq", "dk", "dv")}
    errs["lse"] = _rel(got["lse"][live], ref["lse"][live])
    print(name, "relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs["o"] < TOL_O and errs["lse"] < TOL_LSE, errs
    assert errs["dq"] < TOL_G and errs["dk"] < TOL_G and errs["dv"] < TOL_G, errs
    for key in ("o", "dq", "dk", "dv"):
        assert torch.isfinite(got[key]).all(), key
    assert torch.isfinite(got["lse"][live]).all()
    for b, n in enumerate(L.tolist()):
        for key in ("dk", "dv"):  # rows at or past the length: written, as exact zeros
            assert (got[key][b, :, n:] == 0).all(), (key, b)
        if n == 0:
            assert (got["lse"][b] == INF).all(), b
            for key in ("o", "dq", "dk", "dv"):
                assert (got[key][b] == 0).all(), (key, b)


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_key_lengths_vs_fp32(ffC, name, variant):
    """Forward structures 0, 1, 3 (bitwise equal to each other) and backward structures 2 and 10
    with lengths that hit a full row, a mid-tile cut, a tile edge, a single key, a key block that is
    wholly padding and (case f) an empty sample, against the fp32 reference; plus the exact zeros."""
    B, H, Sq, Sk, D, causal, lens = CASES[name]
    q, k, v, do, kl, scale, ref = _case(name)
    o, lse = _fwd(ffC, q, k, v, kl, scale, causal)
    for fv in (0, 1, 3):
        o2, lse2 = _fwd(ffC, q, k, v, kl, scale, causal, fv)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o, lse, do, kl, scale, causal, variant)
    got = dict(o=o, lse=lse.view(B, H, Sq), dq=dq, dk=dk, dv=dv)
    _check_against_ref(f"case {name} bwd {variant}", got, ref, lens, Sk)


@pytest.mark.parametrize("variant", [2, 10])
def test_key_lengths_fused_qkv_layout_and_bias_grad(ffC, variant):
    """Case f through the fused [B, S, 3, H, D] projection layout. Variant 10 (the chained
    attn_bwd1b_kernel) adds the QKV bias gradient itself: it must equal the column sums of the fp32
    reference's dq / dk / dv within the gradient tolerance, with key blocks that are skipped for
    some samples and an empty sample contributing zeros. Variant 2 declines and leaves dbias alone."""
    B, H, S, _, D, causal, lens = CASES["f"]
    q, k, v, do, kl, scale, ref = _case("f")
    qkv = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2).contiguous()  # [B, S, 3, H, D]
    o = torch.full((B, S, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B * H * S,), float("nan"), device=DEV)
    sq, so = [S * 3 * H * D, D, 3 * H * D], [S * H * D, D, H * D]
    base = qkv.view(-1)
    ffC.attn_fwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, lse, B, H, S, S, D, scale, causal, kl)
    dqkv = _nan_like(qkv)
    g = dqkv.view(-1)
    dob = do.permute(0, 2, 1, 3).contiguous()
    n = ffC.attn_bwd_ws(B, H, S, S, D)
    ws = torch.full((n + 65536,), 7.0, device=DEV)
    dbias = torch.full((3 * H * D,), 0.5, device=DEV)
    prev = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    try:
        done = ffC.attn_bwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, dob, so, lse, g, sq, g[H * D:], sq,
                            g[2 * H * D:], sq, ws[:n], B, H, S, S, D, scale, causal, dbias, kl)
    finally:
        ffC.attn_set_bwd_variant(prev)
    assert torch.equal(ws[n:], torch.full_like(ws[n:], 7.0)), "attn_bwd wrote past its workspace"
    got = dict(o=o.permute(0, 2, 1, 3), lse=lse.view(B, H, S),
               **{key: dqkv[:, :, i].permute(0, 2, 1, 3) for i, key in enumerate(("dq", "dk", "dv"))})
    _check_against_ref(f"case f fused layout bwd {variant}", got, ref, lens, S)
    assert done == (variant == 10)
    if done:
        want = torch.stack([ref[key].sum(dim=(0, 2)) for key in ("dq", "dk", "dv")]).reshape(-1)  # [3][H][D]
        err = _rel(dbias - 0.5, want)
        print("fused QKV bias gradient relative error", f"{err:.2e}")
        assert torch.isfinite(dbias).all() and err < TOL_G, err
    else:
        assert torch.equal(dbias, torch.full_like(dbias, 0.5))


@pytest.mark.parametrize("name,variant", [("a", 10), ("a", 2), ("d", 10), ("f", 10), ("f", 2)])
def test_padding_content_does_not_matter(ffC, name, variant):
    """K / V rows at or past the length as zeros or as 1e3 * randn (finite): o, lse, dq and the valid
    rows of dk / dv are bitwise equal. The first run repeated is bitwise equal in every output (no
    atomics anywhere)."""
    B, H, Sq, Sk, D, causal, lens = CASES[name]
    q, k, v, do, kl, scale, _ = _case(name)
    pad = (torch.arange(Sk, device=DEV)[None, :] >= kl.clamp(0, Sk)[:, None])[:, None, :, None]
    g = torch.Generator().manual_seed(77)
    noise = [(1e3 * torch.randn(B, H, Sk, D, generator=g)).bfloat16().to(DEV) for _ in range(2)]
    runs = []
    for fill in (0, 0, 1):
        k2 = torch.where(pad, noise[0] if fill else torch.zeros_like(k), k)
        v2 = torch.where(pad, noise[1] if fill else torch.zeros_like(v), v)
        o, lse = _fwd(ffC, q, k2, v2, kl, scale, causal)
        dq, dk, dv = _bwd(ffC, q, k2, v2, o, lse, do, kl, scale, causal, variant)
        runs.append(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv))
    first, again, noisy = runs
    for key in first:  # repeatability
        assert torch.equal(first[key], again[key]), key
    for key in ("o", "lse", "dq"):
        assert torch.equal(first[key], noisy[key]), key
    for key in ("dk", "dv"):
        assert torch.isfinite(noisy[key]).all()
        assert torch.equal(first[key], noisy[key]), key  # valid rows equal; the others are zeros in both


@pytest.mark.parametrize("S,causal", [(512, False), (384, True)])
@pytest.mark.parametrize("variant", [2, 10])
def test_full_lengths_change_nothing(ffC, S, causal, variant):
    """key_lens filled with Sk: o and lse bitwise equal to the call without key_lens (S = 512
    non-causal: the MASK = false against the MASK = true instantiation), gradients within tolerance."""
    B, H, D = 2, 3, 64
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(4))
    full = torch.full((B,), S, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(D)
    for fv in (0, 1, 3):
        o0, lse0 = _fwd(ffC, q, k, v, None, scale, causal, fv)
        o1, lse1 = _fwd(ffC, q, k, v, full, scale, causal, fv)
        assert torch.equal(o0, o1) and torch.equal(lse0, lse1), fv
    dq, dk, dv = _bwd(ffC, q, k, v, o1, lse1, do, full, scale, causal, variant)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    o, lse = _ref_attn(qf, kf, vf, full, scale, causal)
    o.backward(do.float())
    ref = dict(o=o.detach(), lse=lse, dq=qf.grad, dk=kf.grad, dv=vf.grad)
    _check_against_ref(f"full lengths S{S} bwd {variant}", dict(o=o1, lse=lse1.view(B, H, S), dq=dq, dk=dk, dv=dv),
                       ref, [S] * B, S)


def test_key_lens_argument_is_checked(ffC):
    q, k, v, do, kl, scale, _ = _case("c")
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, kl[:1], scale, False)  # numel != B
    with pytest.raises(RuntimeError):
        _fwd(ffC, q, k, v, kl.long(), scale, False)  # not int32


# ------------------------------------------------------------------------------------- op level
def _run_mha(dtype, E, H, S, lens, causal=False):
    """MultiHeadAttention with a lengths input through OpCtx on the device (the helper of
    tests/test_ops_cpu.py::run_layer), and fp32 torch on the same weights: relative errors of the
    output, the input gradient and every weight / bias gradient."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B = len(lens)
    g = torch.Generator().manual_seed(9)
    ff = FFModel(FFConfig([]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    tl = ff.create_tensor([B], DataType.DT_INT32)
    L = ff.multihead_attention(tx, tx, tx, E, H, causal=causal, key_lengths=tl).owner_layer
    assert L.attrs["fused_qkv"]
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    x = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    ws = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).to(DEV, dtype) for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims, device=DEV) for w in L.weights]
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    y = L.impl.forward(ctx, [x, x, x, kl], ws)[0]
    dy = torch.randn(B, S, E, generator=g).to(DEV, dtype)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == 4 and dxs[1] is None and dxs[2] is None and dxs[3] is None
    torch.cuda.synchronize()
    # fp32 torch on the same (rounded) weights
    xf = x.float().requires_grad_()
    wf = [w.float().requires_grad_() for w in ws]
    D = E // H
    W, bb = wf[0].reshape(3, H * D, E), wf[1].reshape(3, H * D)
    qq, kk, vv = ((xf @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    o, _ = _ref_attn(qq, kk, vv, kl, 1.0 / math.sqrt(D), causal)
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
def test_mha_op_bf16_key_lengths(ffC, H):
    """bf16 fused self-attention, E = 128, S = 128, B = 4, lengths [128, 70, 64, 3]: head dim 64 (the
    flash kernels on the fused QKV buffer) and head dim 32 (zero-padded to 64)."""
    _, _, errs, _ = _run_mha(torch.bfloat16, 128, H, 128, [128, 70, 64, 3])
    assert errs.pop("y") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


def test_mha_op_fp32_device_key_lengths(ffC):
    """--dtype fp32 on the device (f32 MFMA GEMMs + key-length mask + row softmax), lengths with a 0.
    The path rounds like the fp32 reference (exact f32 products, fp32 sums of <= 128 terms, ~1e-6
    relative): 1e-4 leaves two orders of margin. The empty sample's output rows are the output bias."""
    y, yr, errs, ws = _run_mha(torch.float32, 128, 2, 128, [128, 0, 64, 3])
    assert all(e < 1e-4 for e in errs.values()), errs
    assert torch.equal(y[1], ws[3].expand(128, 128))


# --------------------------------------------------------------------------------- step capture
def _train_bert(flags, with_lens, steps=6):
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(0)
    B, bc = 4, BertConfig.tiny(64)
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    kl = ff.create_tensor([B], DataType.DT_INT32, name="key_lengths") if with_lens else None
    ids, pos, _ = build_bert(ff, B, bc, key_lengths=kl)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    lens = rng.integers(1, bc.seq + 1, N).astype(np.int32)
    tok = rng.integers(1, bc.vocab, (N, bc.seq)).astype(np.int32)
    tok[np.arange(bc.seq)[None, :] >= lens[:, None]] = 0  # right-padded with token 0
    loaders = [ff.create_data_loader(ids, tok),
               ff.create_data_loader(pos, np.tile(np.arange(bc.seq, dtype=np.int32), (N, 1))),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, bc.vocab, (N, bc.seq, 1)).astype(np.int32))]
    if with_lens:
        loaders.append(ff.create_data_loader(kl, lens))
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


def test_bert_key_lengths_train_under_step_capture():
    """bert-tiny (BertConfig.tiny(64), batch 4) with lengths fed by a data loader, hipGraph step
    capture on and off. A step is captured only after three eager warm-up steps, so 6 steps run
    (3 eager, the capture, 2 replays) rather than 3, and the graph must exist. Losses and weights
    agree as tests/test_runtime_gpu.py::test_graph_captures_adam_update asks of captured against
    eager steps (rtol 1e-5, atol 1e-6); the losses differ from the same run without lengths, so the
    input reaches the kernels inside the graph (a run that ignored it would be bit-identical)."""
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
    print("losses without lengths", ld)
    assert np.abs(ld[3:] - lg[3:]).max() > 1e-6, (ld, lg)  # the replayed steps see the lengths
