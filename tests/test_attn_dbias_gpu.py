"""The score-bias gradient kernel (attn_dbias.hip) through kernels.flash_attn_bwd(dbias_out=) against the float64
oracle of attn_rows_common, and through scaled_dot_product_attention(attn_bias_grad=True). Per-element tolerance:
GPU_FACTOR * sum e_ij + ACC * sum |dS_ij| over the reduction set, e_ij = U |dS_ij| + (P + [P = 0] P0)_ij eps_i as
attn_rows_common.bounds() forms it (eps_i: the error of delta_i, inherited from the rounded O)."""
import math

import pytest
import torch

import attn_rows_common as A
from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 3, 4
FMIN = torch.finfo(torch.float32).min


def _c(Sq, Sk, D, ext, Hkv=None, causal=False, lens=None, thr=0, holes=None, offset=0):
    return dict(Sq=Sq, Sk=Sk, D=D, ext=ext, Hkv=Hkv or H, causal=causal, lens=lens, thr=thr, holes=holes, offset=offset)


# ext: the bias extents (Bb, Hb); offset: floats by which the bias and its gradient are shifted off 16-B alignment
CASES = {
    "cross_tile_1H": _c(160, 200, 64, (1, H)),  # both cross the 128 tile, Sk % 32 != 0
    "unaligned_BH": _c(64, 130, 64, (B, H), offset=1),  # the 4-byte store path
    "d128_1H": _c(160, 200, 128, (1, H)),
    "d128_11": _c(64, 130, 128, (1, 1)),
    "gqa_B1": _c(160, 200, 64, (B, 1), Hkv=1),
    "causal_1H": _c(192, 192, 64, (1, H), causal=True),
    "lens_11": _c(160, 200, 64, (1, 1), lens=[0, 70, 200]),
    "drop_1H": _c(160, 200, 64, (1, H), thr=64),
    "neginf_BH": _c(160, 200, 128, (B, H), holes="inf"),
    "finfo_min_1H": _c(160, 200, 64, (1, H), holes="min"),
}


def _run(c, seed):
    Sq, Sk, D, Hkv = c["Sq"], c["Sk"], c["D"], c["Hkv"]
    Bb, Hb = c["ext"]
    g = torch.Generator().manual_seed(seed)
    q, do = 1.7 * torch.randn(B, H, Sq, D, generator=g), torch.randn(B, H, Sq, D, generator=g)
    k, v = 1.7 * torch.randn(B, Hkv, Sk, D, generator=g), torch.randn(B, Hkv, Sk, D, generator=g)
    q, k, v, do = (t.bfloat16() for t in (q, k, v, do))
    bias = torch.randn(Bb, Hb, Sq, Sk, generator=g)
    if c["holes"]:
        hole = float("-inf") if c["holes"] == "inf" else FMIN
        bias[:, :, :, 100:107] = hole
        bias[:, :, :, 3] = hole
        bias[:, :, 5] = hole  # a row that loses every key
    see = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if c["causal"]:
        see &= (torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None])
    if c["lens"]:
        for b, n in enumerate(c["lens"]):
            see[b, :, :, n:] = False
    bref = bias.masked_fill(bias == FMIN, float("-inf"))
    see = see & ~torch.isneginf(bref).expand(B, H, Sq, Sk)
    scale = 1.0 / math.sqrt(D)
    keep, drop, ds = None, None, 256.0 / (256 - c["thr"])
    if c["thr"]:
        keep = K.attn_dropout_keep_ref(A.DROP_SEED, A.DROP_LAYER, A.DROP_STEP, B, H, Sq, Sk, c["thr"] / 256.0)
        drop = (c["thr"], torch.tensor([A.DROP_STEP], dtype=torch.int64, device=DEV),
                K.attn_dropout_seed(A.DROP_SEED, A.DROP_LAYER), 0, 0, H)
    f = lambda t: t.to(DEV).flatten(0, 1)  # noqa: E731
    kx, vx = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    r = A.oracle(f(q), f(kx), f(vx), f(do), f(see), scale, f(bref.expand(B, H, Sq, Sk).contiguous()),
                 None if keep is None else f(keep), ds)
    a_o = torch.einsum("gqk,gkd->gqd", r["P"], f(vx).double().abs())
    eps = ((A.U * (a_o + r["o"].abs()) + A.ACC * a_o) * f(do).double().abs()).sum(-1)
    e = A.U * r["dS"].abs() + (r["P"] + torch.where(r["P"] == 0, r["P0"], torch.zeros_like(r["P"]))) * eps[..., None]
    bdims = [d for d, n in enumerate((Bb, Hb)) if n == 1]  # the dims the bias broadcasts over
    red = lambda t: t.unflatten(0, (B, H)).sum(bdims, keepdim=True) if bdims else t.unflatten(0, (B, H))  # noqa: E731
    ref, tol = red(r["dS"]), A.GPU_FACTOR * red(e) + A.ACC * red(r["dS"].abs())

    lens = torch.tensor(c["lens"], dtype=torch.int32, device=DEV) if c["lens"] else None
    qd, kd_, vd, dod = (t.to(DEV).contiguous() for t in (q, k, v, do))
    qs, ks = [H * Sq * D, Sq * D, D], [Hkv * Sk * D, Sk * D, D]
    n, off = bias.numel(), c["offset"]
    bd = torch.zeros(n + 8, device=DEV)[off:off + n].view(bias.shape).copy_(bias)
    guard = A.GUARD_ROWS * Sk
    obuf = torch.full((n + 2 * guard + 8,), float("nan"), device=DEV)
    out = obuf[guard + off:guard + off + n].view(bias.shape)
    o, dq, dk, dv = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(kd_), torch.empty_like(vd)
    lse = K.flash_attn_fwd(qd, qs, kd_, ks, vd, ks, o, qs, B, H, Sq, Sk, D, scale, c["causal"], key_lens=lens, drop=drop,
                           bias=bd, Hkv=Hkv)
    K.flash_attn_bwd(qd, qs, kd_, ks, vd, ks, o, qs, dod, qs, lse, dq, qs, dk, ks, dv, ks, B, H, Sq, Sk, D, scale,
                     c["causal"], key_lens=lens, drop=drop, bias=bd, Hkv=Hkv, dbias_out=out)
    torch.cuda.synchronize()
    assert bool(obuf[:guard + off].isnan().all()) and bool(obuf[guard + off + n:].isnan().all()), "wrote outside dbias_out"
    return out.clone(), ref, tol


@pytest.mark.parametrize("name", list(CASES))
def test_dbias_kernel_against_float64(ffC, name):
    """Largest err / tol measured on an MI355X: see docs/PERFORMANCE.md 'Score-bias gradient'."""
    got, ref, tol = _run(CASES[name], 100 + list(CASES).index(name))
    err = (got.double() - ref).abs()  # a NaN fails err <= tol
    ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.zeros_like(err)).max().item()
    print(f"dbias {name}: max err/tol {ratio:.3f}, max |ref| {ref.abs().max().item():.3g}")
    # exact zeros wherever P0 = 0 over the whole reduction set (masked keys, dead rows, above the diagonal): the bound
    # is 0 there. (A row with one visible key has ref = 1 * (dP - delta) = 0 too, but delta's error shows: bound eps_i.)
    assert bool((got[tol == 0] == 0).all()) and bool((ref[tol == 0] == 0).all()), "a masked element is not exactly 0"
    assert bool((err <= tol).all()), f"{name}: err / tol = {ratio:.3f}"
    if name == "cross_tile_1H":  # the same bits on every run
        assert torch.equal(got, _run(CASES[name], 100)[0])


@pytest.mark.parametrize("dtype,D,tol", [(torch.bfloat16, 64, 3e-2), (torch.bfloat16, 32, 3e-2), (torch.float32, 64, 1e-4)])
def test_sdpa_bias_grad(ffC, dtype, D, tol):
    """scaled_dot_product_attention(attn_bias_grad=True) through OpCtx, the bias gathered from a [buckets, H] table
    (embedding -> reshape -> transpose, in torch): dq and the table's gradient, the op's bias gradient pushed
    through that chain, against autograd on the fp32 reference graph. bf16 D = 64: the flash kernels; D = 32: heads
    zero-padded to 64; tolerance that of test_sdpa_op_bf16's dq. fp32: attn_f32_bwd, as test_sdpa_op_fp32_device."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    Bq, S = 2, 96
    g = torch.Generator().manual_seed(5)
    ff = FFModel(FFConfig([]))
    ts = [ff.create_tensor([Bq, H, S, D], DataType.DT_FLOAT) for _ in range(3)] + [ff.create_tensor([1, H, S, S], DataType.DT_FLOAT)]
    L = ff.scaled_dot_product_attention(*ts[:3], attn_bias=ts[3], causal=True, attn_bias_grad=True).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    q, k, v, do = (torch.randn(Bq, H, S, D, generator=g).bfloat16().float() for _ in range(4))
    table = torch.randn(17, H, generator=g).bfloat16().float().requires_grad_()
    idx = (torch.arange(S)[:, None] - torch.arange(S)[None, :]).clamp(-8, 8) + 8
    bias = table[idx.reshape(-1)].reshape(1, S, S, H).permute(0, 3, 1, 2)
    L.impl.forward(ctx, [t.to(DEV, dtype) for t in (q, k, v)] + [bias.detach().to(DEV, dtype).contiguous()], [])
    dxs = L.impl.backward(ctx, [do.to(DEV, dtype)])
    assert dxs[3].dtype == dtype and tuple(dxs[3].shape) == tuple(bias.shape)
    gt, = torch.autograd.grad(bias, table, dxs[3].float().cpu(), retain_graph=True)
    qf = q.clone().requires_grad_()
    s = torch.einsum("bhqd,bhkd->bhqk", qf, k) / math.sqrt(D) + bias
    (torch.softmax(s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf")), -1) @ v).backward(do)
    rel = lambda a, b: ((a.float().cpu() - b).norm() / b.norm()).item()  # noqa: E731
    assert rel(dxs[0], qf.grad) < tol and rel(gt, table.grad) < tol
