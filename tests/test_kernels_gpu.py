"""Numerics of the hand-written HIP kernels against plain PyTorch fp32 references (GPU only)."""
import math
import numpy as np

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _gemm(C_, A, B, C, M, N, K, a_k, b_k, bias=None, Z=None, alpha=1.0, beta=0.0, act=10, batch=1, sA=0, sB=0,
          sC=0, splitk=1, ws=None, impl=2):
    lda = A.shape[-1]
    ldb = B.shape[-1]
    ldc = C.shape[-1]
    C_.gemm(A, B, C, bias, Z, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, a_k, b_k, alpha, beta, act, splitk, ws,
            impl)


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(256, 384, 512), (200, 136, 72), (1024, 1024, 1024), (300, 1002, 1030),
                                   (130, 258, 4099), (4096, 1024, 256), (2056, 2000, 192)])
@pytest.mark.parametrize("impl", [6, 2, 1, 0])
def test_gemm_layouts(ffC, a_k, b_k, M, N, K, impl):
    torch.manual_seed(0)
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    _gemm(ffC, A, B, C, M, N, K, a_k, b_k, impl=impl)
    ref = Am.float() @ Bn.float().t()
    assert _rel(C, ref) < 1e-2


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K,splitk", [(8192, 1024, 4096, 1), (8192, 3072, 1024, 2), (1024, 4096, 8192, 4),
                                          (1000, 600, 1056, 1), (2048, 2048, 2048, 3), (3072, 1024, 16384, 5)])
@pytest.mark.parametrize("impl", [6, 2])
def test_gemm256_shapes(ffC, a_k, b_k, M, N, K, splitk, impl):
    """256-row kernels (6: persistent 8-wave ping-pong, uneven split-K slices; 2: gemm256.hip):
    BERT-Large shapes, split-K slabs, edge tiles."""
    torch.manual_seed(11)
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    ref = Am.float() @ Bn.float().t()
    ws = torch.empty(M * N * splitk, device=DEV) if splitk > 1 else None
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    _gemm(ffC, A, B, C, M, N, K, a_k, b_k, splitk=splitk, ws=ws, impl=impl)
    assert _rel(C, ref) < 1e-2
    C32 = torch.ones(M, N, device=DEV)
    _gemm(ffC, A, B, C32, M, N, K, a_k, b_k, beta=1.0, splitk=splitk, ws=ws, impl=impl)
    assert _rel(C32, ref + 1.0) < 1e-3


@pytest.mark.parametrize("impl", [6])
@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(8192, 4096, 1024), (8200, 2056, 512), (16384, 1024, 256), (3000, 1000, 1152),
                                   (2048, 768, 128)])
@pytest.mark.parametrize("out", ["bf16", "f32"])
@pytest.mark.parametrize("bias", [None, "f32", "bf16"])
def test_gemm_persistent(ffC, a_k, b_k, M, N, K, out, bias, impl):
    """Persistent ping-pong GEMM (impl 6, gemm_pp.hip: two wave groups alternating MFMA and memory
    phases over a two-slot BK = 64 ring): several tiles per workgroup, the next tile's DMA in flight
    during the epilogue, edge tiles (rows / columns dropped by the buffer-store range check), bias in
    the epilogue, fp32 / bf16 output; five launches bitwise equal (no race between the epilogue's
    staging image, the ring refill and the next tile's first reads)."""
    torch.manual_seed(5)
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    bv = None
    ref = Am.float() @ Bn.float().t()
    if bias is not None:
        bv = torch.randn(N, device=DEV)
        if bias == "bf16":
            bv = bv.bfloat16()
        ref = ref + bv.float()
    C = torch.full((M, N), 7.0, device=DEV, dtype=torch.float32 if out == "f32" else torch.bfloat16)
    _gemm(ffC, A, B, C, M, N, K, a_k, b_k, bias=bv, impl=impl)
    assert _rel(C, ref) < (1e-3 if out == "f32" else 1e-2)
    first = C.clone()
    for _ in range(4):
        C.fill_(-3.0)
        _gemm(ffC, A, B, C, M, N, K, a_k, b_k, bias=bv, impl=impl)
        assert torch.equal(C, first)


@pytest.mark.parametrize("impl", [6, 2])
@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("M,N,K,splitk", [(512, 512, 512, 1), (512, 512, 512, 2), (1024, 768, 1024, 1)])
def test_gemm_repeat_bitwise(ffC, impl, a_k, b_k, M, N, K, splitk):
    """The inline-asm MFMA kernels pad their hazards by hand (pin_acc + s_nop): a missing pad
    showed as an intermittent wrong 256-column block at 512^3 (round 3, scripts/gemm_race_check.py).
    Twenty launches on fixed inputs: every result bitwise equal to the first and close to fp32."""
    torch.manual_seed(11)
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    ref = Am.float() @ Bn.float().t()
    ws = torch.empty(M * N * splitk, device=DEV) if splitk > 1 else None
    first = None
    for _ in range(20):
        C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        _gemm(ffC, A, B, C, M, N, K, a_k, b_k, splitk=splitk, ws=ws, impl=impl)
        if first is None:
            first = C.clone()
            assert _rel(C, ref) < 1e-2
        else:
            assert torch.equal(C, first)


def test_gemm_epilogue_bias_gelu_f32_beta(ffC):
    torch.manual_seed(1)
    M, N, K = 384, 512, 256
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV)
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    Z = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    _gemm(ffC, A, B, C, M, N, K, True, True, bias=bias, Z=Z, act=14)
    z = A.float() @ B.float().t() + bias
    assert _rel(Z, z) < 1e-2
    assert _rel(C, torch.nn.functional.gelu(z)) < 1e-2
    # fp32 output accumulate (beta=1), alpha scaling
    C32 = torch.randn(M, N, device=DEV)
    base = C32.clone()
    _gemm(ffC, A, B, C32, M, N, K, True, True, alpha=0.5, beta=1.0)
    assert _rel(C32, base + 0.5 * (A.float() @ B.float().t())) < 1e-4


def test_gemm_unaligned_splitk(ffC):
    """vocab-projection-like shapes: odd N / K handled by the element-staged MFMA path (not the
    scalar fallback) including split-K wgrad."""
    torch.manual_seed(9)
    T, V, H = 512, 1002, 256
    dz = torch.randn(T, V, device=DEV).bfloat16()
    x = torch.randn(T, H, device=DEV).bfloat16()
    dW = torch.zeros(V, H, device=DEV)
    ws = torch.empty(V * H * 4, device=DEV)
    _gemm(ffC, dz, x, dW, V, H, T, False, False, beta=1.0, splitk=4, ws=ws)
    assert _rel(dW, dz.float().t() @ x.float()) < 1e-3


def test_gemm_big_splitk_bias(ffC):
    """256x128 LDS-DMA kernel: split-K wgrad and fused bias/GELU epilogue at >=128 tiles."""
    torch.manual_seed(10)
    M, N, K = 1024, 1024, 8192
    dY = torch.randn(K, M, device=DEV).bfloat16()
    X = torch.randn(K, N, device=DEV).bfloat16()
    ws = torch.empty(M * N * 8, device=DEV)
    C = torch.zeros(M, N, device=DEV)
    _gemm(ffC, dY, X, C, M, N, K, False, False, beta=1.0, splitk=8, ws=ws)
    assert _rel(C, dY.float().t() @ X.float()) < 1e-3
    M, N, K = 4096, 2048, 512
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV)
    Cb = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    Z = torch.empty_like(Cb)
    _gemm(ffC, A, B, Cb, M, N, K, True, True, bias=bias, Z=Z, act=14)
    z = A.float() @ B.float().t() + bias
    assert _rel(Z, z) < 1e-2
    assert _rel(Cb, torch.nn.functional.gelu(z)) < 1e-2


def test_gemm_splitk_and_batch(ffC):
    torch.manual_seed(2)
    # wgrad shape: dW[N,K] = dY^T[N,M] X[M,K] with huge reduction dim
    M, N, K = 256, 192, 8192
    dY = torch.randn(K, M, device=DEV).bfloat16()  # [tokens][out]  -> A is [K][M] (M contiguous)
    X = torch.randn(K, N, device=DEV).bfloat16()   # [tokens][in]   -> B is [K][N]
    ws = torch.empty(M * N * 4, device=DEV)
    C = torch.zeros(M, N, device=DEV)
    _gemm(ffC, dY, X, C, M, N, K, False, False, splitk=4, ws=ws)
    assert _rel(C, dY.float().t() @ X.float()) < 1e-3
    # strided batch
    b, M, N, K = 6, 130, 70, 64
    A = torch.randn(b, M, K, device=DEV).bfloat16()
    B = torch.randn(b, N, K, device=DEV).bfloat16()
    C = torch.empty(b, M, N, device=DEV, dtype=torch.bfloat16)
    _gemm(ffC, A, B, C, M, N, K, True, True, batch=b, sA=M * K, sB=N * K, sC=M * N)
    assert _rel(C, torch.bmm(A.float(), B.float().transpose(1, 2))) < 1e-2


_SCATTER_M = 2056
_scatter_cache = {}


def _scatter_case(N, K):
    """Inputs and float64 references of test_gemm_scattered_epilogue, built once per (N, K) and only
    read afterwards: Am [M][K], Bn [N][K] bf16, ab = Am . Bn^T and s = |Am| . |Bn|^T in float64."""
    if (N, K) not in _scatter_cache:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        Am = torch.randn(_SCATTER_M, K, device=DEV, generator=g).bfloat16()
        Bn = torch.randn(N, K, device=DEV, generator=g).bfloat16()
        ab = Am.double() @ Bn.double().t()
        s = Am.double().abs() @ Bn.double().abs().t()
        bias = torch.randn(N, device=DEV, generator=g)
        c0 = torch.randn(_SCATTER_M, N, device=DEV, generator=g)
        _scatter_cache[(N, K)] = (Am, Am.t().contiguous(), Bn, ab, s, bias, c0)
    return _scatter_cache[(N, K)]


def _guarded(M, N, dtype, fill):
    """[M][N] output with ldc = N inside a larger buffer: one guard row before and one after."""
    buf = torch.full(((M + 2) * N,), fill, device=DEV, dtype=dtype)
    return buf, buf[N:(M + 1) * N].view(M, N)


def _guards_intact(buf, M, N, fill):
    return bool((buf[:N] == fill).all()) and bool((buf[(M + 1) * N:] == fill).all())


@pytest.mark.parametrize("a_k,b_k", [(True, True), (False, True)])
@pytest.mark.parametrize("N", [1898, 1900])
@pytest.mark.parametrize("impl", [0, 1, 2])
def test_gemm_scattered_epilogue(ffC, impl, N, a_k, b_k):
    """The scattered epilogue (csrc/kernels/gemm_scatter_epilogue.h, one text shared by gemm.hip,
    gemm_big.hip and gemm256_tile.h) element by element against a float64 reference: a wrong partial
    quad of columns at a tile edge hides inside the Frobenius norms of the other GEMM tests.

    M = 2056 (a multiple of 8, dead rows in the last row tile), N = 1898 (ldc % 4 != 0: no vector
    stores, the last quad of columns partial) and N = 1900 (vector stores, N % 8 == 4: the 256-row
    kernel takes its scattered branch with whole quads); 9 x 15 tiles of 256 x 128 >= the floor of
    gemm_big. Cases: (i) bf16 out, bf16 bias, Z store, GELU; (ii) fp32 out, fp32 bias, alpha 0.5,
    beta 1 over a random C; (iii) fp32 out, split-K 2 with a workspace, beta 1. Outputs without beta
    start as a sentinel, and the guard rows around C and Z (ldc = N, so they are also the columns
    >= N of the neighbouring rows) must keep theirs.

    Tolerances, derived (s = sum_k |a_k| |b_k|): fp32 accumulation of K <= 128 products errs by at
    most K 2^-24 s = 2^-17 s, rounding to bf16 by 2^-9 |ref|; with a factor of two (GELU' <= 1.13)
    fp32 outputs must be within 2^-15 s + 2^-20 |ref| and bf16 outputs within 2^-8 |ref| + 2^-14 s.
    A plain fp32 torch evaluation of the same formulas on the CPU stays inside these bounds (largest
    error / bound over all elements: 0.007 for the fp32 cases, 0.97 for the bf16 case, where a
    round-to-nearest just above a power of two takes all of 2^-8 |ref|), so they are not tighter
    than the arithmetic allows. No element is exempt."""
    M = _SCATTER_M
    SENT = 777.0

    def operands(K):
        Am, At, Bn, ab, s, bias, c0 = _scatter_case(N, K)
        return (Am if a_k else At), Bn, ab, s, bias, c0

    def check(name, got, ref, s, bf16):
        err = (got.double() - ref).abs()
        tol = (2.0 ** -8 * ref.abs() + 2.0 ** -14 * s) if bf16 else (2.0 ** -15 * s + 2.0 ** -20 * ref.abs())
        worst = (err / tol).max().item()
        print(f"{name}: impl {impl} N {N} a_k {a_k}: max err/tol {worst:.3f}, max err {err.max().item():.3e}")
        bad = int((err > tol).sum())
        assert bad == 0, f"{name}: {bad} of {err.numel()} elements outside the bound (worst err/tol {worst:.2f})"

    # (i) bf16 out, bf16 bias, pre-activation store, GELU
    A, B, ab, s, bias, c0 = operands(64)
    bias16 = bias.bfloat16()
    cbuf, C = _guarded(M, N, torch.bfloat16, SENT)
    zbuf, Z = _guarded(M, N, torch.bfloat16, SENT)
    _gemm(ffC, A, B, C, M, N, 64, a_k, b_k, bias=bias16, Z=Z, act=14, impl=impl)
    z_ref = ab + bias16.double()
    check("Z", Z, z_ref, s, True)
    check("gelu", C, 0.5 * z_ref * (1.0 + torch.erf(z_ref / math.sqrt(2.0))), s, True)
    assert _guards_intact(cbuf, M, N, SENT) and _guards_intact(zbuf, M, N, SENT)

    # (ii) fp32 out, fp32 bias, alpha = 0.5, beta = 1 over a random C
    cbuf, C = _guarded(M, N, torch.float32, SENT)
    C.copy_(c0)
    _gemm(ffC, A, B, C, M, N, 64, a_k, b_k, bias=bias, alpha=0.5, beta=1.0, impl=impl)
    check("f32 alpha beta bias", C, 0.5 * ab + c0.double() + bias.double(), s, False)
    assert _guards_intact(cbuf, M, N, SENT)

    # (iii) fp32 out, split-K 2 through a workspace, beta = 1
    A, B, ab, s, bias, c0 = operands(128)
    cbuf, C = _guarded(M, N, torch.float32, SENT)
    C.copy_(c0)
    ws = torch.full((2 * M * N,), SENT, device=DEV)
    _gemm(ffC, A, B, C, M, N, 128, a_k, b_k, beta=1.0, splitk=2, ws=ws, impl=impl)
    check("f32 split-K", C, ab + c0.double(), s, False)
    assert _guards_intact(cbuf, M, N, SENT)


def _attn_ref(q, k, v, scale, causal):
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if causal:
        Sq, Sk = s.shape[-2:]
        mask = torch.ones(Sq, Sk, device=s.device, dtype=torch.bool).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhqk,bhkd->bhqd", p, v), torch.logsumexp(s, -1)


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("S,D,causal", [(512, 64, False), (200, 64, False), (256, 128, False), (384, 64, True),
                                        (640, 64, True), (300, 128, True), (1024, 64, True), (512, 128, False)])
def test_flash_attention(ffC, S, D, causal, variant):
    """Both backward structures (2: attn_bwd_kernel through registers, chained or with dQ slabs;
    10, the default: the one-barrier-per-query-tile attn_bwd1b_kernel chained at B*H >= 256, else
    attn_bwd_kernel with LDS-DMA Q / dO tiles and slabs) against an fp32 PyTorch reference, incl.
    ragged and causal key blocks (B*H = 6 here: the slab forms; the chained forms are covered at
    B*H = 256 by the tests below)."""
    torch.manual_seed(3)
    prev_variant = ffC.attn_bwd_variant()
    ffC.attn_set_bwd_variant(variant)
    B, H = 2, 3
    q = torch.randn(B, H, S, D, device=DEV).bfloat16()
    k = torch.randn(B, H, S, D, device=DEV).bfloat16()
    v = torch.randn(B, H, S, D, device=DEV).bfloat16()
    o = torch.empty_like(q)
    lse = torch.empty(B * H * S, device=DEV)
    st = [H * S * D, S * D, D]
    scale = 1.0 / math.sqrt(D)
    ffC.attn_fwd(q, st, k, st, v, st, o, st, lse, B, H, S, S, D, scale, causal)
    # the forward structures (0: 4 waves, register-staged K/V; 1: 4 waves, LDS-DMA; 3: 64 rows
    # per wave) run the same per-row arithmetic: bitwise equal
    prev_fwd = ffC.attn_fwd_variant()
    for fv in (0, 1, 3):
        ffC.attn_set_fwd_variant(fv)
        o2, lse2 = torch.full_like(o, 3.0), torch.full_like(lse, 3.0)
        ffC.attn_fwd(q, st, k, st, v, st, o2, st, lse2, B, H, S, S, D, scale, causal)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), fv
    ffC.attn_set_fwd_variant(prev_fwd)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    ref, ref_lse = _attn_ref(qf, kf, vf, scale, causal)
    assert _rel(o, ref) < 2e-2
    assert _rel(lse.view(B, H, S), ref_lse) < 1e-3
    do = torch.randn_like(q)
    ref.backward(do.float())
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(ffC.attn_bwd_ws(B, H, S, S, D), device=DEV)
    ffC.attn_bwd(q, st, k, st, v, st, o, st, do, st, lse, dq, st, dk, st, dv, st, ws, B, H, S, S, D, scale, causal)
    assert _rel(dv, vf.grad) < 3e-2
    assert _rel(dk, kf.grad) < 3e-2
    assert _rel(dq, qf.grad) < 3e-2
    ffC.attn_set_bwd_variant(prev_variant)


def test_flash_attention_fwd_cross_lengths(ffC):
    """Forward with Sq != Sk at Sq >= 512: Sq = 577 leaves the 64-rows-per-wave form a last query
    block of 65 rows (one full 64-row wave, one wave with a single row, two empty) and the
    32-rows-per-wave forms one of 65 as well; Sk = 130 ends in a 2-key tile. Non-causal. The three
    forward structures are bitwise equal and match fp32 torch."""
    torch.manual_seed(5)
    B, H, D, Sq, Sk = 1, 2, 64, 577, 130
    q = torch.randn(B, H, Sq, D, device=DEV).bfloat16()
    k = torch.randn(B, H, Sk, D, device=DEV).bfloat16()
    v = torch.randn(B, H, Sk, D, device=DEV).bfloat16()
    sq, sk = [H * Sq * D, Sq * D, D], [H * Sk * D, Sk * D, D]
    scale = 1.0 / math.sqrt(D)
    prev_fwd = ffC.attn_fwd_variant()
    outs = {}
    try:
        for fv in (0, 1, 3):
            ffC.attn_set_fwd_variant(fv)
            o, lse = torch.full_like(q, 3.0), torch.full((B * H * Sq,), 3.0, device=DEV)
            ffC.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, Sq, Sk, D, scale, False)
            outs[fv] = (o, lse)
    finally:
        ffC.attn_set_fwd_variant(prev_fwd)
    for fv in (1, 3):
        assert torch.equal(outs[0][0], outs[fv][0]) and torch.equal(outs[0][1], outs[fv][1]), fv
    ref, ref_lse = _attn_ref(q.float(), k.float(), v.float(), scale, False)
    assert _rel(outs[3][0], ref) < 2e-2
    assert _rel(outs[3][1].view(B, H, Sq), ref_lse) < 1e-3


@pytest.mark.parametrize("thr", [0.0, 3.0, 8.0])
@pytest.mark.parametrize("ramp,causal", [(2.0, False), (-2.0, False), (6.0, True), (0.5, True)])
def test_flash_attention_deferred_max(ffC, thr, ramp, causal):
    """Forward deferred-max rescale (T13): scores ramp by `ramp` nats per 64-key tile, so the running
    max grows past the threshold every few tiles (both the keep branch, with P up to 2^thr, and the
    rescale branch run; ramp < 0: the first tile holds the max, no rescale after it). Output and
    logsumexp against fp32 torch, and the backward from that lse."""
    torch.manual_seed(11)
    prev = ffC.attn_rescale_thr()
    ffC.attn_set_rescale_thr(thr)
    try:
        B, H, S, D = 2, 2, 512, 64
        scale = 0.125
        base = torch.randn(D, device=DEV)
        base = base / base.norm()
        q = (torch.randn(B, H, S, D, device=DEV) * 0.2 + 8.0 * base).bfloat16()
        steps = torch.arange(S, device=DEV, dtype=torch.float32) / 64 * ramp / scale / 8.0
        k = (torch.randn(B, H, S, D, device=DEV) * 0.2 + steps[:, None] * base).bfloat16()
        v = torch.randn(B, H, S, D, device=DEV).bfloat16()
        o = torch.empty_like(q)
        lse = torch.empty(B * H * S, device=DEV)
        st = [H * S * D, S * D, D]
        ffC.attn_fwd(q, st, k, st, v, st, o, st, lse, B, H, S, S, D, scale, causal)
        qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
        ref, ref_lse = _attn_ref(qf, kf, vf, scale, causal)
        assert _rel(o, ref) < 2e-2
        assert _rel(lse.view(B, H, S), ref_lse) < 1e-3
        do = torch.randn_like(q)
        ref.backward(do.float())
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty(ffC.attn_bwd_ws(B, H, S, S, D), device=DEV)
        ffC.attn_bwd(q, st, k, st, v, st, o, st, do, st, lse, dq, st, dk, st, dv, st, ws, B, H, S, S, D, scale, causal)
        assert _rel(dv, vf.grad) < 3e-2
        assert _rel(dq, qf.grad) < 5e-2
    finally:
        ffC.attn_set_rescale_thr(prev)


@pytest.mark.parametrize("variant", [10, 2])
def test_flash_attention_bwd_default_chain(ffC, variant):
    """B*H >= 256 takes the chained backward (no dQ slabs, no finishing pass): BERT-Large attention
    shape with the fused [B,S,3,H,D] projection layout, against fp32 autograd; variant 10 (default,
    attn_bwd1b_kernel) and 2 (attn_bwd_kernel chained, the fallback for unaligned rows)."""
    torch.manual_seed(6)
    B, S, H, D = 16, 512, 16, 64
    assert ffC.attn_bwd_variant() == 10
    ffC.attn_set_bwd_variant(variant)
    qkv = torch.randn(B, S, 3, H, D, device=DEV).bfloat16()
    o = torch.empty(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * H * S, device=DEV)
    sq = [S * 3 * H * D, D, 3 * H * D]
    so = [S * H * D, D, H * D]
    base = qkv.view(-1)
    scale = 0.125
    ffC.attn_fwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, lse, B, H, S, S, D, scale, False)
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    db = dqkv.view(-1)
    ws = torch.empty(ffC.attn_bwd_ws(B, H, S, S, D), device=DEV)
    ffC.attn_bwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, do, so, lse, db, sq, db[H * D:], sq,
                 db[2 * H * D:], sq, ws, B, H, S, S, D, scale, False)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float().requires_grad_() for i in range(3))
    ref, _ = _attn_ref(q, k, v, scale, False)
    ref.backward(do.permute(0, 2, 1, 3).float())
    ffC.attn_set_bwd_variant(10)
    for i, t in enumerate((q, k, v)):
        assert _rel(dqkv[:, :, i].permute(0, 2, 1, 3), t.grad) < 3e-2, i


@pytest.mark.parametrize("S,causal,fused", [(512, False, True), (448, False, True), (512, True, False),
                                             (448, True, False)])
def test_flash_attention_fused_qkv_bias_grad(ffC, S, causal, fused):
    """The chained non-causal backward adds the fused QKV projection's bias gradient (column sums of
    dq / dk / dv, bf16 as stored) into dbias itself and says so; causal: it declines (False) and
    leaves dbias untouched. Against fp32 column sums of the dqkv it wrote."""
    torch.manual_seed(8)
    B, H, D = 16, 16, 64  # B*H >= 256: the chained default path
    qkv = torch.randn(B, S, 3, H, D, device=DEV).bfloat16()
    o = torch.empty(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * H * S, device=DEV)
    sq = [S * 3 * H * D, D, 3 * H * D]
    so = [S * H * D, D, H * D]
    base = qkv.view(-1)
    ffC.attn_fwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, lse, B, H, S, S, D, 0.125, causal)
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    g = dqkv.view(-1)
    n = ffC.attn_bwd_ws(B, H, S, S, D)
    wsg = torch.full((n + 65536,), 7.0, device=DEV)  # a guard band after the workspace
    dbias = torch.full((3 * H * D,), 0.5, device=DEV)
    done = ffC.attn_bwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, do, so, lse, g, sq, g[H * D:], sq,
                        g[2 * H * D:], sq, wsg[:n], B, H, S, S, D, 0.125, causal, dbias)
    assert done == fused
    assert torch.equal(wsg[n:], torch.full_like(wsg[n:], 7.0)), "attn_bwd wrote past its workspace"
    # the chained attn_bwd1b_kernel itself (incl. its causal / ragged forms) against fp32 autograd
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float().requires_grad_() for i in range(3))
    ref, _ = _attn_ref(q, k, v, 0.125, causal)
    ref.backward(do.permute(0, 2, 1, 3).float())
    for i, t in enumerate((q, k, v)):
        assert _rel(dqkv[:, :, i].permute(0, 2, 1, 3), t.grad) < 3e-2, i
    if fused:
        ref = dqkv.float().sum(dim=(0, 1)).reshape(-1) + 0.5
        assert torch.allclose(dbias, ref, rtol=1e-4, atol=1e-2), (dbias - ref).abs().max()
    else:
        assert torch.equal(dbias, torch.full_like(dbias, 0.5))


def test_flash_attention_strided_qkv(ffC):
    """Q/K/V read straight out of a fused [B,S,3,H,D] projection, O written as [B,S,H,D]."""
    torch.manual_seed(4)
    B, S, H, D = 2, 256, 4, 64
    qkv = torch.randn(B, S, 3, H, D, device=DEV).bfloat16()
    o = torch.empty(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B * H * S, device=DEV)
    sq = [S * 3 * H * D, D, 3 * H * D]
    so = [S * H * D, D, H * D]
    base = qkv.view(-1)
    ffC.attn_fwd(base, sq, base[H * D:], sq, base[2 * H * D:], sq, o, so, lse, B, H, S, S, D, 0.125, False)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float() for i in range(3))
    ref, _ = _attn_ref(q, k, v, 0.125, False)
    assert _rel(o.permute(0, 2, 1, 3), ref) < 2e-2


@pytest.mark.parametrize("cols,rows", [(1024, 300), (768, 300), (100, 300), (1024, 8200), (1024, 16384)])
def test_layernorm(ffC, cols, rows):
    torch.manual_seed(5)
    x = torch.randn(rows, cols, device=DEV).bfloat16()
    r = torch.randn(rows, cols, device=DEV).bfloat16()
    g = torch.randn(cols, device=DEV).bfloat16()
    b = torch.randn(cols, device=DEV).bfloat16()
    y = torch.empty_like(x)
    s = torch.empty_like(x)
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    ffC.layernorm_fwd(x, r, s, g, b, y, mean, rstd, rows, cols, 1e-5)
    xs = (x.float() + r.float()).requires_grad_()
    gf, bf = g.float().requires_grad_(), b.float().requires_grad_()
    ref = torch.nn.functional.layer_norm(xs, (cols,), gf, bf, 1e-5)
    assert _rel(y, ref) < 1e-2
    dy = torch.randn_like(x)
    ref.backward(dy.float())
    dx = torch.empty_like(x)
    dg = torch.zeros(cols, device=DEV)
    db = torch.zeros(cols, device=DEV)
    ffC.layernorm_bwd(dy, s, g, mean, rstd, dx, None, dg, db, rows, cols, False)
    assert _rel(dx, xs.grad) < 2e-2
    assert _rel(dg, gf.grad) < 2e-2
    assert _rel(db, bf.grad) < 1e-2
    # fused bias gradient of the producing Linear: dsum += colsum(dx), same launch (plus dgamma/dbeta
    # accumulate again on top of the first call's values)
    dsum = torch.full((cols,), 0.5, device=DEV)
    dx2 = torch.empty_like(x)
    ffC.layernorm_bwd(dy, s, g, mean, rstd, dx2, None, dg, db, rows, cols, False, dsum)
    assert torch.equal(dx2, dx)
    assert _rel(dsum - 0.5, dx.float().sum(0)) < 5e-3  # kernel sums the fp32 values before bf16 rounding
    assert _rel(db, 2 * bf.grad) < 1e-2


@pytest.mark.parametrize("cols", [1024, 4096, 30528, 1000])
def test_col_fold_two_level_deterministic(ffC, cols):
    """The bias-gradient column fold of a BERT-Large-sized gradient (16384 rows: 512 slab rows,
    two-level deterministic fold with a last-arriving-block finish) against fp32 torch, and
    bitwise equal over repeated calls (no float atomics, fixed summation order)."""
    torch.manual_seed(8)
    rows = 16384
    dy = torch.randn(rows, cols, device=DEV).bfloat16()
    ref = dy.float().sum(0)
    outs = []
    for _ in range(4):
        db = torch.full((cols,), 0.25, device=DEV)
        ffC.bias_act_bwd(dy, None, None, db, rows, cols, 10)
        outs.append(db.clone())
    assert _rel(outs[0] - 0.25, ref) < 1e-4
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_softmax_and_xent(ffC):
    torch.manual_seed(6)
    rows, cols = 257, 1000
    x = torch.randn(rows, cols, device=DEV)
    y = torch.empty_like(x)
    ffC.softmax_fwd(x, y, rows, cols, 1.0)
    assert _rel(y, torch.softmax(x, -1)) < 1e-5
    dy = torch.randn_like(x)
    dx = torch.empty_like(x)
    ffC.softmax_bwd(y, dy, dx, rows, cols, 1.0, False)
    xr = x.clone().requires_grad_()
    torch.softmax(xr, -1).backward(dy)
    assert _rel(dx, xr.grad) < 1e-4
    labels = torch.randint(0, cols, (rows,), device=DEV, dtype=torch.int32)
    loss = torch.empty(rows, device=DEV)
    dl = torch.empty_like(x)
    ffC.softmax_xent(x, labels, loss, dl, rows, cols, 1.0 / rows)
    xr = x.clone().requires_grad_()
    ref = torch.nn.functional.cross_entropy(xr, labels.long())
    ref.backward()
    assert abs(loss.mean().item() - ref.item()) < 1e-4
    assert _rel(dl, xr.grad) < 1e-4


@pytest.mark.parametrize("cols", [30522, 1001, 64, 8192, 16386, 32768])
def test_softmax_xent_bf16_metrics(ffC, cols):
    """Fused softmax-xent on bf16 logits whose rows start at every 4-B offset (odd vocab), with the
    accuracy / CE metrics folded into the same pass."""
    torch.manual_seed(16)
    rows = 203
    x = (torch.randn(rows, cols, device=DEV) * 3).bfloat16()
    labels = torch.randint(0, cols, (rows,), device=DEV, dtype=torch.int32)
    labels[::7] = x[::7].float().argmax(-1).int()
    loss = torch.empty(rows, device=DEV)
    dl = torch.empty_like(x)
    acc3 = torch.zeros(3, device=DEV)
    ffC.softmax_xent(x, labels, loss, dl, rows, cols, 1.0 / rows, acc3)
    xr = x.float().requires_grad_()
    ref = torch.nn.functional.cross_entropy(xr, labels.long(), reduction="none")
    ref.sum().backward()
    assert _rel(loss, ref) < 1e-3
    assert _rel(dl.float() * rows, xr.grad) < 1e-2
    assert acc3[0].item() == (x.float().argmax(-1) == labels.long()).sum().item()
    assert abs(acc3[1].item() - ref.sum().item()) < 1e-3 * ref.sum().item()
    assert acc3[2].item() == rows


@pytest.mark.parametrize("rows,cols,act", [(8192, 1024, 10), (8192, 4096, 14), (300, 30522, 10), (77, 1000, 12),
                                           (4096, 520, 11)])
def test_bias_act_bwd(ffC, rows, cols, act):
    torch.manual_seed(17)
    dy = torch.randn(rows, cols, device=DEV).bfloat16()
    z = torch.randn(rows, cols, device=DEV).bfloat16()
    db = torch.ones(cols, device=DEV)
    if act == 10:
        ffC.bias_act_bwd(dy, None, None, db, rows, cols, act)
        dz_ref = dy.float()
    else:
        dz = torch.empty_like(dy)
        ffC.bias_act_bwd(dy, z, dz, db, rows, cols, act)
        from flexflow_amd.kernels import act_grad_ref
        dz_ref = dy.float() * act_grad_ref(z.float(), act)
        assert _rel(dz, dz_ref) < 1e-2
    assert _rel(db, 1.0 + dz_ref.sum(0)) < 1e-3


@pytest.mark.parametrize("a_k,b_k", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(512, 1024, 256), (300, 136, 72), (1000, 4096, 1024), (256, 200, 64)])
@pytest.mark.parametrize("act", [14, 11, 15])  # GELU, RELU, stored act' (GRADMUL)
@pytest.mark.parametrize("impl", [2, 6])
def test_gemm_dact(ffC, a_k, b_k, M, N, K, act, impl):
    """Consumer dgrad GEMM with the producer's act' and bias-gradient column sums in the epilogue
    (impl 2: gemm256.hip dact mode; impl 6: gemm_pp.hip DACT epilogue, dgrad layout only) against
    fp32 torch."""
    from flexflow_amd.kernels import act_grad_ref
    torch.manual_seed(3)
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    z = torch.randn(M, N, device=DEV).bfloat16()
    C = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
    db = torch.ones(N, device=DEV)
    ok = ffC.gemm_dact(A, B, C, z, db, M, N, K, A.shape[-1], B.shape[-1], N, a_k, b_k, act, impl)
    if impl == 6:  # the ping-pong kernel's DACT epilogue: stored act' (GRADMUL), dgrad layout
        assert ok == (act == 15 and a_k and not b_k and N % 8 == 0 and K % 64 == 0)
    else:
        assert ok == (N % 8 == 0 and K % 64 == 0 and (a_k or M % 8 == 0))
    if not ok:
        return
    ref = (Am.float() @ Bn.float().t()) * act_grad_ref(z.float(), act)
    assert _rel(C, ref) < 1e-2
    assert _rel(db, 1.0 + ref.sum(0)) < 1e-2


def test_gemm_dact_dispatch_matches_unfused():
    """kernels.gemm_dact's autotuned choice and its GEMM + in-place bias_act_bwd alternative agree."""
    from flexflow_amd import kernels as K
    torch.manual_seed(4)
    M, N, Kd = 768, 512, 256
    dy = torch.randn(M, Kd, device=DEV).bfloat16()
    w = torch.randn(Kd, N, device=DEV).bfloat16()
    z = torch.randn(M, N, device=DEV).bfloat16()
    outs = []
    for fused in ("fused_pp", "fused", "unfused"):
        K._tuned[("dact", M, N, Kd, True, False, Kd, N, N, 14, True)] = fused
        C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        db = torch.zeros(N, device=DEV)
        K.gemm_dact(dy, w, C, z, db, M, N, Kd, True, False, Kd, N, N, 14)
        outs.append((C.float(), db))
    for o in outs[:2]:
        assert _rel(o[0], outs[2][0]) < 1e-2
        assert _rel(o[1], outs[2][1]) < 1e-2


def test_adam_sgd_embedding_dropout(ffC):
    torch.manual_seed(7)
    n = 10001
    w = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    low = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    w0 = w.clone()
    ffC.adam_update(w, g, m, v, low, 1e-3, 0.9, 0.999, 0.0, 1e-8, 1.0)
    mr = 0.1 * g
    vr = 0.001 * g * g
    assert _rel(w, w0 - 1e-3 * mr / (vr.sqrt() + 1e-8)) < 1e-6
    assert _rel(low, w) < 1e-2
    mom = torch.zeros(n, device=DEV)
    w1 = w.clone()
    ffC.sgd_update(w, g, mom, None, 0.1, 0.9, False, 0.0, 1.0)
    assert _rel(w, w1 - 0.1 * g) < 1e-6
    # embedding bag sum
    table = torch.randn(100, 64, device=DEV).bfloat16()
    idx = torch.randint(0, 100, (32, 3), device=DEV, dtype=torch.int64)
    out = torch.empty(32, 64, device=DEV, dtype=torch.bfloat16)
    ffC.embedding_fwd(idx, table, out, 32, 3, 64, False)
    assert _rel(out, table.float()[idx].sum(1)) < 1e-2
    dt = torch.zeros(100, 64, device=DEV)
    dout = torch.randn(32, 64, device=DEV).bfloat16()
    ffC.embedding_bwd(idx, dout, dt, 32, 3, 64, False)
    ref = torch.zeros(100, 64, device=DEV).index_add_(0, idx.view(-1), dout.float().repeat_interleave(3, 0))
    assert _rel(dt, ref) < 1e-5
    # dropout keeps ~(1-rate) and rescales
    x = torch.ones(1 << 16, device=DEV)
    y = torch.empty_like(x)
    mask = torch.empty(x.numel(), device=DEV, dtype=torch.uint8)
    ffC.dropout_fwd(x, y, mask, 0.25, 1234, 0)
    keep = mask.float().mean().item()
    assert abs(keep - 0.75) < 0.01
    assert torch.allclose(y[mask.bool()], torch.full_like(y[mask.bool()], 1 / 0.75))


@pytest.mark.parametrize("act,with_bias,with_z", [(14, True, True), (11, False, True), (10, True, False)])
def test_lib_gemm_bias_act_epilogue(ffC, act, with_bias, with_z):
    """Library GEMM + our fused bias/activation pass (the tuner's 'lib_act' candidate) and the
    autotuned wrapper agree with the fp32 reference."""
    from flexflow_amd import kernels as Kn
    torch.manual_seed(12)
    M, N, K = 512, 384, 256
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV) if with_bias else None
    z = A.float() @ B.float().t() + (bias if with_bias else 0.0)
    ref = Kn.act_ref(z, act)
    for fn in ("lib_act", "tuned"):
        C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        Z = torch.empty_like(C) if with_z else None
        if fn == "lib_act":
            Kn._lib_gemm_act(A, B, C, Z, M, N, K, True, True, K, K, bias, act)
        else:
            Kn.gemm(A, B, C, M, N, K, True, True, K, K, N, bias=bias, Z=Z, act=act)
        assert _rel(C, ref) < 1e-2
        if with_z:
            assert _rel(Z, z) < 1e-2


@pytest.mark.parametrize("a_k,b_k", [(False, False), (True, True), (True, False)])
@pytest.mark.parametrize("S,beta", [(2, 0.0), (4, 1.0), (8, 1.0)])
def test_lib_splitk_wgrad(ffC, a_k, b_k, S, beta):
    """Split-K library GEMM (S K-slices in one strided-batched GEMM, fp32 slabs) + slab_sum, fp32
    out with beta accumulate: the weight-gradient path, against an fp32 reference."""
    from flexflow_amd import kernels as K
    M, N, Kd = 768, 512, 8192
    g = torch.Generator(device=DEV).manual_seed(0)
    A = (torch.randn(M, Kd, device=DEV, generator=g) if a_k else torch.randn(Kd, M, device=DEV, generator=g)).bfloat16()
    B = (torch.randn(N, Kd, device=DEV, generator=g) if b_k else torch.randn(Kd, N, device=DEV, generator=g)).bfloat16()
    C = torch.randn(M, N, device=DEV, generator=g)
    Af = A.float() if a_k else A.float().t()
    Bf = B.float().t() if b_k else B.float()
    ref = Af @ Bf + beta * C
    K._lib_gemm_splitk(A, B, C, M, N, Kd, a_k, b_k, A.shape[-1], B.shape[-1], beta, S)
    assert _rel(C, ref) < 2e-3


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("out_f32,beta,with_bias", [(False, 0.0, False), (False, 0.0, True), (True, 1.0, False),
                                                    (False, 1.0, False)])
def test_hipblaslt_direct(ffC, a_k, b_k, out_f32, beta, with_bias):
    """Direct hipBLASLt plans (csrc/kernels/blaslt.cpp): every candidate the tuner may pick computes
    the same GEMM (row-major <-> column-major mapping, bias epilogue, beta accumulate, fp32 out)."""
    from flexflow_amd import kernels as Kn
    torch.manual_seed(3)
    M, N, K = 640, 384, 320
    Am = torch.randn(M, K, device=DEV).bfloat16()
    Bn = torch.randn(N, K, device=DEV).bfloat16()
    A = Am if a_k else Am.t().contiguous()
    B = Bn if b_k else Bn.t().contiguous()
    bias = torch.randn(N, device=DEV).bfloat16() if with_bias else None
    C0 = torch.randn(M, N, device=DEV).to(torch.float32 if out_f32 else torch.bfloat16)
    ref = Am.float() @ Bn.float().t() + beta * C0.float() + (bias.float() if with_bias else 0.0)
    C = C0.clone()
    pid, n = Kn._lt_plan(A, B, C, M, N, K, a_k, b_k, A.shape[-1], B.shape[-1], N, 1, 0, 0, 0, bias, beta,
                         Kn.EPI_BIAS if with_bias else Kn.EPI_NONE, max_algos=64)
    assert n > 0
    for a in sorted({0, n // 2, n - 1}):
        C.copy_(C0)
        Kn._lt_run(pid, a, A, B, C, bias, 1.0, beta)
        assert _rel(C, ref) < 1e-2, (a, ffC.lt_algo_name(pid, a))


def test_hipblaslt_splitk_and_tuned_choice(ffC):
    """Split-K strided-batched hipBLASLt GEMM into fp32 slabs + slab_sum (weight-gradient form), and
    gemm()'s autotuner with the hipBLASLt candidates enabled on a BERT-shaped wgrad."""
    from flexflow_amd import kernels as Kn
    g = torch.Generator(device=DEV).manual_seed(1)
    M, N, Kd, S = 1024, 768, 8192, 4
    A = torch.randn(Kd, M, device=DEV, generator=g).bfloat16()   # dz^T layout: a_k = False
    B = torch.randn(Kd, N, device=DEV, generator=g).bfloat16()   # x layout: b_k = False
    C0 = torch.randn(M, N, device=DEV, generator=g)
    ref = A.float().t() @ B.float() + C0
    kc = Kd // S
    slabs = torch.empty((S, M, N), device=DEV, dtype=torch.float32)
    pid, n = Kn._lt_plan(A, B, slabs, M, N, kc, False, False, M, N, N, S, kc * M, kc * N, M * N, None, 0.0,
                         Kn.EPI_NONE, max_algos=16)
    assert n > 0
    C = C0.clone()
    Kn._lt_splitk(pid, 0, A, B, C, M, N, S, 1.0)
    assert _rel(C, ref) < 2e-3
    C = C0.clone()
    Kn.gemm(A, B, C, M, N, Kd, False, False, M, N, N, beta=1.0)
    assert _rel(C, ref) < 2e-3


@pytest.mark.parametrize("cl", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape,relu", [((8, 64, 14, 14), True), ((3, 5, 7, 9), False), ((3, 3, 1, 1), True),
                                        ((64, 16, 32, 32), False), ((4, 200, 9, 9), True), ((2, 512, 7, 7), False)])
def test_batchnorm(shape, relu, dtype, cl, monkeypatch):
    """HIP batch norm (split Welford statistics, fused ReLU) against torch's fp32 batch_norm:
    output, running statistics, and dx / dgamma / dbeta. cl: bf16 tensors with C % 8 == 0 take the
    channel-last kernels (column reductions over [N*H*W][C])."""
    from flexflow_amd import kernels as K
    monkeypatch.setattr(K, "CHANNELS_LAST", cl)
    torch.manual_seed(21)
    N, C = shape[:2]
    x = (torch.randn(shape, device=DEV) * 2 + 3).to(dtype)  # offset mean: Welford, not sum-of-squares
    g = (torch.rand(C, device=DEV) + 0.5).to(dtype)
    b = torch.randn(C, device=DEV).to(dtype)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, mean, rstd = K.batchnorm_fwd(x, g, b, rm, rv, True, relu)
    assert K.is_nhwc(y) == (K.cl_ok(x, C) or K.is_nhwc(x))
    xr, gr, br = (t.float().requires_grad_() for t in (x, g, b))
    rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    ref = torch.nn.functional.batch_norm(xr, rm2, rv2, gr, br, training=True, momentum=0.1, eps=1e-5)
    if relu:
        ref = torch.relu(ref)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    assert _rel(y, ref) < tol
    assert _rel(rm, rm2) < 1e-5 and _rel(rv, rv2) < 1e-5
    dy = torch.randn(shape, device=DEV).to(dtype)
    ref.backward(dy.float())
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = K.batchnorm_bwd(x, dy, g, b, mean, rstd, dg, db, relu)
    assert _rel(dx, xr.grad) < (3e-2 if dtype == torch.bfloat16 else 1e-4)
    assert _rel(dg, gr.grad) < 1e-3 and _rel(db, br.grad) < 1e-3
    # inference: running statistics
    y2, _, _ = K.batchnorm_fwd(x, g, b, rm, rv, False, relu)
    ref2 = torch.nn.functional.batch_norm(x.float(), rm, rv, g.float(), b.float(), training=False, eps=1e-5)
    assert _rel(y2, torch.relu(ref2) if relu else ref2) < tol


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k,s,p,is_max,inc,relu", [(3, 2, 1, True, True, False), (2, 2, 0, True, True, True),
                                                   (3, 1, 1, False, True, False), (3, 2, 1, False, False, True),
                                                   (5, 3, 2, False, False, False), (3, 2, 0, True, True, True)])
def test_pool2d(k, s, p, is_max, inc, relu, dtype):
    """HIP max / average pooling (+ReLU) forward and backward against torch (fp32 reference)."""
    from flexflow_amd import kernels as K
    torch.manual_seed(22)
    x = torch.randn(4, 6, 17, 15, device=DEV).to(dtype)
    y, idx = K.pool2d_fwd(x, k, k, s, s, (p, p, p, p), is_max, inc, relu, True)
    xr = x.float().requires_grad_()
    ref = K._pool_ref(xr, k, k, s, s, (p, p, p, p), is_max, inc, relu)
    assert y.shape == ref.shape
    assert _rel(y, ref) < (1e-2 if dtype == torch.bfloat16 else 1e-6)
    dy = torch.randn_like(ref).to(dtype)
    ref.backward(dy.float())
    dx = K.pool2d_bwd(x, y, dy, idx, k, k, s, s, (p, p, p, p), is_max, inc, relu)
    assert _rel(dx, xr.grad) < (1e-2 if dtype == torch.bfloat16 else 1e-6)


@pytest.mark.parametrize("cl", [True, False])
@pytest.mark.parametrize("shape,k,s,p,is_max", [((8, 32, 35, 35), 3, 1, 1, False),   # Inception A/C/E pools
                                                 ((4, 16, 147, 147), 3, 2, 0, True),  # Inception stem
                                                 ((2, 3, 64, 48), 3, 3, 1, True),
                                                 ((1, 2, 260, 260), 2, 1, 0, False),  # plane past LDS: fallback
                                                 ((1, 2, 260, 260), 2, 1, 0, True)])
def test_pool2d_planes(shape, k, s, p, is_max, cl, monkeypatch):
    """Large-plane pooling: the LDS plane-staged backward (several planes per workgroup) and the
    memory-gather fallback for planes too large for LDS (NCHW), or the channel-last kernels (cl,
    C % 8 == 0), against torch fp32."""
    from flexflow_amd import kernels as K
    monkeypatch.setattr(K, "CHANNELS_LAST", cl)
    torch.manual_seed(24)
    x = torch.randn(*shape, device=DEV).bfloat16()
    y, idx = K.pool2d_fwd(x, k, k, s, s, (p, p, p, p), is_max, True, False, True)
    xr = x.float().requires_grad_()
    ref = K._pool_ref(xr, k, k, s, s, (p, p, p, p), is_max, True, False)
    assert _rel(y, ref) < 1e-2
    dy = torch.randn_like(ref).bfloat16()
    ref.backward(dy.float())
    dx = K.pool2d_bwd(x, y, dy, idx, k, k, s, s, (p, p, p, p), is_max, True, False)
    assert _rel(dx, xr.grad) < 1e-2


@pytest.mark.parametrize("is_max,inc", [(True, True), (False, True), (False, False)])
def test_pool2d_asymmetric_pads(is_max, inc):
    """A spatially split block pads only its global edges: (top, bottom, left, right) pads."""
    from flexflow_amd import kernels as K
    torch.manual_seed(23)
    x = torch.randn(2, 3, 9, 8, device=DEV)
    pads = (1, 0, 0, 1)
    y, idx = K.pool2d_fwd(x, 3, 3, 2, 2, pads, is_max, inc, False, True)
    xr = x.clone().requires_grad_()
    ref = K._pool_ref(xr, 3, 3, 2, 2, pads, is_max, inc, False)
    assert _rel(y, ref) < 1e-6
    dy = torch.randn_like(ref)
    ref.backward(dy)
    assert _rel(K.pool2d_bwd(x, y, dy, idx, 3, 3, 2, 2, pads, is_max, inc, False), xr.grad) < 1e-6


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("geo", [
    # N, C, H, W, K, (kh, kw), (sh, sw), (ph, pw), groups
    (2, 3, 32, 32, 16, (3, 3), (1, 1), (1, 1), 1),
    (2, 3, 63, 63, 64, (11, 11), (4, 4), (2, 2), 1),   # AlexNet conv1 shape class
    (4, 64, 14, 14, 128, (3, 3), (2, 2), (1, 1), 1),
    (2, 256, 7, 7, 64, (1, 1), (1, 1), (0, 0), 1),
    (2, 32, 9, 9, 64, (3, 3), (1, 1), (1, 1), 4),
    (3, 20, 11, 13, 36, (5, 3), (2, 1), (2, 1), 1),
    (1, 130, 17, 17, 200, (1, 7), (1, 1), (0, 3), 1),   # Inception 1x7, channels past one tile
    (2, 192, 35, 35, 64, (1, 1), (1, 1), (0, 0), 1),   # Inception A 1x1: 3 channel tiles, odd HW
    (2, 64, 16, 16, 64, (3, 3), (1, 1), (1, 1), 32),   # ResNeXt grouped 3x3: Cp = 8 per group
    (2, 256, 8, 8, 128, (1, 1), (1, 1), (0, 0), 2),    # grouped 1x1, 128 channels per group: no pack pass
    # stride-phase backward-data: phases without taps (1x1 s2), odd extents, the 7x7 s2 stem, grouped
    (2, 128, 15, 15, 256, (1, 1), (2, 2), (0, 0), 1),
    (2, 96, 17, 17, 96, (3, 3), (2, 2), (0, 0), 1),
    (2, 3, 40, 40, 64, (7, 7), (2, 2), (3, 3), 1),
    (2, 64, 14, 14, 64, (3, 3), (2, 2), (1, 1), 32),
])
def test_conv2d_implicit_gemm(geo, layout, monkeypatch):
    """Our implicit-GEMM MFMA convolution (forward with bias + ReLU, backward data, backward filter
    through float atomics) against fp32 torch autograd on the same bf16 inputs; nhwc: channel-last
    activations read in place (channels per group % 8 == 0, else staged) and channel-last outputs
    through the LDS epilogue (output channels per group % 8 == 0)."""
    from flexflow_amd import kernels as K
    monkeypatch.setattr(K, "CHANNELS_LAST", layout == "nhwc")
    torch.manual_seed(31)
    N, C, H, W, Ko, (kh, kw), st, pad, G = geo
    x = torch.randn(N, C, H, W, device=DEV).bfloat16()
    x = K.cl_dense(x, K.cl_ok(x, C // G))
    w = (torch.randn(Ko, C // G, kh, kw, device=DEV) / math.sqrt(C // G * kh * kw)).bfloat16()
    b = torch.randn(Ko, device=DEV).bfloat16()
    g = K.conv_geometry(x, w, st, pad, G)
    y_nhwc = K.cl_ok(x, Ko // G)
    y = K._conv_ours_fwd(x, w, b, g, True, y_nhwc)
    assert K.is_nhwc(y) == y_nhwc or y.is_contiguous()
    xr, wr, br = (t.float().requires_grad_() for t in (x, w, b))
    ref = torch.relu(torch.nn.functional.conv2d(xr, wr, br, st, pad, 1, G))
    assert y.shape == ref.shape
    assert _rel(y, ref) < 1e-2
    dy = torch.randn_like(ref).bfloat16()
    ref.backward(dy.float())
    dz = K.conv_bias_relu_bwd(dy, y, None)
    dz = K.cl_dense(dz, K.cl_ok(dz, Ko // G))
    dx = torch.empty_like(x)
    dw = torch.zeros(w.shape, device=DEV)
    K._conv_ours_bwd(x, w, dz, g, dx, dw)
    assert _rel(dx, xr.grad) < 1.5e-2
    assert _rel(dw, wr.grad) < 1e-2
    # the backward-data operand packed by the forward's pack launch: the same dgrad, bitwise
    wpb = torch.empty(K.ext().conv_wpack(g), device=DEV, dtype=torch.bfloat16)
    y2 = K._conv_ours_fwd(x, w, b, g, True, y_nhwc, wpb)
    assert torch.equal(y2, y)
    dx2 = torch.empty_like(x)
    K._conv_ours_bwd(x, w, dz, g, dx2, None, False, wpb)
    assert torch.equal(dx2, dx)
    # dgrad accumulating into an existing gradient (a tensor with several consumers)
    acc0 = torch.randn_like(x)
    acc = acc0.clone()
    K._conv_ours_bwd(x, w, dz, g, acc, None, True)
    assert _rel(acc, acc0.float() + xr.grad) < 1.5e-2
    db = torch.zeros(Ko, device=DEV)
    K.conv_bias_relu_bwd(dy, y, db)
    assert _rel(db, br.grad) < 1e-3


@pytest.mark.parametrize("N,C,H,W,Ko", [(2, 64, 14, 14, 256), (4, 512, 7, 7, 128), (1, 256, 5, 3, 64)])
def test_conv_pointwise_gemm(N, C, H, W, Ko):
    """1x1 stride-1 convolutions over channel-last tensors as plain GEMMs over the pixel rows (the
    conv pick's "gemm" candidate): forward with bias + ReLU, backward data (also accumulating into an
    existing gradient) and backward filter (fp32, +=) against fp32 torch autograd."""
    from flexflow_amd import kernels as K
    torch.manual_seed(37)
    x = K.cl_dense(torch.randn(N, C, H, W, device=DEV).bfloat16(), True)
    w = (torch.randn(Ko, C, 1, 1, device=DEV) / math.sqrt(C)).bfloat16()
    b = torch.randn(Ko, device=DEV).bfloat16()
    g = K.conv_geometry(x, w, (1, 1), (0, 0), 1)
    assert K._pointwise_gemm_ok(g, x)
    y = K._conv_gemm_fwd(x, w, b, g, True)
    assert K.is_nhwc(y)
    xr, wr, br = (t.float().requires_grad_() for t in (x, w, b))
    ref = torch.relu(torch.nn.functional.conv2d(xr, wr, br))
    assert _rel(y, ref) < 1e-2
    dy = K.cl_dense(torch.randn_like(ref).bfloat16(), True)
    ref.backward(dy.float() * (ref > 0).float())
    dz = K.cl_dense((dy.float() * (y.float() > 0).float()).bfloat16(), True)
    dx = torch.empty_like(x)
    dw = torch.ones(w.shape, device=DEV)
    K._conv_gemm_bwd(x, w, dz, g, dx, dw)
    assert _rel(dx, xr.grad) < 1.5e-2
    assert _rel(dw - 1.0, wr.grad) < 1e-2
    acc0 = K.cl_dense(torch.randn_like(x), True)
    acc = acc0.clone()
    K._conv_gemm_bwd(x, w, dz, g, acc, None, True)
    assert _rel(acc, acc0.float() + xr.grad) < 1.5e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,d", [(300, 512), (64, 4096), (33, 100), (8, 8192)])
def test_rmsnorm(rows, d, dtype):
    """HIP RMS norm forward / backward (dx, fp32 dw) against fp32 torch autograd."""
    from flexflow_amd import kernels as K
    torch.manual_seed(41)
    x = torch.randn(rows, d, device=DEV).to(dtype)
    w = (torch.rand(d, device=DEV) + 0.5).to(dtype)
    y, rstd = K.rmsnorm_fwd(x, w, 1e-6)
    xr, wr = x.float().requires_grad_(), w.float().requires_grad_()
    ref = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * wr
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-5
    assert _rel(y, ref) < tol
    dy = torch.randn(rows, d, device=DEV).to(dtype)
    ref.backward(dy.float())
    dw = torch.zeros(d, device=DEV)
    dx = K.rmsnorm_bwd(x, w, dy, rstd, dw)
    assert _rel(dx, xr.grad) < (2e-2 if dtype == torch.bfloat16 else 1e-5)
    assert _rel(dw, wr.grad) < 1e-3


@pytest.mark.parametrize("cl", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (64, 32, 35, 35), (2, 3, 1, 1), (16, 48, 17, 17), (1, 7, 64, 64),
                                   (8, 768, 17, 17)])
def test_chan_sum_relu_mask(shape, cl, monkeypatch):
    """Per-channel bias gradient with the ReLU mask (chan_sum_kernel: 4 loads in flight per lane,
    incremental (image, pixel) indexing across odd planes and the tail; cl: the channel-last
    column reduction) against torch."""
    from flexflow_amd import kernels as K
    monkeypatch.setattr(K, "CHANNELS_LAST", cl)
    torch.manual_seed(43)
    dy = torch.randn(*shape, device=DEV).bfloat16()
    y = torch.randn(*shape, device=DEV).bfloat16()
    db = torch.full((shape[1],), 0.5, device=DEV)
    dz = K.conv_bias_relu_bwd(dy, y, db)
    ref = dy.float() * (y.float() > 0)
    assert torch.equal(dz.float(), ref.bfloat16().float())
    assert _rel(db, 0.5 + ref.sum((0, 2, 3))) < 1e-4


@pytest.mark.parametrize("k,s,p,is_max,inc,relu", [(3, 2, 1, True, True, False), (2, 2, 0, True, True, True),
                                                   (3, 1, 1, False, True, False), (3, 1, 1, False, False, False),
                                                   (3, 1, 1, False, True, True), (3, 1, 1, False, False, True),
                                                   (3, 2, 1, False, False, True),
                                                   (5, 3, 2, False, False, False), (8, 8, 0, False, True, False)])
def test_pool2d_channel_last(k, s, p, is_max, inc, relu):
    """Channel-last pooling (one thread per pixel x 8 channels, winner bytes in NHWC order; 3 x 3
    / s1 / p1 average pools: the sliding-row-window kernels) forward and backward against torch
    fp32, on channel-last bf16 inputs."""
    from flexflow_amd import kernels as K
    if not K.CHANNELS_LAST:
        pytest.skip("FF_CHANNELS_LAST=0")
    torch.manual_seed(25)
    x = torch.randn(4, 48, 17, 15, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    y, idx = K.pool2d_fwd(x, k, k, s, s, (p, p, p, p), is_max, inc, relu, True)
    assert K.is_nhwc(y)
    # reference in NCHW: torch's channel-last avg_pool2d backward disagreed with both its own NCHW
    # result and our two kernels on this image (seen on MI355X, torch 2.10 ROCm)
    xr = x.float().contiguous().requires_grad_()
    ref = K._pool_ref(xr, k, k, s, s, (p, p, p, p), is_max, inc, relu)
    assert _rel(y, ref) < 1e-2
    dy = torch.randn_like(ref).bfloat16()  # NCHW: the wrapper re-lays it out
    ref.backward(dy.float())
    dx = K.pool2d_bwd(x, y, dy, idx, k, k, s, s, (p, p, p, p), is_max, inc, relu)
    assert K.is_nhwc(dx)
    # (avg + ReLU: the mask of outputs within rounding of 0 can differ from the fp32 reference's;
    # the generic and the sliding-window kernels give the same 0.021-0.023 there)
    assert _rel(dx, xr.grad) < (3e-2 if (relu and not is_max) else 2e-2)


def test_elementwise_channel_last():
    """Unary / binary elementwise kernels index channel-last operands flat and keep the layout;
    mixed layouts are re-laid out to the first operand's."""
    from flexflow_amd import kernels as K
    torch.manual_seed(26)
    a = torch.randn(4, 24, 9, 7, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    b = torch.randn(4, 24, 9, 7, device=DEV).bfloat16()
    y = K.unary_fwd("relu", a)
    assert K.is_nhwc(y) and torch.equal(y.float(), torch.relu(a.float()))
    dx = K.unary_bwd("relu", a, y, b)
    assert torch.equal(dx.float(), (b.float() * (a.float() > 0)))
    c = K.binary_fwd("add", a, b)
    assert K.is_nhwc(c) and _rel(c, a.float() + b.float()) < 1e-2
    ar, br = a.float().requires_grad_(), b.float().requires_grad_()
    (ar * br).backward(b.float())
    da, db = K.binary_bwd("mul", a, b, b.contiguous(memory_format=torch.channels_last))
    assert _rel(da, ar.grad) < 1e-2 and _rel(db, br.grad) < 1e-2
    # a channel slice of a channel-last tensor (a concat's backward split) stays channel-last
    part = K.dense(a[:, 8:16])
    assert K.is_nhwc(part) and torch.equal(part, a[:, 8:16])


def test_tune_cache_skips_timing(tmp_path, monkeypatch):
    """A GEMM call site tuned in one run is dispatched from FF_TUNE_CACHE in the next, without timing."""
    from flexflow_amd import kernels as K
    path = str(tmp_path / "tune.json")
    M, N, Kd = 512, 768, 1024
    A = torch.randn(M, Kd, device=DEV).bfloat16()
    B = torch.randn(N, Kd, device=DEV).bfloat16()
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    monkeypatch.setattr(K, "_tuned", {})
    monkeypatch.setattr(K, "_cached", {"gemm": {}, "conv": {}})
    K.gemm(A, B, C, M, N, Kd, True, True, Kd, Kd, N)
    first = next(iter(K._tuned.values()))
    n_log = len(K.TUNE_LOG)
    K.tune_cache_save(path)
    monkeypatch.setattr(K, "_tuned", {})
    monkeypatch.setattr(K, "_TUNE_CACHE", path)
    K.tune_cache_load(path)
    C2 = torch.empty_like(C)
    K.gemm(A, B, C2, M, N, Kd, True, True, Kd, Kd, N)
    torch.cuda.synchronize()
    if isinstance(first, str):  # a named choice persists: the second run takes it without timing
        assert len(K.TUNE_LOG) == n_log and next(iter(K._tuned.values())) == first
    assert _rel(C2, A.float() @ B.float().t()) < 1e-2


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K,batch", [(256, 384, 512, 1), (200, 136, 72, 3), (1000, 1001, 1030, 1), (5, 7, 9, 2)])
def test_gemm_f32(ffC, a_k, b_k, M, N, K, batch):
    """fp32 GEMM on the f32-input MFMA (gemm_f32.hip) against torch fp32: layouts, edges, batches,
    alpha / beta / bias / GELU / pre-activation epilogue."""
    torch.manual_seed(4)
    Am = torch.randn(batch, M, K, device=DEV)
    Bn = torch.randn(batch, N, K, device=DEV)
    A = Am if a_k else Am.transpose(1, 2).contiguous()
    B = Bn if b_k else Bn.transpose(1, 2).contiguous()
    ref = torch.bmm(Am.double(), Bn.double().transpose(1, 2))
    C = torch.empty(batch, M, N, device=DEV)
    ffC.gemm_f32(A, B, C, None, None, M, N, K, A.shape[-1], B.shape[-1], N, A.shape[-1] * A.shape[-2],
                 B.shape[-1] * B.shape[-2], M * N, batch, a_k, b_k, 1.0, 0.0, 10)
    assert _rel(C, ref) < 1e-6
    bias = torch.randn(N, device=DEV)
    C0 = torch.randn(batch, M, N, device=DEV)
    C2, Z = C0.clone(), torch.empty(batch, M, N, device=DEV)
    ffC.gemm_f32(A, B, C2, bias, Z, M, N, K, A.shape[-1], B.shape[-1], N, A.shape[-1] * A.shape[-2],
                 B.shape[-1] * B.shape[-2], M * N, batch, a_k, b_k, 0.5, 1.0, 14)
    z = 0.5 * ref + C0.double() + bias.double()
    assert _rel(Z, z) < 1e-6
    assert _rel(C2, torch.nn.functional.gelu(z)) < 1e-5


@pytest.mark.parametrize("S", [24, 80])  # 80: a causal row spans lanes that see only masked (-inf) scores
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_attention_f32_path(causal, fused, S):
    """--dtype fp32 attention runs our kernels (f32 MFMA GEMMs + mask + softmax), not einsum: the op's
    forward and input gradients against the fp32 autograd reference."""
    from flexflow_amd.core import DataType, FFConfig, FFModel, SGDOptimizer
    cfg = FFConfig(["--dtype", "fp32", "--no-hip-graphs"])
    cfg.batch_size = 2
    ff = FFModel(cfg)
    x = ff.create_tensor([2, S, 64], DataType.DT_FLOAT)
    if fused:
        y = ff.multihead_attention(x, x, x, 64, 4, causal=causal)
    else:
        x2 = ff.create_tensor([2, S, 64], DataType.DT_FLOAT)
        y = ff.multihead_attention(x, x2, x2, 64, 4, causal=causal)
    ff.optimizer = SGDOptimizer(ff, 0.0)
    ff.compile()
    L = [l for l in ff.layers if l.op_type.name == "OP_MULTIHEAD_ATTENTION"][0]
    assert L.attrs["fused_qkv"] == fused
    rng = torch.Generator().manual_seed(0)
    xv = torch.randn(2, S, 64, generator=rng)
    x.set_tensor(ff, xv.numpy())
    if not fused:
        x2.set_tensor(ff, xv.numpy())
    ff.forward()
    ex = ff.executor
    assert "P" in ex.ctx[L.name].saved and "lse" not in ex.ctx[L.name].saved  # the fp32 kernel path ran
    out = torch.from_numpy(ff._get_tensor_value(y))
    # reference: the op's own weights through torch autograd in fp64
    W = {w.short_name: torch.from_numpy(np.asarray(w.get_weights(ff))).double() for w in L.weights}
    xr = xv.double()
    if fused:
        qkv = xr.reshape(2 * S, 64) @ W["qkv_weight"].reshape(-1, 64).t() + W["qkv_bias"].reshape(-1)
        qkv = qkv.view(2, S, 3, 4, 16)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        proj = lambda n: (xr.reshape(2 * S, 64) @ W[f"{n}_weight"].reshape(-1, 64).t() + W[f"{n}_bias"].reshape(-1)).view(2, S, 4, 16)  # noqa: E731
        q, k, v = proj("q"), proj("k"), proj("v")
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(16)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(2 * S, 64)
    ref = (o @ W["o_weight"].reshape(64, 64).t() + W["o_bias"]).view(2, S, 64)
    assert torch.isfinite(out).all()
    assert _rel(out, ref) < 1e-5


@pytest.mark.parametrize("act", [14, 11])  # GELU, RELU
@pytest.mark.parametrize("M,N,K", [(16384, 4096, 1024), (1000, 1032, 256), (520, 264, 128)])
def test_gemm_pp_activation_epilogue(ffC, M, N, K, act):
    """Ping-pong GEMM (impl 6) with bias, activation and the pre-activation store in its epilogue
    (the FFN1 forward of BERT: y = act(x W^T + b), z = x W^T + b) against fp32 torch; repeat bitwise."""
    from flexflow_amd.kernels import act_ref
    torch.manual_seed(8)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV).bfloat16()
    zref = A.float() @ B.float().t() + bias.float()
    yref = act_ref(zref.bfloat16().float(), act)
    first = None
    for _ in range(3):
        C = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
        Z = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
        ffC.gemm(A, B, C, bias, Z, M, N, K, K, K, N, 0, 0, 0, 1, True, True, 1.0, 0.0, act, 1, None, 6)
        if first is None:
            first = (C.clone(), Z.clone())
            assert _rel(Z, zref) < 1e-2 and _rel(C, yref) < 1e-2
        else:
            assert torch.equal(C, first[0]) and torch.equal(Z, first[1])
