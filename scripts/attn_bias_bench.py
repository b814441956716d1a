"""Kernel-level cost of the attention score bias at B32 H16 S512 D64 (docs/PERFORMANCE.md, "Attention
score bias"): forward + backward of
  (i)   the default kernels without a bias (attn_fwd2_kernel / attn_bwd1b_kernel),
  (ii)  the generic MASK = true kernels without a bias (forward variant 1, backward variant 2; full
        key lengths select MASK = true without masking anything),
  (iii) the BIAS kernels with an fp32 [1, 16, 512, 512] bias (the LDS-DMA forms behind the default
        variants, and the register-staged forms behind forward 0 / backward 2),
  (iv)  the five-op unfused path the importer emits without fuse_sdpa (batch_matmul, scalar multiply,
        add, softmax, batch_matmul through the project's ops, forward + backward),
on the same tensors, alternating in one process, device events, with an A/A repeat of (iii).

    python scripts/attn_bias_bench.py [--reps 20] [--rounds 5]
"""
import argparse
import math
import os
import sys

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from flexflow_amd import _C as X
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    dev = "cuda"
    B, H, S, D = 32, 16, 512, 64
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(dev) for _ in range(4))
    bias = torch.randn(1, H, S, S, generator=g).to(dev)
    scale = 1.0 / math.sqrt(D)
    st = [H * S * D, S * D, D]
    o, lse = torch.empty_like(q), torch.empty(B * H * S, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(X.attn_bwd_ws(B, H, S, S, D), device=dev)
    full = torch.full((B,), S, dtype=torch.int32, device=dev)  # selects MASK = true without masking anything

    def flash(fv, bv, kl=None, sb=None):
        kw = dict(sbias=sb, sbias_sb=0, sbias_sh=S * S) if sb is not None else {}

        def run():
            X.attn_set_fwd_variant(fv)
            X.attn_set_bwd_variant(bv)
            X.attn_fwd(q, st, k, st, v, st, o, st, lse, B, H, S, S, D, scale, False, kl, **kw)
            X.attn_bwd(q, st, k, st, v, st, o, st, do, st, lse, dq, st, dk, st, dv, st, ws, B, H, S, S, D, scale, False,
                       None, kl, **kw)
        return run

    # (iv): the importer's unfused graph, built from the project's own ops
    ff = FFModel(FFConfig(["--dtype", "bf16"]))
    tq = ff.create_tensor([B, H, S, D], DataType.DT_FLOAT)
    tkt = ff.create_tensor([B, H, D, S], DataType.DT_FLOAT)
    tv = ff.create_tensor([B, H, S, D], DataType.DT_FLOAT)
    tb = ff.create_tensor([1, H, S, S], DataType.DT_FLOAT)
    s1 = ff.batch_matmul(tq, tkt)
    s2 = ff.scalar_multiply(s1, scale, inplace=False)
    s3 = ff.add(s2, tb)
    p = ff.softmax(s3, 3)
    out = ff.batch_matmul(p, tv)
    layers = [t.owner_layer for t in (s1, s2, s3, p, out)]
    kt = k.transpose(2, 3).contiguous()
    bias16 = bias.bfloat16()

    def ctx_of(L):
        n = len(L.impl.axis_sizes())
        from flexflow_amd.type import DataType as DT
        return OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n, compute_dtype=DT.DT_BF16)

    def unfused():
        cs = [ctx_of(L) for L in layers]
        a1 = layers[0].impl.forward(cs[0], [q, kt], [])[0]
        a2 = layers[1].impl.forward(cs[1], [a1], [])[0]
        a3 = layers[2].impl.forward(cs[2], [a2, bias16], [])[0]
        a4 = layers[3].impl.forward(cs[3], [a3], [])[0]
        layers[4].impl.forward(cs[4], [a4, v], [])
        g4 = layers[4].impl.backward(cs[4], [do])
        g3 = layers[3].impl.backward(cs[3], [g4[0]])
        g2 = layers[2].impl.backward(cs[2], [g3[0]])
        g1 = layers[1].impl.backward(cs[1], [g2[0]])
        layers[0].impl.backward(cs[0], [g1[0]])

    variants = [
        ("i    default, no bias (fwd 3 / bwd 10)", flash(3, 10)),
        ("ii   generic MASK, no bias (fwd 1 / bwd 2)", flash(1, 2, kl=full)),
        ("iii  BIAS (fwd 1 form / bwd 10 form)", flash(3, 10, sb=bias)),
        ("iii' BIAS, A/A repeat", flash(3, 10, sb=bias)),
        ("iii2 BIAS (fwd 0 / bwd 2: register staging)", flash(0, 2, sb=bias)),
        ("iv   unfused five ops (bf16)", unfused),
    ]
    fv0, bv0 = X.attn_fwd_variant(), X.attn_bwd_variant()
    times = {n: [] for n, _ in variants}
    try:
        for n, f in variants:  # warm-up (and any kernel selection)
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) / a.reps * 1e3)
    finally:
        X.attn_set_fwd_variant(fv0)
        X.attn_set_bwd_variant(bv0)
    print(f"B{B} H{H} S{S} D{D}, forward + backward, kernel-level, us per call; {a.rounds} rounds x {a.reps} calls")
    flops = 4.0 * B * H * S * S * D * 3.5
    for n, _ in variants:
        t = sorted(times[n])
        med = t[len(t) // 2]
        print(f"{n:48s} median {med:8.1f}  min {t[0]:8.1f}  max {t[-1]:8.1f}  ({flops / med * 1e-6:6.1f} TF/s)  all {['%.1f' % x for x in times[n]]}")


if __name__ == "__main__":
    main()
