"""Kernel-level cost of sliding-window attention (docs/PERFORMANCE.md, "Sliding-window attention"): forward
and backward, timed apart, of
  (a) full causal attention (the default kernels),
  (b) the same window as an fp32 [1, 1, S, S] score bias of 0 / -inf beside causal (the BIAS kernels),
  (c) window= (the SEG kernels on the bounds of attn_band_bounds), with an A/A repeat (c'),
at B8 H32 S4096 D64 and B8 H32 / Hkv8 S4096 D128, both causal (B H = 256: the chained backward), for
W = 512 and 1024 keys per query, the query included (window (W - 1, 0)). One process, the same tensors,
alternating variants, device events, warm-up.

    python scripts/attn_window_bench.py [--reps 5] [--rounds 5] [--seq 4096]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seq", type=int, default=4096)
    a = ap.parse_args()
    from flexflow_amd import _C as X
    from flexflow_amd import kernels as K
    dev = "cuda"
    S = a.seq
    for B, H, Hkv, D in ((8, 32, 32, 64), (8, 32, 8, 128)):
        g = torch.Generator().manual_seed(0)
        q, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(dev) for _ in range(2))
        k, v = (torch.randn(B, Hkv, S, D, generator=g).bfloat16().to(dev) for _ in range(2))
        scale = 1.0 / math.sqrt(D)
        sq, sk = [H * S * D, S * D, D], [Hkv * S * D, S * D, D]
        o, lse = torch.empty_like(q), torch.empty(B * H * S, device=dev)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty(X.attn_bwd_ws(B, H, S, S, D, Hkv), device=dev)
        i, j = torch.arange(S, device=dev)[:, None], torch.arange(S, device=dev)[None, :]

        def pair(kw):
            def fwd():
                X.attn_fwd(q, sq, k, sk, v, sk, o, sq, lse, B, H, S, S, D, scale, True, Hkv=Hkv, **kw)

            def bwd():
                X.attn_bwd(q, sq, k, sk, v, sk, o, sq, do, sq, lse, dq, sq, dk, sk, dv, sk, ws, B, H, S, S, D, scale, True,
                           Hkv=Hkv, **kw)
            return fwd, bwd

        variants = [("a  full causal", pair({}))]
        for W in (512, 1024):
            bias = torch.where(j >= i - (W - 1), 0.0, float("-inf")).to(torch.float32)[None, None].contiguous()
            lo, hi, klo, khi = K.attn_band_bounds(S, W - 1, -1, B=B, device=dev)
            win = dict(seg_lo=lo, seg_hi=hi, seg_klo=klo, seg_khi=khi)
            variants += [(f"b  W{W} as fp32 [1,1,S,S] bias", pair(dict(sbias=bias, sbias_sb=0, sbias_sh=0))),
                         (f"c  W{W} window=", pair(win)), (f"c' W{W} window=, A/A repeat", pair(win))]
        times = {(n, d): [] for n, _ in variants for d in ("fwd", "bwd")}
        for n, (fwd, bwd) in variants:  # warm-up
            for _ in range(2):
                fwd()
                bwd()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, (fwd, bwd) in variants:
                fwd()  # the backward below reads this variant's o / lse
                for d, f in (("fwd", fwd), ("bwd", bwd)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[n, d].append(e0.elapsed_time(e1) / a.reps * 1e3)
        print(f"B{B} H{H} Hkv{Hkv} S{S} D{D} causal, kernel-level, us per call; {a.rounds} rounds x {a.reps} calls")
        med = {}
        for n, _ in variants:
            for d in ("fwd", "bwd"):
                t = sorted(times[n, d])
                med[n, d] = t[len(t) // 2]
                print(f"  {n:34s} {d} median {med[n, d]:9.1f}  min {t[0]:9.1f}  max {t[-1]:9.1f}")
        for W in (512, 1024):
            c, c2, b_ = f"c  W{W} window=", f"c' W{W} window=, A/A repeat", f"b  W{W} as fp32 [1,1,S,S] bias"
            for d in ("fwd", "bwd"):
                aa = abs(med[c, d] - med[c2, d]) / med[c, d]
                print(f"  W{W} {d}: a / c = {med['a  full causal', d] / med[c, d]:.2f}x   b / c = {med[b_, d] / med[c, d]:.2f}x"
                      f"   A/A spread {100 * aa:.1f} %")
        del q, k, v, do, o, dq, dk, dv, ws


if __name__ == "__main__":
    main()
