#!/usr/bin/env python3
"""Time the rotary launch (kernels.rope, rope.hip) on the device against two references on the same bytes:

  copy   a device copy that reads and writes as many bytes as the rotation of Q and K does
         (the kernel is a copy with a little arithmetic);
  torch  the same rotation composed from torch ops on the same strided views (HuggingFace's
         q * cos + rotate_half(q) * sin, written back in place).

Shapes: B32 S512 H16 D64 (multi-head) and B32 S512 H32 Hkv8 D128 (grouped-query), each with Q and K inside
one fused [T, heads, D] projection buffer (V behind them, untouched) and in separate buffers. Every timed
launch works on another copy of the buffers, enough of them to pass the 256 MB last-level cache, so the
times are those of data coming from HBM; device events around `--launches` launches, the median of
`--rounds` rounds. Prints one JSON line per shape and layout.

    python scripts/rope_bench.py [--launches 12] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flexflow_amd import kernels as K  # noqa: E402


def _timed(fns, rounds):
    """Median over rounds of the mean device time (us) of one call of fns[i], i over all of fns."""
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in fns:  # warm-up: code objects, allocator
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        st.record()
        for f in fns:
            f()
        en.record()
        torch.cuda.synchronize()
        ts.append(st.elapsed_time(en) * 1e3 / len(fns))
    return statistics.median(ts), min(ts), max(ts)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def bench(B, S, H, Hkv, D, fused, launches, rounds, dev):
    T = B * S
    table = K.rope_table(D, S, device=dev)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D))[None]
    cos = torch.cat((torch.cos(ang), torch.cos(ang)), -1).to(dev, torch.bfloat16)[None, None]  # [1, 1, S, D]
    sin = torch.cat((torch.sin(ang), torch.sin(ang)), -1).to(dev, torch.bfloat16)[None, None]
    if fused:
        W = (H + 2 * Hkv) * D
        qs, ks = [S * W, D, W], [S * W, D, W]
        mk = lambda: (lambda b: (b, b[H * D:]))(torch.randn(T * W, device=dev).bfloat16())  # noqa: E731
    else:
        qs, ks = [S * H * D, D, H * D], [S * Hkv * D, D, Hkv * D]
        mk = lambda: (torch.randn(T * H * D, device=dev).bfloat16(), torch.randn(T * Hkv * D, device=dev).bfloat16())  # noqa: E731
    moved = 2 * 2 * T * (H + Hkv) * D  # bytes read + written
    n = max(launches, int(800e6 // (moved // 2)) + 1)
    bufs = [mk() for _ in range(n)]
    v4 = lambda t, st, h: t.as_strided((B, h, S, D), (st[0], st[1], st[2], 1))  # noqa: E731

    def torch_rope(q, k):
        for t, st, h in ((q, qs, H), (k, ks, Hkv)):
            x = v4(t, st, h)
            x.copy_(x * cos + _rotate_half(x) * sin)

    src = [torch.randn(moved // 4, device=dev).bfloat16() for _ in range(n)]
    dst = [torch.empty_like(s) for s in src[:2]]
    # results must agree before times are compared: the kernel against the composition, loosely (bf16
    # intermediates in the composition)
    a, b = mk(), None
    b = tuple(t.clone() for t in a) if not fused else (lambda c: (c, c[H * D:]))(a[0].clone())
    K.rope(a[0], qs, a[1], ks, B, H, Hkv, S, S, D, D, table)
    torch_rope(*b)
    err = float((v4(a[0], qs, H).float() - v4(b[0], qs, H).float()).abs().max())
    assert err < 0.1, err
    kern = _timed([lambda q=q, k=k: K.rope(q, qs, k, ks, B, H, Hkv, S, S, D, D, table) for q, k in bufs], rounds)
    copy = _timed([lambda s=s, i=i: dst[i % 2].copy_(s) for i, s in enumerate(src)], rounds)
    comp = _timed([lambda q=q, k=k: torch_rope(q, k) for q, k in bufs], rounds)
    return dict(shape=f"B{B} S{S} H{H} Hkv{Hkv} D{D}", layout="fused" if fused else "separate", bytes=moved, buffers=n,
                rope_us=round(kern[0], 1), rope_min_max_us=[round(kern[1], 1), round(kern[2], 1)],
                rope_GBps=round(moved / kern[0] / 1e3, 1),
                copy_us=round(copy[0], 1), copy_GBps=round(moved / copy[0] / 1e3, 1),
                torch_us=round(comp[0], 1), rope_over_copy=round(kern[0] / copy[0], 3),
                torch_over_rope=round(comp[0] / kern[0], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rope_bench.py needs a GPU: a time taken elsewhere says nothing about the kernel")
    dev = torch.device("cuda")
    lines = []
    for H, Hkv, D in ((16, 16, 64), (32, 8, 128)):
        for fused in (True, False):
            r = bench(32, 512, H, Hkv, D, fused, args.launches, args.rounds, dev)
            print(json.dumps(r), flush=True)
            lines.append(r)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
