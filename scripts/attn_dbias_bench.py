#!/usr/bin/env python3
"""Time the score-bias gradient launch (attn_dbias.hip) next to the flash backward it follows, and the
backward of the unfused matmul / add / softmax / matmul composition, which is the other way to train such a
bias (it materialises [B, H, S, S] scores and probabilities).

Shapes: B 32, H 16, S 512 and 2048, D 64 and 128, bias [1, H, S, S] and [B, H, S, S], causal or not, bf16.
Per shape, in one child process: `bwd` is kernels.flash_attn_bwd with the bias, `bwd_dbias` the same call with
dbias_out, timed window by window in turn; the dbias launch is their difference (it runs behind the backward on
the same stream). `unfused` is torch autograd's backward of the bf16 composition with the bias as a leaf
(S = 2048 needs ~20 GB for it). Device events around `--calls` calls, the median of `--windows` windows.
Prints one JSON line per shape. This script starts the children one after the other and does not touch
the GPU itself.

    python scripts/attn_dbias_bench.py [--calls 10] [--windows 5] [--out FILE] [--no-unfused]
"""
import argparse
import itertools
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H = 32, 16


def one(S, D, full, causal, calls, windows, unfused):
    import torch
    sys.path.insert(0, ROOT)
    from flexflow_amd import kernels as K
    if not torch.cuda.is_available():
        sys.exit("attn_dbias_bench.py needs a GPU: a time taken elsewhere says nothing about the kernel")
    dev = torch.device("cuda")
    q, k, v, do = (torch.randn(B, H, S, D, device=dev).bfloat16() for _ in range(4))
    bias = torch.randn(B if full else 1, H, S, S, device=dev)
    st = [H * S * D, S * D, D]
    scale = 1.0 / math.sqrt(D)
    o = torch.empty_like(q)
    lse = K.flash_attn_fwd(q, st, k, st, v, st, o, st, B, H, S, S, D, scale, causal, bias=bias)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    db = torch.empty_like(bias)

    def bwd(out):
        K.flash_attn_bwd(q, st, k, st, v, st, o, st, do, st, lse, dq, st, dk, st, dv, st, B, H, S, S, D, scale, causal,
                         bias=bias, dbias_out=out)

    kinds = {"bwd": lambda: bwd(None), "bwd_dbias": lambda: bwd(db)}
    if unfused:
        bl = bias.bfloat16().requires_grad_()
        ql, kl, vl = (t.detach().requires_grad_() for t in (q, k, v))
        s = ql @ kl.transpose(-1, -2) * scale + bl
        if causal:
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=dev).triu(1), float("-inf"))
        y = torch.softmax(s, -1) @ vl
        kinds["unfused"] = lambda: torch.autograd.grad(y, (ql, kl, vl, bl), do, retain_graph=True)
    for f in kinds.values():
        f()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {n: [] for n in kinds}
    for _ in range(windows):
        for n, f in kinds.items():
            a.record()
            for _ in range(calls):
                f()
            e.record()
            torch.cuda.synchronize()
            ts[n].append(a.elapsed_time(e) * 1e3 / calls)
    med = {n: statistics.median(t) for n, t in ts.items()}
    flops = 4.0 * B * H * S * S * D * (0.5 if causal else 1.0)  # the kernel's two GEMMs
    dbias_us = med["bwd_dbias"] - med["bwd"]
    print(json.dumps(dict(shape=f"B{B} H{H} S{S} D{D}", bias="[B,H,S,S]" if full else "[1,H,S,S]", causal=causal,
                          bwd_us=round(med["bwd"], 1), bwd_dbias_us=round(med["bwd_dbias"], 1), dbias_us=round(dbias_us, 1),
                          dbias_over_bwd=round(dbias_us / med["bwd"], 2), dbias_TFs=round(flops / dbias_us / 1e6, 1),
                          unfused_bwd_us=round(med["unfused"], 1) if unfused else None, calls=calls, windows=windows)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-unfused", action="store_true")
    ap.add_argument("--one", nargs=4, metavar=("S", "D", "FULL", "CAUSAL"), help="run one shape in this process")
    args = ap.parse_args()
    if args.one:
        S, D, full, causal = (int(x) for x in args.one)
        return one(S, D, bool(full), bool(causal), args.calls, args.windows, not args.no_unfused)
    lines = []
    for S, D, full, causal in itertools.product((512, 2048), (64, 128), (0, 1), (0, 1)):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(S), str(D), str(full), str(causal), "--calls",
               str(args.calls), "--windows", str(args.windows)] + (["--no-unfused"] if args.no_unfused else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.exit(f"S{S} D{D} full{full} causal{causal} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
