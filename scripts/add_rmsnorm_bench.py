#!/usr/bin/env python3
"""Time the residual-RMSNorm launches (kernels.add_rmsnorm_fwd / add_rmsnorm_bwd, add_rmsnorm.hip) on the
device at the decoder's shape, T = 32 x 512 rows and d in {1024, 4096, 8192} columns in bf16, against two
references timed in the same process, interleaved window by window:

  unfused  what the unfused graph launches for the same work: forward binary_fwd add + rmsnorm_fwd (5 row
           passes against the fused launch's 4); backward rmsnorm_bwd + the add of the two gradients that
           meet on the sum (6 against 4);
  copy     a device copy that reads and writes as many bytes as the fused launch moves.

One process per (d, direction): this script starts them one after the other and does not touch the GPU
itself. In a child every timed call works on another set of buffers; device events around `--calls` calls,
the median of `--windows` windows per kind. Prints one JSON line per measurement.

    python scripts/add_rmsnorm_bench.py [--calls 40] [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32 * 512
WIDTHS = (1024, 4096, 8192)
EPS = 1e-6


def one(d, direction, calls, windows):
    import torch
    sys.path.insert(0, ROOT)
    from flexflow_amd import kernels as K
    if not torch.cuda.is_available():
        sys.exit("add_rmsnorm_bench.py needs a GPU: a time taken elsewhere says nothing about the kernel")
    dev = torch.device("cuda")
    bwd = direction == "bwd"
    moved = 4 * T * d * 2  # bytes the fused launch reads + writes (rstd, w and the dw slab left out)
    nset = 3

    def mk():
        s = {k: torch.randn(T, d, device=dev).bfloat16() for k in ("x", "res", "dy", "ds")}
        s["w"] = (1 + 0.5 * torch.randn(d, device=dev)).bfloat16()
        s["s"], _, s["rstd"] = K.add_rmsnorm_fwd(s["x"], s["res"], s["w"], EPS)
        s["dw"] = torch.zeros(d, device=dev)
        return s

    sets = [mk() for _ in range(nset)]
    src = [torch.randn(moved // 4, device=dev).bfloat16() for _ in range(nset)]
    dst = torch.empty_like(src[0])

    def fused(s):
        if bwd:
            return K.add_rmsnorm_bwd(s["s"], s["w"], s["rstd"], s["dy"], s["ds"], s["dw"])
        return K.add_rmsnorm_fwd(s["x"], s["res"], s["w"], EPS)[1]

    def unfused(s):
        if bwd:
            return K.binary_fwd("add", K.rmsnorm_bwd(s["s"], s["w"], s["dy"], s["rstd"], s["dw"]), s["ds"])
        return K.rmsnorm_fwd(K.binary_fwd("add", s["x"], s["res"]), s["w"], EPS)[0]

    # results must agree before times are compared (the unfused backward rounds dx before it adds ds)
    a, b = fused(sets[0]).float(), unfused(sets[0]).float()
    err = float((a - b).abs().max())
    assert err < 0.25, err
    kinds = {"fused": lambda i: fused(sets[i % nset]), "unfused": lambda i: unfused(sets[i % nset]),
             "copy": lambda i: dst.copy_(src[i % nset])}
    for f in kinds.values():  # warm-up: code objects, allocator
        for i in range(nset):
            f(i)
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in kinds}
    for _ in range(windows):
        for k, f in kinds.items():
            st.record()
            for i in range(calls):
                f(i)
            en.record()
            torch.cuda.synchronize()
            ts[k].append(st.elapsed_time(en) * 1e3 / calls)
    med = {k: statistics.median(v) for k, v in ts.items()}
    print(json.dumps(dict(
        shape=f"T{T} d{d} bf16", direction=direction, bytes=moved, calls=calls, windows=windows,
        fused_us=round(med["fused"], 1), fused_min_max_us=[round(min(ts["fused"]), 1), round(max(ts["fused"]), 1)],
        fused_GBps=round(moved / med["fused"] / 1e3, 1), copy_us=round(med["copy"], 1),
        copy_GBps=round(moved / med["copy"] / 1e3, 1), fraction_of_copy_bandwidth=round(med["copy"] / med["fused"], 3),
        unfused_us=round(med["unfused"], 1), unfused_over_fused=round(med["unfused"] / med["fused"], 2),
        max_abs_diff=err)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--one", nargs=2, metavar=("D", "DIRECTION"), help="run one measurement in this process")
    args = ap.parse_args()
    if args.one:
        return one(int(args.one[0]), args.one[1], args.calls, args.windows)
    lines = []
    for d in WIDTHS:
        for direction in ("fwd", "bwd"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(d), direction, "--calls",
                                str(args.calls), "--windows", str(args.windows)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.exit(f"d={d} {direction} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
