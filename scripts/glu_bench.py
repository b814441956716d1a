#!/usr/bin/env python3
"""Time the gated-linear-unit launches (kernels.glu_fwd / glu_bwd, glu.hip) on the device at the decoder's
shape, T = 32 x 512 rows and F = 4096 columns in bf16, against two references timed in the same process,
interleaved window by window:

  unfused  the same result from the project's own unfused kernels: unary silu then the binary product
           (forward: 5 streams of T x F against the fused launch's 3), the product's backward then silu's
           (backward: 9 against 5). In the packed form the halves of the [T, 2F] buffer are strided, so
           the unfused kernels first copy them dense and the backward concatenates dg | du: what a graph of
           split / silu / multiply would do;
  copy     a device copy that reads and writes as many bytes as the fused launch moves.

Forms: `separate` (gate and up in two [T, F] tensors) and `packed` (the halves of one [T, 2F] buffer, dg / du
written into one [T, 2F] gradient). One process per (form, direction): this script starts them one after
the other and does not touch the GPU itself. In a child every timed call works on another set of buffers
(each tensor is 128 MiB, a launch moves 384 to 640 MiB, past the 256 MB last-level cache); device events
around `--calls` calls, the median of `--windows` windows per kind. Prints one JSON line per measurement.

    python scripts/glu_bench.py [--calls 60] [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, F_ = 32 * 512, 4096
ACT = "silu"


def one(form, direction, calls, windows):
    import torch
    sys.path.insert(0, ROOT)
    from flexflow_amd import kernels as K
    if not torch.cuda.is_available():
        sys.exit("glu_bench.py needs a GPU: a time taken elsewhere says nothing about the kernel")
    dev = torch.device("cuda")
    bwd = direction == "bwd"
    streams = 5 if bwd else 3
    moved = streams * T * F_ * 2  # bytes the fused launch reads + writes
    nset = 3

    def mk():
        s = {}
        if form == "packed":
            s["x"] = (torch.randn(T, 2 * F_, device=dev) * 2).bfloat16()
            s["g"], s["u"] = s["x"][:, :F_], s["x"][:, F_:]
            s["dx"] = torch.empty_like(s["x"])
            s["dg"], s["du"] = s["dx"][:, :F_], s["dx"][:, F_:]
        else:
            s["g"], s["u"] = ((torch.randn(T, F_, device=dev) * 2).bfloat16() for _ in range(2))
            s["dg"], s["du"] = torch.empty_like(s["g"]), torch.empty_like(s["g"])
        s["y"] = torch.empty(T, F_, dtype=torch.bfloat16, device=dev)
        s["dy"] = torch.randn(T, F_, device=dev).bfloat16()
        s["a"] = K.unary_fwd("silu", s["g"])  # the activation the unfused backward has saved
        return s

    sets = [mk() for _ in range(nset)]
    src = [torch.randn(moved // 4, device=dev).bfloat16() for _ in range(nset)]
    dst = torch.empty_like(src[0])

    def fused(s):
        if bwd:
            K.glu_bwd(s["g"], s["u"], s["dy"], ACT, dg=s["dg"], du=s["du"])
        else:
            K.glu_fwd(s["g"], s["u"], ACT, out=s["y"])

    def unfused(s):
        if bwd:
            da, du = K.binary_bwd("mul", s["a"], s["u"], s["dy"])
            dg = K.unary_bwd("silu", s["g"], s["a"], da)
            return torch.cat((dg, du), -1) if form == "packed" else (dg, du)
        return K.binary_fwd("mul", K.unary_fwd("silu", s["g"]), s["u"])

    # results must agree before times are compared (bf16 intermediates in the unfused pair)
    s = sets[0]
    fused(s)
    r = unfused(s)
    if bwd:
        rg, ru = (r[:, :F_], r[:, F_:]) if form == "packed" else r
        err = max(float((s["dg"].float() - rg.float()).abs().max()), float((s["du"].float() - ru.float()).abs().max()))
    else:
        err = float((s["y"].float() - r.float()).abs().max())
    assert err < 0.5, err
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
        shape=f"T{T} F{F_} bf16 {ACT}", form=form, direction=direction, bytes=moved, calls=calls, windows=windows,
        fused_us=round(med["fused"], 1), fused_min_max_us=[round(min(ts["fused"]), 1), round(max(ts["fused"]), 1)],
        fused_GBps=round(moved / med["fused"] / 1e3, 1), copy_us=round(med["copy"], 1),
        copy_GBps=round(moved / med["copy"] / 1e3, 1), fraction_of_copy_bandwidth=round(med["copy"] / med["fused"], 3),
        unfused_us=round(med["unfused"], 1), unfused_over_fused=round(med["unfused"] / med["fused"], 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--one", nargs=2, metavar=("FORM", "DIRECTION"), help="run one measurement in this process")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.calls, args.windows)
    lines = []
    for form in ("separate", "packed"):
        for direction in ("fwd", "bwd"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", form, direction, "--calls",
                                str(args.calls), "--windows", str(args.windows)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.exit(f"{form} {direction} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
