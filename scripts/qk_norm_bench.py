#!/usr/bin/env python3
"""Time the fused QK-norm + rotary launches (kernels.qk_norm_rope / qk_norm_rope_bwd, qknorm.hip) on the device
at the decoder's shape, T = 32 x 512 tokens in bf16 with (H 16, Hkv 4, D 64) and (H 32, Hkv 8, D 128), against
two references timed in the same process, interleaved window by window:

  unfused  the sequence the project's other kernels give for the same work on contiguous [T, H, D] heads:
           forward rmsnorm_fwd on the [T H, D] rows of Q and of K, then one rope launch in place; backward one
           inverse rope launch, then rmsnorm_bwd of Q and of K (two reads and writes of Q and K per direction
           against the fused launch's one);
  copy     a device copy that reads and writes as many bytes as the fused launch moves.

One process per (shape, direction): this script starts them one after the other and does not touch the GPU
itself. In a child every timed call works on another set of buffers; device events around `--calls` calls,
the median of `--windows` windows per kind. Prints one JSON line per measurement.

    python scripts/qk_norm_bench.py [--calls 40] [--windows 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 32, 512
SHAPES = {"h16_kv4_d64": (16, 4, 64), "h32_kv8_d128": (32, 8, 128)}
EPS = 1e-6


def one(shape, direction, calls, windows):
    import torch
    sys.path.insert(0, ROOT)
    from flexflow_amd import kernels as K
    if not torch.cuda.is_available():
        sys.exit("qk_norm_bench.py needs a GPU: a time taken elsewhere says nothing about the kernel")
    dev = torch.device("cuda")
    H, Hkv, D = SHAPES[shape]
    T, bwd = B * S, direction == "bwd"
    moved = (3 if bwd else 2) * T * (H + Hkv) * D * 2  # bytes the fused launch reads + writes (rstd, w, table left out)
    table = K.rope_table(D, S, device=dev)
    qs, ks = [S * H * D, D, H * D], [S * Hkv * D, D, Hkv * D]
    nset = 3

    def mk():
        s = {k: torch.randn(T * h * D, device=dev).bfloat16() for k, h in (("q", H), ("k", Hkv), ("dq", H), ("dk", Hkv))}
        s["wq"], s["wk"] = ((1 + 0.25 * torch.randn(D, device=dev)).bfloat16() for _ in range(2))
        s["qn"], s["kn"] = torch.empty_like(s["q"]), torch.empty_like(s["k"])
        s["rq"], s["rk"] = K.qk_norm_rope(s["q"], qs, s["qn"], qs, s["wq"], s["k"], ks, s["kn"], ks, s["wk"], B, H, Hkv, S, S, D,
                                          EPS, rd=D, table=table)
        s["dwq"], s["dwk"] = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        return s

    def fused(s):
        if bwd:
            K.qk_norm_rope_bwd(s["q"], qs, s["dq"], qs, s["wq"], s["rq"], s["dwq"], s["k"], ks, s["dk"], ks, s["wk"], s["rk"],
                               s["dwk"], B, H, Hkv, S, S, D, rd=D, table=table)
            return s["dq"], s["dk"]
        K.qk_norm_rope(s["q"], qs, s["qn"], qs, s["wq"], s["k"], ks, s["kn"], ks, s["wk"], B, H, Hkv, S, S, D, EPS, rd=D,
                       table=table)
        return s["qn"], s["kn"]

    def unfused(s):
        if bwd:
            K.rope(s["dq"], qs, s["dk"], ks, B, H, Hkv, S, S, D, D, table, inverse=True)
            return (K.rmsnorm_bwd(s["q"].view(T * H, D), s["wq"], s["dq"].view(T * H, D), s["rq"].view(-1), s["dwq"]),
                    K.rmsnorm_bwd(s["k"].view(T * Hkv, D), s["wk"], s["dk"].view(T * Hkv, D), s["rk"].view(-1), s["dwk"]))
        yq, yk = K.rmsnorm_fwd(s["q"].view(T * H, D), s["wq"], EPS)[0], K.rmsnorm_fwd(s["k"].view(T * Hkv, D), s["wk"], EPS)[0]
        K.rope(yq.view(-1), qs, yk.view(-1), ks, B, H, Hkv, S, S, D, D, table)
        return yq, yk

    # results must agree before times are compared (the unfused sequence rounds between its launches)
    chk = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in mk().items()} for _ in range(1)] * 2
    ref = {k: v.clone() for k, v in chk[0].items()}
    a = [t.float().view(-1).clone() for t in fused(chk[0])]
    b = [t.float().view(-1).clone() for t in unfused(ref)]
    err = max(float((x - y).abs().max() / (y.abs().max() + 1e-30)) for x, y in zip(a, b))
    assert err < 0.05, err
    sets = [mk() for _ in range(nset)]
    src = [torch.randn(moved // 4, device=dev).bfloat16() for _ in range(nset)]
    dst = torch.empty_like(src[0])
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
        shape=f"T{T} H{H} Hkv{Hkv} D{D} bf16", direction=direction, bytes=moved, calls=calls, windows=windows,
        fused_us=round(med["fused"], 1), fused_min_max_us=[round(min(ts["fused"]), 1), round(max(ts["fused"]), 1)],
        fused_GBps=round(moved / med["fused"] / 1e3, 1), copy_us=round(med["copy"], 1),
        copy_GBps=round(moved / med["copy"] / 1e3, 1), fraction_of_copy_bandwidth=round(med["copy"] / med["fused"], 3),
        unfused_us=round(med["unfused"], 1), unfused_min_max_us=[round(min(ts["unfused"]), 1), round(max(ts["unfused"]), 1)],
        unfused_over_fused=round(med["unfused"] / med["fused"], 2), max_rel_diff=err)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--one", nargs=2, metavar=("SHAPE", "DIRECTION"), help="run one measurement in this process")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.calls, args.windows)
    lines = []
    for shape in SHAPES:
        for direction in ("fwd", "bwd"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, direction, "--calls",
                                str(args.calls), "--windows", str(args.windows)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.exit(f"{shape} {direction} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
