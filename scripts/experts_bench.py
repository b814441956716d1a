#!/usr/bin/env python3
"""Grouped expert GEMMs against the per-expert dense path they replace, on the device.

For each (n experts, alpha, routing) at D = 1024, ffn = 4096 and B * k = 16384 routed pairs, and for both
layers of an expert FFN (up: D -> ffn with GELU, down: ffn -> D), times per direction

  grouped : one K.experts_fwd / K.experts_bwd_data / K.experts_bwd_weight launch (tile_m as chosen by
            the launcher, and forced to 64 and 128 for the two row directions)
  dense   : the n K.linear_fwd / K.linear_bwd calls of the n dense layers of ff.moe, each over all cap
            rows (autotuned per call site as in a training run, tuned before the timed window)

in one process, alternating the variants round by round, each round timed with device events around
`--reps` back-to-back calls. Prints one JSON line per case; --out also writes them to a file.

Routing: 'uniform' gives every expert B * k / n rows; 'overloaded' gives expert 0 four times that
(clamped to the capacity) and spreads the rest evenly.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from flexflow_amd import kernels as K  # noqa: E402

D, FFN, PAIRS = 1024, 4096, 16384


def loads(n, cap, routing):
    mean = PAIRS // n
    if routing == "uniform":
        return [min(mean, cap)] * n
    big = 4 * mean
    rest = (PAIRS - big) // (n - 1)
    return [min(big, cap)] + [min(rest, cap)] * (n - 1)


def time_interleaved(variants, rounds, reps):
    """{name: fn} -> {name: median ms per call}; the variants alternate inside every round."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / reps)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def run_case(n, alpha, routing, layer, rounds, reps):
    dev = "cuda"
    cap = int(math.ceil(alpha * PAIRS / n))
    din, dout, act = (D, FFN, K.ACT_GELU) if layer == "up" else (FFN, D, K.ACT_NONE)
    ld = loads(n, cap, routing)
    load = torch.tensor(ld, device=dev, dtype=torch.int32)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    xs, dys = [], []
    for r in ld:  # what group_by / aggregate's backward hand over: zeros past the load
        x, dy = rnd(cap, din), rnd(cap, dout)
        x[r:], dy[r:] = 0, 0
        xs.append(x)
        dys.append(dy)
    w = rnd(n, dout, din) * 0.03
    b = rnd(n * dout)
    bs = [b[e * dout:(e + 1) * dout] for e in range(n)]
    dw = torch.zeros(n, dout, din, device=dev)
    db = torch.zeros(n * dout, device=dev)
    dbs = [db[e * dout:(e + 1) * dout] for e in range(n)]
    _, z = K.experts_fwd(xs, w, b, load, act, save_z=True)
    dzs = list(K.experts_act_bwd(dys, z, load, act).unbind(0)) if z is not None else dys
    zs = [None] * n if z is None else list(z.unbind(0))

    def dense_fwd():
        for e in range(n):
            K.linear_fwd(xs[e], w[e], bs[e], act, save_z=True)

    # the dense layers' input gradient reads a transposed weight copy (K.weight_t); its refresh is not timed
    wts = [w[e].t().contiguous() for e in range(n)]

    def dense_bwd(need_dx, want_dw):
        for e in range(n):  # dz handed in, so each direction is the GEMM alone, as on the grouped side
            K.linear_bwd(dzs[e], xs[e], w[e], None, K.ACT_NONE, dw[e] if want_dw else None, dbs[e] if want_dw else None,
                         need_dx=need_dx, wt=wts[e])

    useful = 2.0 * sum(ld) * din * dout
    out = dict(n=n, alpha=alpha, routing=routing, layer=layer, cap=cap, load_max=max(ld), load_min=min(ld),
               rows_live=sum(ld), rows_capacity=n * cap, auto_tile_m=int(K.ext().experts_tile_m(cap)))
    t = time_interleaved({"grouped": lambda: K.experts_fwd(xs, w, b, load, act, save_z=True),
                          "grouped_tile64": lambda: K.experts_fwd(xs, w, b, load, act, save_z=True, tile_m=64),
                          "grouped_tile128": lambda: K.experts_fwd(xs, w, b, load, act, save_z=True, tile_m=128),
                          "dense": dense_fwd}, rounds, reps)
    out["fwd_ms"] = {k: round(v, 4) for k, v in t.items()}
    t = time_interleaved({"grouped": lambda: K.experts_bwd_data(dzs, w, load),
                          "grouped_tile64": lambda: K.experts_bwd_data(dzs, w, load, tile_m=64),
                          "grouped_tile128": lambda: K.experts_bwd_data(dzs, w, load, tile_m=128),
                          "dense": lambda: dense_bwd(True, False)}, rounds, reps)
    out["dgrad_ms"] = {k: round(v, 4) for k, v in t.items()}
    t = time_interleaved({"grouped": lambda: K.experts_bwd_weight(dzs, xs, load, dw, db),
                          "dense": lambda: dense_bwd(False, True)}, rounds, reps)
    out["wgrad_ms"] = {k: round(v, 4) for k, v in t.items()}
    out["useful_tflops_grouped"] = {d: round(useful / (out[d + "_ms"]["grouped"] * 1e9), 1) for d in ("fwd", "dgrad", "wgrad")}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--experts", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--alpha", type=float, nargs="+", default=[1.0, 2.0])
    ap.add_argument("--routing", nargs="+", default=["uniform", "overloaded"])
    ap.add_argument("--layers", nargs="+", default=["up", "down"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("experts_bench: needs the GPU (a CPU timing says nothing about these kernels)")
    sink = open(a.out, "w") if a.out else None
    for n in a.experts:
        for alpha in a.alpha:
            for routing in a.routing:
                for layer in a.layers:
                    line = json.dumps(run_case(n, alpha, routing, layer, a.rounds, a.reps))
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
