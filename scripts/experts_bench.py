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

--gated times the gated (SwiGLU) up layer instead, D -> (ffn gate | ffn up) -> ffn, SiLU gate, per case:

  forward  : one K.experts_glu_fwd (default epilogue, with and without save_z, and the LDS-staged and the
             direct epilogue forced) against K.experts_fwd(N = 2 ffn, ACT_NONE) plus the n K.glu_fwd
             launches on the packed halves of its slab
  backward : one K.experts_glu_bwd against the n K.glu_bwd launches

and prints the medians with the spread (min .. max) of the rounds.

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


def time_interleaved(variants, rounds, reps, spread=False):
    """{name: fn} -> {name: median ms per call}; the variants alternate inside every round. spread: the
    values are [median, min, max] over the rounds."""
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
    if spread:
        return {k: [round(t, 4) for t in (sorted(v)[len(v) // 2], min(v), max(v))] for k, v in times.items()}
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


def run_gated_case(n, alpha, routing, rounds, reps, act="silu"):
    dev = "cuda"
    cap = int(math.ceil(alpha * PAIRS / n))
    ld = loads(n, cap, routing)
    load = torch.tensor(ld, device=dev, dtype=torch.int32)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    xs, dhs = [], []
    for r in ld:
        x, dh = rnd(cap, D), rnd(cap, FFN)
        x[r:], dh[r:] = 0, 0
        xs.append(x)
        dhs.append(dh)
    w = rnd(n, 2 * FFN, D) * 0.03
    b = rnd(n * 2 * FFN)
    h = torch.empty(n, cap, FFN, device=dev, dtype=torch.bfloat16)
    _, z = K.experts_glu_fwd(xs, w, b, load, act, save_z=True)
    dz = torch.empty_like(z)

    def unfused_fwd():
        y, _ = K.experts_fwd(xs, w, b, load, K.ACT_NONE)
        for e in range(n):
            K.glu_fwd(y[e, :, :FFN], y[e, :, FFN:], act, out=h[e])

    def unfused_bwd():
        for e in range(n):
            K.glu_bwd(z[e, :, :FFN], z[e, :, FFN:], dhs[e], act, dg=dz[e, :, :FFN], du=dz[e, :, FFN:])

    out = dict(gated=act, n=n, alpha=alpha, routing=routing, cap=cap, load_max=max(ld), load_min=min(ld),
               rows_live=sum(ld), rows_capacity=n * cap, auto_tile_m=int(K.ext().experts_tile_m(cap)))
    fused = lambda **kw: (lambda: K.experts_glu_fwd(xs, w, b, load, act, **kw))  # noqa: E731
    out["fwd_ms"] = time_interleaved({"fused": fused(), "fused_save_z": fused(save_z=True),
                                      "staged_save_z": fused(save_z=True, epilogue=1),
                                      "direct_save_z": fused(save_z=True, epilogue=2),
                                      "staged": fused(epilogue=1), "direct": fused(epilogue=2),
                                      "unfused": unfused_fwd}, rounds, reps, spread=True)
    out["gate_bwd_ms"] = time_interleaved({"fused": lambda: K.experts_glu_bwd(dhs, z, load, act),
                                           "unfused": unfused_bwd}, rounds, reps, spread=True)
    out["useful_tflops_fused"] = round(2.0 * sum(ld) * D * 2 * FFN / (out["fwd_ms"]["fused_save_z"][0] * 1e9), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--experts", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--alpha", type=float, nargs="+", default=[1.0, 2.0])
    ap.add_argument("--routing", nargs="+", default=["uniform", "overloaded"])
    ap.add_argument("--layers", nargs="+", default=["up", "down"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gated", action="store_true", help="the gated up layer against its unfused form")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("experts_bench: needs the GPU (a CPU timing says nothing about these kernels)")
    sink = open(a.out, "w") if a.out else None
    for n in a.experts:
        for alpha in a.alpha:
            for routing in a.routing:
                for layer in (["gated"] if a.gated else a.layers):
                    res = (run_gated_case(n, alpha, routing, a.rounds, a.reps) if a.gated
                           else run_case(n, alpha, routing, layer, a.rounds, a.reps))
                    line = json.dumps(res)
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
