"""Cost of AdamW against Adam: the update launch alone over one arena with BERT-Large's entry
layout (the whole arena and the 4 Mi-element piece the overlapped update launches; adamw_update
with one workgroup per chunk and with a capped grid striding over the chunks, against adam_update
over the same buffers, alternating in one process, device events), then the bench.py flagship
shapes (BERT-Large, batch 32, seq 512, bf16) trained with AdamWOptimizer against AdamOptimizer, both
overlapped with the backward, the two models alternating in one process on one GPU.
Results: docs/PERFORMANCE.md, profiles/adamw_probe.txt.

    python scripts/adamw_probe.py [--model bert-large] [--rounds 5] [--steps 10] [--first adam] [--out FILE]
"""
import argparse
import bisect
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexflow_amd import kernels as K  # noqa: E402

PIECE = 4 << 20  # FF_UPD_CHUNK's default: the overlapped update's launch size


def build(model, batch, seq, kind):
    from flexflow_amd.core import AdamOptimizer, AdamWOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    cfg = FFConfig(["--dtype", "bf16", "--search", "unity"])
    cfg.batch_size = batch
    ff = FFModel(cfg)
    bc = {"bert-large": BertConfig.large, "bert-base": BertConfig.base, "bert-tiny": BertConfig.tiny}[model](seq)
    bc.seq = seq
    bc.max_pos = max(bc.max_pos, seq)
    bc.pad_vocab_multiple = 64
    ids, pos, _ = build_bert(ff, batch, bc)
    ff.optimizer = AdamWOptimizer(ff, 1e-4) if kind == "adamw" else AdamOptimizer(ff, 1e-4)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(1234)
    ids.set_tensor(ff, rng.integers(0, bc.vocab, (batch, seq), dtype=np.int32))
    pos.set_tensor(ff, np.tile(np.arange(seq, dtype=np.int32), (batch, 1)))
    ff.label_tensor.set_tensor(ff, rng.integers(0, bc.vocab, (batch, seq, 1), dtype=np.int32))
    return ff


def steps_ms(ff, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ff.train_step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def timed(fn, reps=10):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def update_probe(entries, size, rounds, say):
    """The update launches alone over one arena with the model's entry layout."""
    w = torch.randn(size, device="cuda") * 0.02
    g = torch.randn(size, device="cuda") * 1e-3
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    lowp = torch.zeros(size, dtype=torch.bfloat16, device="cuda")
    ent = [(off, n, i, 0.01 if len(shape) > 1 else 0.0, False) for i, (off, n, shape) in enumerate(entries)]
    # the piece: PIECE elements from the start of the arena's largest entry (or the whole of it)
    off, n = max(((o, k) for o, k, _ in entries), key=lambda e: e[1])
    lo, hi = off, off + min(PIECE, n // 8 * 8)
    tab = K.lamb_table(ent, [(0, lo), (lo, hi), (hi, size)], len(ent), size, "cuda")
    starts = [s for s, _, _ in tab.rows()]
    p0, p1 = bisect.bisect_left(starts, lo), bisect.bisect_left(starts, hi)
    hyper = torch.tensor([1e-4, 10.0, 1000.0], device="cuda")
    say("update alone: %d elements, %d weights, %d chunks of at most %d (16 B of table each); piece [%d, %d) = %d "
        "chunks; 30 B per element both ways" % (size, len(ent), tab.n_chunks, K.LAMB_CHUNK, lo, hi, p1 - p0))

    def adamw(c0, c1, mb):
        return lambda: K.adamw_update(w, g, m, v, lowp, tab, c0, c1, hyper, None, 0.9, 0.999, 1e-8, max_blocks=mb)

    def adam(a, b):
        return lambda: K.adam_update(w[a:b], g[a:b], m[a:b], v[a:b], lowp[a:b], 1e-4, 0.9, 0.999, 0.0, 1e-8)

    cands = [("adam whole", adam(0, size), size), ("adamw whole", adamw(0, tab.n_chunks, 0), size),
             ("adamw whole/2048", adamw(0, tab.n_chunks, 2048), size),
             ("adamw whole/8192", adamw(0, tab.n_chunks, 8192), size),
             ("adam whole B", adam(0, size), size),  # Adam again: the spread between repeated Adam timings
             ("adam piece", adam(lo, hi), hi - lo), ("adamw piece", adamw(p0, p1, 0), hi - lo),
             ("adamw piece/256", adamw(p0, p1, 256), hi - lo), ("adam piece B", adam(lo, hi), hi - lo)]
    for _, fn, _ in cands:
        fn()
        fn()
    res = {name: [] for name, _, _ in cands}
    for r in range(rounds):
        for name, fn, _ in cands:  # alternate all of them in every round
            res[name].append(timed(fn))
        say("round %d: " % r + ", ".join("%s %.1f" % (name, res[name][-1] * 1e3) for name, _, _ in cands) + " us")
    med = {}
    for name, _, k in cands:
        t = res[name]
        med[name] = float(np.median(t))
        say("%-17s median %.1f us (min %.1f, max %.1f) over %d x 10, %.2f TB/s" %
            (name, med[name] * 1e3, min(t) * 1e3, max(t) * 1e3, rounds, 30 * k / med[name] / 1e9))
    for kind in ("whole", "piece"):
        a = res["adam " + kind] + res["adam %s B" % kind]
        am = float(np.median(a))
        say("%s: Adam %.1f us, spread of its timings %.1f .. %.1f us (%.1f%%)" %
            (kind, am * 1e3, min(a) * 1e3, max(a) * 1e3, (max(a) - min(a)) / am * 100))
        for name in med:
            if name.startswith("adamw " + kind):
                say("  %-17s %.1f us, ratio to Adam %.3f" % (name, med[name] * 1e3, med[name] / am))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-large")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--first", default="adam", choices=["adam", "adamw"],
                    help="which model is built, warmed up and timed first in every round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adamw_probe: needs a GPU")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    order = ["adam", "adamw"] if args.first == "adam" else ["adamw", "adam"]
    models = {}
    for k in order:
        print("building the %s model" % k, flush=True)
        models[k] = build(args.model, args.batch, args.seq, k)
    arenas = [ar for ar in models["adamw"].executor.arenas.values() if ar.size]
    n = sum(ar.size for ar in arenas)
    say("%s batch %d seq %d bf16, %d arena elements; Adam against AdamW, %s first; overlapped update possible: "
        "adam %s, adamw %s" % (args.model, args.batch, args.seq, n, order[0],
                               models["adam"].executor._overlap_possible(),
                               models["adamw"].executor._overlap_possible()))
    big = max(arenas, key=lambda ar: ar.size)
    update_probe([(off, k, shape) for _, off, k, shape in big.entries], big.size, args.rounds, say)
    torch.cuda.empty_cache()
    for k, ff in models.items():
        say("%s warm-up: %.1f ms/step over 5 steps" % (k, steps_ms(ff, 5)))
    res = {k: [] for k in models}
    for r in range(args.rounds):
        for k, ff in models.items():  # alternate the two in every round
            res[k].append(steps_ms(ff, args.steps))
        say("round %d: adam %.3f ms/step, adamw %.3f ms/step" % (r, res["adam"][-1], res["adamw"][-1]))
    for k, v in res.items():
        say("%-5s median %.3f ms/step (min %.3f, max %.3f) over %d rounds of %d steps"
            % (k, float(np.median(v)), min(v), max(v), args.rounds, args.steps))
    a, b = float(np.median(res["adam"])), float(np.median(res["adamw"]))
    say("adamw - adam: %+.3f ms/step (medians), step ratio %.4f; spread of adam %.3f ms"
        % (b - a, b / a, max(res["adam"]) - min(res["adam"])))
    losses = {k: ff.get_perf_metrics().get_loss() for k, ff in models.items()}
    say("loss after %d steps: adam %.4f, adamw %.4f" % (5 + args.rounds * args.steps, losses["adam"], losses["adamw"]))


if __name__ == "__main__":
    main()
