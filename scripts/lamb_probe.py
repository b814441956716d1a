"""Cost of LAMB: the bench.py flagship shapes (BERT-Large, batch 32, seq 512, bf16) trained with
LAMBOptimizer against Adam with clip_norm=1.0 (likewise not overlapped with the backward),
alternating the two models in one process on one GPU, and the update launches alone (both LAMB
passes with the norms in between, against one fused Adam launch) over one arena of the same size.
Results: docs/PERFORMANCE.md, profiles/lamb_probe.txt.

    python scripts/lamb_probe.py [--model bert-large] [--rounds 5] [--steps 10] [--first lamb] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexflow_amd import kernels as K  # noqa: E402


def build(model, batch, seq, kind):
    from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, LAMBOptimizer, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    cfg = FFConfig(["--dtype", "bf16", "--search", "unity"])
    cfg.batch_size = batch
    ff = FFModel(cfg)
    bc = {"bert-large": BertConfig.large, "bert-base": BertConfig.base, "bert-tiny": BertConfig.tiny}[model](seq)
    bc.seq = seq
    bc.max_pos = max(bc.max_pos, seq)
    bc.pad_vocab_multiple = 64
    ids, pos, _ = build_bert(ff, batch, bc)
    ff.optimizer = LAMBOptimizer(ff, 1e-4) if kind == "lamb" else AdamOptimizer(ff, 1e-4, clip_norm=1.0)
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


def timed(fn, reps=10, rounds=5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(2):
        fn()
    times = []
    for _ in range(rounds):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / reps)
    return times


def update_probe(entries, size, say):
    """The update launches alone over one arena with the model's entry layout."""
    w = torch.randn(size, device="cuda") * 0.02
    g = torch.randn(size, device="cuda") * 1e-3
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    lowp = torch.zeros(size, dtype=torch.bfloat16, device="cuda")
    ent = [(off, n, i, 0.01 if len(shape) > 1 else 0.0, len(shape) > 1) for i, (off, n, shape) in enumerate(entries)]
    tab = K.lamb_table(ent, [(0, size)], len(ent), size, "cuda")
    part = torch.zeros(2 * tab.n_chunks, device="cuda")
    norms = torch.zeros(2 * len(ent), device="cuda")
    hyper = torch.tensor([1e-4, 10.0, 1000.0], device="cuda")
    one = torch.ones(1, device="cuda")
    say("update alone: %d elements, %d weights, %d chunks of at most %d" % (size, len(ent), tab.n_chunks, K.LAMB_CHUNK))

    def report(name, times, bytes_per_el):
        best = min(times)
        say("%-14s %.1f us best of %d x 10 (%.1f .. %.1f us), %.2f TB/s at %d B per element"
            % (name, best * 1e3, len(times), min(times) * 1e3, max(times) * 1e3, bytes_per_el * size / best / 1e9,
               bytes_per_el))
        return best

    s1 = report("lamb_moments", timed(lambda: K.lamb_moments(w, g, m, v, tab, hyper, one, 0.9, 0.999, 1e-6, part)), 24)
    sn = report("lamb_norms", timed(lambda: K.lamb_norms(part, tab, True, norms)), 0)
    s2 = report("lamb_apply", timed(lambda: K.lamb_apply(w, m, v, lowp, tab, hyper, 1e-6, norms)), 18)
    ad = report("adam_update", timed(lambda: K.adam_update(w, g, m, v, lowp, 1e-4, 0.9, 0.999, 0.0, 1e-8,
                                                           gscale_dev=one)), 30)
    say("LAMB launches %.1f us against Adam's %.1f us: ratio %.3f (bytes: 42 / 30 = 1.400)"
        % ((s1 + sn + s2) * 1e3, ad * 1e3, (s1 + sn + s2) / ad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-large")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--first", default="adam", choices=["adam", "lamb"],
                    help="which model is built, warmed up and timed first in every round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lamb_probe: needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    order = ["adam", "lamb"] if args.first == "adam" else ["lamb", "adam"]
    models = {k: build(args.model, args.batch, args.seq, k) for k in order}
    arenas = [ar for ar in models["lamb"].executor.arenas.values() if ar.size]
    n = sum(ar.size for ar in arenas)
    say("%s batch %d seq %d bf16, %d arena elements; Adam clip_norm=1 against LAMB, %s first; overlapped update "
        "possible: adam %s, lamb %s" % (args.model, args.batch, args.seq, n, order[0],
                                        models["adam"].executor._overlap_possible(),
                                        models["lamb"].executor._overlap_possible()))
    big = max(arenas, key=lambda ar: ar.size)
    entries, size = [(off, k, shape) for _, off, k, shape in big.entries], big.size
    for ff in models.values():
        steps_ms(ff, 5)  # warm-up
    res = {k: [] for k in models}
    for r in range(args.rounds):
        for k, ff in models.items():  # alternate the two in every round
            res[k].append(steps_ms(ff, args.steps))
        say("round %d: adam+clip %.3f ms/step, lamb %.3f ms/step" % (r, res["adam"][-1], res["lamb"][-1]))
    for k, v in res.items():
        say("%-5s median %.3f ms/step (min %.3f, max %.3f) over %d rounds of %d steps"
            % (k, float(np.median(v)), min(v), max(v), args.rounds, args.steps))
    a, b = float(np.median(res["adam"])), float(np.median(res["lamb"]))
    say("lamb - adam+clip: %+.3f ms/step (medians), step ratio %.4f" % (b - a, b / a))
    losses = {k: ff.get_perf_metrics().get_loss() for k, ff in models.items()}
    say("loss after %d steps: adam %.4f, lamb %.4f" % (5 + args.rounds * args.steps, losses["adam"], losses["lamb"]))
    del models, arenas, big
    torch.cuda.empty_cache()
    update_probe(entries, size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
