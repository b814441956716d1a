"""Cost of gradient clipping by global norm: the bench.py flagship (BERT-Large, batch 32, seq 512,
bf16, Adam) with clip_norm=1.0 against the same tree without clipping, alternating the two models
in one process on one GPU, and the grad_sumsq kernel alone over an arena of the same size.
Results: docs/PERFORMANCE.md, profiles/clip_probe.txt.

    python scripts/clip_probe.py [--model bert-large] [--rounds 5] [--steps 10] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexflow_amd import kernels as K  # noqa: E402


def build(model, batch, seq, clip):
    from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    cfg = FFConfig(["--dtype", "bf16", "--search", "unity"])
    cfg.batch_size = batch
    ff = FFModel(cfg)
    bc = {"bert-large": BertConfig.large, "bert-base": BertConfig.base, "bert-tiny": BertConfig.tiny}[model](seq)
    bc.seq = seq
    bc.max_pos = max(bc.max_pos, seq)
    bc.pad_vocab_multiple = 64
    ids, pos, _ = build_bert(ff, batch, bc)
    ff.optimizer = AdamOptimizer(ff, 1e-4, clip_norm=clip)
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


def sumsq_probe(n, say):
    x = torch.randn(n, device="cuda") * 1e-3
    ws = torch.empty(K.GRAD_SUMSQ_PARTIALS, device="cuda")
    out = torch.zeros(1, device="cuda")
    for _ in range(3):
        K.grad_sumsq(x, ws, out)
    ref = float((x.double() ** 2).sum())
    say("grad_sumsq n=%d: rel err vs fp64 %.2e" % (n, abs(out.item() - ref) / ref))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps, times = 20, []
    for _ in range(5):
        ev[0].record()
        for _ in range(reps):
            K.grad_sumsq(x, ws, out)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / reps)
    best = min(times)
    say("grad_sumsq n=%d: %.1f us best of 5 x %d (%.1f .. %.1f us), %.2f TB/s of fp32 read"
        % (n, best * 1e3, reps, min(times) * 1e3, max(times) * 1e3, 4.0 * n / best / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-large")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_probe: needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    models = {"plain": build(args.model, args.batch, args.seq, None),
              "clip": build(args.model, args.batch, args.seq, args.clip)}
    n = sum(ar.size for ar in models["clip"].executor.arenas.values())
    say("%s batch %d seq %d bf16 Adam, %d arena elements, clip_norm %g; overlapped update possible: plain %s, clip %s"
        % (args.model, args.batch, args.seq, n, args.clip, models["plain"].executor._overlap_possible(),
           models["clip"].executor._overlap_possible()))
    for ff in models.values():
        steps_ms(ff, 5)  # warm-up
    res = {k: [] for k in models}
    for r in range(args.rounds):
        for k, ff in models.items():  # alternate the two in every round
            res[k].append(steps_ms(ff, args.steps))
        say("round %d: plain %.3f ms/step, clip %.3f ms/step" % (r, res["plain"][-1], res["clip"][-1]))
    for k, v in res.items():
        say("%-5s median %.3f ms/step (min %.3f, max %.3f) over %d rounds of %d steps"
            % (k, float(np.median(v)), min(v), max(v), args.rounds, args.steps))
    say("clip - plain: %+.3f ms/step (medians)" % (float(np.median(res["clip"])) - float(np.median(res["plain"]))))
    say("last global gradient norm: %r" % models["clip"].get_grad_norm())
    del models
    torch.cuda.empty_cache()
    sumsq_probe(n, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
