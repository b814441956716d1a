#!/usr/bin/env python3
"""Time the fused softmax-xent kernel with and without ignore_index on the BERT-Large MLM shape
(16384 x 30522 bf16), interleaved in one process:

  a  the call without ignore_index (the IGNORE = false instantiation: the kernel as it was)
  b  ignore_index set, no row ignored
  c  ignore_index set, 85 % of the rows ignored
  d  as c, with the device-side count (count_valid_labels + the valid_count pointer form)

Every round times each variant once (device events around `--iters` calls, after a warm-up of
every variant), in the order a b c d a ...; the report gives each variant's mean and the spread
(min .. max) of its rounds, and the bytes the kernel has to move: valid rows are read twice and
written once, ignored rows written once.

`--root DIR` imports flexflow_amd from another checkout (e.g. a build of the parent commit) and
times only `a` there, to alternate processes of two builds on one box.

    python scripts/xent_ignore_probe.py [rows cols] [--rounds 5] [--iters 20] [--root DIR]
"""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, default=[16384, 30522])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--frac", type=float, default=0.85)
ap.add_argument("--root", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root) if args.root else __file__.rsplit("/scripts/", 1)[0])
from flexflow_amd import _C as ffC  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
rows, cols = args.shape
IGN = -100
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(rows, cols, device="cuda", generator=g).bfloat16()
labels = torch.randint(0, cols, (rows,), device="cuda", dtype=torch.int32, generator=g)
masked = labels.clone()
masked[torch.rand(rows, device="cuda", generator=g) < args.frac] = IGN
n_valid = int((masked != IGN).sum())
loss = torch.empty(rows, device="cuda")
dl = torch.empty_like(x)
acc3 = torch.zeros(3, device="cuda")


def plain():
    ffC.softmax_xent(x, labels, loss, dl, rows, cols, 1.0 / rows, acc3)


def none_ignored():
    ffC.softmax_xent(x, labels, loss, dl, rows, cols, 1.0 / rows, acc3, ignore_index=IGN)


def ignored():
    ffC.softmax_xent(x, masked, loss, dl, rows, cols, 1.0 / rows, acc3, ignore_index=IGN)


def ignored_counted():
    vc = ffC.count_valid_labels(masked, IGN)
    ffC.softmax_xent(x, masked, loss, dl, rows, cols, 1.0 / rows, acc3, ignore_index=IGN, valid_count=vc)


row_bytes = cols * x.element_size()
full = 3 * rows * row_bytes
part = 3 * n_valid * row_bytes + (rows - n_valid) * row_bytes
variants = [("a plain", plain, full)]
if not args.root:
    variants += [("b ignore_index, none ignored", none_ignored, full),
                 (f"c {args.frac:.0%} ignored", ignored, part),
                 (f"d {args.frac:.0%} ignored, device count", ignored_counted, part + 4 * rows)]
for _, f, _ in variants:
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in variants}
for _ in range(args.rounds):
    for name, f, _ in variants:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            f()
        e.record()
        e.synchronize()
        times[name].append(s.elapsed_time(e) / args.iters * 1e3)
tag = f"softmax_xent {rows}x{cols} bf16" + (f" [{args.root}]" if args.root else "")
for name, _, nbytes in variants:
    t = times[name]
    mean = sum(t) / len(t)
    print(f"{tag} {name}: mean {mean:.1f} us, rounds {min(t):.1f} .. {max(t):.1f} us, {nbytes / 1e9:.2f} GB, "
          f"{nbytes / mean / 1e6:.2f} TB/s")
