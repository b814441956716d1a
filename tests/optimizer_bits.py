"""The update kernels' outputs as sha256 digests, for test_optimizer_bits_cpu.py (the CPU fallbacks
of flexflow_amd.kernels) and test_optimizer_bits_gpu.py (the HIP kernels): a change that is meant to
leave the arithmetic alone must leave every digest of tests/golden/optimizer_kernels_sha256.json
alone. Only K.* functions are called, so the same file records the digests on the commit to pin.

One flat arena: entries of 2 * 8192 + 404, 9, 1, 64, 8192 and 37 elements, each padded to 8 (a weight
of three chunks, chunk tails of 0 and 1 elements, a single-element weight, padding after every odd
size). Real elements are random, from a seeded CPU generator (both devices see the same values);
the padding of w and of the bf16 copy holds 4096, so a write into it changes the digest. Lambda
alternates 0.01, 0; adapt where an entry has more than 64 elements; gscale_dev = 0.125; three steps
with a fresh gradient each."""
import hashlib
import json
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_kernels_sha256.json")
SIZES = [2 * 8192 + 404, 9, 1, 64, 8192, 37]
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.999, 1e-8, 0.01
STEPS = 3
PAD = 4096.0


def _entries():
    ent, off = [], 0
    for i, n in enumerate(SIZES):
        ent.append((off, n, i, WD if i % 2 == 0 else 0.0, n > 64))
        off += (n + 7) // 8 * 8
    return ent, off


ENT, SIZE = _entries()
CUT = 8192 + 400  # inside the second chunk of the first weight, a multiple of 4
# flat ranges for sgd_update / adam_update: starts are multiples of 4, the last one has a tail element
SLICES = [(0, 8588), (8588, 16808), (16808, SIZE - 3)]
WHOLE = [(0, SIZE)]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class _State:
    def __init__(self, dev, n_state):
        self.gen = torch.Generator().manual_seed(20240)
        real = torch.zeros(SIZE, dtype=torch.bool)
        for o, n, *_ in ENT:
            real[o:o + n] = True
        w = torch.full((SIZE,), PAD)
        w[real] = torch.randn(int(real.sum()), generator=self.gen)
        self.dev = dev
        self.w = w.to(dev)
        self.lowp = torch.full((SIZE,), PAD, dtype=torch.bfloat16).to(dev)
        self.state = [torch.zeros(SIZE, device=dev) for _ in range(n_state)]
        self.gsd = torch.tensor([0.125]).to(dev)

    def grad(self):
        return torch.randn(SIZE, generator=self.gen).to(self.dev)

    def digests(self, **extra):
        d = {"w": _sha(self.w), "lowp": _sha(self.lowp)}
        d.update({f"state{i}": _sha(t) for i, t in enumerate(self.state)})
        d.update({k: _sha(t) for k, t in extra.items()})
        return d


def _sgd(dev, momentum, nesterov, wd, ranges, max_blocks):
    from flexflow_amd import kernels as K
    s = _State(dev, 1 if momentum > 0 else 0)
    for _ in range(STEPS):
        g = s.grad()
        for lo, hi in reversed(ranges):
            K.sgd_update(s.w[lo:hi], g[lo:hi], s.state[0][lo:hi] if momentum > 0 else None, s.lowp[lo:hi], LR,
                         momentum, nesterov, wd, max_blocks=max_blocks, gscale_dev=s.gsd)
    return s.digests()


def _adam(dev, alpha_dev, wd, ranges, max_blocks):
    from flexflow_amd import kernels as K
    s = _State(dev, 2)
    m, v = s.state
    adev = torch.zeros(1).to(dev) if alpha_dev else None
    for t in range(1, STEPS + 1):
        g = s.grad()
        alpha_t = LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        if adev is not None:
            adev.fill_(alpha_t)
        for lo, hi in reversed(ranges):
            # with alpha_dev the argument is a decoy: the kernel must read the device scalar
            K.adam_update(s.w[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], s.lowp[lo:hi], 1.0 if alpha_dev else alpha_t,
                          B1, B2, wd, EPS, max_blocks=max_blocks, alpha_dev=adev, gscale_dev=s.gsd)
    return s.digests()


def _hyper(dev, t):
    return torch.tensor([LR, 1 / (1 - B1 ** t), 1 / (1 - B2 ** t)], dtype=torch.float32).to(dev)


def _lamb(dev, ranges, count):
    from flexflow_amd import kernels as K
    s = _State(dev, 2)
    m, v = s.state
    tab = K.lamb_table(ENT, ranges, len(ENT), SIZE, dev)
    partials = torch.zeros(2 * tab.n_chunks, device=dev)
    norms = torch.zeros(2 * len(ENT), device=dev)
    for t in range(1, STEPS + 1):
        g = s.grad()
        hyper = _hyper(dev, t)
        K.lamb_moments(s.w, g, m, v, tab, hyper, s.gsd, B1, B2, EPS, partials)
        K.lamb_norms(partials, tab, count, norms)
        K.lamb_apply(s.w, m, v, s.lowp, tab, hyper, EPS, norms)
    return s.digests(partials=partials, norms=norms)


def _adamw(dev, split, max_blocks):
    from flexflow_amd import kernels as K
    s = _State(dev, 2)
    m, v = s.state
    tab = K.lamb_table(ENT, [(0, CUT), (CUT, SIZE)] if split else WHOLE, len(ENT), SIZE, dev)
    runs = [(0, tab.n_chunks)]
    if split:
        a = [st for st, _, _ in tab.rows()].index(CUT)
        runs = [(a, tab.n_chunks), (0, a)]  # two chunk runs, the later one first
    for t in range(1, STEPS + 1):
        g = s.grad()
        hyper = _hyper(dev, t)
        for c0, c1 in runs:
            K.adamw_update(s.w, g, m, v, s.lowp, tab, c0, c1, hyper, s.gsd, B1, B2, EPS, max_blocks=max_blocks)
    return s.digests()


def _cases():
    c = {}
    for name, (mom, nest, wd) in {"sgd_plain": (0.0, False, 0.0), "sgd_nesterov_wd": (0.9, True, WD)}.items():
        c[f"{name}_whole"] = lambda dev, a=(mom, nest, wd): _sgd(dev, *a, WHOLE, 0)
        for mb in (0, 3, -2):
            c[f"{name}_slices_mb{mb}"] = lambda dev, a=(mom, nest, wd), mb=mb: _sgd(dev, *a, SLICES, mb)
    for name, (adev, wd) in {"adam_alpha_dev": (True, 0.0), "adam_alpha_arg": (False, 0.0),
                             "adam_wd": (False, WD)}.items():
        c[f"{name}_whole"] = lambda dev, a=(adev, wd): _adam(dev, *a, WHOLE, 0)
        for mb in (0, 3, -2):
            c[f"{name}_slices_mb{mb}"] = lambda dev, a=(adev, wd), mb=mb: _adam(dev, *a, SLICES, mb)
    c["lamb_whole"] = lambda dev: _lamb(dev, WHOLE, True)
    c["lamb_two_ranges"] = lambda dev: _lamb(dev, [(0, CUT), (CUT, SIZE)], True)
    c["lamb_no_count"] = lambda dev: _lamb(dev, WHOLE, False)
    for mb in (0, 3):
        c[f"adamw_whole_mb{mb}"] = lambda dev, mb=mb: _adamw(dev, False, mb)
        c[f"adamw_two_runs_mb{mb}"] = lambda dev, mb=mb: _adamw(dev, True, mb)
    return c


CASES = _cases()


def run(name, dev):
    return CASES[name](dev)


def golden(kind):
    with open(GOLDEN) as f:
        gold = json.load(f)
    return gold[kind]


def record(kind, dev, out, commit):
    """Write (or update) the section `kind` ("cpu" / "gpu") of the digest file at `out`."""
    gold = {}
    if os.path.exists(out):
        with open(out) as f:
            gold = json.load(f)
    gold[kind] = {"commit": commit, "cases": {name: run(name, dev) for name in CASES}}
    with open(out, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
