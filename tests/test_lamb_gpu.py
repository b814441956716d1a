"""LAMB on the device: the chunk-table kernels (lamb_moments, lamb_norms, lamb_apply) against the
float64 oracle kernels.lamb_ref, ranges split as two ZeRO ranks would split them, the edge cases
of the trust ratio, argument checks, and LAMB training steps (eager, clipped, captured into a
hipGraph)."""
import math

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ULP32 = 2.0 ** -23
GUARD = 4096.0  # exact in bf16; its square would swamp any norm that read it
C = K.LAMB_CHUNK
MARGIN = 16     # guard elements on each side of every buffer (64 bytes: the slices stay aligned)
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-6, 1e-2, 0.01


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.detach().cpu().double()


def _close(got, ref64, atol, what):
    err = (_d(got) - ref64).abs() - atol
    i = int(err.argmax())
    assert err[i] <= 0, f"{what}: element {i}: got {_d(got)[i].item()!r}, ref {ref64[i].item()!r}"


def _opt_tol(ref64, step):
    """The project's optimizer tolerance (tests/test_grad_clip_gpu.py): 16 fp32 ulps of
    max(1, |value|) per step taken."""
    return 16 * step * ULP32 * ref64.abs().clamp_min(1.0)


def _chain(n):
    """d: the longest chain of fp32 additions an element's square passes through in lamb_moments
    and lamb_norms for a weight of n elements in one piece, as the comment in
    csrc/kernels/optimizer.hip gives it."""
    cc = -(-n // C)
    return C // 1024 + 2 + 1 + 10 + -(-cc // 256) + 10


def _norm_tol(n):
    return (_chain(n) + 2) * 2.0 ** -24


def test_chunk_constant_and_chain(ffC):
    assert ffC.lamb_chunk() == C and C % 1024 == 0
    assert _chain(1) == 32 and _chain(3 * C + 5) == 32 and _chain(257 * C) == 33


# --------------------------------------------------------------------------------- the hand-made arena
SIZES = [(1,), (7,), (8,), (9,), (C - 1,), (C,), (C + 1,), (3 * C + 5,), (37,)]
# all but the last are treated as matrices (decay and trust ratio); the last is the 1-D entry
RULES = [(WD, True)] * (len(SIZES) - 1) + [(0.0, False)]


def _entries(sizes=SIZES, rules=RULES):
    ent, off = [], 0
    for i, (shape, (lam, adapt)) in enumerate(zip(sizes, rules)):
        n = int(math.prod(shape))
        ent.append((off, n, i, lam, adapt))
        off += (n + 7) // 8 * 8  # WeightArena.add
    return ent, off


class Arena:
    """w, g, m, v (and a bf16 copy) with GUARD in all padding and around the buffers."""

    def __init__(self, ent, size, seed, lowp=True):
        self.ent, self.size = ent, size
        real = torch.zeros(size, dtype=torch.bool)
        for off, n, *_ in ent:
            real[off:off + n] = True
        self.real = real
        g = _gen(seed)
        self.host = {}
        self.buf = {}
        for name in ("w", "g", "m", "v"):
            x = torch.full((size,), GUARD)
            x[real] = torch.randn(int(real.sum()), generator=g) if name in ("w", "g") else 0.0
            self.host[name] = x
            self.buf[name] = torch.full((size + 2 * MARGIN,), GUARD, device=DEV)
            self.buf[name][MARGIN:MARGIN + size].copy_(x)
        self.buf["lowp"] = torch.full((size + 2 * MARGIN,), GUARD, dtype=BF16, device=DEV) if lowp else None
        self.hyper = torch.zeros(3, device=DEV)

    def t(self, name):
        b = self.buf[name]
        return None if b is None else b[MARGIN:MARGIN + self.size]

    def set_grad(self, seed):
        g = torch.full((self.size,), GUARD)
        g[self.real] = torch.randn(int(self.real.sum()), generator=_gen(seed))
        self.t("g").copy_(g)
        return g

    def set_hyper(self, step, lr=LR, bias_correction=True):
        rc = (1 / (1 - B1 ** step), 1 / (1 - B2 ** step)) if bias_correction else (1.0, 1.0)
        self.hyper.copy_(torch.tensor([lr, *rc], dtype=F32))

    def check_guards(self, what):
        pad = ~self.real.to(DEV)
        for name, b in self.buf.items():
            if b is None:
                continue
            assert bool((b[:MARGIN] == GUARD).all()) and bool((b[-MARGIN:] == GUARD).all()), f"{what}: {name} margin"
            assert bool((b[MARGIN:MARGIN + self.size][pad] == GUARD).all()), f"{what}: {name} padding"


def _guarded(n):
    buf = torch.full((n + 2 * MARGIN,), GUARD, device=DEV)
    return buf, buf[MARGIN:MARGIN + n]


def _guard_ok(buf):
    return bool((buf[:MARGIN] == GUARD).all()) and bool((buf[-MARGIN:] == GUARD).all())


def _step(ar, tabs, gscale_dev=None):
    """One LAMB step over the tables (one table = one rank's ranges): stage 1 and the norms per
    table, the norm vectors summed by hand, stage 2 per table. Returns (norms, [partials])."""
    nw = tabs[0].n_weights
    vecs, parts, bufs = [], [], []
    for tab in tabs:
        pbuf, part = _guarded(2 * tab.n_chunks)
        nbuf, norms = _guarded(2 * nw)
        K.lamb_moments(ar.t("w"), ar.t("g"), ar.t("m"), ar.t("v"), tab, ar.hyper, gscale_dev, B1, B2, EPS, part)
        K.lamb_norms(part, tab, True, norms)
        vecs.append(norms)
        parts.append(part)
        bufs += [pbuf, nbuf]
    total = vecs[0] if len(vecs) == 1 else torch.stack(vecs).sum(0)
    for tab in tabs:
        K.lamb_apply(ar.t("w"), ar.t("m"), ar.t("v"), ar.t("lowp"), tab, ar.hyper, EPS, total)
    assert all(_guard_ok(b) for b in bufs), "a guard around the partials or the norms was written"
    return total, parts


def _run(tabs_of, steps=3, seed=7, bias_correction=True, ent_size=None, coef=None):
    """steps LAMB steps on a fresh arena; every step is checked against lamb_ref: m, v, w against
    the float64 run from the start, the norms against lamb_ref applied to the device's own state."""
    ent, size = ent_size or _entries()
    ar = Arena(ent, size, seed)
    tabs = tabs_of(ent, size)
    w64, m64, v64 = (ar.host[k].double() for k in ("w", "m", "v"))
    gsd = torch.tensor([coef], device=DEV) if coef is not None else None
    out = []
    for step in range(1, steps + 1):
        g = ar.set_grad(1000 * seed + step)
        ar.set_hyper(step, bias_correction=bias_correction)
        before = tuple(ar.t(k).clone() for k in ("w", "g", "m", "v"))
        norms, parts = _step(ar, tabs, gsd)
        torch.cuda.synchronize()
        kw = dict(bias_correction=bias_correction, coef=1.0 if coef is None else coef)
        w64, m64, v64, _ = K.lamb_ref(w64, g, m64, v64, ent, step, LR, B1, B2, EPS, **kw)
        real = ar.real
        for name, ref in (("m", m64), ("v", v64), ("w", w64)):
            _close(ar.t(name)[real.to(DEV)], ref[real], _opt_tol(ref[real], step), f"{name} step {step}")
        _, _, _, n64 = K.lamb_ref(*before, ent, step, LR, B1, B2, EPS, **kw)
        got = _d(norms).view(-1, 2)
        for off, n, wi, *_ in ent:
            for j, what in enumerate(("sum w^2", "sum u^2")):
                rel = abs(got[wi, j].item() - n64[wi, j].item()) / n64[wi, j].item()
                print(f"step {step} weight {wi} (n={n}) {what}: rel err {rel:.3e}, allowed {_norm_tol(n):.3e}")
                assert rel <= _norm_tol(n), (step, wi, n, what, got[wi, j].item(), n64[wi, j].item())
        assert torch.equal(ar.t("lowp")[real.to(DEV)], ar.t("w")[real.to(DEV)].bfloat16()), f"lowp step {step}"
        assert torch.equal(ar.t("g"), before[1]), "the gradient was written"
        ar.check_guards(f"step {step}")
        out.append({k: ar.t(k).clone() for k in ("w", "m", "v", "lowp")} | {"norms": norms.clone(), "parts": parts})
    return out


def _whole(ent, size):
    return [K.lamb_table(ent, [(0, size)], len(ent), size, DEV)]


_UNSPLIT = {}


def _unsplit():
    if not _UNSPLIT:
        _UNSPLIT["run"] = _run(_whole)
    return _UNSPLIT["run"]


def test_table_layout():
    ent, size = _entries()
    tab = _whole(ent, size)[0]
    rows = tab.rows()
    assert tab.n_chunks == len(rows) == sum(-(-n // C) for _, n, *_ in ent)
    covered = torch.zeros(size, dtype=torch.int32)
    for s, ln, wi in rows:
        assert s % 4 == 0 and 0 < ln <= C
        covered[s:s + ln] += 1
        off, n = ent[wi][0], ent[wi][1]
        assert off <= s and s + ln <= off + n
    real = torch.zeros(size, dtype=torch.bool)
    for off, n, *_ in ent:
        real[off:off + n] = True
    assert torch.equal(covered, real.int())  # every element once, the padding never
    assert size > int(real.sum())            # and there is padding


def test_three_steps_match_float64():
    _unsplit()


def test_second_run_gives_the_same_bits():
    a, b = _unsplit(), _run(_whole)
    for x, y in zip(a, b):
        for k in ("w", "m", "v", "lowp", "norms"):
            assert torch.equal(x[k], y[k]), k
        assert all(torch.equal(p, q) for p, q in zip(x["parts"], y["parts"]))


def test_ranges_split_mid_chunk_match_unsplit():
    """Two ranges that cut the largest entry inside its second chunk, as two ZeRO ranks would hold
    it: each side's norms are summed by hand before stage 2."""
    ent, size = _entries()
    off, n = ent[7][0], ent[7][1]
    assert n == 3 * C + 5
    cut = off + C + 400

    def tabs_of(ent, size):
        return [K.lamb_table(ent, r, len(ent), size, DEV) for r in ([(0, cut)], [(cut, size)])]

    tabs = tabs_of(ent, size)
    assert (cut - 400, 400, 7) in tabs[0].rows() and tabs[1].rows()[0] == (cut, C, 7)  # the cut falls inside a chunk
    split, whole = _run(tabs_of), _unsplit()
    real = torch.zeros(size, dtype=torch.bool)
    for o, k, *_ in ent:
        real[o:o + k] = True
    for step, (x, y) in enumerate(zip(split, whole), 1):
        for k in ("w", "m", "v"):
            ref = _d(y[k])[real]
            _close(x[k][real.to(DEV)], ref, _opt_tol(ref, step), f"split {k} step {step}")
        got, ref = _d(x["norms"]), _d(y["norms"])
        rel = ((got - ref).abs() / ref).max().item()
        assert rel <= _norm_tol(3 * C + 5), rel


def test_more_than_one_range_per_table_and_empty_weights():
    """A table over two disjoint ranges, with weights that have no chunk on this 'rank': their
    norms are written as zeros (no memset), and so are the rows of weights named in owned."""
    ent, size = _entries()
    nw = len(ent) + 2
    lo, hi = ent[4][0], ent[6][0]  # entries 4 and 5 only
    tab = K.lamb_table(ent, [(ent[1][0], ent[2][0]), (lo, hi)], nw, size, DEV, owned=[nw - 1])
    assert [int(c) for c in tab.wtab_host[:, 3]] == [0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    ar = Arena(ent, size, 3)
    ar.set_hyper(1)
    part = torch.zeros(2 * tab.n_chunks, device=DEV)
    norms = torch.full((2 * nw,), GUARD, device=DEV)
    K.lamb_moments(ar.t("w"), ar.t("g"), ar.t("m"), ar.t("v"), tab, ar.hyper, None, B1, B2, EPS, part)
    K.lamb_norms(part, tab, True, norms)
    n2 = norms.view(-1, 2).cpu()
    for wi in range(nw):
        if wi in (1, 4, 5):
            assert n2[wi, 0] > 0 and n2[wi, 1] > 0
        elif wi == nw - 2:
            assert n2[wi, 0] == GUARD and n2[wi, 1] == GUARD  # a row this table does not own
        else:
            assert n2[wi, 0] == 0 and n2[wi, 1] == 0
    # count=False: a replica another rank counts writes zeros for every row it owns
    K.lamb_norms(part, tab, False, norms)
    n2 = norms.view(-1, 2).cpu()
    assert all(bool((n2[wi] == 0).all()) for wi in range(nw) if wi != nw - 2) and n2[nw - 2, 0] == GUARD
    # m, v moved inside the ranges only
    m = ar.t("m").cpu()
    touched = torch.zeros(size, dtype=torch.bool)
    for wi in (1, 4, 5):
        touched[ent[wi][0]:ent[wi][0] + ent[wi][1]] = True
    assert bool((m[touched] != 0).all()) and bool((m[ar.real & ~touched] == 0).all())
    ar.check_guards("partial ranges")


# --------------------------------------------------------------------------------------- edge cases
def _small(sizes, rules, seed=11):
    ent, size = _entries(sizes, rules)
    return ent, size, Arena(ent, size, seed)


def test_all_zero_weight_and_zero_update():
    """|w| = 0 gives r = 1 (the weight moves by lr * u, no NaN); zero gradient and zero state with
    lambda = 0 gives |u| = 0, r = 1 and the weight does not move at all."""
    ent, size, ar = _small([(C + 3,), (21, 3), (9,)], [(WD, True), (0.0, True), (0.0, False)])
    w0 = ar.t("w").clone()
    w0[ent[0][0]:ent[0][0] + ent[0][1]] = 0.0
    ar.t("w").copy_(w0)
    g = ar.set_grad(5)
    g[ent[1][0]:ent[1][0] + ent[1][1]] = 0.0
    ar.t("g").copy_(g)
    ar.set_hyper(1)
    norms, _ = _step(ar, _whole(ent, size))
    n2 = norms.view(-1, 2).cpu()
    assert n2[0, 0] == 0 and n2[0, 1] > 0 and n2[1, 0] > 0 and n2[1, 1] == 0
    w = ar.t("w")
    assert bool(torch.isfinite(w[ar.real.to(DEV)]).all())
    ref, _, _, _ = K.lamb_ref(w0, g, torch.zeros(size), torch.zeros(size), ent, 1, LR, B1, B2, EPS)
    _close(w[ar.real.to(DEV)], ref[ar.real], _opt_tol(ref[ar.real], 1), "w")
    s0 = slice(ent[0][0], ent[0][0] + ent[0][1])
    assert bool((w[s0].abs() > 0.5 * LR).all())  # r = 1: a full Adam-sized first step from zero
    s1 = slice(ent[1][0], ent[1][0] + ent[1][1])
    assert torch.equal(w[s1], w0[s1])
    ar.check_guards("zero cases")


def test_one_d_entry_is_plain_adam_without_decay():
    ent, size, ar = _small([(33, 5), (37,)], [(WD, True), (0.0, False)])
    off, n = ent[1][0], ent[1][1]
    s = slice(off, off + n)
    w64 = ar.host["w"].double()[s]
    m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        g = ar.set_grad(40 + step).double()[s]
        ar.set_hyper(step)
        _step(ar, _whole(ent, size))
        m64 = B1 * m64 + (1 - B1) * g
        v64 = B2 * v64 + (1 - B2) * g * g
        w64 = w64 - LR * (m64 / (1 - B1 ** step)) / ((v64 / (1 - B2 ** step)).sqrt() + EPS)
        _close(ar.t("w")[s], w64, _opt_tol(w64, step), f"1-D w step {step}")


def test_without_bias_correction():
    _run(_whole, steps=2, bias_correction=False, ent_size=_entries([(C + 9,), (5, 3), (11,)],
                                                                   [(WD, True), (WD, True), (0.0, False)]))


def test_clip_coefficient_from_the_device():
    _run(_whole, steps=2, coef=0.125, ent_size=_entries([(C + 9,), (5, 3), (11,)],
                                                        [(WD, True), (WD, True), (0.0, False)]))


def test_nan_gradient_stays_in_its_weight():
    sizes, rules = [(C + 9,), (5, 3), (11,), (2 * C,)], [(WD, True), (WD, True), (0.0, False), (WD, True)]
    ent, size, ar = _small(sizes, rules)
    g = ar.set_grad(9)
    g[ent[1][0] + 4] = float("nan")
    ar.t("g").copy_(g)
    ar.set_hyper(1)
    w0 = ar.t("w").clone()
    _step(ar, _whole(ent, size))
    w = ar.t("w").cpu()
    assert math.isnan(w[ent[1][0] + 4].item())
    # the same step with that one entry's gradient made finite: every other entry has the same bits
    ar2 = Arena(ent, size, 11)
    assert torch.equal(ar2.t("w"), w0)
    g2 = g.clone()
    g2[ent[1][0] + 4] = 0.0
    ar2.t("g").copy_(g2)
    ar2.set_hyper(1)
    _step(ar2, _whole(ent, size))
    ref, _, _, _ = K.lamb_ref(w0, g2, torch.zeros(size), torch.zeros(size), ent, 1, LR, B1, B2, EPS)
    for i in (0, 2, 3):
        s = slice(ent[i][0], ent[i][0] + ent[i][1])
        assert bool(torch.isfinite(w[s]).all()), i
        assert torch.equal(w[s], ar2.t("w")[s].cpu()), i
        _close(w[s], ref[s], _opt_tol(ref[s], 1), f"entry {i}")


# ---------------------------------------------------------------------------------- argument checks
def test_bad_arguments_raise(ffC):
    ent, size = _entries([(C + 9,), (11,)], [(WD, True), (0.0, False)])
    with pytest.raises(RuntimeError):
        K.lamb_table(ent, [(2, size)], 2, size, DEV)  # a range that does not start on 16 bytes
    with pytest.raises(RuntimeError):
        K.lamb_table(ent, [(0, size + 8)], 2, size, DEV)  # past the arena
    with pytest.raises(RuntimeError):
        K.lamb_table([(4, 9, 0, 0.0, True), (14, 3, 1, 0.0, True)], [(0, size)], 2, size, DEV)  # misaligned entry
    with pytest.raises(RuntimeError):
        K.lamb_table(ent, [(0, size)], 1, size, DEV)  # weight index outside the table
    tab = K.lamb_table(ent, [(0, size)], 2, size, DEV)
    w, g, m, v = (torch.zeros(size, device=DEV) for _ in range(4))
    lowp = torch.zeros(size, dtype=BF16, device=DEV)
    hyper = torch.tensor([LR, 1.0, 1.0], device=DEV)
    part, norms = torch.zeros(2 * tab.n_chunks, device=DEV), torch.zeros(4, device=DEV)
    ok = (w, g, m, v, tab.chunks, tab.wtab, hyper, None, B1, B2, EPS, part)
    ffC.lamb_moments(*ok)

    def moments(**kw):
        names = ("master", "grad", "m", "v", "chunks", "wtab", "hyper", "gscale_dev", "b1", "b2", "eps", "partials")
        a = dict(zip(names, ok)) | kw
        with pytest.raises(RuntimeError):
            ffC.lamb_moments(*[a[k] for k in names])

    moments(partials=part[:-1])                                # workspace too short
    moments(grad=g.double())                                   # wrong dtype
    moments(m=m.bfloat16())
    moments(chunks=tab.chunks.int())                           # the table's dtype
    moments(wtab=tab.wtab.long())
    moments(master=torch.zeros(size + 4, device=DEV)[1:size + 1])  # not 16-byte aligned
    moments(v=torch.zeros(size - 8, device=DEV))               # a shorter state than the arena
    moments(hyper=hyper[:2])
    moments(hyper=hyper.cpu())
    moments(gscale_dev=torch.ones(2, device=DEV))
    with pytest.raises(RuntimeError):
        ffC.lamb_norms(part[:-1], tab.n_chunks, tab.wtab, True, norms)
    with pytest.raises(RuntimeError):
        ffC.lamb_norms(part, tab.n_chunks, tab.wtab, True, norms[:3])
    with pytest.raises(RuntimeError):
        ffC.lamb_apply(w, m, v, lowp, tab.chunks, tab.wtab, hyper, EPS, norms[:3])
    with pytest.raises(RuntimeError):
        ffC.lamb_apply(w, m, v, lowp.float(), tab.chunks, tab.wtab, hyper, EPS, norms)
    with pytest.raises(RuntimeError):
        ffC.lamb_apply(w, m, v, lowp[:-8], tab.chunks, tab.wtab, hyper, EPS, norms)
    ffC.lamb_norms(part, tab.n_chunks, tab.wtab, True, norms)
    ffC.lamb_apply(w, m, v, lowp, tab.chunks, tab.wtab, hyper, EPS, norms)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ training steps
B = 8


def _mlp(ff):
    """Odd layer widths: no weight's size is a multiple of the arena padding."""
    from flexflow_amd.core import ActiMode, DataType
    x = ff.create_tensor([B, 37], DataType.DT_FLOAT)
    t = ff.dense(x, 61, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 43, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 11, name="d3"))
    rng = np.random.default_rng(0)
    return [(x, rng.standard_normal((B, 37)).astype(np.float32))], rng.integers(0, 11, (B, 1)).astype(np.int32)


def _bert(ff):
    from flexflow_amd.models.bert import BertConfig, build_bert
    bc = BertConfig.tiny(32)
    ids, pos, _ = build_bert(ff, B, bc)
    rng = np.random.default_rng(0)
    return ([(ids, rng.integers(0, bc.vocab, (B, bc.seq), dtype=np.int32)),
             (pos, np.tile(np.arange(bc.seq, dtype=np.int32), (B, 1)))],
            rng.integers(0, bc.vocab, (B, bc.seq, 1), dtype=np.int32))


def _model(kind, dtype, make_opt, flags=()):
    from flexflow_amd.core import FFConfig, FFModel, LossType, MetricsType
    cfg = FFConfig(["--search", "dp", "--no-hip-graphs", "--dtype", dtype, *flags])
    cfg.batch_size = B
    ff = FFModel(cfg)
    feeds, labels = (_mlp if kind == "mlp" else _bert)(ff)
    ff.optimizer = make_opt(ff)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    for t, a in feeds:
        t.set_tensor(ff, a)
    ff.label_tensor.set_tensor(ff, labels)
    return ff


@pytest.mark.parametrize("clip", [None, "below"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["mlp", "bert"])
def test_training_steps_match_float64(kind, dtype, clip):
    """Three eager steps; each update is compared with lamb_ref driven by the model's own
    gradients, weights and moments (read from the arenas just before the update)."""
    from flexflow_amd.core import LAMBOptimizer
    clip_norm = 1e-3 if clip else None  # far below any gradient norm of these models
    ff = _model(kind, dtype, lambda ff: LAMBOptimizer(ff, LR, B1, B2, WD, EPS, clip_norm=clip_norm))
    ex, opt = ff.executor, ff.optimizer
    assert ex._overlap_possible() is False  # LAMB needs every gradient before any weight moves
    slot = {}
    for L in ff.layers:
        for w in L.weights:
            slot.setdefault(w.guid, len(slot))
    arenas = [ar for ar in ex.arenas.values() if ar.size]
    assert arenas and any(len(sh) <= 1 for ar in arenas for *_, sh in ar.entries)
    if kind == "mlp":  # entries followed by padding
        assert any(n % 8 for ar in arenas for _, _, n, _ in ar.entries)
    for step in (1, 2, 3):
        ff.zero_gradients()
        ff.forward()
        ff.backward()
        torch.cuda.synchronize()
        snap, sumsq = [], 0.0
        for ar in arenas:
            m, v = opt.state[id(ar)]
            snap.append(tuple(_d(x[:ar.size]) for x in (ar.master, ar.grad, m, v)))
            for _, off, n, _ in ar.entries:
                sumsq += float((snap[-1][1][off:off + n] ** 2).sum())
        coef = 1.0
        if clip:
            norm = math.sqrt(sumsq)
            assert norm > clip_norm
            coef = clip_norm / (norm + 1e-6)
        ff.update()
        torch.cuda.synchronize()
        for ar, (w0, g, m0, v0) in zip(arenas, snap):
            ent = [(off, n, slot[w.guid], 0.0 if len(sh) <= 1 else WD, len(sh) > 1) for w, off, n, sh in ar.entries]
            w64, m64, v64, _ = K.lamb_ref(w0, g, m0, v0, ent, step, LR, B1, B2, EPS, coef=coef)
            m, v = opt.state[id(ar)]
            for name, got, ref in (("m", m, m64), ("v", v, v64), ("w", ar.master, w64)):
                _close(got[:ar.size], ref, _opt_tol(ref, 1), f"{kind} {dtype} {name} step {step}")
            assert float((w64 - w0).abs().max()) > 1e-4  # the step moved the weights
            if dtype == "bf16":
                assert torch.equal(ar.lowp[:ar.size], ar.master[:ar.size].bfloat16())
            else:
                assert ar.lowp is None
        if clip:
            assert abs(ff.get_grad_norm() - norm) <= 1e-5 * norm


def _run_model(make_opt, flags, steps):
    from flexflow_amd.core import FFConfig, FFModel
    from flexflow_amd.models import build
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = 64
    ff = FFModel(cfg)
    inputs, out, loss, mets, make_batch = build("mlp_unify", ff, 64, small=True)
    ff.optimizer = make_opt(ff)
    ff.compile(loss_type=loss, metrics=mets)
    rng = np.random.default_rng(0)
    for _ in range(steps):
        arrs, lab = make_batch(rng)
        for t, a in zip(inputs, arrs):
            t.set_tensor(ff, a)
        ff.label_tensor.set_tensor(ff, lab)
        ff.train_step()
    torch.cuda.synchronize()
    return ff, [np.asarray(w.get_weights(ff)) for L in ff.layers for w in L.weights]


def test_graph_captures_lamb_update(monkeypatch):
    """FF_GRAPH_UPDATE=1: the captured whole step holds both LAMB passes and the norms; its
    weights equal the eager run's bit for bit."""
    from flexflow_amd.core import LAMBOptimizer
    monkeypatch.setenv("FF_GRAPH_UPDATE", "1")

    def make(ff):
        return LAMBOptimizer(ff, 1e-3)

    ffe, b = _run_model(make, ["--no-hip-graphs"], 4)
    ff, a = _run_model(make, ["--hip-graphs"], 4)
    sg = ff._step_graph
    assert sg.graph is not None and not sg.failed
    assert sg._full_step(ff, ff.executor)
    assert ff.optimizer.hyper_dev is not None
    assert ff.optimizer.beta1_t == ffe.optimizer.beta1_t and ff.executor.step_idx == ffe.executor.step_idx == 4
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=str(k))


def test_adam_launches_no_lamb_kernel(monkeypatch):
    from flexflow_amd.core import AdamOptimizer

    def boom(*a, **kw):
        raise AssertionError("a LAMB entry point ran under Adam")

    for name in ("lamb_table", "lamb_moments", "lamb_norms", "lamb_apply"):
        monkeypatch.setattr(K, name, boom)
    ff = _model("mlp", "bf16", lambda ff: AdamOptimizer(ff, 1e-3))
    assert ff.executor._overlap_possible() is True
    for _ in range(2):
        ff.train_step()
    torch.cuda.synchronize()
    assert getattr(ff.executor, "_lamb", None) is None


def test_set_learning_rate_reaches_the_device():
    from flexflow_amd.core import LAMBOptimizer
    ff = _model("mlp", "fp32", lambda ff: LAMBOptimizer(ff, LR))
    ff.train_step()
    ff.optimizer.set_learning_rate(0.0)
    before = [ar.master.clone() for ar in ff.executor.arenas.values()]
    ff.train_step()
    torch.cuda.synchronize()
    assert ff.optimizer.hyper_dev[0].item() == 0.0
    for ar, w in zip(ff.executor.arenas.values(), before):
        assert torch.equal(ar.master, w)
