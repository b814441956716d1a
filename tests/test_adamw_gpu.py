"""AdamW on the device: the one-pass chunk-table kernel (adamw_update) against the float64 oracle
kernels.adamw_ref — whole arena, split ranges, partial runs, decoupling, a clip coefficient from
the device, a NaN gradient, argument checks — and AdamW training steps (eager, clipped, overlapped
with the backward, captured into a hipGraph)."""
import math

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ULP32 = 2.0 ** -23
GUARD = 4096.0  # exact in bf16
C = K.LAMB_CHUNK
MARGIN = 16     # guard elements on each side of every buffer (64 bytes: the slices stay aligned)
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-8, 1e-2, 0.01
NAMES = ("w", "m", "v", "lowp")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.detach().cpu().double()


def _close(got, ref64, atol, what):
    err = (_d(got) - ref64).abs() - atol
    i = int(err.argmax())
    assert err[i] <= 0, f"{what}: element {i}: got {_d(got)[i].item()!r}, ref {ref64[i].item()!r}"


def _opt_tol(ref64, step):
    """The project's optimizer tolerance (tests/test_lamb_gpu.py, tests/test_grad_clip_gpu.py):
    16 fp32 ulps of max(1, |value|) per step taken."""
    return 16 * step * ULP32 * ref64.abs().clamp_min(1.0)


# --------------------------------------------------------------------------------- the hand-made arena
SIZES = [1, 7, 8, 9, C - 1, C, C + 1, 3 * C + 5, 37]


def _entries(sizes=SIZES):
    """Entries padded to 8 (WeightArena.add); lambda alternates WD, 0, WD, ...: every entry boundary
    is a change of lambda."""
    ent, off = [], 0
    for i, n in enumerate(sizes):
        ent.append((off, n, i, WD if i % 2 == 0 else 0.0, False))
        off += (n + 7) // 8 * 8
    return ent, off


class Arena:
    """w, g, m, v (and a bf16 copy) with GUARD in all padding and around the buffers."""

    def __init__(self, ent, size, seed):
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
        self.buf["lowp"] = torch.full((size + 2 * MARGIN,), GUARD, dtype=BF16, device=DEV)
        self.hyper = torch.zeros(3, device=DEV)

    def t(self, name):
        return self.buf[name][MARGIN:MARGIN + self.size]

    def set_grad(self, seed=None, host=None):
        if host is None:
            host = torch.full((self.size,), GUARD)
            host[self.real] = torch.randn(int(self.real.sum()), generator=_gen(seed))
        self.t("g").copy_(host)
        return host

    def set_hyper(self, step, lr=LR):
        self.hyper.copy_(torch.tensor([lr, 1 / (1 - B1 ** step), 1 / (1 - B2 ** step)], dtype=F32))

    def update(self, tab, c0, c1, gscale_dev=None, max_blocks=0):
        K.adamw_update(self.t("w"), self.t("g"), self.t("m"), self.t("v"), self.t("lowp"), tab, c0, c1, self.hyper,
                       gscale_dev, B1, B2, EPS, max_blocks=max_blocks)

    def snap(self):
        return {k: self.t(k).clone() for k in NAMES}

    def check_guards(self, what):
        pad = ~self.real.to(DEV)
        for name, b in self.buf.items():
            assert bool((b[:MARGIN] == GUARD).all()) and bool((b[-MARGIN:] == GUARD).all()), f"{what}: {name} margin"
            assert bool((b[MARGIN:MARGIN + self.size][pad] == GUARD).all()), f"{what}: {name} padding"


def _whole(ent, size):
    tab = K.lamb_table(ent, [(0, size)], len(ent), size, DEV)
    return tab, [(0, tab.n_chunks)]


def _cuts(ent, size):
    """A table cut inside the second chunk of the 3C+5 entry and at one entry boundary."""
    cut1, cut2 = ent[7][0] + C + 400, ent[5][0]
    tab = K.lamb_table(ent, [(0, cut2), (cut2, cut1), (cut1, size)], len(ent), size, DEV)
    rows = tab.rows()
    starts = [s for s, _, _ in rows]
    assert (cut1 - 400, 400, 7) in rows and cut1 in starts and cut2 in starts
    a, b = starts.index(cut2), starts.index(cut1)
    return tab, a, b


def _split(ent, size):
    tab, a, b = _cuts(ent, size)
    return tab, [(b, tab.n_chunks), (a, b), (0, a)]  # three launches, in reverse order


def _run(runs_of, steps=3, seed=7, coef=None, max_blocks=0):
    """steps AdamW steps on a fresh arena; after each one w, m, v are checked against adamw_ref
    run in float64 from the start, the bf16 copy, the gradient and every guard too."""
    ent, size = _entries()
    ar = Arena(ent, size, seed)
    tab, runs = runs_of(ent, size)
    w64, m64, v64 = (ar.host[k].double() for k in ("w", "m", "v"))
    gsd = torch.tensor([coef], device=DEV) if coef is not None else None
    real, rd = ar.real, ar.real.to(DEV)
    out = []
    for step in range(1, steps + 1):
        g = ar.set_grad(1000 * seed + step)
        ar.set_hyper(step)
        g_before = ar.t("g").clone()
        for c0, c1 in runs:
            ar.update(tab, c0, c1, gsd, max_blocks)
        torch.cuda.synchronize()
        w64, m64, v64 = K.adamw_ref(w64, g, m64, v64, ent, step, LR, B1, B2, EPS, coef=1.0 if coef is None else coef)
        for name, ref in (("m", m64), ("v", v64), ("w", w64)):
            err = ((_d(ar.t(name)) - ref).abs() / ref.abs().clamp_min(1.0))[real].max().item() / ULP32
            print(f"step {step} {name}: worst error {err:.2f} ulp of max(1, |ref|), allowed {16 * step}")
            _close(ar.t(name)[rd], ref[real], _opt_tol(ref[real], step), f"{name} step {step}")
        assert torch.equal(ar.t("lowp")[rd], ar.t("w")[rd].bfloat16()), f"lowp step {step}"
        assert torch.equal(ar.t("g"), g_before), "the gradient was written"
        ar.check_guards(f"step {step}")
        out.append(ar.snap())
    return out


_UNSPLIT = {}


def _unsplit():
    if not _UNSPLIT:
        _UNSPLIT["run"] = _run(_whole)
    return _UNSPLIT["run"]


def _same_bits(a, b):
    for x, y in zip(a, b):
        for k in NAMES:
            assert torch.equal(x[k], y[k]), k


def test_three_steps_match_float64():
    _unsplit()


def test_second_run_gives_the_same_bits():
    _same_bits(_unsplit(), _run(_whole))


def test_three_ranges_in_reverse_order_equal_one_launch():
    _same_bits(_unsplit(), _run(_split))


def test_capped_grid_strides_over_the_chunks():
    """max_blocks = 3: three workgroups take the arena's chunks in turn; the bits do not change."""
    _same_bits(_unsplit(), _run(_whole, max_blocks=3))


def test_partial_run_changes_nothing_outside_it():
    ent, size = _entries()
    ar = Arena(ent, size, 7)
    tab, a, b = _cuts(ent, size)
    rows = tab.rows()
    lo, hi = rows[a][0], rows[b][0]
    ar.set_grad(7001)
    ar.set_hyper(1)
    before = ar.snap()
    ar.update(tab, a, b)
    torch.cuda.synchronize()
    after = ar.snap()
    inside = torch.zeros(size, dtype=torch.bool)
    inside[lo:hi] = True
    inside &= ar.real
    ins, outs = inside.to(DEV), (~inside).to(DEV)
    for k in NAMES:
        assert torch.equal(after[k][outs], before[k][outs]), k
        assert bool((after[k][ins] != before[k][ins]).any()), k
    # and inside it has the bits of the whole-arena launch
    for k in NAMES:
        assert torch.equal(after[k][ins], _unsplit()[0][k][ins]), k
    ar.check_guards("partial run")


def test_decay_is_decoupled_from_the_moments():
    """g = 0, m = v = 0: the decayed entries shrink by (1 - lr * WD) and the moments stay zero; the
    others keep every bit. Adam's coupled weight decay moves m off zero on the same input."""
    ent, size = _entries()
    ar = Arena(ent, size, 7)
    host = torch.full((size,), GUARD)
    host[ar.real] = 0.0
    ar.set_grad(host=host)
    ar.set_hyper(1)
    w0 = ar.t("w").clone()
    tab, runs = _whole(ent, size)
    ar.update(tab, *runs[0])
    torch.cuda.synchronize()
    w = ar.t("w")
    for off, n, _, lam, _ in ent:
        s = slice(off, off + n)
        assert not ar.t("m")[s].any() and not ar.t("v")[s].any()
        if lam == 0.0:
            assert torch.equal(w[s], w0[s])
        else:
            ref = _d(w0[s]) * (1 - LR * WD)
            ulp = 2.0 ** torch.floor(torch.log2(ref.abs())) * ULP32  # one fp32 ulp at |ref|
            assert bool(((_d(w[s]) - ref).abs() <= ulp).all()), off
            assert bool((w[s] != w0[s]).any())
    ar.check_guards("decoupling")
    n = ent[7][1]
    s = slice(ent[7][0], ent[7][0] + n)
    m = torch.zeros(n, device=DEV)
    K.adam_update(w0[s].clone(), torch.zeros(n, device=DEV), m, torch.zeros(n, device=DEV), None, LR, B1, B2, WD, EPS)
    assert bool((m != 0).any())  # coupled (L2) decay goes through the moments


def test_clip_coefficient_from_the_device():
    _run(_whole, steps=2, coef=0.125)


def test_nan_gradient_stays_in_its_element():
    ent, size = _entries()
    tab, runs = _whole(ent, size)
    bad = ent[7][0] + C + 3
    res = []
    for val in (float("nan"), 0.0):
        ar = Arena(ent, size, 11)
        g = ar.host["g"].clone()
        g[bad] = val
        ar.set_grad(host=g)
        ar.set_hyper(1)
        ar.update(tab, *runs[0])
        torch.cuda.synchronize()
        ar.check_guards("nan")
        res.append(ar.snap())
    nan, fin = res
    others = torch.ones(size, dtype=torch.bool, device=DEV)
    others[bad] = False
    for k in NAMES:
        assert math.isnan(nan[k][bad].item()), k
        assert bool(torch.isfinite(fin[k].float()).all()), k
        assert torch.equal(nan[k][others], fin[k][others]), k


# ---------------------------------------------------------------------------------- argument checks
def test_bad_arguments_raise(ffC):
    ent, size = _entries([C + 9, 11])
    tab = K.lamb_table(ent, [(0, size)], 2, size, DEV)
    w, g, m, v = (torch.zeros(size, device=DEV) for _ in range(4))
    lowp = torch.zeros(size, dtype=BF16, device=DEV)
    hyper = torch.tensor([LR, 1.0, 1.0], device=DEV)
    names = ("master", "grad", "m", "v", "lowp", "chunks", "wtab", "c0", "c1", "hyper", "gscale_dev", "b1", "b2",
             "eps", "max_blocks")
    ok = (w, g, m, v, lowp, tab.chunks, tab.wtab, 0, tab.n_chunks, hyper, None, B1, B2, EPS, 0)
    ffC.adamw_update(*ok)

    def bad(**kw):
        a = dict(zip(names, ok)) | kw
        with pytest.raises(RuntimeError):
            ffC.adamw_update(*[a[k] for k in names])

    bad(grad=g.double())                                       # wrong dtype
    bad(m=m.bfloat16())
    bad(lowp=lowp.float())
    bad(chunks=tab.chunks.int())                               # the table's dtype
    bad(wtab=tab.wtab.long())
    bad(master=torch.zeros(size + 4, device=DEV)[1:size + 1])  # not 16-byte aligned
    bad(v=torch.zeros(size - 8, device=DEV))                   # a shorter state than the arena
    bad(lowp=lowp[:-8])
    bad(c1=tab.n_chunks + 1)
    bad(c0=2, c1=1)
    bad(c0=-1)
    bad(hyper=hyper[:2])
    bad(hyper=hyper.cpu())
    bad(gscale_dev=torch.ones(2, device=DEV))
    ffC.adamw_update(*ok)
    K.adamw_update(w, g, m, v, lowp, tab, 0, tab.n_chunks, hyper, torch.ones(1, device=DEV), B1, B2, EPS)
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


def _adamw(ff, **kw):
    from flexflow_amd.core import AdamWOptimizer
    return AdamWOptimizer(ff, LR, B1, B2, WD, EPS, **kw)


@pytest.mark.parametrize("clip", [None, "below"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["mlp", "bert"])
def test_training_steps_match_float64(kind, dtype, clip):
    """Three eager steps; each update is compared with adamw_ref driven by the model's own
    gradients, weights and moments (read from the arenas just before the update)."""
    clip_norm = 1e-3 if clip else None  # far below any gradient norm of these models
    ff = _model(kind, dtype, lambda ff: _adamw(ff, clip_norm=clip_norm))
    ex, opt = ff.executor, ff.optimizer
    assert ex._overlap_possible() is (clip is None)
    arenas = [ar for ar in ex.arenas.values() if ar.size]
    assert arenas and any(len(sh) <= 1 for ar in arenas for *_, sh in ar.entries)  # some entry has lambda = 0
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
            ent = [(off, n, i, 0.0 if len(sh) <= 1 else WD, False) for i, (_, off, n, sh) in enumerate(ar.entries)]
            w64, m64, v64 = K.adamw_ref(w0, g, m0, v0, ent, step, LR, B1, B2, EPS, coef=coef)
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


def _masters(ff):
    return [ar.master.clone() for ar in ff.executor.arenas.values() if ar.size]


@pytest.mark.parametrize("kind", ["mlp", "bert"])
def test_overlapped_update_equals_the_update_after_the_backward(kind, monkeypatch):
    """The per-bucket launches on the side stream (cut into small FF_UPD_CHUNK pieces here, so a
    bucket is several launches) and the whole-arena launch after the backward give equal bits."""
    monkeypatch.setenv("FF_UPD_CHUNK", "1024")
    res = []
    for flags in ((), ("--no-overlap-update",)):
        ff = _model(kind, "bf16", _adamw, ("--grad-bucket-mb", "0.02", *flags))
        assert ff.executor._overlap_possible() is True
        calls = []
        orig = ff.optimizer.step_range
        ff.optimizer.step_range = lambda *a, _o=orig, **kw: (calls.append(a[1:3]), _o(*a, **kw))[1]
        for _ in range(3):
            ff.train_step()
        torch.cuda.synchronize()
        res.append((_masters(ff), calls))
    (a, ca), (b, cb) = res
    assert len(set(ca)) > 1 and len(cb) <= 3 * len(a)  # ranged launches on one side, whole arenas on the other
    for x, y in zip(a, b):
        assert torch.equal(x, y)


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


def test_graph_captures_adamw_update(monkeypatch):
    """FF_GRAPH_UPDATE=1: the captured whole step holds the AdamW launches; its weights equal the
    eager run's bit for bit."""
    from flexflow_amd.core import AdamWOptimizer
    monkeypatch.setenv("FF_GRAPH_UPDATE", "1")

    def make(ff):
        return AdamWOptimizer(ff, 1e-3)

    ffe, b = _run_model(make, ["--no-hip-graphs"], 4)
    ff, a = _run_model(make, ["--hip-graphs"], 4)
    sg = ff._step_graph
    assert sg.graph is not None and not sg.failed
    assert sg._full_step(ff, ff.executor)
    assert ff.optimizer.hyper_dev is not None
    assert ff.optimizer.beta1_t == ffe.optimizer.beta1_t and ff.executor.step_idx == ffe.executor.step_idx == 4
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=str(k))


@pytest.mark.parametrize("wd", [WD, 0.0])
def test_set_learning_rate_reaches_the_device(wd):
    from flexflow_amd.core import AdamWOptimizer
    ff = _model("mlp", "fp32", lambda ff: AdamWOptimizer(ff, LR, weight_decay=wd))
    ff.train_step()
    ff.optimizer.set_learning_rate(0.0)
    before = _masters(ff)
    ff.train_step()
    torch.cuda.synchronize()
    assert ff.optimizer.hyper_dev[0].item() == 0.0
    arenas = [ar for ar in ff.executor.arenas.values() if ar.size]
    for ar, w in zip(arenas, before):
        for _, off, n, sh in ar.entries:
            if wd == 0.0 or len(sh) <= 1:  # lambda = 0: no bit changes (elsewhere w - 0 * u is w too)
                assert torch.equal(ar.master[off:off + n], w[off:off + n])
        assert torch.equal(ar.master, w)


@pytest.mark.parametrize("which", ["adam", "lamb"])
def test_adam_and_lamb_call_no_adamw_entry_point(which, monkeypatch):
    from flexflow_amd.core import AdamOptimizer, LAMBOptimizer
    from flexflow_amd.core.optimizers import AdamWOptimizer

    def boom(*a, **kw):
        raise AssertionError(f"an AdamW entry point ran under {which}")

    monkeypatch.setattr(K, "adamw_update", boom)
    monkeypatch.setattr(AdamWOptimizer, "set_table", boom)
    ff = _model("mlp", "bf16", lambda ff: (AdamOptimizer if which == "adam" else LAMBOptimizer)(ff, 1e-3))
    assert ff.executor._overlap_possible() is (which == "adam")
    for _ in range(2):
        ff.train_step()
    torch.cuda.synchronize()
    assert getattr(ff.executor, "_adamw_key", None) is None
