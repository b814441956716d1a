"""AdamW on the host: the float64 oracle adamw_ref against torch.optim.AdamW, the kernel's CPU
fallback against the oracle over whole and split ranges, the optimizer's chunk runs, training
against float64 autograd, two gloo ranks (data parallel, --zero) against the single process,
checkpoint and resume, the front ends that build an AdamWOptimizer, and the C / C++ declarations."""
import os
import shutil
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B = 8
ULP32 = 2.0 ** -23
STEPS = 3
ADAMW = dict(lr=1e-2, beta1=0.9, beta2=0.999, weight_decay=0.01, epsilon=1e-8)
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-8, 1e-2, 0.01


def _opt_tol(ref, step):
    """The project's optimizer tolerance: 16 fp32 ulps of max(1, |value|) per step taken."""
    return 16 * step * ULP32 * np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------------------ the hand-made arena
def _sizes():
    from flexflow_amd import kernels as K
    C = K.LAMB_CHUNK
    return [1, 7, 8, 9, C - 1, C, C + 1, 3 * C + 5, 37]


def _entries(lams=None):
    """Entries padded to 8 (WeightArena.add); lambda alternates WD, 0, WD, ... unless given."""
    ent, off = [], 0
    for i, n in enumerate(_sizes()):
        ent.append((off, n, i, (WD if i % 2 == 0 else 0.0) if lams is None else lams[i], False))
        off += (n + 7) // 8 * 8
    real = torch.zeros(off, dtype=torch.bool)
    for o, n, *_ in ent:
        real[o:o + n] = True
    return ent, off, real


# ------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("exclude_1d", [True, False])
def test_oracle_matches_torch_adamw(exclude_1d):
    """adamw_ref against torch.optim.AdamW on float64 parameters: two groups (decay / no decay), or
    one group when every entry decays. 1e-13 of max(1, |w|): about 100 float64 roundings."""
    from flexflow_amd import kernels as K
    ent, size, real = _entries(None if exclude_1d else [WD] * len(_sizes()))
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(size, generator=gen, dtype=torch.float64)
    params = [w[o:o + n].clone().requires_grad_(True) for o, n, *_ in ent]
    groups = {}
    for p, (_, _, _, lam, _) in zip(params, ent):
        groups.setdefault(lam, []).append(p)
    assert len(groups) == (2 if exclude_1d else 1)
    opt = torch.optim.AdamW([dict(params=ps, weight_decay=lam) for lam, ps in groups.items()], lr=LR,
                            betas=(B1, B2), eps=EPS, amsgrad=False)
    m, v = torch.zeros(size, dtype=torch.float64), torch.zeros(size, dtype=torch.float64)
    worst = 0.0
    for step in range(1, 6):
        g = torch.randn(size, generator=gen, dtype=torch.float64)
        for p, (o, n, *_) in zip(params, ent):
            p.grad = g[o:o + n].clone()
        opt.step()
        w0 = w
        w, m, v = K.adamw_ref(w, g, m, v, ent, step, LR, B1, B2, EPS)
        assert torch.equal(w[~real], w0[~real]) and not m[~real].any()  # elements in no entry are copied
        for p, (o, n, *_) in zip(params, ent):
            rel = ((w[o:o + n] - p.detach()).abs() / p.detach().abs().clamp_min(1.0)).max().item()
            worst = max(worst, rel)
    print(f"adamw_ref vs torch.optim.AdamW, 5 steps: worst relative difference {worst:.3e}")
    assert worst <= 1e-13


def test_oracle_clip_coefficient_scales_the_gradient_only():
    from flexflow_amd import kernels as K
    ent, size, _ = _entries()
    gen = torch.Generator().manual_seed(6)
    w, g = torch.randn(size, generator=gen), torch.randn(size, generator=gen)
    z = torch.zeros(size)
    a = K.adamw_ref(w, g, z, z, ent, 1, LR, B1, B2, EPS, coef=0.125)
    b = K.adamw_ref(w, 0.125 * g.double(), z, z, ent, 1, LR, B1, B2, EPS)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------- fallback
def _fallback_run(ent, size, real, runs_of, coef=None):
    """Three steps through K.adamw_update's CPU path; runs_of(table) -> [(c0, c1)] launched in turn."""
    from flexflow_amd import kernels as K
    gen = torch.Generator().manual_seed(3)
    w = torch.full((size,), 4096.0)
    w[real] = torch.randn(int(real.sum()), generator=gen)
    m, v, lowp = torch.zeros(size), torch.zeros(size), torch.full((size,), 4096.0, dtype=torch.bfloat16)
    w64, m64, v64 = w.double(), m.double(), v.double()
    gsd = torch.tensor([coef]) if coef else None
    tab, runs = runs_of()
    out = []
    for step in (1, 2, 3):
        g = torch.randn(size, generator=gen)
        g0 = g.clone()
        hyper = torch.tensor([LR, 1 / (1 - B1 ** step), 1 / (1 - B2 ** step)])
        for c0, c1 in runs:
            K.adamw_update(w, g, m, v, lowp, tab, c0, c1, hyper, gsd, B1, B2, EPS)
        w64, m64, v64 = K.adamw_ref(w64, g, m64, v64, ent, step, LR, B1, B2, EPS, coef=coef or 1.0)
        for got, ref in ((w, w64), (m, m64), (v, v64)):
            tol = torch.from_numpy(_opt_tol(ref.numpy(), step))
            assert bool(((got.double() - ref).abs()[real] <= tol[real]).all())
        assert torch.equal(g, g0)
        assert torch.equal(lowp[real], w[real].bfloat16())
        assert bool((w[~real] == 4096.0).all()) and bool((lowp[~real] == 4096.0).all())  # padding untouched
        assert not m[~real].any() and not v[~real].any()
        out.append((w.clone(), m.clone(), v.clone()))
    return out


def test_cpu_fallback_matches_adamw_ref_whole_and_split():
    from flexflow_amd import kernels as K
    C = K.LAMB_CHUNK
    ent, size, real = _entries()
    nw = len(ent)
    cut1 = ent[7][0] + C + 400  # inside the second chunk of the 3C+5 entry
    cut2 = ent[5][0]            # an entry boundary

    def whole():
        tab = K.lamb_table(ent, [(0, size)], nw, size, "cpu")
        return tab, [(0, tab.n_chunks)]

    def split():
        tab = K.lamb_table(ent, [(0, cut2), (cut2, cut1), (cut1, size)], nw, size, "cpu")
        starts = [s for s, _, _ in tab.rows()]
        assert (cut1 - 400, 400, 7) in tab.rows() and cut1 in starts and cut2 in starts
        a, b = starts.index(cut2), starts.index(cut1)
        return tab, [(b, tab.n_chunks), (a, b), (0, a)]  # three runs, in reverse order

    x = _fallback_run(ent, size, real, whole)
    y = _fallback_run(ent, size, real, split)
    for s, t in zip(x, y):
        for p, q in zip(s, t):
            assert torch.equal(p, q)  # elementwise arithmetic: the cut changes no bit
    _fallback_run(ent, size, real, whole, coef=0.125)
    tab, _ = whole()
    z = torch.zeros(size)
    for c0, c1 in ((-1, 2), (3, 2), (0, tab.n_chunks + 1)):
        with pytest.raises(RuntimeError):
            K.adamw_update(z, z, z, z, None, tab, c0, c1, torch.ones(3), None, B1, B2, EPS)


# ------------------------------------------------------------------------- the optimizer's chunk runs
class _Arena:
    def __init__(self, size):
        self.master = torch.zeros(size)
        self.grad = torch.zeros(size)
        self.lowp = None


def test_step_range_resolves_cuts_and_builds_tables_for_new_ranges():
    from flexflow_amd import kernels as K
    from flexflow_amd.core import AdamWOptimizer
    C = K.LAMB_CHUNK
    ent, size, real = _entries()
    opt = AdamWOptimizer(None, **ADAMW)
    ar = _Arena(size)
    with pytest.raises(RuntimeError):
        opt.step(ar)  # no table yet
    opt.init_state(ar)
    cut = ent[7][0] + C + 400
    opt.set_table(ar, ent, [0, cut, size])
    tabs = opt._plans[id(ar)].tables
    assert len(tabs) == 1
    ar.master[real] = 1.0
    ar.grad[:] = 0.5  # the padding too: an update that touched it would move it
    start = ar.master.clone()
    opt.next()
    opt.step_range(ar, cut, size)
    opt.step_range(ar, 0, cut)
    end9 = ent[3][0] + ent[3][1]  # the end of the 9-element entry: odd, but no chunk lies across it
    opt.step_range(ar, end9, end9)
    assert len(tabs) == 1  # every bound was a cut
    first = tabs[0][0]
    moved = ar.master != start
    assert torch.equal(moved, real)  # each element once, the padding never
    # a bound that is a multiple of 4 but no cut: one more table, the first one stays alive
    lo = ent[7][0] + 2 * C + 64
    before = ar.master.clone()
    opt.next()
    opt.step_range(ar, lo, size)
    assert len(tabs) == 2 and tabs[0][0] is first
    assert torch.equal(ar.master[:lo], before[:lo]) and bool((ar.master[lo:][real[lo:]] != before[lo:][real[lo:]]).all())
    opt.step_range(ar, lo, size)
    assert len(tabs) == 2  # cached
    with pytest.raises(RuntimeError):
        opt.step_range(ar, ent[7][0] + 6, size)  # inside a weight, not a multiple of 4
    with pytest.raises(RuntimeError):
        opt.step_range(ar, 0, size + 8)


# ------------------------------------------------------------------------------------- training
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():
    rng = np.random.default_rng(0)
    return rng.standard_normal((B, 40)).astype(np.float32), rng.integers(0, 10, (B, 1)).astype(np.int32)


def _model(flags, clip=None):
    """The three-Dense MLP of tests/test_lamb_cpu.py (40 -> 64 -> 48 -> 10; the 10-element bias is
    followed by padding in its arena), with the layer names of tests/dist_models.py."""
    from flexflow_amd.core import ActiMode, AdamWOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    cfg = FFConfig(["--grad-bucket-mb", "0.02"] + flags)  # many small buckets
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 64, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 48, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 10, name="d3"), name="sm")
    ff.optimizer = AdamWOptimizer(ff, clip_norm=clip, **ADAMW)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    X, y = _data()
    x.set_tensor(ff, X)
    ff.label_tensor.set_tensor(ff, y)
    return ff


def _weights(ff):
    return {f"{L.name}.{i}": np.asarray(w.get_weights(ff), dtype=np.float32)
            for L in ff.layers for i, w in enumerate(L.weights)}


def _train(flags, steps=STEPS):
    ff = _model(flags)
    res = {"init." + k: v for k, v in _weights(ff).items()}
    for _ in range(steps):
        ff.train_step()
    res.update(_weights(ff))
    return res


_SINGLE = {}


def _single():
    if not _SINGLE:
        _SINGLE.update(_train(["--search", "dp"]))
    return _SINGLE


def _lin(h, W, b):
    return (h @ W if W.shape[0] == h.shape[1] else h @ W.T) + b


def test_single_process_matches_float64_autograd():
    """A float64 torch replica trained with torch.optim.AdamW in two groups (matrices decay, biases
    do not); the coupled form (Adam with L2) and the decay of biases both show at this tolerance."""
    res = _single()
    X, y = _data()
    X, y = torch.tensor(X, dtype=torch.float64), torch.tensor(y.reshape(-1), dtype=torch.int64)
    kw = dict(lr=ADAMW["lr"], betas=(ADAMW["beta1"], ADAMW["beta2"]), eps=ADAMW["epsilon"])
    wd = ADAMW["weight_decay"]

    def replica(make_opt):
        P = {k[5:]: torch.tensor(v, dtype=torch.float64, requires_grad=True)
             for k, v in res.items() if k.startswith("init.")}
        opt = make_opt([p for p in P.values() if p.dim() > 1], [p for p in P.values() if p.dim() <= 1])
        for _ in range(STEPS):
            h = torch.relu(_lin(X, P["d1.0"], P["d1.1"]))
            h = torch.relu(_lin(h, P["d2.0"], P["d2.1"]))
            loss = torch.nn.functional.cross_entropy(_lin(h, P["d3.0"], P["d3.1"]), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return {k: p.detach().numpy() for k, p in P.items()}

    P = replica(lambda mats, vecs: torch.optim.AdamW([dict(params=mats, weight_decay=wd),
                                                      dict(params=vecs, weight_decay=0.0)], **kw))
    for k, p in P.items():
        np.testing.assert_allclose(res[k], p, rtol=1e-4, atol=1e-5, err_msg=k)
    # coupled decay (Adam with L2, what AdamOptimizer(weight_decay=) does) lands elsewhere
    L2 = replica(lambda mats, vecs: torch.optim.Adam([dict(params=mats, weight_decay=wd),
                                                      dict(params=vecs, weight_decay=0.0)], **kw))
    assert max(float(np.abs(L2[k] - P[k]).max()) for k in P) > 1e-3


def _worker(rank, world, port, flags, out_file):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world), FF_DIST_BACKEND="gloo")
    os.environ["CUDA_VISIBLE_DEVICES"] = ""
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    res = _train(flags)
    np.savez(out_file.replace(".npz", f"{rank}.npz"), **res)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def _run(flags, world=2):
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "out.npz")
    mp.start_processes(_worker, args=(world, _free_port(), flags, out), nprocs=world, join=True, start_method="spawn")
    return [dict(np.load(out.replace(".npz", f"{r}.npz"))) for r in range(world)]


@pytest.mark.parametrize("mode", ["dp", "zero"])
def test_two_ranks_match_single_process(mode):
    single = _single()
    flags = {"dp": ["--search", "dp"], "zero": ["--search", "dp", "--zero"]}[mode]
    ranks = _run(flags)
    for k, v in single.items():
        for r in range(2):
            err = np.abs(ranks[r][k].astype(np.float64) - v)
            tol = _opt_tol(v.astype(np.float64), STEPS)
            print(f"{mode} rank{r} {k}: max err {err.max():.3e}, allowed {tol.min():.3e}")
            assert (err <= tol).all(), (mode, r, k, float(err.max()))
        # the replicas of the two ranks do not drift apart
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=f"{mode} {k}")


def test_checkpoint_resume_matches_unbroken_run(tmp_path):
    ff = _model(["--search", "dp"])
    for _ in range(2):
        ff.train_step()
    ff.save_checkpoint(str(tmp_path / "ck"))
    ff2 = _model(["--search", "dp"])
    assert ff2.load_checkpoint(str(tmp_path / "ck")) == 2
    assert ff2.optimizer.beta1_t == ff.optimizer.beta1_t and ff2.optimizer.beta2_t == ff.optimizer.beta2_t
    for step in (3, 4):
        ff.train_step()
        ff2.train_step()
        a, b = _weights(ff), _weights(ff2)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"step {step} {k}")


# ------------------------------------------------------------------------------------ front ends
def test_front_ends_build_an_adamw_optimizer():
    from flexflow_amd import capi_impl
    from flexflow_amd.core import AdamWOptimizer, FFConfig, FFModel
    from flexflow_amd.core.optimizers import Optimizer
    from flexflow_amd.keras import optimizers as KO
    ff = FFModel(FFConfig([]))
    d = AdamWOptimizer(ff)
    assert (d.lr, d.beta1, d.beta2, d.weight_decay, d.epsilon) == (1e-3, 0.9, 0.999, 0.01, 1e-8)
    assert d.exclude_1d and d.clip_norm is None and isinstance(d, Optimizer) and not getattr(d, "two_phase", False)
    assert d.weight_rule((64, 40)) == 0.01 and d.weight_rule((64,)) == 0.0 and d.weight_rule(()) == 0.0
    assert AdamWOptimizer(ff, exclude_1d=False, weight_decay=0.1).weight_rule((64,)) == 0.1
    h = KO.AdamW().create_ffhandle(ff)  # Keras' own defaults: every variable decays
    assert isinstance(h, AdamWOptimizer)
    assert (h.lr, h.beta1, h.beta2, h.epsilon, h.weight_decay) == (0.001, 0.9, 0.999, 1e-7, 0.004)
    assert h.exclude_1d is False and h.clip_norm is None
    k = KO.AdamW(learning_rate=0.02, beta_1=0.8, beta_2=0.95, epsilon=1e-5, weight_decay=0.1, exclude_1d=True,
                 global_clipnorm=0.7)
    h = k.create_ffhandle(ff)
    assert (h.lr, h.beta1, h.beta2, h.epsilon, h.weight_decay) == (0.02, 0.8, 0.95, 1e-5, 0.1)
    assert h.exclude_1d is True and h.clip_norm == 0.7
    k.set_learning_rate(0.5)
    assert h.lr == 0.5
    byname = KO.get("adamw")
    assert isinstance(byname, KO.AdamW) and isinstance(KO.get("AdamW").create_ffhandle(ff), AdamWOptimizer)
    assert byname.create_ffhandle(ff).weight_decay == 0.004
    c = capi_impl.adamw_create(ff, 0.03, 0.7, 0.9, 0.2, 1e-4, 0)
    assert isinstance(c, AdamWOptimizer)
    assert (c.lr, c.beta1, c.beta2, c.weight_decay, c.epsilon) == (0.03, 0.7, 0.9, 0.2, 1e-4)
    assert c.exclude_1d is False
    capi_impl.optimizer_set_lr(c, 0.25)
    assert c.lr == 0.25
    clipped = FFModel(FFConfig(["--clip-grad-norm", "0.7"]))
    assert AdamWOptimizer(clipped).clip_norm == 0.7  # the config's threshold, as for SGD and Adam


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=float("nan")), dict(beta1=1.0), dict(beta1=-0.1),
                                dict(beta2=1.5), dict(weight_decay=-0.01), dict(epsilon=0.0), dict(epsilon=-1e-6),
                                dict(epsilon=float("inf")), dict(lr="fast"), dict(clip_norm=-1.0)])
def test_bad_hyper_parameters_raise(kw):
    from flexflow_amd.core import AdamWOptimizer
    with pytest.raises(ValueError) as e:
        AdamWOptimizer(None, **kw)
    assert next(iter(kw)) in str(e.value)


def test_adamw_steps_need_the_executor():
    from flexflow_amd.core import AdamWOptimizer
    with pytest.raises(RuntimeError):
        AdamWOptimizer().step(None)
    with pytest.raises(RuntimeError):
        AdamWOptimizer().step_range(None, 0, 8)


def test_cpp_and_c_declarations_build_and_run(tmp_path):
    """tests/capi/adamw_cpp/adamw.cc uses flexflow::AdamWOptimizer and the four C entry points; it
    is built by examples/cpp/build.sh, as the C++ examples are, and trains a few steps on the host."""
    lib = os.path.join(ROOT, "flexflow_amd", "libflexflow_c.so")
    if not os.path.exists(lib):
        sys.path.insert(0, ROOT)
        import build_ext
        build_ext.build_capi()
    ex = os.path.join(ROOT, "examples", "cpp")
    work = tmp_path / "adamw_cpp"
    work.mkdir()
    shutil.copy(os.path.join(HERE, "capi", "adamw_cpp", "adamw.cc"), work / "adamw.cc")
    subprocess.run([os.path.join(ex, "build.sh"), os.path.relpath(str(work), ex)], check=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([str(work / "adamw"), "-b", "4", "--iterations", "2"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "THROUGHPUT" in r.stdout and "C handle step ok" in r.stdout, r.stdout + r.stderr
