"""LAMB on the host: the kernels' CPU fallbacks against the float64 oracle lamb_ref, two gloo ranks
(data parallel, --zero, a parameter-split strategy) against the single-process run, checkpoint and
resume, the front ends that build a LAMBOptimizer, and the C / C++ declarations."""
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
LAMB = dict(lr=1e-2, beta1=0.9, beta2=0.999, weight_decay=0.01, epsilon=1e-6)


def _opt_tol(ref, step):
    """The project's optimizer tolerance: 16 fp32 ulps of max(1, |value|) per step taken."""
    return 16 * step * ULP32 * np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------------------------- fallbacks
def test_cpu_fallbacks_match_lamb_ref():
    from flexflow_amd import kernels as K
    C = K.LAMB_CHUNK
    sizes = [1, 7, 8, 9, C - 1, C + 1, 2 * C + 5, 37]
    ent, off = [], 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        ent.append((off, n, i, 0.0 if last else 0.01, not last))
        off += (n + 7) // 8 * 8
    size, nw = off, len(sizes)
    cut = ent[6][0] + C + 400  # inside the second chunk of the largest entry
    whole = [K.lamb_table(ent, [(0, size)], nw, size, "cpu")]
    split = [K.lamb_table(ent, [(0, cut)], nw, size, "cpu"), K.lamb_table(ent, [(cut, size)], nw, size, "cpu")]
    real = torch.zeros(size, dtype=torch.bool)
    for o, n, *_ in ent:
        real[o:o + n] = True
    for tabs, bias_correction, coef in ((whole, True, None), (split, True, 0.125), (whole, False, None)):
        gen = torch.Generator().manual_seed(3)
        w = torch.full((size,), 4096.0)
        w[real] = torch.randn(int(real.sum()), generator=gen)
        m, v, lowp = torch.zeros(size), torch.zeros(size), torch.full((size,), 4096.0, dtype=torch.bfloat16)
        w64, m64, v64 = w.double(), m.double(), v.double()
        gsd = torch.tensor([coef]) if coef else None
        for step in (1, 2, 3):
            g = torch.randn(size, generator=gen)
            rc = (1 / (1 - 0.9 ** step), 1 / (1 - 0.999 ** step)) if bias_correction else (1.0, 1.0)
            hyper = torch.tensor([1e-2, *rc])
            vecs = []
            for tab in tabs:
                part, norms = torch.zeros(2 * tab.n_chunks), torch.full((2 * nw,), 4096.0)
                K.lamb_moments(w, g, m, v, tab, hyper, gsd, 0.9, 0.999, 1e-6, part)
                K.lamb_norms(part, tab, True, norms)
                vecs.append(norms)
                zeros = torch.full((2 * nw,), 4096.0)
                K.lamb_norms(part, tab, False, zeros)
                assert not zeros.any()
            total = torch.stack(vecs).sum(0)
            for tab in tabs:
                K.lamb_apply(w, m, v, lowp, tab, hyper, 1e-6, total)
            w64, m64, v64, n64 = K.lamb_ref(w64, g, m64, v64, ent, step, 1e-2, 0.9, 0.999, 1e-6,
                                            bias_correction=bias_correction, coef=coef or 1.0)
            for got, ref in ((w, w64), (m, m64), (v, v64)):
                tol = torch.from_numpy(_opt_tol(ref.numpy(), step))
                assert bool(((got.double() - ref).abs()[real] <= tol[real]).all())
            np.testing.assert_allclose(total.view(-1, 2).double().numpy(), n64.numpy(), rtol=1e-5)
            assert torch.equal(lowp[real], w[real].bfloat16())
            assert bool((w[~real] == 4096.0).all()) and bool((lowp[~real] == 4096.0).all())  # padding untouched
            assert not m[~real].any() and not v[~real].any()


def test_table_rejects_bad_ranges():
    from flexflow_amd import kernels as K
    ent = [(0, 9, 0, 0.01, True), (16, 3, 1, 0.0, False)]
    for ranges in ([(2, 24)], [(0, 32)], [(0, 16), (8, 24)]):
        with pytest.raises(RuntimeError):
            K.lamb_table(ent, ranges, 2, 24, "cpu")
    with pytest.raises(RuntimeError):
        K.lamb_table([(0, 9, 0, 0.01, True), (10, 3, 1, 0.0, False)], [(0, 24)], 2, 24, "cpu")
    with pytest.raises(RuntimeError):
        K.lamb_table(ent, [(0, 24)], 2, 24, "cpu", owned=[1])


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
    """The three-Dense MLP of tests/test_grad_clip_cpu.py (40 -> 64 -> 48 -> 10; the 10-element bias
    is followed by padding in its arena), with the layer names of tests/dist_models.py."""
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel, LAMBOptimizer, LossType, MetricsType
    cfg = FFConfig(["--grad-bucket-mb", "0.02"] + flags)  # many small buckets
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 64, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 48, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 10, name="d3"), name="sm")
    ff.optimizer = LAMBOptimizer(ff, clip_norm=clip, **LAMB)
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
    """torch autograd in float64 for the gradients, the issue's formulas by hand for the update:
    the trust ratio, the decoupled decay and the 1-D exclusion all show at this tolerance."""
    res = _single()
    X, y = _data()
    X, y = torch.tensor(X, dtype=torch.float64), torch.tensor(y.reshape(-1), dtype=torch.int64)
    P = {k[5:]: torch.tensor(v, dtype=torch.float64, requires_grad=True)
         for k, v in res.items() if k.startswith("init.")}
    m = {k: torch.zeros_like(p) for k, p in P.items()}
    v = {k: torch.zeros_like(p) for k, p in P.items()}
    plain = {k: p.detach().clone() for k, p in P.items()}  # the same run without trust ratio and exclusion
    b1, b2, eps, lr, wd = LAMB["beta1"], LAMB["beta2"], LAMB["epsilon"], LAMB["lr"], LAMB["weight_decay"]
    for t in range(1, STEPS + 1):
        h = torch.relu(_lin(X, P["d1.0"], P["d1.1"]))
        h = torch.relu(_lin(h, P["d2.0"], P["d2.1"]))
        loss = torch.nn.functional.cross_entropy(_lin(h, P["d3.0"], P["d3.1"]), y)
        for p in P.values():
            p.grad = None
        loss.backward()
        with torch.no_grad():
            for k, p in P.items():
                m[k] = b1 * m[k] + (1 - b1) * p.grad
                v[k] = b2 * v[k] + (1 - b2) * p.grad ** 2
                adam = (m[k] / (1 - b1 ** t)) / ((v[k] / (1 - b2 ** t)).sqrt() + eps)
                lam = 0.0 if p.dim() <= 1 else wd
                u = adam + lam * p
                wn, un = p.norm(), u.norm()
                r = wn / un if p.dim() > 1 and wn > 0 and un > 0 else 1.0
                plain[k] -= lr * (adam + wd * plain[k])
                p -= lr * r * u
    for k, p in P.items():
        np.testing.assert_allclose(res[k], p.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    assert max(float((plain[k] - P[k].detach()).abs().max()) for k in P) > 1e-3  # the ratio is no no-op here


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


def _tp_strategy_file():
    """As tests/test_grad_clip_cpu.py: column-parallel d1 and d2 (each rank holds half of every
    weight, in a rank-private arena: the whole-weight norms need both halves), data-parallel d3."""
    sys.path.insert(0, HERE)
    import dist_models
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel
    from flexflow_amd.pcg.strategy import OpConfig, save_strategy
    cfg = FFConfig([])
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 64, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 48, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 10, name="d3"), name="sm")
    s = dist_models.strategy("mlp_tp", ff, 2)
    s["d2"] = OpConfig(s["d1"].degrees, s["d1"].devices)
    path = os.path.join(tempfile.mkdtemp(), "s.json")
    save_strategy(path, s, 2)
    return path


@pytest.mark.parametrize("mode", ["dp", "zero", "tp"])
def test_two_ranks_match_single_process(mode):
    single = _single()
    flags = {"dp": ["--search", "dp"], "zero": ["--search", "dp", "--zero"],
             "tp": ["--import-strategy", _tp_strategy_file()] if mode == "tp" else None}[mode]
    ranks = _run(flags)
    for k, v in single.items():
        # a shard counted twice or missed in a norm changes that weight's trust ratio
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
def test_front_ends_build_a_lamb_optimizer():
    from flexflow_amd import capi_impl
    from flexflow_amd.core import FFConfig, FFModel, LAMBOptimizer
    from flexflow_amd.core.optimizers import Optimizer
    from flexflow_amd.keras import optimizers as KO
    ff = FFModel(FFConfig([]))
    d = LAMBOptimizer(ff)
    assert (d.lr, d.beta1, d.beta2, d.weight_decay, d.epsilon) == (1e-3, 0.9, 0.999, 0.01, 1e-6)
    assert d.bias_correction and d.exclude_1d and d.clip_norm is None and isinstance(d, Optimizer)
    assert d.weight_rule((64, 40)) == (0.01, True) and d.weight_rule((64,)) == (0.0, False) \
        and d.weight_rule(()) == (0.0, False)
    assert LAMBOptimizer(ff, exclude_1d=False, weight_decay=0.1).weight_rule((64,)) == (0.1, True)
    k = KO.Lamb(learning_rate=0.02, beta_1=0.8, beta_2=0.95, epsilon=1e-5, weight_decay=0.1, bias_correction=False,
                exclude_1d=False, global_clipnorm=0.7)
    h = k.create_ffhandle(ff)
    assert isinstance(h, LAMBOptimizer)
    assert (h.lr, h.beta1, h.beta2, h.epsilon, h.weight_decay) == (0.02, 0.8, 0.95, 1e-5, 0.1)
    assert h.bias_correction is False and h.exclude_1d is False and h.clip_norm == 0.7
    k.set_learning_rate(0.5)
    assert h.lr == 0.5
    byname = KO.get("lamb")
    assert isinstance(byname, KO.Lamb) and isinstance(KO.get("LAMB").create_ffhandle(ff), LAMBOptimizer)
    c = capi_impl.lamb_create(ff, 0.03, 0.7, 0.9, 0.2, 1e-4, 0, 1)
    assert isinstance(c, LAMBOptimizer)
    assert (c.lr, c.beta1, c.beta2, c.weight_decay, c.epsilon) == (0.03, 0.7, 0.9, 0.2, 1e-4)
    assert c.bias_correction is False and c.exclude_1d is True
    capi_impl.optimizer_set_lr(c, 0.25)
    assert c.lr == 0.25
    clipped = FFModel(FFConfig(["--clip-grad-norm", "0.7"]))
    assert LAMBOptimizer(clipped).clip_norm == 0.7  # the config's threshold, as for SGD and Adam


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=float("nan")), dict(beta1=1.0), dict(beta1=-0.1),
                                dict(beta2=1.5), dict(weight_decay=-0.01), dict(epsilon=0.0), dict(epsilon=-1e-6),
                                dict(epsilon=float("inf")), dict(lr="fast"), dict(clip_norm=-1.0)])
def test_bad_hyper_parameters_raise(kw):
    from flexflow_amd.core import LAMBOptimizer
    with pytest.raises(ValueError):
        LAMBOptimizer(None, **kw)


def test_lamb_steps_need_the_executor():
    from flexflow_amd.core import LAMBOptimizer
    with pytest.raises(RuntimeError):
        LAMBOptimizer().step(None)


def test_cpp_and_c_declarations_build_and_run(tmp_path):
    """tests/capi/lamb_cpp/lamb.cc uses flexflow::LAMBOptimizer and the four C entry points; it is
    built by examples/cpp/build.sh, as the C++ examples are, and trains a few steps on the host."""
    lib = os.path.join(ROOT, "flexflow_amd", "libflexflow_c.so")
    if not os.path.exists(lib):
        sys.path.insert(0, ROOT)
        import build_ext
        build_ext.build_capi()
    ex = os.path.join(ROOT, "examples", "cpp")
    work = tmp_path / "lamb_cpp"
    work.mkdir()
    shutil.copy(os.path.join(HERE, "capi", "lamb_cpp", "lamb.cc"), work / "lamb.cc")
    subprocess.run([os.path.join(ex, "build.sh"), os.path.relpath(str(work), ex)], check=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([str(work / "lamb"), "-b", "4", "--iterations", "2"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "THROUGHPUT" in r.stdout and "C handle step ok" in r.stdout, r.stdout + r.stderr
