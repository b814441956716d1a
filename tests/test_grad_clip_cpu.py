"""Gradient clipping by global norm (clip_norm / --clip-grad-norm), on the host: parity with
torch.nn.utils.clip_grad_norm_ followed by this project's Adam / SGD recurrences in fp64, two gloo
ranks (data parallel, --zero, a parameter-split strategy) against the single-process clipped run,
and the ways the threshold reaches an optimizer."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
B = 8
CLIP = 0.5
ADAM = dict(alpha=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
SGD = dict(lr=0.05, momentum=0.9)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():
    rng = np.random.default_rng(0)
    return rng.standard_normal((B, 40)).astype(np.float32), rng.integers(0, 10, (B, 1)).astype(np.int32)


def _model(flags):
    """The three-Dense MLP of tests/test_zero_cpu.py (40 -> 64 -> 48 -> 10; the 10-element bias is
    no multiple of the arena's 8-element padding), with the layer names of tests/dist_models.py."""
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel
    cfg = FFConfig(["--grad-bucket-mb", "0.02"] + flags)  # many small buckets
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 64, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 48, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 10, name="d3"), name="sm")
    return ff, x


def _weights(ff):
    return {f"{L.name}.{i}": np.asarray(w.get_weights(ff), dtype=np.float32)
            for L in ff.layers for i, w in enumerate(L.weights)}


def _train(flags, kind, clip=CLIP, steps=3):
    from flexflow_amd.core import AdamOptimizer, LossType, MetricsType, SGDOptimizer
    ff, x = _model(flags)
    if kind == "adam":
        ff.optimizer = AdamOptimizer(ff, ADAM["alpha"], ADAM["beta1"], ADAM["beta2"], 0.0, ADAM["eps"], clip_norm=clip)
    else:
        ff.optimizer = SGDOptimizer(ff, SGD["lr"], SGD["momentum"], clip_norm=clip)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    X, y = _data()
    x.set_tensor(ff, X)
    ff.label_tensor.set_tensor(ff, y)
    res = {"init." + k: v for k, v in _weights(ff).items()}
    norms = []
    for _ in range(steps):
        ff.train_step()
        norms.append(ff.get_grad_norm())
    res.update(_weights(ff))
    res["norms"] = np.array(norms, dtype=np.float64)
    return res


def _lin(h, W, b):
    return (h @ W if W.shape[0] == h.shape[1] else h @ W.T) + b


def _reference(init, kind, clip=CLIP, steps=3):
    """torch in fp64: autograd gradients, clip_grad_norm_, then this project's recurrences by hand
    (torch.optim.Adam puts eps inside the bias correction: sqrt(v / (1 - b2^t)) + eps; the kernel
    computes alpha_t * m / (sqrt(v) + eps) with alpha_t = alpha * sqrt(1 - b2^t) / (1 - b1^t))."""
    X, y = _data()
    X = torch.tensor(X, dtype=torch.float64)
    y = torch.tensor(y.reshape(-1), dtype=torch.int64)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in init.items()}
    m = {k: torch.zeros_like(p) for k, p in P.items()}
    v = {k: torch.zeros_like(p) for k, p in P.items()}
    norms = []
    b1t = b2t = 1.0
    for _ in range(steps):
        h = torch.relu(_lin(X, P["d1.0"], P["d1.1"]))
        h = torch.relu(_lin(h, P["d2.0"], P["d2.1"]))
        loss = torch.nn.functional.cross_entropy(_lin(h, P["d3.0"], P["d3.1"]), y)
        for p in P.values():
            p.grad = None
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(P.values()), clip)))
        with torch.no_grad():
            if kind == "adam":
                b1t *= ADAM["beta1"]
                b2t *= ADAM["beta2"]
                alpha_t = ADAM["alpha"] * (1 - b2t) ** 0.5 / (1 - b1t)
            for k, p in P.items():
                g = p.grad
                if kind == "adam":
                    m[k] = ADAM["beta1"] * m[k] + (1 - ADAM["beta1"]) * g
                    v[k] = ADAM["beta2"] * v[k] + (1 - ADAM["beta2"]) * g * g
                    p -= alpha_t * m[k] / (v[k].sqrt() + ADAM["eps"])
                else:
                    m[k] = SGD["momentum"] * m[k] + g
                    p -= SGD["lr"] * m[k]
    return {k: p.detach().numpy() for k, p in P.items()}, norms


_SINGLE = {}


def _single(kind):
    if kind not in _SINGLE:
        _SINGLE[kind] = _train(["--search", "dp"], kind)
    return _SINGLE[kind]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_matches_torch_clip_grad_norm(kind):
    res = _single(kind)
    init = {k[5:]: v for k, v in res.items() if k.startswith("init.")}
    ref, norms = _reference(init, kind)
    assert all(n > CLIP for n in norms), norms  # every step clips
    np.testing.assert_allclose(res["norms"], norms, rtol=1e-5)
    for k, v in ref.items():
        np.testing.assert_allclose(res[k], v, rtol=1e-4, atol=1e-5, err_msg=k)
    # and the clipping is not a no-op at this tolerance
    unclipped, _ = _reference(init, kind, clip=1e30)
    assert max(np.abs(unclipped[k] - ref[k]).max() for k in ref) > 1e-3


def _worker(rank, world, port, flags, out_file):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world), FF_DIST_BACKEND="gloo")
    os.environ["CUDA_VISIBLE_DEVICES"] = ""
    sys.path.insert(0, os.path.dirname(HERE))
    torch.set_num_threads(1)
    res = _train(flags, "adam")
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
    """dist_models' mlp_tp strategy: column-parallel d1 (a parameter-split Linear), data-parallel d3;
    d2 column-parallel too (mlp_tp's row-parallel d2 has no activation, this model's d2 has a
    ReLU). d1 / d2's shards are rank-private arenas, d3's is replicated over both ranks."""
    sys.path.insert(0, HERE)
    import dist_models
    from flexflow_amd.pcg.strategy import OpConfig, save_strategy
    ff, _ = _model([])
    s = dist_models.strategy("mlp_tp", ff, 2)
    s["d2"] = OpConfig(s["d1"].degrees, s["d1"].devices)
    path = os.path.join(tempfile.mkdtemp(), "s.json")
    save_strategy(path, s, 2)
    return path


@pytest.mark.parametrize("mode", ["dp", "zero", "tp"])
def test_two_ranks_match_single_process(mode):
    single = _single("adam")
    flags = {"dp": ["--search", "dp"], "zero": ["--search", "dp", "--zero"],
             "tp": ["--import-strategy", _tp_strategy_file()] if mode == "tp" else None}[mode]
    ranks = _run(flags)
    assert all(n > CLIP for n in single["norms"])
    for r in range(2):
        # a replica counted twice or a shard missed shows here first
        np.testing.assert_allclose(ranks[r]["norms"], single["norms"], rtol=1e-5, err_msg=f"{mode} rank{r} norm")
        for k, v in single.items():
            if k != "norms":
                np.testing.assert_allclose(ranks[r][k], v, rtol=1e-4, atol=1e-5, err_msg=f"{mode} rank{r} {k}")


def test_config_and_front_ends():
    from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, SGDOptimizer
    from flexflow_amd.keras.optimizers import SGD as KSGD, Adam as KAdam
    ff = FFModel(FFConfig(["--clip-grad-norm", "0.7"]))
    assert ff.config.clip_grad_norm == 0.7
    assert AdamOptimizer(ff, 1e-3).clip_norm == 0.7 and SGDOptimizer(ff, 0.1).clip_norm == 0.7
    assert AdamOptimizer(ff, 1e-3, clip_norm=0.3).clip_norm == 0.3  # the keyword wins
    assert SGDOptimizer(ff, 0.1, clip_norm=0).clip_norm is None     # and can switch it off
    plain = FFModel(FFConfig([]))
    assert plain.config.clip_grad_norm == 0.0
    assert AdamOptimizer(plain, 1e-3).clip_norm is None and SGDOptimizer().clip_norm is None
    assert plain.get_grad_norm() is None
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            AdamOptimizer(plain, 1e-3, clip_norm=bad)
        with pytest.raises(ValueError):
            SGDOptimizer(plain, 0.1, clip_norm=bad)
    assert KAdam(global_clipnorm=0.7).create_ffhandle(plain).clip_norm == 0.7
    assert KSGD(global_clipnorm=0.7).create_ffhandle(plain).clip_norm == 0.7
    # per-variable clipnorm and element-wise clipvalue stay unimplemented and ignored
    assert KAdam(clipnorm=1.0, clipvalue=0.5).create_ffhandle(plain).clip_norm is None


def test_cpu_fallbacks_of_the_kernels():
    from flexflow_amd import kernels as K
    x = torch.arange(11, dtype=torch.float32)
    ws, out = torch.empty(K.GRAD_SUMSQ_PARTIALS), torch.full((1,), 5.0)
    K.grad_sumsq(x, ws, out)
    assert out.item() == 385.0
    K.grad_sumsq(x[:4], ws, out, accumulate=True)
    assert out.item() == 399.0
    norm, coef = torch.zeros(1), torch.zeros(1)
    K.clip_coef(torch.tensor([4.0]), 1.0, norm, coef)
    assert norm.item() == 2.0 and abs(coef.item() - 1 / (2 + 1e-6)) < 1e-7
    K.clip_coef(torch.tensor([0.25]), 1.0, norm, coef)
    assert coef.item() == 1.0
    # gscale_dev multiplies gscale and leaves the weight-decay term alone
    w, g = torch.ones(5), torch.full((5,), 2.0)
    K.sgd_update(w, g, None, None, 0.1, 0.0, False, 0.5, 0.5, gscale_dev=torch.tensor([0.25]))
    np.testing.assert_allclose(w.numpy(), 1 - 0.1 * (2 * 0.125 + 0.5), rtol=1e-6)
