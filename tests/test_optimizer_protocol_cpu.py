"""What the runtime asks of an optimizer (core/optimizers.py: ranged, two_phase, chunk_table,
capturable, use_device_alpha, state_tensors), on the host: user optimizers that implement step()
alone or step_range(arena, lo, hi) without max_blocks, state_tensors of every optimizer,
determinism_check over a bare momentum tensor, and checkpoints of SGD with momentum and of AdamW
(the saved tensor keys, and the state bit for bit after loading)."""
import numpy as np
import pytest
import torch

B = 8


def _mlp(make_opt):
    """Two Dense layers (40 -> 32 -> 10): weights of 1280, 32, 320 and 10 elements."""
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel, LossType, MetricsType
    cfg = FFConfig(["--search", "dp"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 32, ActiMode.AC_MODE_RELU, name="d1")
    ff.softmax(ff.dense(t, 10, name="d2"), name="sm")
    ff.optimizer = make_opt(ff)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    x.set_tensor(ff, rng.standard_normal((B, 40)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (B, 1)).astype(np.int32))
    return ff


def _arenas(ff):
    return [ar for ar in ff.executor.arenas.values() if ar.size]


def _masters(ff):
    return [ar.master.clone() for ar in _arenas(ff)]


def _make(which):
    from flexflow_amd.core import AdamOptimizer, AdamWOptimizer, LAMBOptimizer, SGDOptimizer
    return {"sgd": lambda ff: SGDOptimizer(ff, 0.05), "sgdm": lambda ff: SGDOptimizer(ff, 0.05, momentum=0.9),
            "adam": lambda ff: AdamOptimizer(ff, 1e-2), "adamw": lambda ff: AdamWOptimizer(ff, 1e-2),
            "lamb": lambda ff: LAMBOptimizer(ff, 1e-2)}[which]


def test_step_only_optimizer_trains_and_is_never_overlapped():
    from flexflow_amd.core.optimizers import Optimizer

    class Plain(Optimizer):
        def step(self, arena):
            arena.master.sub_(self.lr * arena.grad)

    ff = _mlp(lambda ff: Plain(ff, 0.05))
    opt = ff.optimizer
    assert not opt.ranged and not opt.two_phase and not opt.chunk_table and not opt.capturable
    assert ff.executor._overlap_possible() is False
    w0 = _masters(ff)
    ff.train_step()
    w1 = _masters(ff)
    ff.train_step()
    w2 = _masters(ff)
    assert all(not torch.equal(a, b) for a, b in zip(w0, w1)) and all(not torch.equal(a, b) for a, b in zip(w1, w2))
    # the same two steps by SGDOptimizer without momentum: w -= lr * g
    ref = _mlp(_make("sgd"))
    for _ in range(2):
        ref.train_step()
    for a, b in zip(w2, _masters(ref)):
        assert torch.equal(a, b)


def test_step_range_without_max_blocks_counts_as_ranged():
    from flexflow_amd.core.optimizers import Optimizer

    class Ranged(Optimizer):
        def step(self, arena):
            self.step_range(arena, 0, arena.master.numel())

        def step_range(self, arena, lo, hi):
            arena.master[lo:hi].sub_(self.lr * arena.grad[lo:hi])

    assert Ranged(None, 0.05).ranged
    assert not Optimizer().ranged
    ff = _mlp(lambda ff: Ranged(ff, 0.05))
    ref = _mlp(_make("sgd"))
    for _ in range(2):
        ff.train_step()
        ref.train_step()
    for a, b in zip(_masters(ff), _masters(ref)):
        assert torch.equal(a, b)


def test_declared_defaults_of_the_shipped_optimizers():
    from flexflow_amd.core import AdamOptimizer, AdamWOptimizer, LAMBOptimizer, SGDOptimizer
    from flexflow_amd.core.optimizers import Optimizer
    # (ranged, two_phase, chunk_table, capturable)
    want = {Optimizer: (False, False, False, False), SGDOptimizer: (True, False, False, False),
            AdamOptimizer: (True, False, False, True), AdamWOptimizer: (True, False, True, True),
            LAMBOptimizer: (False, True, False, True)}
    for cls, flags in want.items():
        o = cls()
        assert (o.ranged, o.two_phase, o.chunk_table, o.capturable) == flags, cls.__name__
        assert o.use_device_alpha("cpu") is None  # every optimizer has the hook


@pytest.mark.parametrize("which", ["sgd", "sgdm", "adam", "adamw", "lamb"])
def test_state_tensors(which):
    from flexflow_amd.core.optimizers import Optimizer
    ff = _mlp(_make(which))
    opt = ff.optimizer
    for ar in _arenas(ff):
        assert Optimizer().state_tensors(ar) == ()
        st = opt.state_tensors(ar)
        assert isinstance(st, tuple) and len(st) == {"sgd": 0, "sgdm": 1}.get(which, 2)
        held = opt.state.get(id(ar))
        if which == "sgdm":
            assert st[0] is held  # the momentum tensor itself, not its rows
        elif which != "sgd":
            assert st[0] is held[0] and st[1] is held[1]
        assert all(t.shape == ar.master.shape for t in st)


def test_determinism_check_with_sgd_momentum():
    from flexflow_amd.runtime.health import determinism_check
    ff = _mlp(_make("sgdm"))
    ff.train_step()  # a non-zero momentum to restore
    w, mom = _masters(ff), [ff.optimizer.state_tensors(ar)[0].clone() for ar in _arenas(ff)]
    assert determinism_check(ff, steps=2) is True
    for ar, a, b in zip(_arenas(ff), w, mom):  # the starting state is back
        assert torch.equal(ar.master, a) and torch.equal(ff.optimizer.state_tensors(ar)[0], b)


@pytest.mark.parametrize("which,n_state", [("sgdm", 1), ("adamw", 2)])
def test_checkpoint_keys_and_state_round_trip(which, n_state, tmp_path):
    from safetensors.torch import load_file
    ff = _mlp(_make(which))
    for _ in range(2):
        ff.train_step()
    path = ff.save_checkpoint(str(tmp_path / "ck"))
    saved = load_file(str(tmp_path / "ck" / "rank0.safetensors"))
    ex = ff.executor
    idx = [i for i, ar in enumerate(ex.arenas.values()) if ar.size]
    assert set(saved) == {f"arena{i}.master" for i in idx} | {f"arena{i}.opt{j}" for i in idx for j in range(n_state)}
    for i, ar in zip(idx, _arenas(ff)):
        assert torch.equal(saved[f"arena{i}.master"], ar.master)
        for j, t in enumerate(ff.optimizer.state_tensors(ar)):  # opt0 = momentum / m, opt1 = v
            assert torch.equal(saved[f"arena{i}.opt{j}"], t)
    ff2 = _mlp(_make(which))
    assert ff2.load_checkpoint(path) == 2
    for a, b in zip(_arenas(ff), _arenas(ff2)):
        assert torch.equal(a.master, b.master)
        sa, sb = ff.optimizer.state_tensors(a), ff2.optimizer.state_tensors(b)
        assert len(sa) == len(sb) == n_state
        for x, y in zip(sa, sb):
            assert torch.equal(x, y) and bool(x.any())
    ff.train_step()
    ff2.train_step()
    for a, b in zip(_masters(ff), _masters(ff2)):
        assert torch.equal(a, b)
