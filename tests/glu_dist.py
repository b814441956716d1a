"""Helper of test_glu_cpu.py: a gated FFN (FFModel.gated_ffn) run through the multi-rank harness of
test_multirank_cpu.py (its _train / _worker / _compare), in the manner of rope_dist.py. Case "tp": the ffn
axis split over the ranks (gate and up column-parallel, the glu on its shard of the columns, down
row-parallel); "batch": data-parallel; "gelu_tanh": another activation, to show that it matters."""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

B, S, E, FFN = 8, 6, 16, 24


def _build(case, ff):
    from flexflow_amd.core import DataType, LossType
    rng = np.random.default_rng(8)
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT, name="x")
    feeds = [rng.standard_normal((B, S, E)).astype(np.float32)]
    t = ff.dense(x, E, name="pre")  # carries the FFN's input gradient into a weight
    t = ff.gated_ffn(t, FFN, activation="gelu_tanh" if case == "gelu_tanh" else "silu", name="ffn")
    t = ff.dense(t, 10, name="head")
    ff.softmax(t, name="sm")
    lab = rng.integers(0, 10, (B, S, 1)).astype(np.int32)
    return [x], feeds, lab, LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


def _strategy(case, ff, world):
    from flexflow_amd.pcg.strategy import OpConfig
    L = {l.name: l for l in ff.layers}

    def cfg(name, degs):
        n = len(L[name].impl.axis_sizes())
        d = list(degs) + [1] * (n - len(degs))
        return OpConfig(tuple(d), tuple(range(int(np.prod(d)))))

    st = {n: cfg(n, [world]) for n in L}
    if case == "tp":  # dense axes: batch, sequence, out, in (the reduction); glu axes: batch, sequence, ffn
        st["ffn_gate"] = cfg("ffn_gate", [1, 1, world])
        st["ffn_up"] = cfg("ffn_up", [1, 1, world])
        st["ffn_glu"] = cfg("ffn_glu", [1, 1, world])
        st["ffn_down"] = cfg("ffn_down", [1, 1, 1, world])
    return st


@contextlib.contextmanager
def _harness():
    """test_multirank_cpu with this module's model in place of its cases; put back on exit."""
    import test_multirank_cpu as T
    old = T._build, T._strategy, T.B
    T._build, T._strategy, T.B = _build, _strategy, B
    try:
        yield T
    finally:
        T._build, T._strategy, T.B = old


def worker(rank, world, port, case, flags, out_dir):
    with _harness() as T:
        T._worker(rank, world, port, case, flags, out_dir)


def run(case, world):
    """(rank 0's weights and output after the harness's two SGD steps on `world` gloo ranks, the
    strategy that ran)."""
    import test_multirank_cpu as T
    from flexflow_amd.core import FFConfig, FFModel
    from flexflow_amd.pcg.strategy import save_strategy
    tmp = tempfile.mkdtemp()
    ff = FFModel(FFConfig([]))
    ff.config.batch_size = B
    _build(case, ff)
    sf = os.path.join(tmp, "s.json")
    save_strategy(sf, _strategy(case, ff, world), world)
    mp.start_processes(worker, args=(world, T._free_port(), case, ["--import-strategy", sf], tmp), nprocs=world,
                       join=True, start_method="spawn")
    with open(os.path.join(tmp, "search.json")) as f:
        search = json.load(f)
    return dict(np.load(os.path.join(tmp, "out.npz"))), search["strategy"]


def single(case):
    with _harness() as T:
        return T._single(case)
