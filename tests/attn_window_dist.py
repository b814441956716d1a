"""Helper of test_attn_window_cpu.py: an attention model with a sliding window inside packed rows run
through the multi-rank harness of test_multirank_cpu.py (its _train / _worker / _compare), in the manner
of attn_segments_dist.py."""
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

B, S, E, H = 8, 6, 16, 4
WINDOW = (2, 1)  # asymmetric, narrower than the longer runs
# both halves of the batch hold whole rows, cut rows, padding and an all-padding row
SEG = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, -1], [-1, 2, 2, 2, 2, 2], [-1, -1, -1, -1, -1, -1],
                [3, 3, 3, 3, 3, 3], [0, 1, 1, 1, 1, 1], [4, 4, 4, 4, 4, -1], [7, 7, 7, 8, 8, 8]], dtype=np.int32)


def _build(case, ff):
    from flexflow_amd.core import DataType, LossType
    rng = np.random.default_rng(5)
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT, name="x")
    sg = ff.create_tensor([B, S], DataType.DT_INT32, name="seg")
    ins, feeds = [x, sg], [rng.standard_normal((B, S, E)).astype(np.float32), SEG.copy()]
    t = ff.multihead_attention(x, x, x, E, H, name="attn", segment_ids=sg, window=None if case == "nowin" else WINDOW)
    assert ("window_left" in t.owner_layer.attrs) == (case != "nowin")
    t = ff.dense(t, 10, name="head")
    ff.softmax(t, name="sm")
    lab = rng.integers(0, 10, (B, S, 1)).astype(np.int32)
    return ins, feeds, lab, LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


def _strategy(case, ff, world):
    from flexflow_amd.pcg.strategy import OpConfig
    L = {l.name: l for l in ff.layers}

    def cfg(name, degs):
        n = len(L[name].impl.axis_sizes())
        d = list(degs) + [1] * (n - len(degs))
        return OpConfig(tuple(d), tuple(range(int(np.prod(d)))))

    st = {n: cfg(n, [world]) for n in ("x", "seg", "head", "sm")}
    # attention axes: batch, sequence, embed, heads
    st["attn"] = cfg("attn", [world]) if case == "batch" else cfg("attn", [1, 1, 1, world])
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
