"""Helper of test_attn_bias_cpu.py: attention models with a [B, H, S, S] score bias run through the
multi-rank harness of test_multirank_cpu.py (its _train / _worker / _compare), with this module's
models and strategies in place of that file's cases. Cases: "<op>_<axis>" with op sdpa (dense q / k / v
projections around scaled_dot_product_attention) or mha (a dense layer ahead of a biased
multihead_attention), axis batch or heads. The trainable layers ahead of the attention make its input
gradients show in the compared weights."""
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


def bias_values():
    rng = np.random.default_rng(11)
    b = rng.standard_normal((B, H, S, S)).astype(np.float32)
    b[rng.random((B, H, S, S)) < 0.2] = -np.inf
    b[..., 0] = 0.0  # every row keeps a key
    return b


def _build(case, ff):
    from flexflow_amd.core import DataType, LossType
    rng = np.random.default_rng(5)
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT, name="x")
    bias = ff.create_tensor([B, H, S, S], DataType.DT_FLOAT, create_grad=False, name="bias")
    feeds = [rng.standard_normal((B, S, E)).astype(np.float32), bias_values()]
    if case.startswith("sdpa"):
        heads = []
        for n in ("wq", "wk", "wv"):
            t = ff.reshape(ff.dense(x, E, name=n), [B, S, H, E // H], name=n + "_r")
            heads.append(ff.transpose(t, [0, 2, 1, 3], name=n + "_t"))
        t = ff.scaled_dot_product_attention(*heads, attn_bias=bias if "nobias" not in case else None, name="attn")
        t = ff.reshape(ff.transpose(t, [0, 2, 1, 3], name="o_t"), [B, S, E], name="o_r")
    else:
        h = ff.dense(x, E, name="pre")
        t = ff.multihead_attention(h, h, h, E, H, name="attn", attn_bias=bias if "nobias" not in case else None)
    t = ff.dense(t, 10, name="head")
    ff.softmax(t, name="sm")
    lab = rng.integers(0, 10, (B, S, 1)).astype(np.int32)
    return [x, bias], feeds, lab, LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


def _strategy(case, ff, world):
    from flexflow_amd.pcg.strategy import OpConfig

    def cfg(layer, degs):
        n = len(layer.impl.axis_sizes())
        d = list(degs) + [1] * (n - len(degs))
        return OpConfig(tuple(d), tuple(range(int(np.prod(d)))))

    st = {l.name: cfg(l, [world]) for l in ff.layers}
    if case.endswith("heads"):  # sdpa axes: batch, heads, rows, dim; mha axes: batch, sequence, embed, heads
        L = next(l for l in ff.layers if l.name == "attn")
        st["attn"] = cfg(L, [1, world] if case.startswith("sdpa") else [1, 1, 1, world])
    return st


@contextlib.contextmanager
def _harness():
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
