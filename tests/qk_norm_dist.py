"""Helper of test_qk_norm_cpu.py: rope_dist.py's rotary grouped-query attention model with qk_norm=True (case
"plain": without), run through that module's multi-rank harness with this module's model in place of its own.
On the heads axis every rank holds half of the heads and adds their part of the gradient of the replicated
q_norm_weight / k_norm_weight."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import rope_dist as A  # noqa: E402

_rope_worker = A.worker


def _build(case, ff):
    from flexflow_amd.core import DataType, LossType
    rng = np.random.default_rng(6)
    x = ff.create_tensor([A.B, A.S, A.E], DataType.DT_FLOAT, name="x")
    pos = ff.create_tensor([A.B, A.S], DataType.DT_INT32, name="pos")
    t = ff.dense(x, A.E, name="pre")
    t = ff.multihead_attention(t, t, t, A.E, A.H, name="attn", causal=True, num_kv_heads=A.HKV, rope_position_ids=pos,
                               rotary=dict(max_positions=A.MAXP), qk_norm=case != "plain")
    ff.softmax(ff.dense(t, 10, name="head"), name="sm")
    feeds = [rng.standard_normal((A.B, A.S, A.E)).astype(np.float32), rng.integers(0, A.MAXP, (A.B, A.S)).astype(np.int32)]
    return [x, pos], feeds, rng.integers(0, 10, (A.B, A.S, 1)).astype(np.int32), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


def worker(*args):  # in a spawned rank: rope_dist's worker on this module's model
    A._build = _build
    _rope_worker(*args)


def _with_model(fn, *args):
    old = A._build, A.worker
    A._build, A.worker = _build, worker
    try:
        return fn(*args)
    finally:
        A._build, A.worker = old


def run(case, world):
    return _with_model(A.run, case, world)


def single(case):
    return _with_model(A.single, case)
