"""attn_bias_grad on the CPU path: builder errors, needs_input_grad, the bias gradient against torch autograd, a table
that a training step moves, and the same table on two gloo ranks (attn_bias_dist.py's harness, this module's model)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import attn_bias_dist as A
from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType

B, S, E, H = A.B, A.S, A.E, A.H
_WORKER, _BUILD, _STRATEGY = A.worker, A._build, A._strategy


def _qkvb(ff, ext=(1, H)):
    return [ff.create_tensor([B, H, S, 8], DataType.DT_FLOAT) for _ in range(3)] + \
        [ff.create_tensor([ext[0], ext[1], S, S], DataType.DT_FLOAT)]


def test_builder_errors():
    ff = FFModel(FFConfig([]))
    q, k, v, b = _qkvb(ff)
    ids, x = ff.create_tensor([B, S], DataType.DT_INT32), ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    for call in (lambda: ff.scaled_dot_product_attention(q, k, v, attn_bias_grad=True),
                 lambda: ff.multihead_attention(x, x, x, E, H, attn_bias_grad=True),
                 lambda: ff.scaled_dot_product_attention(q, k, v, segment_ids=ids, attn_bias_grad=True),
                 lambda: ff.multihead_attention(x, x, x, E, H, window=2, attn_bias_grad=True)):
        with pytest.raises(ValueError, match="attn_bias"):
            call()


@pytest.mark.parametrize("grad", [False, True])
def test_needs_input_grad_and_attrs(grad):
    ff = FFModel(FFConfig([]))
    q, k, v, b = _qkvb(ff)
    L = ff.scaled_dot_product_attention(q, k, v, attn_bias=b, **(dict(attn_bias_grad=True) if grad else {})).owner_layer
    assert [L.impl.needs_input_grad(i) for i in range(4)] == [True, True, True, grad]
    assert ("attn_bias_grad" in L.attrs) == grad  # without the keyword the attributes are what they were
    assert L.impl.flops([t.dims for t in L.inputs], None, []) == 2.0 * B * H * S * S * 16 * (2 if grad else 1)


@pytest.mark.parametrize("ext", [(1, H), (B, 1), (1, 1), (B, H)])
def test_cpu_path_gradient_against_autograd(ext):
    from flexflow_amd.ops import OpCtx
    g = torch.Generator().manual_seed(3)
    ff = FFModel(FFConfig([]))
    ts = _qkvb(ff, ext)
    L = ff.scaled_dot_product_attention(*ts[:3], attn_bias=ts[3], causal=True, attn_bias_grad=True).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    q, k, v, do = (torch.randn(B, H, S, 8, generator=g) for _ in range(4))
    bias = torch.randn(*ext, S, S, generator=g)
    bias[..., 3] = float("-inf")
    L.impl.forward(ctx, [q, k, v, bias], [])
    dxs = L.impl.backward(ctx, [do])
    bf = bias.clone().requires_grad_()
    s = (q @ k.transpose(-1, -2) / math.sqrt(8) + bf).masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    (torch.softmax(s, -1) @ v).backward(do)
    assert dxs[3].shape == bias.shape and torch.allclose(dxs[3], bf.grad, atol=1e-5, rtol=1e-5)
    ctx.extra["in_grad"] = (True, True, True, False)  # nothing upstream can use it: not computed
    L.impl.forward(ctx, [q, k, v, bias], [])
    assert L.impl.backward(ctx, [do])[3] is None


def _build(case, ff):
    """x -> dense -> multihead_attention with a [1, H, S, S] bias: embedding table -> reshape -> transpose."""
    rng = np.random.default_rng(5)
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT, name="x")
    idx = ff.create_tensor([1, S * S], DataType.DT_INT32, name="rel")
    rel = (np.arange(S)[:, None] - np.arange(S)[None, :] + S - 1).reshape(1, -1).astype(np.int32)
    t = ff.reshape(ff.embedding(idx, 2 * S - 1, H, name="rel_table"), [1, S, S, H], name="rel_r")
    h = ff.dense(x, E, name="pre")
    t = ff.multihead_attention(h, h, h, E, H, name="attn", attn_bias=ff.transpose(t, [0, 3, 1, 2], name="rel_t"),
                               **(dict(attn_bias_grad=True) if case != "frozen" else {}))
    ff.softmax(ff.dense(t, 10, name="head"), name="sm")
    lab = rng.integers(0, 10, (B, S, 1)).astype(np.int32)
    return [x, idx], [rng.standard_normal((B, S, E)).astype(np.float32), rel], lab, LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


@pytest.mark.parametrize("case", ["trained", "frozen"])
def test_table_moves_only_with_attn_bias_grad(case):
    cfg = FFConfig(["--no-hip-graphs", "--device", "cpu", "--dtype", "fp32"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    ins, feeds, lab, loss = _build(case, ff)
    ff.optimizer = AdamOptimizer(ff, 1e-2)
    ff.compile(loss_type=loss, metrics=[MetricsType.METRICS_ACCURACY])
    for t, f in zip(ins + [ff.label_tensor], feeds + [lab]):
        t.set_tensor(ff, f)
    table = next(w for L in ff.layers for w in L.weights if L.name == "rel_table")
    before = np.asarray(table.get_weights(ff)).copy()
    ff.forward()
    ff.zero_gradients()
    ff.backward()
    ff.update()
    moved = np.abs(np.asarray(table.get_weights(ff)) - before).max()
    assert moved > 1e-4 if case == "trained" else moved == 0  # frozen: today's behaviour, pinned


def _strategy(case, ff, world):
    st = _STRATEGY(case, ff, world)
    for l in ff.layers:  # the table and its views have no batch to split: one part
        if l.name.startswith("rel"):
            st[l.name] = type(st[l.name])((1,) * len(st[l.name].degrees), (0,))
    return st


@contextlib.contextmanager
def _patched():
    A._build, A._strategy, A.worker = _build, _strategy, worker
    try:
        yield
    finally:
        A._build, A._strategy, A.worker = _BUILD, _STRATEGY, _WORKER


def worker(*args):  # the spawned ranks enter here
    with _patched():
        _WORKER(*args)


def test_table_gradient_two_ranks_match_single():
    """Batch-sharded on 2 gloo ranks the bias is a replicated input: each rank sums its own samples, the backward
    transfer sums the replicas, and every weight after the harness's two SGD steps equals the one-rank run's."""
    from test_multirank_cpu import _compare
    with _patched():
        ref = A.single("mha_batch")
        par, strat = A.run("mha_batch", 2)
    assert strat["attn"]["degrees"][0] == 2, strat["attn"]
    assert any("OP_EMBEDDING" in k for k in ref)  # the table is among the compared weights
    _compare(par, ref, "score-bias gradient batch@2")
