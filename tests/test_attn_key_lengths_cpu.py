"""Per-sample key lengths of MultiHeadAttention (right-padded batches) on the CPU path: the op against
fp32 torch, pad invariance through bert-tiny, two gloo ranks against one process, and the cost
model's stand-in lengths. The torch references slice the keys to the sample's length instead of
masking them, so they share no code path with the op."""
import math
import os
import sys

import numpy as np
import torch

from flexflow_amd.core import *  # noqa: F401,F403
from flexflow_amd.ops import OpCtx

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


# ---- the helper of tests/test_ops_cpu.py (run_layer / ref_grads / close / check)
def run_layer(build, inputs, seed=0, int_inputs=()):
    torch.manual_seed(seed)
    ff = FFModel(FFConfig([]))
    ts = []
    for i, x in enumerate(inputs):
        dt = DataType.DT_INT32 if i in int_inputs else DataType.DT_FLOAT
        ts.append(ff.create_tensor(list(x.shape), dt))
    out = build(ff, ts)
    L = out.owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    ws = [torch.randn(w.dims) * 0.3 for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims) for w in L.weights]
    clones = [x.clone() for x in inputs]
    slot = [next(i for i, t in enumerate(ts) if t is u) for u in L.inputs]
    xs = [clones[i] for i in slot]
    ys = L.impl.forward(ctx, xs, ws)
    dys = [torch.randn(y.shape) for y in ys]
    dslot = L.impl.backward(ctx, dys)
    assert len(dslot) == len(L.inputs)
    dxs = [None] * len(inputs)
    for i, d in zip(slot, dslot):
        if d is not None:
            dxs[i] = d if dxs[i] is None else dxs[i] + d
    return L, clones, ws, ys, dys, dxs, ctx.wgrads


def ref_grads(fn, inputs, ws, dys, int_inputs=()):
    xi = [x.clone().requires_grad_(i not in int_inputs and x.is_floating_point()) for i, x in enumerate(inputs)]
    wi = [w.clone().requires_grad_() for w in ws]
    out = fn(xi, wi)
    loss = (out.float() * dys[0]).sum()
    req = [t for t in xi + wi if t.requires_grad]
    gs = torch.autograd.grad(loss, req, allow_unused=True)
    it = iter(gs)
    gx = [next(it) if t.requires_grad else None for t in xi]
    gw = [next(it) for _ in wi]
    return out, gx, gw


def close(a, b, tol):
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, f"max err {err} (scale {scale})"


def check(build, fn, inputs, int_inputs=(), tol=1e-4):
    L, xs, ws, ys, dys, dxs, wg = run_layer(build, inputs, int_inputs=int_inputs)
    out, gx, gw = ref_grads(fn, inputs, ws, dys, int_inputs)
    close(ys[0], out, tol)
    for i, (d, g) in enumerate(zip(dxs, gx)):
        if i in int_inputs:
            assert d is None  # the lengths take no gradient
        else:
            close(d, g if g is not None else torch.zeros_like(d), tol)
    for d, g in zip(wg, gw):
        close(d, g if g is not None else torch.zeros_like(d), tol)
    return L


def _sliced_attention(qq, kk, vv, lens, causal):
    """[B, H, Sq, D] attention of each sample over its first clamp(lens[b], 0, Sk) keys; zeros for a
    sample without keys."""
    Sq, Sk = qq.shape[2], kk.shape[2]
    outs = []
    for b in range(qq.shape[0]):
        n = min(max(int(lens.reshape(-1)[b]), 0), Sk)
        if n == 0:
            outs.append(torch.zeros(qq.shape[1], Sq, vv.shape[-1]))
            continue
        s = qq[b] @ kk[b, :, :n].transpose(-1, -2) / math.sqrt(qq.shape[-1])
        if causal:
            s = s.masked_fill(torch.ones(Sq, n, dtype=torch.bool).triu(1), float("-inf"))
        outs.append(torch.softmax(s, -1) @ vv[b, :, :n])
    return torch.stack(outs)


def _self_ref(x, lens, w, H, causal):
    B, S, E = x.shape
    D = w[0].shape[2]
    W, bb = w[0].reshape(3, H * D, E), w[1].reshape(3, H * D)
    qq, kk, vv = ((x @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    o = _sliced_attention(qq, kk, vv, lens, causal).transpose(1, 2).reshape(B, S, H * D)
    return o @ w[2].reshape(w[2].shape[0], -1).t() + w[3]


def _cross_ref(x, lens, w, H, D, causal):
    q, k, v = x
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    qq = (q @ w[0].reshape(H * D, -1).t() + w[3].reshape(-1)).view(B, Sq, H, D).transpose(1, 2)
    kk = (k @ w[1].reshape(H * D, -1).t() + w[4].reshape(-1)).view(B, Sk, H, D).transpose(1, 2)
    vv = (v @ w[2].reshape(H * D, -1).t() + w[5].reshape(-1)).view(B, Sk, H, D).transpose(1, 2)
    o = _sliced_attention(qq, kk, vv, lens, causal).transpose(1, 2).reshape(B, Sq, H * D)
    return o @ w[6].reshape(w[6].shape[0], -1).t() + w[7]


# lengths: a mid cut, an empty sample, above Sk (clamps to Sk), negative (clamps to 0)
def test_mha_key_lengths_self_and_cross():
    for causal in (False, True):
        x = torch.randn(4, 5, 16)
        lens = torch.tensor([3, 0, 99, -2], dtype=torch.int32)
        L = check(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4, causal=causal, key_lengths=t[1]),
                  lambda x, w: _self_ref(x[0], x[1], w, 4, causal), [x, lens], int_inputs=(1,), tol=2e-4)
        assert L.attrs["fused_qkv"] and len(L.inputs) == 4 and not L.impl.needs_input_grad(3)
        assert L.impl.input_maps()[3] == (0,)
        q, kv = torch.randn(4, 5, 16), torch.randn(4, 7, 12)
        lens = torch.tensor([[7], [4], [0], [1]], dtype=torch.int32)  # [B, 1] is accepted
        L = check(lambda ff, t: ff.multihead_attention(t[0], t[1], t[2], 16, 2, 8, 8, causal=causal, key_lengths=t[3]),
                  lambda x, w: _cross_ref(x[:3], x[3], w, 2, 8, causal), [q, kv, kv.clone(), lens], int_inputs=(3,),
                  tol=2e-4)
        assert L.impl.input_maps()[3] == (0, None)


def test_mha_empty_sample_is_exact_zero():
    """L_b = 0: the sample's attention output is exactly 0 (the layer's output rows equal the output
    bias) and it contributes exactly nothing to the input gradient."""
    x = torch.randn(3, 6, 16)
    lens = torch.tensor([6, 0, 2], dtype=torch.int32)
    L, xs, ws, ys, dys, dxs, wg = run_layer(
        lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4, key_lengths=t[1]), [x, lens], int_inputs=(1,))
    assert torch.equal(ys[0][1], ws[3].expand(6, 16))
    assert torch.equal(dxs[0][1], torch.zeros(6, 16))
    assert all(torch.isfinite(g).all() for g in wg)


def test_full_lengths_match_no_lengths():
    x = torch.randn(2, 5, 16)
    full = torch.tensor([5, 5], dtype=torch.int32)
    a = run_layer(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4, key_lengths=t[1]), [x, full],
                  int_inputs=(1,))
    b = run_layer(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4), [x])
    close(a[3][0], b[3][0], 1e-6)
    close(a[5][0], b[5][0], 1e-6)


def _bert_probs(ids_arr, lens_arr):
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(0)
    B, bc = ids_arr.shape[0], BertConfig.tiny(16)
    cfg = FFConfig(["--no-hip-graphs"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    kl = ff.create_tensor([B], DataType.DT_INT32, name="key_lengths") if lens_arr is not None else None
    ids, pos, out = build_bert(ff, B, bc, key_lengths=kl)
    ff.optimizer = SGDOptimizer(ff, 0.0)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    ids.set_tensor(ff, ids_arr)
    pos.set_tensor(ff, np.tile(np.arange(bc.seq, dtype=np.int32), (B, 1)))
    if kl is not None:
        kl.set_tensor(ff, lens_arr)
    ff.forward()
    return np.asarray(ff._get_tensor_value(ff.output_tensor()), dtype=np.float32)


def test_bert_pad_invariance():
    """bert-tiny, CPU fp32: with key_lengths, the token ids at positions >= L_b do not reach the
    output probabilities at positions < L_b; without key_lengths they do (the same edit, so the
    first assertion cannot pass vacuously)."""
    rng = np.random.default_rng(1)
    B, S = 4, 16
    lens = np.array([16, 9, 4, 1], dtype=np.int32)
    ids = rng.integers(0, 1000, (B, S)).astype(np.int32)
    edited = ids.copy()
    for b in range(B):
        edited[b, lens[b]:] = rng.integers(0, 1000, S - lens[b])
    assert (edited != ids).any()
    valid = np.arange(S)[None, :] < lens[:, None]
    with_a, with_b = _bert_probs(ids, lens), _bert_probs(edited, lens)
    assert np.isfinite(with_a).all()
    d_with = np.abs(with_a - with_b)[valid].max()
    without_a, without_b = _bert_probs(ids, None), _bert_probs(edited, None)
    d_without = np.abs(without_a - without_b)[valid].max()
    print("pad edit moves the valid positions' probabilities by", d_with, "with key_lengths,", d_without, "without")
    assert d_with <= 1e-5
    assert d_without > 1e-5
    assert np.abs(with_a - without_a)[valid].max() > 1e-5  # the lengths change what the model computes


def test_key_lengths_two_ranks_match_single():
    """An attention model with key lengths on 2 gloo ranks, batch-parallel and heads-parallel, gives
    the single-process output and weights after the harness's SGD steps (tests/test_multirank_cpu.py
    tolerance); and the lengths matter to that result."""
    import attn_lens_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("batch")
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"attn key_lengths {case}@2")
    dense = A.single("nolens")
    assert np.abs(dense["__output__"] - ref["__output__"]).max() > 1e-4


def test_costmodel_fabricates_full_lengths():
    """The cost model times an attention layer with lengths as a dense batch: its stand-in lengths
    all equal Sk (random small integers would price a nearly empty attention)."""
    from flexflow_amd.pcg.costmodel import fabricate_int_input
    from flexflow_amd.pcg.strategy import OpConfig
    ff = FFModel(FFConfig([]))
    q = ff.create_tensor([4, 5, 16], DataType.DT_FLOAT)
    kv = ff.create_tensor([4, 7, 16], DataType.DT_FLOAT)
    kl = ff.create_tensor([4], DataType.DT_INT32)
    L = ff.multihead_attention(q, kv, kv, 16, 2, key_lengths=kl).owner_layer
    assert len(L.inputs) == 4
    cfg = OpConfig((1,) * len(L.impl.axis_sizes()), (0,))
    t = fabricate_int_input(L, 3, (4,), cfg, "cpu")
    assert t.dtype == torch.int32 and t.shape == (4,) and (t == 7).all()
    # priced as the dense layer: the same cost key as the layer without lengths
    from flexflow_amd.pcg.costmodel import cost_key
    L3 = ff.multihead_attention(q, kv, kv, 16, 2).owner_layer
    assert cost_key(L, cfg, DataType.DT_BF16) == cost_key(L3, cfg, DataType.DT_BF16)
    emb = ff.embedding(ff.create_tensor([4, 5], DataType.DT_INT32), 50, 8, AggrMode.AGGR_MODE_NONE).owner_layer
    e = fabricate_int_input(emb, 0, (4, 5), OpConfig((1,) * len(emb.impl.axis_sizes()), (0,)), "cpu")
    assert e.shape == (4, 5) and int(e.min()) >= 0 and int(e.max()) < 50


def test_varlen_example_runs():
    """examples/python/native/bert_varlen.py (bert-tiny on right-padded batches, lengths from the data
    loader) runs end to end in its own process, as tests/test_examples_cpu.py runs the other examples."""
    import subprocess
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", FF_TUNABLEOP="off")
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "python", "native", "bert_varlen.py"), "-b", "4",
                        "--seq-length", "16", "--iterations", "3"], cwd=root, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bert-tiny varlen: 3 iterations" in r.stdout and "nan" not in r.stdout.lower(), r.stdout[-500:]
