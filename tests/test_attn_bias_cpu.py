"""The additive attention score bias on the CPU (the reference path of ops/attention.py): the
scaled_dot_product_attention op, multihead_attention(attn_bias=...), the fused HuggingFace import
(PyTorchModel(fuse_sdpa=True)), two-rank sharding of the bias, and argument validation."""
import math

import numpy as np
import pytest
import torch

from flexflow_amd.core import DataType, FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
from flexflow_amd.ops import OpCtx
from flexflow_amd.type import OperatorType

INF = float("inf")


def _ctx(L):
    n = len(L.impl.axis_sizes())
    return OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)


# ------------------------------------------------------------------------------------- OP_SDPA
@pytest.mark.parametrize("causal", [False, True])
def test_sdpa_op_matches_torch(causal):
    """B=2, H=4, Sq=10, Sk=12, D=16, a bias with -inf entries, with and without causal: forward and
    q / k / v gradients against torch's scaled_dot_product_attention (rtol 1e-4, the importer test's)."""
    B, H, Sq, Sk, D = 2, 4, 10, 12, 16
    g = torch.Generator().manual_seed(3)
    ff = FFModel(FFConfig(["--device", "cpu"]))
    tq, tk, tv = (ff.create_tensor([B, H, s, D], DataType.DT_FLOAT) for s in (Sq, Sk, Sk))
    tb = ff.create_tensor([1, H, Sq, Sk], DataType.DT_FLOAT)
    L = ff.scaled_dot_product_attention(tq, tk, tv, attn_bias=tb, scale=0.3, causal=causal).owner_layer
    assert L.op_type == OperatorType.OP_SDPA and not L.weights and tuple(L.outputs[0].dims) == (B, H, Sq, D)
    assert L.impl.flops([(B, H, Sq, D), (B, H, Sk, D), (B, H, Sk, D)], [(B, H, Sq, D)], []) == 2 * B * H * Sq * Sk * 2 * D
    q, k, v = (torch.randn(B, H, s, D, generator=g) for s in (Sq, Sk, Sk))
    bias = torch.randn(1, H, Sq, Sk, generator=g)
    bias[..., 3:5] = -INF
    bias[..., 0] = 0.0  # column 0 stays: no empty row, also under the causal mask
    ctx = _ctx(L)
    y = L.impl.forward(ctx, [q, k, v, bias], [])[0]
    dy = torch.randn(y.shape, generator=g)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == 4 and dxs[3] is None  # the bias takes no gradient
    assert not L.impl.needs_input_grad(3)
    qf, kf, vf = (t.clone().requires_grad_() for t in (q, k, v))
    m = bias
    if causal:
        m = bias.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), -INF)
    yr = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=m, scale=0.3)
    yr.backward(dy)
    for got, ref in ((y, yr), (dxs[0], qf.grad), (dxs[1], kf.grad), (dxs[2], vf.grad)):
        np.testing.assert_allclose(got.detach().numpy(), ref.detach().numpy(), rtol=1e-4, atol=1e-4 * ref.abs().max().item())


def test_sdpa_empty_rows_and_key_lengths():
    """A query row whose every key is removed gives zeros (torch: NaN) and takes part in no gradient;
    key lengths combine with the bias."""
    B, H, Sq, Sk, D = 2, 2, 5, 7, 8
    g = torch.Generator().manual_seed(4)
    ff = FFModel(FFConfig(["--device", "cpu"]))
    tq, tk, tv = (ff.create_tensor([B, H, s, D], DataType.DT_FLOAT) for s in (Sq, Sk, Sk))
    tb = ff.create_tensor([B, 1, Sq, Sk], DataType.DT_FLOAT)
    tl = ff.create_tensor([B], DataType.DT_INT32)
    L = ff.scaled_dot_product_attention(tq, tk, tv, attn_bias=tb, key_lengths=tl).owner_layer
    assert [len(m) for m in L.impl.input_maps()] == [4, 4, 4, 1, 4]
    assert L.impl.input_maps()[4] == (0, None, None, None)
    q, k, v = (torch.randn(B, H, s, D, generator=g) for s in (Sq, Sk, Sk))
    bias = torch.randn(B, 1, Sq, Sk, generator=g)
    bias[0, :, 2] = -INF          # an empty row by the bias alone
    bias[1, :, 3, :4] = -INF      # ... and one by the bias and the length (4) together
    lens = torch.tensor([7, 4], dtype=torch.int32)
    ctx = _ctx(L)
    y = L.impl.forward(ctx, [q, k, v, lens, bias], [])[0]
    dq, dk, dv = L.impl.backward(ctx, [torch.ones_like(y)])[:3]
    for t in (y, dq, dk, dv):
        assert torch.isfinite(t).all()
    assert (y[0, :, 2] == 0).all() and (dq[0, :, 2] == 0).all()
    assert (y[1, :, 3] == 0).all() and (dq[1, :, 3] == 0).all()
    assert (dk[1, :, 4:] == 0).all() and (dv[1, :, 4:] == 0).all()
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / math.sqrt(D) + bias
    s[1, :, :, 4:] = -INF
    live = ~(s == -INF).all(-1)
    ref = torch.einsum("bhqk,bhkd->bhqd", torch.nan_to_num(torch.softmax(s, -1), nan=0.0), v)
    np.testing.assert_allclose(y[live].numpy(), ref[live].numpy(), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------- multihead_attention
def _mha_ref(x, ws, H, bias, lens, causal):
    B, S, E = x.shape
    D = E // H
    W, bb = ws[0].reshape(3, H * D, E), ws[1].reshape(3, H * D)
    q, k, v = ((x @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / math.sqrt(D) + bias
    if lens is not None:
        s = s.masked_fill((torch.arange(S)[None, :] >= lens[:, None])[:, None, None, :], -INF)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), -INF)
    o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), v)
    return o.transpose(1, 2).reshape(B, S, H * D) @ ws[2].reshape(E, -1).t() + ws[3]


@pytest.mark.parametrize("with_lens", [False, True])
def test_mha_attn_bias_matches_explicit_reference(with_lens):
    B, S, E, H = 3, 9, 32, 4
    g = torch.Generator().manual_seed(6)
    ff = FFModel(FFConfig(["--device", "cpu"]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    tl = ff.create_tensor([B], DataType.DT_INT32) if with_lens else None
    tb = ff.create_tensor([1, H, S, S], DataType.DT_FLOAT)
    L = ff.multihead_attention(tx, tx, tx, E, H, key_lengths=tl, attn_bias=tb).owner_layer
    assert L.attrs["attn_bias"] is True and len(L.inputs) == (5 if with_lens else 4) and L.inputs[-1] is tb
    assert L.impl.input_maps()[-1] == (None, 3, None, None)
    # ALiBi: slope_h * -(distance)
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)])
    dist = (torch.arange(S)[:, None] - torch.arange(S)[None, :]).abs().float()
    bias = (-slopes[:, None, None] * dist)[None]
    x = torch.randn(B, S, E, generator=g)
    ws = [torch.randn(w.dims, generator=g) / math.sqrt(E) for w in L.weights]
    lens = torch.tensor([9, 4, 1], dtype=torch.int32)
    ctx = _ctx(L)
    ctx.wgrads = [torch.zeros(w.dims) for w in L.weights]
    xs = [x, x, x] + ([lens] if with_lens else []) + [bias]
    y = L.impl.forward(ctx, xs, ws)[0]
    dy = torch.randn(B, S, E, generator=g)
    dxs = L.impl.backward(ctx, [dy])
    assert len(dxs) == len(xs) and all(d is None for d in dxs[1:])
    assert not L.impl.needs_input_grad(len(xs) - 1)
    xf = x.clone().requires_grad_()
    wf = [w.clone().requires_grad_() for w in ws]
    yr = _mha_ref(xf, wf, H, bias, lens if with_lens else None, False)
    yr.backward(dy)
    np.testing.assert_allclose(y.numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dxs[0].numpy(), xf.grad.numpy(), rtol=1e-4, atol=1e-5)
    for gw, r in zip(ctx.wgrads, wf):
        np.testing.assert_allclose(gw.numpy(), r.grad.numpy(), rtol=1e-4, atol=1e-5)


def test_mha_without_attn_bias_is_built_as_before():
    ff = FFModel(FFConfig(["--device", "cpu"]))
    tx = ff.create_tensor([2, 5, 16], DataType.DT_FLOAT)
    tl = ff.create_tensor([2], DataType.DT_INT32)
    plain = ff.multihead_attention(tx, tx, tx, 16, 2).owner_layer
    lens = ff.multihead_attention(tx, tx, tx, 16, 2, key_lengths=tl).owner_layer
    none = ff.multihead_attention(tx, tx, tx, 16, 2, key_lengths=tl, attn_bias=None).owner_layer
    assert "attn_bias" not in plain.attrs and "attn_bias" not in lens.attrs and "attn_bias" not in none.attrs
    assert len(plain.inputs) == 3 and len(lens.inputs) == 4 and lens.inputs[3] is tl
    assert [w.short_name for w in plain.weights] == ["qkv_weight", "qkv_bias", "o_weight", "o_bias"]
    assert [w.short_name for w in lens.weights] == [w.short_name for w in none.weights] == [w.short_name for w in plain.weights]
    assert lens.impl.input_maps() == none.impl.input_maps() == [(0, 1, None), (0, None, None), (0, None, None), (0,)]
    assert {k: v for k, v in lens.attrs.items() if not k.endswith("init")} == \
        {k: v for k, v in none.attrs.items() if not k.endswith("init")}


def test_shape_and_attribute_validation():
    ff = FFModel(FFConfig(["--device", "cpu"]))
    B, H, S, D = 2, 4, 6, 8
    q = ff.create_tensor([B, H, S, D], DataType.DT_FLOAT)
    x = ff.create_tensor([B, S, H * D], DataType.DT_FLOAT)
    for shape in ([B, H, S], [3, H, S, S], [B, 2, S, S], [B, H, S, S + 1], [B, H, S + 1, S]):
        bad = ff.create_tensor(shape, DataType.DT_FLOAT)
        with pytest.raises(ValueError):
            ff.scaled_dot_product_attention(q, q, q, attn_bias=bad)
        with pytest.raises(ValueError):
            ff.multihead_attention(x, x, x, H * D, H, attn_bias=bad)
    ints = ff.create_tensor([B, H, S, S], DataType.DT_INT32)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, q, q, attn_bias=ints)
    with pytest.raises(ValueError):
        ff.multihead_attention(x, x, x, H * D, H, attn_bias=ints)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, q, q, dropout=1.0)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, ff.create_tensor([B, 2, S, D], DataType.DT_FLOAT), q)  # no GQA
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(x, x, x)  # rank 3
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, q, q, key_lengths=ff.create_tensor([B + 1], DataType.DT_INT32))
    from flexflow_amd import kernels as K
    with pytest.raises(ValueError):
        K.attn_score_bias(torch.zeros(B, H, S, S + 1), B, H, S, S, torch.device("cpu"))
    with pytest.raises(ValueError):
        K.attn_score_bias(torch.zeros(B, H, S, S, dtype=torch.int32), B, H, S, S, torch.device("cpu"))
    ok = K.attn_score_bias(torch.zeros(1, H, S, S, dtype=torch.bfloat16), B, H, S, S, torch.device("cpu"))
    assert ok.dtype == torch.float32 and ok.is_contiguous()


def test_sdpa_drops_attention_and_costmodel_inputs():
    """The executor keeps its step counter for a dropping SDPA layer too; the cost model measures the
    bias as zeros and the lengths as a dense batch."""
    from flexflow_amd.pcg.costmodel import fabricate_int_input, is_score_bias_input
    from flexflow_amd.pcg.strategy import OpConfig
    ff = FFModel(FFConfig(["--device", "cpu"]))
    q = ff.create_tensor([2, 4, 6, 8], DataType.DT_FLOAT)
    kv = ff.create_tensor([2, 4, 9, 8], DataType.DT_FLOAT)
    tl = ff.create_tensor([2], DataType.DT_INT32)
    tb = ff.create_tensor([1, 4, 6, 9], DataType.DT_FLOAT)
    L = ff.scaled_dot_product_attention(q, kv, kv, attn_bias=tb, key_lengths=tl, dropout=0.1).owner_layer
    assert L.impl.drops_attention()
    assert not ff.scaled_dot_product_attention(q, kv, kv).owner_layer.impl.drops_attention()
    assert [is_score_bias_input(L, i) for i in range(5)] == [False, False, False, False, True]
    cfg = OpConfig((1,) * len(L.impl.axis_sizes()), (0,))
    t = fabricate_int_input(L, 3, (2,), cfg, "cpu")
    assert t.dtype == torch.int32 and (t == 9).all()
    x = ff.create_tensor([2, 6, 32], DataType.DT_FLOAT)
    M = ff.multihead_attention(x, x, x, 32, 4, attn_bias=ff.create_tensor([1, 1, 6, 6], DataType.DT_FLOAT)).owner_layer
    assert [is_score_bias_input(M, i) for i in range(4)] == [False, False, False, True]
    P = ff.multihead_attention(x, x, x, 32, 4, key_lengths=tl).owner_layer
    assert not any(is_score_bias_input(P, i) for i in range(4))


# ------------------------------------------------------------------------------ fused HF import
def _fused_mt5():
    import test_hf_import_cpu as T
    from flexflow_amd.torch.model import PyTorchModel
    m = T._mt5()
    fc = FFConfig(["--device", "cpu"])
    fc.batch_size = T.B
    ff = FFModel(fc)
    ins = [ff.create_tensor([T.B, T.S], DataType.DT_INT64), ff.create_tensor([T.B, T.S], DataType.DT_INT64),
           ff.create_tensor([T.B, T.T], DataType.DT_INT64)]
    hf = PyTorchModel(m, is_hf_model=True, input_names=["input_ids", "attention_mask", "decoder_input_ids"],
                      batch_size=T.B, seq_length=(T.S, T.T), fuse_sdpa=True)
    return T, m, ff, ins, hf.torch_to_ff(ff, ins)


def test_mt5_fused_sdpa_logits_match_torch():
    pytest.importorskip("transformers")
    T, m, ff, ins, outs = _fused_mt5()
    kinds = [L.op_type for L in ff.layers]
    assert kinds.count(OperatorType.OP_SDPA) == 6 and OperatorType.OP_BATCHMATMUL not in kinds
    assert OperatorType.OP_SOFTMAX not in kinds
    for L in ff.layers:
        if L.op_type == OperatorType.OP_SDPA:  # relative-position bias (+ causal mask), the same for every sample
            assert L.attrs["attn_bias"] and L.attrs["scale"] == 1.0 and L.inputs[-1].dims[0] == 1
    ff.optimizer = SGDOptimizer(ff, 0.01)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    ids, dec = rng.integers(1, T.V, (T.B, T.S)), rng.integers(1, T.V, (T.B, T.T))
    ins[0].set_tensor(ff, ids.astype(np.int64))
    ins[1].set_tensor(ff, np.ones((T.B, T.S), np.int64))
    ins[2].set_tensor(ff, dec.astype(np.int64))
    ff.forward()
    got = np.asarray(outs[0].get_tensor(ff))
    with torch.no_grad():
        ref = m.eval()(input_ids=torch.tensor(ids), attention_mask=torch.ones(T.B, T.S, dtype=torch.long),
                       decoder_input_ids=torch.tensor(dec), use_cache=False).logits.numpy()
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_mt5_fused_sdpa_trains():
    pytest.importorskip("transformers")
    T, _, ff, ins, outs = _fused_mt5()
    ff.optimizer = SGDOptimizer(ff, 0.05)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(1)
    src = rng.integers(1, T.V, (T.B, T.S))
    tgt = src[:, :T.T]
    dec = np.concatenate([np.zeros((T.B, 1), np.int64), tgt[:, :-1]], 1)
    ins[0].set_tensor(ff, src.astype(np.int64))
    ins[1].set_tensor(ff, np.ones((T.B, T.S), np.int64))
    ins[2].set_tensor(ff, dec.astype(np.int64))
    ff.label_tensor.set_tensor(ff, tgt.reshape(T.B, T.T, 1).astype(np.int32))
    losses = []
    for _ in range(4):
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_fuse_sdpa_defaults_off():
    from flexflow_amd.torch.export import ExportImporter
    from flexflow_amd.torch.model import PyTorchModel
    assert PyTorchModel(torch.nn.Linear(2, 2)).fuse_sdpa is False
    assert ExportImporter(torch.nn.Linear(2, 2), ["x"]).fuse_sdpa is False


# ------------------------------------------------------------------------------------ two ranks
@pytest.mark.parametrize("op", ["sdpa", "mha"])
def test_score_bias_two_ranks_match_single(op):
    """A [B, H, S, S] bias on 2 gloo ranks, batch-sharded and then heads-sharded: output and weights
    (the layers ahead of the attention carry its input gradients) equal the one-rank run, so each rank
    read its own slice of the bias; and the bias matters to that result."""
    import attn_bias_dist as A
    from test_multirank_cpu import _compare
    ref = A.single(f"{op}_batch")
    for axis in ("batch", "heads"):
        par, strat = A.run(f"{op}_{axis}", 2)
        want = {("sdpa", "batch"): [2, 1, 1, 1], ("sdpa", "heads"): [1, 2, 1, 1],
                ("mha", "batch"): [2, 1, 1, 1], ("mha", "heads"): [1, 1, 1, 2]}[(op, axis)]
        assert strat["attn"]["degrees"] == want, strat["attn"]
        _compare(par, ref, f"{op} score bias {axis}@2")
    if op == "mha":
        plain = A.single("mha_nobias_batch")
        assert np.abs(plain["__output__"] - ref["__output__"]).max() > 1e-4
