"""Gated experts_dense (gate_activation) at the op level, on the torch fallback in fp32: against the unfused
graph it replaces (experts_dense of 2F outputs, then the packed ff.glu per expert), and the ff.moe_ffn block
built with it."""
import numpy as np
import pytest
import torch

from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
from flexflow_amd.type import OperatorType

B, N_EXP, K_SEL, HID, FFN = 64, 4, 2, 16, 24
LIN, EXD = OperatorType.OP_LINEAR, OperatorType.OP_EXPERTS_DENSE
TOL = dict(rtol=1e-5, atol=1e-6)  # fp32 round-off: the same sums in another order


def _model(block, lr=0.0):
    """dense -> block -> dense -> softmax on fixed data; the leading dense shows the expert inputs' gradient."""
    cfg = FFConfig(["--device", "cpu", "--no-hip-graphs"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, HID], DataType.DT_FLOAT)
    out = ff.softmax(ff.dense(block(ff, ff.dense(x, HID, name="first")), 10, name="last"))
    ff.optimizer = SGDOptimizer(ff, lr)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
               metrics=[MetricsType.METRICS_SPARSE_CATEGORICAL_CROSSENTROPY])
    rng = np.random.default_rng(5)
    x.set_tensor(ff, rng.standard_normal((B, HID)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (B, 1)).astype(np.int32))
    return ff, out


def _unfused(act):
    """moe_ffn's graph with the gate spelled out: an experts_dense of 2F outputs and a packed glu per expert."""
    def block(ff, h):
        gate = ff.dense(h, N_EXP, name="ffn_gate")
        topk_v, topk_i = ff.top_k(gate, K_SEL, False)
        zs = ff.experts_dense(ff.group_by(h, topk_i, N_EXP, 2.0), topk_i, 2 * FFN, name="ffn_up")
        y = ff.experts_dense([ff.glu(z, activation=act) for z in zs], topk_i, HID, name="ffn_down")
        return ff.aggregate([ff.softmax(topk_v), topk_i, topk_i, gate] + y, N_EXP, 0.0)
    return block


@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
def test_gated_layer_matches_unfused_graph(act):
    plain, pout = _model(_unfused(act))
    fused, fout = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, FFN, gate_activation=act, name="ffn"))
    names = ["first", "ffn_gate", "ffn_up", "ffn_down", "last"]
    rng = np.random.default_rng(6)
    for nm in names:
        a, b = plain.get_layer_by_name(nm), fused.get_layer_by_name(nm)
        assert [tuple(w.dims) for w in a.weights] == [tuple(w.dims) for w in b.weights]
        for wa, wb in zip(a.weights, b.weights):
            v = wa.get_weights(plain)
            if v.ndim == 1:  # biases away from zero
                v = rng.uniform(0.1, 0.5, v.shape).astype(np.float32)
                wa.set_weights(plain, v)
            wb.set_weights(fused, v)
    outs = []
    for ff, out in ((plain, pout), (fused, fout)):
        ff.forward()
        ff.zero_gradients()
        ff.backward()
        outs.append(torch.from_numpy(np.asarray(out.get_tensor(ff), dtype=np.float32)))
    torch.testing.assert_close(outs[1], outs[0], **TOL)
    grad = lambda ff, w: ff.executor.get_weight_grad(w).float().cpu()  # noqa: E731
    for nm in names:  # ffn_up: kernel and bias gradient; first: the gradient that reached the layer in front
        for wa, wb in zip(plain.get_layer_by_name(nm).weights, fused.get_layer_by_name(nm).weights):
            torch.testing.assert_close(grad(fused, wb), grad(plain, wa), **TOL)
            assert float(grad(fused, wb).abs().max()) > 0, nm


def test_gated_moe_ffn_builds_and_learns():
    ff, _ = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, 32, gate_activation="silu", use_bias=False, name="ffn"),
                   lr=0.2)
    kinds = [L.op_type for L in ff.layers]
    assert kinds.count(EXD) == 2 and kinds.count(LIN) == 3 and OperatorType.OP_GLU not in kinds
    up, down = ff.get_layer_by_name("ffn_up"), ff.get_layer_by_name("ffn_down")
    assert [tuple(w.dims) for w in up.weights] == [(N_EXP, 64, HID)]
    assert [tuple(w.dims) for w in down.weights] == [(N_EXP, HID, 32)]
    assert [tuple(t.dims) for t in up.outputs] == [(64, 32)] * N_EXP
    assert up.impl.flops([(64, HID)] * N_EXP, None, None) == 2.0 * N_EXP * 64 * HID * 64
    losses = []
    for _ in range(8):
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    assert losses[-1] < 0.9 * losses[0], losses


def test_default_moe_ffn_is_unchanged():
    ff, _ = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, 32, name="ffn"))
    assert [L.op_type.name[3:] for L in ff.layers] == (
        ["INPUT", "LINEAR", "LINEAR", "TOPK", "GROUP_BY", "EXPERTS_DENSE", "EXPERTS_DENSE", "SOFTMAX", "AGGREGATE",
         "LINEAR", "SOFTMAX"])
    up, down = ff.get_layer_by_name("ffn_up"), ff.get_layer_by_name("ffn_down")
    assert [tuple(w.dims) for w in up.weights] == [(N_EXP, 32, HID), (N_EXP * 32,)]
    assert [tuple(w.dims) for w in down.weights] == [(N_EXP, HID, 32), (N_EXP * HID,)]
    assert "gate_activation" not in up.attrs and up.attrs["activation"] == ActiMode.AC_MODE_GELU


def test_builders_refuse_gate_with_activation_and_unknown_gates():
    ff = FFModel(FFConfig(["--device", "cpu"]))
    xs = [ff.create_tensor([8, 16], DataType.DT_FLOAT) for _ in range(2)]
    idx, x = ff.create_tensor([8, 1], DataType.DT_INT32), ff.create_tensor([8, 16], DataType.DT_FLOAT)
    with pytest.raises(ValueError, match="only one"):
        ff.experts_dense(xs, idx, 8, ActiMode.AC_MODE_RELU, gate_activation="silu")
    with pytest.raises(ValueError, match="only one"):
        ff.moe_ffn(x, 2, 1, 8, activation=ActiMode.AC_MODE_RELU, gate_activation="silu")
    with pytest.raises(ValueError, match="unknown activation"):
        ff.experts_dense(xs, idx, 8, gate_activation="swish")
    with pytest.raises(ValueError, match="unknown activation"):
        ff.moe_ffn(x, 2, 1, 8, gate_activation="swish")


def test_each_half_is_initialised_as_its_own_dense_weight():
    ff, _ = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, 48, gate_activation="silu", name="ffn"))
    w = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    bound = (6.0 / (HID + 48)) ** 0.5  # Glorot for (F, in), not for (2F, in)
    assert w.shape == (N_EXP, 96, HID)
    halves = [w[e, h * 48:(h + 1) * 48] for e in range(N_EXP) for h in range(2)]
    assert all(0.9 * bound < np.abs(v).max() <= bound for v in halves)
    assert all(not np.array_equal(halves[0], v) for v in halves[1:])
