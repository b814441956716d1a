"""experts_dense at the op level, on the torch fallback: ff.moe(fused_experts=True) against the per-expert
dense layers it replaces, and the ff.moe_ffn block."""
import numpy as np
import pytest
import torch

from flexflow_amd.core import DataType, FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
from flexflow_amd.type import OperatorType

B, N_EXP, K_SEL, HID = 64, 4, 2, 16
LIN, EXD = OperatorType.OP_LINEAR, OperatorType.OP_EXPERTS_DENSE


def _model(block, lr=0.0):
    """dense -> block -> dense -> softmax on fixed data. The leading dense makes the expert inputs'
    gradient visible: it reaches that layer's weight gradient through group_by's backward."""
    cfg = FFConfig(["--device", "cpu", "--no-hip-graphs"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, HID], DataType.DT_FLOAT)
    out = ff.softmax(ff.dense(block(ff, ff.dense(x, HID)), 10))
    ff.optimizer = SGDOptimizer(ff, lr)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
               metrics=[MetricsType.METRICS_SPARSE_CATEGORICAL_CROSSENTROPY])
    rng = np.random.default_rng(5)
    x.set_tensor(ff, rng.standard_normal((B, HID)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (B, 1)).astype(np.int32))
    return ff, out


def _step(ff, out):
    ff.forward()
    ff.zero_gradients()
    ff.backward()
    return torch.from_numpy(np.asarray(out.get_tensor(ff), dtype=np.float32))


def _grad(ff, w):
    return ff.executor.get_weight_grad(w).float().cpu()


def test_fused_moe_matches_per_expert_dense():
    plain, pout = _model(lambda ff, h: ff.moe(h, N_EXP, K_SEL, HID, 2.0, 0.04))
    fused, fout = _model(lambda ff, h: ff.moe(h, N_EXP, K_SEL, HID, 2.0, 0.04, fused_experts=True))
    pl = [L for L in plain.layers if L.op_type == LIN]          # first, gate, n experts, last
    fl = [L for L in fused.layers if L.op_type == LIN]          # first, gate, last
    ex = [L for L in fused.layers if L.op_type == EXD]
    assert len(pl) == N_EXP + 3 and len(fl) == 3 and len(ex) == 1
    assert tuple(ex[0].weights[0].dims) == (N_EXP, HID, HID) and tuple(ex[0].weights[1].dims) == (N_EXP * HID,)
    experts, others = pl[2:2 + N_EXP], pl[:2] + pl[-1:]
    for a, b in zip(others, fl):
        for wa, wb in zip(a.weights, b.weights):
            wb.set_weights(fused, wa.get_weights(plain))
    # bias away from zero, so that the padding rows of the unfused experts (relu(bias)) differ from zeros
    rng = np.random.default_rng(6)
    for L in experts:
        L.weights[1].set_weights(plain, rng.uniform(0.1, 0.5, HID).astype(np.float32))
    ex[0].weights[0].set_weights(fused, np.stack([L.weights[0].get_weights(plain) for L in experts]))
    ex[0].weights[1].set_weights(fused, np.concatenate([L.weights[1].get_weights(plain) for L in experts]))

    yp, yf = _step(plain, pout), _step(fused, fout)
    tol = dict(rtol=1e-5, atol=1e-6)  # fp32 round-off: the same sums in another order
    torch.testing.assert_close(yf, yp, **tol)
    for a, b in zip(others, fl):
        for wa, wb in zip(a.weights, b.weights):
            torch.testing.assert_close(_grad(fused, wb), _grad(plain, wa), **tol)
    torch.testing.assert_close(_grad(fused, ex[0].weights[0]),
                               torch.stack([_grad(plain, L.weights[0]) for L in experts]), **tol)
    torch.testing.assert_close(_grad(fused, ex[0].weights[1]),
                               torch.cat([_grad(plain, L.weights[1]) for L in experts]), **tol)
    assert float(_grad(fused, ex[0].weights[0]).abs().max()) > 0 and float(_grad(fused, fl[0].weights[0]).abs().max()) > 0


def test_default_moe_keeps_its_layers():
    ff, _ = _model(lambda ff, h: ff.moe(h, N_EXP, K_SEL, HID, 2.0, 0.04))
    got = [L.op_type.name[3:] for L in ff.layers]
    want = (["INPUT", "LINEAR", "LINEAR", "TOPK", "GROUP_BY", "SOFTMAX"] + ["LINEAR", "SOFTMAX"] * N_EXP
            + ["AGGREGATE", "LINEAR", "SOFTMAX"])
    assert got == want


def test_per_expert_initialisation():
    """Each expert's slice is drawn as a dense [out, in] weight: Glorot's bound from the expert's own fans."""
    ff, _ = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, 48, name="ffn"))
    w = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    bound = (6.0 / (HID + 48)) ** 0.5
    assert w.shape == (N_EXP, 48, HID) and np.abs(w).max() <= bound and np.abs(w).max() > 0.9 * bound
    assert all(not np.array_equal(w[0], w[e]) for e in range(1, N_EXP))
    assert not ff.get_layer_by_name("ffn_up").weights[1].get_weights(ff).any()


def test_moe_ffn_builds_and_learns():
    ff, out = _model(lambda ff, h: ff.moe_ffn(h, N_EXP, K_SEL, 32, name="ffn"), lr=0.2)
    kinds = [L.op_type for L in ff.layers]
    assert kinds.count(EXD) == 2 and kinds.count(LIN) == 3  # first, gate, last: no Linear per expert
    up, down = ff.get_layer_by_name("ffn_up"), ff.get_layer_by_name("ffn_down")
    assert [tuple(t.dims) for t in up.outputs] == [(64, 32)] * N_EXP  # cap = ceil(2 * 2 / 4 * 64)
    assert [tuple(t.dims) for t in down.outputs] == [(64, HID)] * N_EXP
    assert up.impl.flops([(64, HID)] * N_EXP, None, None) == 2.0 * N_EXP * 64 * HID * 32
    losses = []
    for _ in range(8):
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    assert losses[-1] < 0.9 * losses[0], losses


def test_builder_refuses_mismatched_expert_inputs():
    ff = FFModel(FFConfig(["--device", "cpu"]))
    a, b = ff.create_tensor([8, 16], DataType.DT_FLOAT), ff.create_tensor([8, 24], DataType.DT_FLOAT)
    idx = ff.create_tensor([16, 1], DataType.DT_INT32)
    with pytest.raises(ValueError, match="one shape"):
        ff.experts_dense([a, b], idx, 8)
