"""Gated linear units on the GPU: glu.hip element by element against the float64 oracle of
tests/glu_common.py (its docstring has the oracle, the bounds and the measured figures), the unary silu
under the same two bounds, and the gated FFN through its layers against fp32 torch on the same weights.

Kernel cases (CASES in glu_common.py) are the smallest shapes that reach each branch: fewer elements than
a vector, the flat path with a scalar tail, strided rows on the vector path, the scalar path chosen from a
stride / from a base pointer / from a packed buffer whose second half starts off 16 bytes, the packed form
with dg and du written into one buffer, one block whose threads loop (over one flat row, and over strided
rows, where a thread's steps carry from a row into the next), six different row strides, and
extreme gates with exact zeros. Every case runs the five activations, forward and backward, in bf16 and
fp32; all launches are legal ones (the misaligned cases must pick the scalar path). Outputs start between
sentinel guards; guards, row gaps and inputs are compared bit for bit afterwards.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import glu_common as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ffC():
    from flexflow_amd import _C
    return _C


# ------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("name", list(G.CASES))
def test_glu_kernel_bf16(ffC, name):
    w = G.check_case(name, torch.bfloat16, DEV)
    print(f"glu {name} bf16: worst |err| / tol {w:.3f}")


@pytest.mark.parametrize("name", list(G.CASES))
def test_glu_kernel_fp32(ffC, name):
    G.check_case(name, torch.float32, DEV)


def test_arguments_are_checked(ffC):
    a = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
    y = torch.empty_like(a)
    x2 = torch.zeros(4, 32, dtype=torch.bfloat16, device=DEV)
    ffC.glu_fwd(a, a, y, 0)
    ffC.glu_fwd(a, a, y, 4, 1)
    for bad in (lambda: ffC.glu_fwd(a, a, y, 5),  # no such activation
                lambda: ffC.glu_fwd(a, a[:, :8], y, 0),  # another width
                lambda: ffC.glu_fwd(a, a.float(), y, 0),  # another dtype
                lambda: ffC.glu_fwd(a, a, y.t().contiguous().t(), 0),  # no contiguous last dim
                lambda: ffC.glu_fwd(a, a, y[:1].expand(4, 16), 0),  # output rows on top of each other
                lambda: ffC.glu_fwd(a.cpu(), a.cpu(), y.cpu(), 0),
                lambda: ffC.glu_bwd(a, a, a, y, y[:, :8], 0),
                lambda: ffC.glu_fwd(a, a, a, 0),  # the output on top of an input
                lambda: ffC.glu_bwd(a, a, a, y, y, 0),  # dg and du the same view
                lambda: ffC.glu_bwd(a, a, a, x2[:, :16], x2[:, 8:24], 0)):  # halves that share columns
        with pytest.raises(RuntimeError):
            bad()
    ffC.glu_bwd(a, a, a, x2[:, :16], x2[:, 16:], 0)  # the halves of one buffer interleave: no overlap
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- unary silu
def _silu64(x):
    x = x.double()
    s, oms = torch.special.expit(x), torch.special.expit(-x)
    return x * s, s + x * s * oms


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", ["flat", "off1", "extremes"])
def test_unary_silu(ffC, dtype, mode):
    """unary silu forward / backward: bf16 by |err| <= 2^-8 |ref| + 2^-18 s (s = max(1, |x|), times |dy| in
    the backward), fp32 by the yardstick against F.silu and its autograd on the device."""
    from flexflow_amd import kernels as K
    g = torch.Generator().manual_seed(41)
    n = 4099
    x, dy = (torch.randn(n, generator=g) * 2).to(dtype), (torch.randn(n, generator=g) * 2).to(dtype)
    if mode == "extremes":
        x[:16] = torch.tensor(G.EXTREME_G).to(dtype)
        dy[3:9] = 0
    if mode == "off1":  # contiguous views one element into their buffers: the scalar path
        xb, db = (torch.full((n + 2,), 4096.0, dtype=dtype, device=DEV) for _ in range(2))
        xd, dyd = xb[1:-1], db[1:-1]
        xd.copy_(x), dyd.copy_(dy)
        assert xd.data_ptr() % 16 != 0
    else:
        xd, dyd = x.to(DEV), dy.to(DEV)
    y = K.unary_fwd("silu", xd)
    dx = K.unary_bwd("silu", xd, y, dyd)
    torch.cuda.synchronize()
    if mode == "off1":
        assert all(float(b[0]) == 4096.0 and float(b[-1]) == 4096.0 for b in (xb, db))
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    f, d = _silu64(x)
    m = x.double().abs().clamp(min=1.0)
    refs = {"fwd": (y, f, m), "bwd": (dx, dy.double() * d, m * dy.double().abs())}
    if dtype == torch.bfloat16:
        for what, (got, ref, s) in refs.items():
            miss, w = G.bf16_check(got, ref, s)
            print(f"unary silu {what} bf16 {mode}: {miss} outside, worst ratio {w:.3f}")
            assert miss == 0, (what, miss, w)
    else:
        xr = xd.detach().clone().requires_grad_()
        yt = F.silu(xr)
        (dxt,) = torch.autograd.grad(yt, xr, dyd)
        G.yardstick(y, yt.detach(), f, m, "unary silu", "fwd", f"unary silu fwd {mode}")
        G.yardstick(dx, dxt, refs["bwd"][1], refs["bwd"][2], "unary silu", "bwd", f"unary silu bwd {mode}")


# ------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("need_dx", [True, False], ids=["dx", "no_dx"])
@pytest.mark.parametrize("fused", [False, True], ids=["two_gemms", "fused_gate_up"])
def test_gated_ffn_op(ffC, fused, need_dx):
    """The tiny gated FFN (hidden 16, ffn 24, batch 4) through its layers in bf16 on the device against fp32
    torch on the same weights: output, input gradient (when asked for) and the three weight gradients."""
    g = torch.Generator().manual_seed(43)
    x = torch.randn(G.BATCH, G.HID, generator=g).bfloat16().float()
    dy = torch.randn(G.BATCH, G.HID, generator=g).bfloat16().float()
    W = G.ffn_weights()
    _, got = G.ffn_step(x, W, dy, DEV, torch.bfloat16, fused=fused, need_dx=need_dx)
    torch.cuda.synchronize()
    want = G.ffn_torch(x, W, dy)
    if not need_dx:
        assert "dx" not in got
        want.pop("dx")
    assert set(got) == set(want), (sorted(got), sorted(want))
    errs = {n: G.rel(got[n], want[n]) for n in got}
    print("gated ffn relative errors", fused, need_dx, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(torch.isfinite(t).all() for t in got.values())
    assert errs.pop("y") < G.TOL_O and all(e < G.TOL_G for e in errs.values()), errs
    other = G.ffn_torch(x, W, dy, act="gelu_tanh")
    assert G.rel(other["y"], want["y"]) > 5 * G.TOL_O  # the activation matters at this bound


def test_glu_op_fp32_device_path(ffC):
    """The op alone in fp32 on the device, both forms, against float64: the packed backward returns one
    [.., 2F] gradient."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    g = torch.Generator().manual_seed(45)
    a, b, dy = (torch.randn(3, 5, 24, generator=g) for _ in range(3))
    f, d = G.act64(a.double(), "gelu_tanh")
    ff = FFModel(FFConfig([]))
    ta, tb = (ff.create_tensor([3, 5, 24], DataType.DT_FLOAT) for _ in range(2))
    tp = ff.create_tensor([3, 5, 48], DataType.DT_FLOAT)
    for L, xs in ((ff.glu(ta, tb, activation="gelu_tanh").owner_layer, [a, b]),
                  (ff.glu(tp, activation="gelu_tanh").owner_layer, [torch.cat([a, b], -1)])):
        ctx = OpCtx(layer=L, part_coords=(0, 0, 0), degrees=(1, 1, 1))
        y = L.impl.forward(ctx, [t.to(DEV) for t in xs], [])[0]
        ds = L.impl.backward(ctx, [dy.to(DEV)])
        torch.cuda.synchronize()
        assert len(ds) == len(xs) and all(t.shape == x.shape for t, x in zip(ds, xs))
        dg, du = (ds[0][..., :24], ds[0][..., 24:]) if len(xs) == 1 else ds
        for got, ref in ((y, f * b.double()), (dg, dy.double() * b.double() * d), (du, dy.double() * f)):
            assert G.rel(got, ref) < 1e-5


# ------------------------------------------------------------------------------------- training
def _train_decoder(flags, fused, steps=6):
    from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    torch.manual_seed(0)
    B = 4
    dc = DecoderConfig(hidden=128, heads=2, kv_heads=1, layers=2, ffn=256, vocab=1000, seq=64, mlp="swiglu",
                       fused_gate_up=fused)
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    ids, _ = build_rope_decoder(ff, B, dc)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    tok = rng.integers(1, dc.vocab, (N, dc.seq)).astype(np.int32)
    loaders = [ff.create_data_loader(ids, tok),
               ff.create_data_loader(ff.label_tensor, ((tok + 1) % dc.vocab)[..., None].astype(np.int32))]
    losses = []
    for _ in range(steps):
        for dl in loaders:
            dl.next_batch(ff)
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    torch.cuda.synchronize()
    weights = [np.asarray(w.get_weights(ff)) for L in ff.layers for w in L.weights]
    return ff, np.asarray(losses, dtype=np.float64), weights


@pytest.mark.parametrize("fused", [False, True], ids=["two_gemms", "fused_gate_up"])
def test_swiglu_decoder_trains_under_step_capture(fused, monkeypatch):
    """The rotary decoder with a SwiGLU MLP (2 blocks, hidden 128, ffn 256, batch 4, S 64), the whole step
    captured into a hipGraph (FF_GRAPH_UPDATE=1) against eager steps: the graph must exist (the glu op does
    not synchronise with the host), and losses and weights agree as test_rope_gpu.py asks of captured against
    eager steps (rtol 1e-5, atol 1e-6)."""
    monkeypatch.setenv("FF_GRAPH_UPDATE", "1")
    ffg, lg, wg = _train_decoder(["--hip-graphs"], fused)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    assert sum(L.op_type.name == "OP_GLU" for L in ffg.layers) == 2
    _, le, we = _train_decoder(["--no-hip-graphs"], fused)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
