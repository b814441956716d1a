"""Gated grouped expert GEMMs (experts_glu_rows_kernel / experts_glu_bwd_kernel of csrc/kernels/experts.hip)
element by element against a float64 loop over the experts, with NaN in every padding row of the inputs and
a sentinel in the outputs, at test_experts_gpu.py's routing, and the gated moe_ffn's captured training step.

Bounds, written down before any run. With dg, du = (K + 1) 2^-23 mag_g, mag_u the fp32 accumulation bounds of
zg, zu (mag = sum |x_i| |w_i| + |bias|):
  Z: 2 * 2^-8 |ref| + (dg | du)                               one bf16 rounding with a factor 2 of margin
  H: 2 * 2^-8 |h| + 1.13 dg (|zu| + du) + max(1, |zg|) du + 2^-18 max(1, |zg|) |zu|
     the accumulation bounds pushed through act(zg) zu with |act'| < 1.13 and |act(x)| <= max(1, |x|), plus
     glu_common.py's term for the fp32 activation arithmetic
  dZ: glu_common.py's dg / du bounds from the stored bf16 values."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import glu_common as G  # noqa: E402
from flexflow_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_EXP, CAP, LOADS = 4, 160, (0, 1, 129, 160)  # 270 tokens for expert 3, clamped to the capacity
EPS_BF16, EPS_F32 = 2.0 ** -8, 2.0 ** -23
DIMS = [(64, 64), (72, 72), (256, 8)]  # tile-exact; partial K tile and the up half inside a gate tile's span; narrow


@functools.lru_cache(maxsize=None)
def _case(din, F_):
    """Inputs (padding rows poisoned) and the float64 sums of one (in_dim, F), computed once."""
    g = torch.Generator().manual_seed(din * 1000 + F_)
    assign = torch.tensor([1] + [2] * 129 + [3] * 270, dtype=torch.int32)[torch.randperm(400, generator=g)]
    load = K.moe_route(assign.to(DEV).view(400, 1), N_EXP, CAP)[2]
    assert load.tolist() == [0, 1, 129, 270]
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)  # noqa: E731
    xs, dhs = [bf(CAP, din) for _ in range(N_EXP)], [bf(CAP, F_) for _ in range(N_EXP)]
    w, b, zin = bf(N_EXP, 2 * F_, din) * 0.25, bf(N_EXP * 2 * F_), bf(N_EXP, CAP, 2 * F_) * 2
    z = torch.zeros(N_EXP, CAP, 2 * F_, dtype=torch.float64)  # (zg | zu) without the bias
    zmag = torch.zeros_like(z)
    for e, r in enumerate(LOADS):
        x, we = xs[e][:r].double(), w[e].double()
        z[e, :r], zmag[e, :r] = x @ we.t(), x.abs() @ we.abs().t()
        xs[e][r:], dhs[e][r:], zin[e, r:] = float("nan"), float("nan"), float("nan")
    dev = lambda ts: [t.to(DEV) for t in ts]  # noqa: E731
    return dict(load=load, xs=dev(xs), dhs=dev(dhs), w=w.to(DEV), b=b.to(DEV), zin=zin.to(DEV),
                bd=b.double().view(N_EXP, 1, 2 * F_), z=z, zmag=zmag)


def _within(name, got, ref, tol):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    err = (got - ref).abs()
    print(f"{name}: max |err| {float(err.max()):.3e}, worst |err| / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all()), f"{name}: {int((err > tol).sum())} elements beyond the bound"


def _padding_is(slab, value):
    return all(bool((slab[e, r:] == value).all()) for e, r in enumerate(LOADS))


@pytest.mark.parametrize("epilogue", [1, 2])  # staged through LDS, direct
@pytest.mark.parametrize("tile_m", [64, 128])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", ["silu", "gelu_tanh", "relu"])
@pytest.mark.parametrize("din,F_", DIMS)
def test_forward(din, F_, act, bias, tile_m, epilogue):
    c = _case(din, F_)
    h = torch.full((N_EXP, CAP, F_), 7.0, device=DEV, dtype=torch.bfloat16)
    z = torch.full((N_EXP, CAP, 2 * F_), 7.0, device=DEV, dtype=torch.bfloat16)
    assert K.ext().experts_glu_fwd(c["xs"], c["w"], c["b"] if bias else None, c["load"], h, z, K.GLU_ACTS[act], tile_m,
                                   epilogue)
    live = (torch.arange(CAP)[None, :] < torch.tensor(LOADS)[:, None])[:, :, None]
    zr = torch.where(live, c["z"] + (c["bd"] if bias else 0.0), 0.0)
    acc = (din + 1) * EPS_F32 * (c["zmag"] + (c["bd"].abs() if bias else 0.0))
    _within("z", z, zr, 2 * EPS_BF16 * zr.abs() + acc)
    zg, zu, dg, du = zr[..., :F_], zr[..., F_:], acc[..., :F_], acc[..., F_:]
    hr = G.act64(zg, act)[0] * zu
    m = zg.abs().clamp(min=1.0)
    _within("h", h, hr, 2 * EPS_BF16 * hr.abs() + 1.13 * dg * (zu.abs() + du) + m * du + G.AT_BF16 * m * zu.abs())
    assert _padding_is(h, 0) and _padding_is(z, 0)


@pytest.mark.parametrize("act", ["silu", "gelu_tanh", "relu"])
@pytest.mark.parametrize("din,F_", DIMS)
def test_gate_backward(din, F_, act):
    c = _case(din, F_)
    dz = torch.full((N_EXP, CAP, 2 * F_), 7.0, device=DEV, dtype=torch.bfloat16)
    assert K.ext().experts_glu_bwd(c["dhs"], c["zin"], dz, c["load"], K.GLU_ACTS[act])
    assert _padding_is(dz, 7.0)  # rows past the load and all of expert 0 untouched
    for e, r in enumerate(LOADS):
        if r == 0:
            continue
        refs = G.oracle(c["zin"][e, :r, :F_].cpu(), c["zin"][e, :r, F_:].cpu(), c["dhs"][e][:r].cpu(), act)
        for o, got in (("dg", dz[e, :r, :F_]), ("du", dz[e, :r, F_:])):
            miss, worst = G.bf16_check(got, *refs[o])
            print(f"{o}[{e}] {act}: {miss} of {got.numel()} outside, worst ratio {worst:.3f}")
            assert miss == 0, (o, e, miss, worst)


def test_refused_shape_falls_back():
    """F % 8 != 0 is refused by the launcher; the entry point then runs the torch loop, same semantics."""
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(16, 8, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2)]
    w = torch.randn(2, 24, 8, generator=g).to(torch.bfloat16).to(DEV)
    load = torch.tensor([16, 3], device=DEV, dtype=torch.int32)
    h = torch.empty(2, 16, 12, device=DEV, dtype=torch.bfloat16)
    assert not K.ext().experts_glu_fwd(xs, w, None, load, h, None, K.GLU_ACTS["silu"], 0)
    got, z = K.experts_glu_fwd(xs, w, None, load, "silu", save_z=True)
    zr = torch.stack([x.float() @ w[e].float().t() for e, x in enumerate(xs)])
    zr[1, 3:] = 0
    torch.testing.assert_close(z.float(), zr, rtol=2 ** -7, atol=1e-6)
    torch.testing.assert_close(got.float(), torch.nn.functional.silu(zr[..., :12]) * zr[..., 12:], rtol=2 ** -7, atol=1e-6)


def test_gated_moe_ffn_step_captures():
    """Six bf16 training steps of the gated moe_ffn block under --hip-graphs: the step graph is captured."""
    import numpy as np
    from flexflow_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig(["--hip-graphs", "--dtype", "bf16"])
    cfg.batch_size = 64
    ff = FFModel(cfg)
    x = ff.create_tensor([64, 64], DataType.DT_FLOAT)
    ff.softmax(ff.dense(ff.moe_ffn(ff.dense(x, 64), 4, 2, 128, gate_activation="silu", use_bias=False, name="ffn"), 10))
    ff.optimizer = SGDOptimizer(ff, 0.01)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[])
    rng = np.random.default_rng(0)
    x.set_tensor(ff, rng.standard_normal((64, 64)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (64, 1)).astype(np.int32))
    w0 = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    assert w0.shape == (4, 256, 64)
    for _ in range(6):
        ff.train_step()
    torch.cuda.synchronize()
    sg = ff._step_graph
    assert sg is not None and not sg.failed and sg.graph is not None
    w1 = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    assert np.isfinite(w1).all() and not np.array_equal(w0, w1)
