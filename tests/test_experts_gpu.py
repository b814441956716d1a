"""Grouped expert GEMMs (csrc/kernels/experts.hip) element by element against a float64 loop over the
experts, with NaN in every padding row of the inputs and a sentinel in the outputs, and the moe_ffn
model's captured training step.

Bounds: a bf16 output may differ from the exact value by one bf16 rounding, 2^-8 |ref| with a factor 2
of margin, plus the fp32 accumulation bound L 2^-23 sum |a_i| |b_i| over the L terms of its sum; an
fp32 output (dW, db) by the second term only, L = the expert's live rows."""
import functools

import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_EXP, CAP, LOADS = 4, 160, (0, 1, 129, 160)  # B = 400, k = 1, alpha = 1.6; 270 tokens for expert 3, clamped
EPS_BF16, EPS_F32 = 2.0 ** -8, 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(din, dout):
    """Inputs (padding rows poisoned) and the float64 references of one (in_dim, out_dim), computed once."""
    g = torch.Generator().manual_seed(din * 1000 + dout)
    assign = torch.tensor([1] + [2] * 129 + [3] * 270, dtype=torch.int32)[torch.randperm(400, generator=g)]
    load = K.moe_route(assign.to(DEV).view(400, 1), N_EXP, CAP)[2]
    assert load.tolist() == [0, 1, 129, 270]
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    xs, dys = [bf(CAP, din) for _ in range(N_EXP)], [bf(CAP, dout) for _ in range(N_EXP)]
    w, b = bf(N_EXP, dout, din) * 0.25, bf(N_EXP * dout)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    z, zmag = f64(N_EXP, CAP, dout), f64(N_EXP, CAP, dout)       # pre-activation without the bias
    dx, dxmag = f64(N_EXP, CAP, din), f64(N_EXP, CAP, din)
    dw, dwmag, db, dbmag = f64(N_EXP, dout, din), f64(N_EXP, dout, din), f64(N_EXP, dout), f64(N_EXP, dout)
    for e, r in enumerate(LOADS):
        x, dy, we = xs[e][:r].double(), dys[e][:r].double(), w[e].double()
        z[e, :r], zmag[e, :r] = x @ we.t(), x.abs() @ we.abs().t()
        dx[e, :r], dxmag[e, :r] = dy @ we, dy.abs() @ we.abs()
        dw[e], dwmag[e] = dy.t() @ x, dy.abs().t() @ x.abs()
        db[e], dbmag[e] = dy.sum(0), dy.abs().sum(0)
        xs[e][r:], dys[e][r:] = float("nan"), float("nan")
    dev = lambda ts: [t.to(DEV) for t in ts]
    return dict(load=load, xs=dev(xs), dys=dev(dys), w=w.to(DEV), b=b.to(DEV), bd=b.double().view(N_EXP, 1, dout),
                z=z, zmag=zmag, dx=dx, dxmag=dxmag, dw=dw, dwmag=dwmag, db=db, dbmag=dbmag)


def _check(name, got, ref, mag, terms, out_eps):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    terms = torch.as_tensor(terms, dtype=torch.float64).view(-1, *([1] * (ref.dim() - 1)))
    excess = (got - ref).abs() - (out_eps * ref.abs() + terms * EPS_F32 * mag)
    print(f"{name}: max |err| {float((got - ref).abs().max()):.3e}, max excess over the bound {float(excess.max()):.3e}")
    assert float(excess.max()) <= 0, f"{name}: {int((excess > 0).sum())} elements beyond the bound"


def _padding_is_zero(slab):
    return all(bool((slab[e, r:] == 0).all()) for e, r in enumerate(LOADS))


DIMS = [(64, 128), (72, 136), (256, 8)]  # tile-exact; partial tiles in N and K; a narrow output


@pytest.mark.parametrize("tile_m", [64, 128])
@pytest.mark.parametrize("act,bias", [(K.ACT_NONE, False), (K.ACT_NONE, True), (K.ACT_RELU, False), (K.ACT_RELU, True)])
@pytest.mark.parametrize("din,dout", DIMS)
def test_forward(din, dout, act, bias, tile_m):
    c = _case(din, dout)
    y = torch.full((N_EXP, CAP, dout), 7.0, device=DEV, dtype=torch.bfloat16)
    z = torch.full_like(y, 7.0)
    assert K.ext().experts_fwd(c["xs"], c["w"], c["b"] if bias else None, c["load"], y, z, act, tile_m)
    live = (torch.arange(CAP)[None, :] < torch.tensor(LOADS)[:, None])[:, :, None]
    zr = torch.where(live, c["z"] + (c["bd"] if bias else 0.0), 0.0)
    mag = c["zmag"] + (c["bd"].abs() if bias else 0.0)
    _check("z", z, zr, mag, din + 1, EPS_BF16)
    _check("y", y, zr.clamp_min(0) if act == K.ACT_RELU else zr, mag, din + 1, EPS_BF16)
    assert _padding_is_zero(y) and _padding_is_zero(z)
    if act == K.ACT_RELU:  # the activation backward on the kernel's own z: dy or zero, exactly
        dz = torch.full_like(y, 7.0)
        assert K.ext().experts_act_bwd(c["dys"], z, dz, c["load"], act)
        for e, r in enumerate(LOADS):
            assert torch.equal(dz[e, :r], torch.where(z[e, :r] > 0, c["dys"][e][:r], 0.0)) and bool((dz[e, r:] == 7).all())


@pytest.mark.parametrize("tile_m", [64, 128])
@pytest.mark.parametrize("din,dout", DIMS)
def test_input_gradient(din, dout, tile_m):
    c = _case(din, dout)
    dx = torch.full((N_EXP, CAP, din), 7.0, device=DEV, dtype=torch.bfloat16)
    assert K.ext().experts_bwd_data(c["dys"], c["w"], c["load"], dx, tile_m)
    _check("dx", dx, c["dx"], c["dxmag"], dout, EPS_BF16)
    assert _padding_is_zero(dx)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("din,dout", DIMS)
def test_weight_gradient(din, dout, bias):
    c = _case(din, dout)
    g = torch.Generator().manual_seed(3)
    dw0, db0 = torch.randn(N_EXP, dout, din, generator=g), torch.randn(N_EXP * dout, generator=g)
    runs = []
    for _ in range(2):
        dw, db = dw0.to(DEV), db0.to(DEV) if bias else None
        assert K.ext().experts_bwd_weight(c["dys"], c["xs"], c["load"], dw, db, CAP)
        runs.append((dw, db))
    dw, db = runs[0]
    _check("dW", dw.double().cpu() - dw0.double(), c["dw"], c["dwmag"] + dw0.abs().double(), [r + 1 for r in LOADS], 0.0)
    assert torch.equal(dw[0].cpu(), dw0[0]) and torch.equal(runs[1][0], dw)  # expert 0 untouched; same bits
    if bias:
        _check("db", (db.double().cpu() - db0.double()).view(N_EXP, dout), c["db"],
               c["dbmag"] + db0.view(N_EXP, dout).abs().double(), [r + 1 for r in LOADS], 0.0)
        assert torch.equal(db[:dout].cpu(), db0[:dout]) and torch.equal(runs[1][1], db)


def test_gelu_epilogue_matches_linear(monkeypatch):
    """load = cap: each expert is a plain Linear, and GELU is the epilogue function linear_fwd's kernels use."""
    monkeypatch.setattr(K, "_TUNE", False)  # linear_fwd on the project's own GEMM kernel, not the library's
    g = torch.Generator().manual_seed(9)
    n, cap, din, dout = 2, 96, 64, 136
    xs = [torch.randn(cap, din, generator=g).to(torch.bfloat16).to(DEV) for _ in range(n)]
    w = (torch.randn(n, dout, din, generator=g) * 0.25).to(torch.bfloat16).to(DEV)
    b = torch.randn(n * dout, generator=g).to(torch.bfloat16).to(DEV)
    load = torch.full((n,), cap, device=DEV, dtype=torch.int32)
    y, _ = K.experts_fwd(xs, w, b, load, K.ACT_GELU)
    for e in range(n):
        be = b[e * dout:(e + 1) * dout]
        ref, _ = K.linear_fwd(xs[e], w[e], be, K.ACT_GELU, save_z=False)
        mag = xs[e].double().abs() @ w[e].double().abs().t() + be.double().abs()
        _check(f"gelu[{e}]", y[e], ref.double().cpu(), mag.cpu(), din + 1, EPS_BF16)


def test_refused_shapes_fall_back():
    """N % 8 != 0 is refused by the launcher; the entry point then runs the torch loop, same semantics."""
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(16, 8, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2)]
    w = torch.randn(2, 12, 8, generator=g).to(torch.bfloat16).to(DEV)
    load = torch.tensor([16, 3], device=DEV, dtype=torch.int32)
    y = torch.empty(2, 16, 12, device=DEV, dtype=torch.bfloat16)
    assert not K.ext().experts_fwd(xs, w, None, load, y, None, K.ACT_NONE, 0)
    got, _ = K.experts_fwd(xs, w, None, load, K.ACT_NONE)
    ref = torch.stack([x.float() @ w[e].float().t() for e, x in enumerate(xs)])
    ref[1, 3:] = 0
    torch.testing.assert_close(got.float(), ref, rtol=2 ** -7, atol=1e-6)


def test_moe_ffn_step_captures():
    """Six bf16 training steps of the moe_ffn block under --hip-graphs: the step graph is captured."""
    import numpy as np
    from flexflow_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig(["--hip-graphs", "--dtype", "bf16"])
    cfg.batch_size = 64
    ff = FFModel(cfg)
    x = ff.create_tensor([64, 64], DataType.DT_FLOAT)
    ff.softmax(ff.dense(ff.moe_ffn(ff.dense(x, 64), 4, 2, 128, name="ffn"), 10))
    ff.optimizer = SGDOptimizer(ff, 0.01)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[])
    rng = np.random.default_rng(0)
    x.set_tensor(ff, rng.standard_normal((64, 64)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (64, 1)).astype(np.int32))
    w0 = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    for _ in range(6):
        ff.train_step()
    torch.cuda.synchronize()
    sg = ff._step_graph
    assert sg is not None and not sg.failed and sg.graph is not None
    w1 = ff.get_layer_by_name("ffn_up").weights[0].get_weights(ff)
    assert np.isfinite(w1).all() and not np.array_equal(w0, w1)
