"""Gradient clipping by global norm on the device: the deterministic sum-of-squares kernel, the
coefficient kernel, the update kernels' device-side gradient scale, and clipped training steps
(eager, captured into a hipGraph, and DLRM's tables falling back to the dense update)."""
import math

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ULP32 = 2.0 ** -23
GUARD = 4096.0  # exact in bf16; its square would swamp any sum that read it


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(v):
    return float(np.float32(v))


def _chain(n):
    """d(n): the longest chain of fp32 additions an element passes through in grad_sumsq, as the
    kernel's comment in csrc/kernels/optimizer.hip gives it."""
    nv = n // 4
    G = min((nv + 256 * 8 - 1) // (256 * 8), 2048)
    iters = -(-nv // (256 * G)) if G else 0
    pf = -(-G // 256)
    return -(-iters // 4) + 2 + 2 + 10 + pf + 10 + 3 + 1


def _sumsq_tol(n):
    return (_chain(n) + 2) * 2.0 ** -24


def test_sumsq_bound_needs_a_tree():
    assert _sumsq_tol(2 ** 22 + 3) <= 1e-5
    assert _chain(2 ** 22 + 3) == 32 and _chain(335_000_000) == 76


# ----------------------------------------------------------------------------------- grad_sumsq
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 255, 10001, 2 ** 22 + 3])
def test_grad_sumsq(ffC, n):
    """Against fp64; accumulate against overwrite; the same bits on a second run; a slice at a
    16-byte offset of a larger buffer, with guards around the slice, the partials and the scalar."""
    x = torch.randn(n, generator=_gen(100 + n % 97))
    ref = float((x.double() ** 2).sum())
    for off in (4, 16):  # floats: 16 and 64 bytes into the buffer
        buf = torch.full((n + 2 * off + 4,), GUARD, device=DEV)
        xs = buf[off:off + n]
        xs.copy_(x)
        ws_buf = torch.full((K.GRAD_SUMSQ_PARTIALS + 16,), GUARD, device=DEV)
        ws = ws_buf[8:8 + K.GRAD_SUMSQ_PARTIALS]
        scal = torch.full((3,), GUARD, device=DEV)
        out = scal[1:2]
        ffC.grad_sumsq(xs, ws, out, False)  # overwrites the guard value in out
        got = out.clone()
        rel = abs(got.item() - ref) / ref
        print(f"grad_sumsq n={n} off={off}: rel err {rel:.3e}, allowed {_sumsq_tol(n):.3e}")
        assert rel <= _sumsq_tol(n), (n, off, got.item(), ref, rel)
        ffC.grad_sumsq(xs, ws, out, False)
        assert torch.equal(out, got), "second run differs"
        out.fill_(7.0)
        ffC.grad_sumsq(xs, ws, out, True)
        assert torch.equal(out, got + 7.0), "accumulate is not out + overwrite"
        # nothing outside the slice, the partials or the scalar was written (or read: see GUARD)
        assert torch.equal(buf[:off], torch.full((off,), GUARD, device=DEV))
        assert torch.equal(buf[off + n:], torch.full((off + 4,), GUARD, device=DEV))
        assert torch.equal(ws_buf[:8], ws_buf[-8:]) and bool((ws_buf[:8] == GUARD).all())
        assert scal[0].item() == GUARD and scal[2].item() == GUARD
        assert torch.equal(xs.cpu(), x), "the input changed"
    # an all-zero range sums to exactly zero, and adds nothing
    z = torch.zeros(n, device=DEV)
    ws = torch.empty(K.GRAD_SUMSQ_PARTIALS, device=DEV)
    out = torch.full((1,), GUARD, device=DEV)
    ffC.grad_sumsq(z, ws, out, False)
    assert out.item() == 0.0
    out.fill_(3.0)
    ffC.grad_sumsq(z, ws, out, True)
    assert out.item() == 3.0


def test_grad_sumsq_rejects_bad_arguments(ffC):
    x = torch.zeros(64, device=DEV)
    out = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError):
        ffC.grad_sumsq(x, torch.empty(K.GRAD_SUMSQ_PARTIALS - 1, device=DEV), out, False)  # workspace too small
    with pytest.raises(RuntimeError):
        ffC.grad_sumsq(x[1:], torch.empty(K.GRAD_SUMSQ_PARTIALS, device=DEV), out, False)  # not 16-byte aligned
    assert ffC.grad_sumsq_partials() == K.GRAD_SUMSQ_PARTIALS


# ------------------------------------------------------------------------------------ clip_coef
def test_clip_coef(ffC):
    eps, max_norm = np.float32(1e-6), np.float32(1.0)
    for s in (0.0, 1e-12, 0.25, 4.0, 1e30):
        scal = torch.full((5,), GUARD, device=DEV)
        sumsq = torch.tensor([s], dtype=F32, device=DEV)
        ffC.clip_coef(sumsq, 1.0, scal[1:2], scal[3:4])
        norm_ref = np.sqrt(np.float32(s))
        coef_ref = min(np.float32(1.0), max_norm / (norm_ref + eps))
        norm, coef = scal[1].item(), scal[3].item()
        assert abs(norm - norm_ref) <= 4 * ULP32 * norm_ref, (s, norm, norm_ref)
        assert abs(coef - coef_ref) <= 4 * ULP32 * coef_ref, (s, coef, coef_ref)
        if norm_ref + eps <= max_norm:
            assert coef == 1.0, (s, coef)
        else:
            assert coef < 1.0, (s, coef)
        assert scal[0].item() == GUARD and scal[2].item() == GUARD and scal[4].item() == GUARD
        assert sumsq.item() == np.float32(s)
    # a non-finite norm propagates, as torch's clamp(max=1) does
    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ffC.clip_coef(torch.tensor([float("nan")], device=DEV), 1.0, norm, coef)
    assert math.isnan(norm.item()) and math.isnan(coef.item())
    ffC.clip_coef(torch.tensor([float("inf")], device=DEV), 1.0, norm, coef)
    assert math.isinf(norm.item()) and coef.item() == 0.0


# --------------------------------------------------------------- sgd / adam with gscale_dev
def _d(t):
    return t.detach().cpu().double()


def _close(got, ref64, atol, what):
    err = (_d(got) - ref64).abs() - atol
    i = int(err.argmax())
    assert err[i] <= 0, f"{what}: element {i}: got {_d(got)[i].item()!r}, ref {ref64[i].item()!r}"


def _opt_tol(ref64, step):
    """As tests/test_small_kernels_gpu.py: 16 fp32 ulps of max(1, |value|) per step taken."""
    return 16 * step * ULP32 * ref64.abs().clamp_min(1.0)


GS_HOST, GS_DEV = 0.5, 0.25  # effective scale 0.125, exact in fp32


@pytest.mark.parametrize("max_blocks", [0, 2, -1, -8])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 10001])
def test_sgd_update_gscale_dev(ffC, n, max_blocks):
    lr = 0.1
    gsd = torch.tensor([GS_DEV], device=DEV)
    for momentum in (0.0, 0.9):
        for nesterov in (False, True):
            for wd in (0.0, 0.01):
                for with_lowp in (False, True):
                    g = _gen(90)
                    w0 = torch.randn(n, generator=g)
                    w = w0.to(DEV)
                    mom = torch.zeros(n, device=DEV) if momentum > 0 else None
                    lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV) if with_lowp else None
                    w64, v64 = w0.double(), torch.zeros(n, dtype=torch.float64)
                    tag = f"sgd n={n} mb={max_blocks} mom={momentum} nest={nesterov} wd={wd}"
                    for step in (1, 2, 3):
                        grad = torch.randn(n, generator=g)
                        ffC.sgd_update(w, grad.to(DEV), mom, lowp, lr, momentum, nesterov, wd, GS_HOST, max_blocks,
                                       gscale_dev=gsd)
                        gt = grad.double() * (GS_HOST * GS_DEV) + _f32(wd) * w64  # weight decay unscaled
                        if momentum > 0:
                            v64 = v64 * _f32(momentum) + gt
                            gt = gt + _f32(momentum) * v64 if nesterov else v64
                        w64 = w64 - _f32(lr) * gt
                        _close(w, w64, _opt_tol(w64, step), f"w step {step} " + tag)
                        if mom is not None:
                            _close(mom, v64, _opt_tol(v64, step), f"mom step {step} " + tag)
                        if lowp is not None:
                            assert torch.equal(lowp, w.bfloat16()), f"lowp step {step} " + tag
    assert gsd.item() == GS_DEV
    # gscale_dev=None: bitwise the call without the argument
    g = _gen(92)
    w0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g).to(DEV)
    res = []
    for kw in ({}, {"gscale_dev": None}):
        w, mom = w0.to(DEV), torch.zeros(n, device=DEV)
        lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV)
        ffC.sgd_update(w, grad, mom, lowp, lr, 0.9, True, 0.01, GS_HOST, max_blocks, **kw)
        res.append((w, mom, lowp))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("max_blocks", [0, 2, -1, -8])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 10001])
def test_adam_update_gscale_dev(ffC, n, max_blocks):
    b1, b2, eps = 0.9, 0.999, 1e-8
    one = np.float32(1.0)
    c1, c2 = float(one - np.float32(b1)), float(one - np.float32(b2))  # 1 - beta as the kernel forms it
    gsd = torch.tensor([GS_DEV], device=DEV)
    for wd in (0.0, 0.01):
        for use_dev in (False, True):
            g = _gen(91)
            w0 = torch.randn(n, generator=g)
            w = w0.to(DEV)
            m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
            lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV)
            alpha_dev = torch.zeros(1, device=DEV) if use_dev else None
            w64 = w0.double()
            m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            tag = f"adam n={n} mb={max_blocks} wd={wd} alpha_dev={use_dev}"
            for step in (1, 2, 3):
                alpha_t = 1e-2 * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
                grad = torch.randn(n, generator=g)
                if use_dev:
                    alpha_dev.fill_(alpha_t)
                    ffC.adam_update(w, grad.to(DEV), m, v, lowp, 123.0, b1, b2, wd, eps, GS_HOST, max_blocks, alpha_dev,
                                    gscale_dev=gsd)
                else:
                    ffC.adam_update(w, grad.to(DEV), m, v, lowp, alpha_t, b1, b2, wd, eps, GS_HOST, max_blocks,
                                    gscale_dev=gsd)
                gt = grad.double() * (GS_HOST * GS_DEV) + _f32(wd) * w64
                m64 = _f32(b1) * m64 + c1 * gt
                v64 = _f32(b2) * v64 + c2 * gt * gt
                w64 = w64 - _f32(alpha_t) * m64 / (v64.sqrt() + _f32(eps))
                _close(w, w64, _opt_tol(w64, step), f"w step {step} " + tag)
                _close(m, m64, _opt_tol(m64, step), f"m step {step} " + tag)
                _close(v, v64, _opt_tol(v64, step), f"v step {step} " + tag)
                assert torch.equal(lowp, w.bfloat16()), f"lowp step {step} " + tag
    g = _gen(93)
    w0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g).to(DEV)
    res = []
    for kw in ({}, {"gscale_dev": None}):
        w, m, v = w0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV)
        ffC.adam_update(w, grad, m, v, lowp, 1e-2, b1, b2, 0.01, eps, GS_HOST, max_blocks, **kw)
        res.append((w, m, v, lowp))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------- training steps
B = 8


def _mlp(flags, make_opt):
    """The three-Dense MLP of tests/test_zero_cpu.py: 40 -> 64 -> 48 -> 10, batch 8. The 10-element
    bias is no multiple of 8, so its arena entry is followed by padding."""
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel, LossType, MetricsType
    cfg = FFConfig(["--search", "dp", "--no-hip-graphs"] + flags)
    cfg.batch_size = B
    ff = FFModel(cfg)
    x = ff.create_tensor([B, 40], DataType.DT_FLOAT)
    t = ff.dense(x, 64, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 48, ActiMode.AC_MODE_RELU, name="d2")
    ff.softmax(ff.dense(t, 10, name="d3"))
    ff.optimizer = make_opt(ff)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    x.set_tensor(ff, rng.standard_normal((B, 40)).astype(np.float32))
    ff.label_tensor.set_tensor(ff, rng.integers(0, 10, (B, 1)).astype(np.int32))
    return ff


def _weights(ff):
    torch.cuda.synchronize()
    return {f"{L.name}.{i}": np.asarray(w.get_weights(ff)) for L in ff.layers for i, w in enumerate(L.weights)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_clipped_sgd_step(dtype):
    from flexflow_amd.core import SGDOptimizer
    lr, clip = 0.05, 0.5
    ff = _mlp(["--dtype", dtype], lambda ff: SGDOptimizer(ff, lr, clip_norm=clip))
    ex = ff.executor
    assert ff.get_grad_norm() == 0.0  # no update yet
    ff.zero_gradients()
    ff.forward()
    ff.backward()
    torch.cuda.synchronize()
    arenas = [ar for ar in ex.arenas.values() if ar.size]
    assert arenas
    sumsq, n_total, odd = 0.0, 0, False
    before = []
    for ar in arenas:
        g = ar.grad[:ar.size].detach().cpu().double()
        real = torch.zeros(ar.size, dtype=torch.bool)
        for _, off, n, _ in ar.entries:
            real[off:off + n] = True
            odd |= n % 8 != 0
        # the update sums whole arenas: the padding between entries must hold exact zeros
        assert not bool(g[~real].any()), "padding gradient is not zero"
        sumsq += float((g[real] ** 2).sum())
        n_total += ar.size
        before.append((ar.master[:ar.size].detach().cpu().double(), g))
    assert odd, "the model has no odd-sized weight: the padding check is vacuous"
    norm = math.sqrt(sumsq)
    assert norm > clip, norm  # the step clips
    coef = min(1.0, clip / (norm + 1e-6))
    ff.update()
    got_norm = ff.get_grad_norm()
    print(f"{dtype}: norm {norm!r}, get_grad_norm {got_norm!r}")
    assert abs(got_norm - norm) <= _sumsq_tol(n_total) * norm, (got_norm, norm)
    moved = 0.0
    for ar, (w0, g) in zip(arenas, before):
        w1 = ar.master[:ar.size].detach().cpu().double()
        step = (w0 - w1) / lr
        tol = 4 * ULP32 * w0.abs().clamp_min(1.0) / lr
        err = (step - coef * g).abs() - tol
        i = int(err.argmax())
        assert err[i] <= 0, (i, step[i].item(), coef * g[i].item(), tol[i].item())
        moved += float((step ** 2).sum())
        if ar.lowp is not None:
            assert torch.equal(ar.lowp[:ar.size], ar.master[:ar.size].bfloat16())
    if dtype == "fp32":
        assert abs(math.sqrt(moved) - clip) <= 1e-5 * clip, math.sqrt(moved)


def test_threshold_above_the_norm_changes_nothing():
    from flexflow_amd.core import AdamOptimizer

    def run(flags, clip):
        ff = _mlp(["--dtype", "bf16"] + flags, lambda ff: AdamOptimizer(ff, 1e-2, clip_norm=clip))
        possible = ff.executor._overlap_possible()
        for _ in range(3):
            ff.train_step()
        return _weights(ff), possible, ff.get_grad_norm()

    a, possible_clip, norm = run([], 1e30)
    b, possible_serial, none = run(["--no-overlap-update"], None)
    _, possible_plain, _ = run([], None)
    assert possible_plain is True and possible_serial is True  # the decision itself ignores the flag
    assert possible_clip is False
    assert none is None and 0.0 < norm < 1e30
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _run_model(model, make_opt, flags, steps):
    from flexflow_amd.core import FFConfig, FFModel
    from flexflow_amd.models import build
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = 64
    ff = FFModel(cfg)
    inputs, out, loss, mets, make_batch = build(model, ff, 64, small=True)
    ff.optimizer = make_opt(ff)
    ff.compile(loss_type=loss, metrics=mets)
    plan = ff.executor._sparse_plan(ff.optimizer)
    rng = np.random.default_rng(0)
    norms = []
    for _ in range(steps):
        arrs, lab = make_batch(rng)
        for t, a in zip(inputs, arrs):
            t.set_tensor(ff, a)
        ff.label_tensor.set_tensor(ff, lab)
        ff.train_step()
        norms.append(ff.get_grad_norm())
    torch.cuda.synchronize()
    return ff, [np.asarray(w.get_weights(ff)) for L in ff.layers for w in L.weights], norms, plan


def test_graph_captures_clipped_adam_update(monkeypatch):
    """The captured step holds the sum of squares, the coefficient and the scaled Adam: replays
    follow a norm that changes every step, clipping some steps and not others."""
    from flexflow_amd.core import AdamOptimizer
    monkeypatch.setenv("FF_GRAPH_UPDATE", "1")
    _, _, free, _ = _run_model("mlp_unify", lambda ff: AdamOptimizer(ff, 1e-3, clip_norm=1e30), ["--no-hip-graphs"], 8)
    clip = float(np.median(free))  # between the unclipped run's norms
    ffe, b, eager, _ = _run_model("mlp_unify", lambda ff: AdamOptimizer(ff, 1e-3, clip_norm=clip), ["--no-hip-graphs"], 8)
    assert any(n > clip for n in eager) and any(n + 1e-6 <= clip for n in eager), (clip, eager)
    ff, a, captured, _ = _run_model("mlp_unify", lambda ff: AdamOptimizer(ff, 1e-3, clip_norm=clip), ["--hip-graphs"], 8)
    sg = ff._step_graph
    assert sg.graph is not None and not sg.failed
    assert ff.optimizer.alpha_dev is not None and ff.optimizer.clip_coef_dev is not None
    assert ff.optimizer.beta1_t == ffe.optimizer.beta1_t and ff.executor.step_idx == ffe.executor.step_idx
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6, err_msg=str(k))
    np.testing.assert_allclose(captured[-1], eager[-1], rtol=1e-5, atol=1e-6)
    assert len(set(captured)) == len(captured)  # the replays did not repeat one step's norm


def test_dlrm_clipped_sgd_runs_dense(monkeypatch):
    """Plain SGD would update DLRM's tables row-sparsely; that kernel has no gradient scale, so
    with clip_norm the plan is empty and the tables take the dense, scaled update."""
    from flexflow_amd.core import SGDOptimizer
    clip = 0.1
    monkeypatch.delenv("FF_SPARSE_EMB", raising=False)
    _, _, _, plain_plan = _run_model("dlrm", lambda ff: SGDOptimizer(ff, 0.05), ["--no-hip-graphs"], 0)
    assert plain_plan  # without clipping the row-sparse plan is what it was
    _, a, norms, plan = _run_model("dlrm", lambda ff: SGDOptimizer(ff, 0.05, clip_norm=clip), ["--no-hip-graphs"], 4)
    assert not plan
    assert all(n > clip for n in norms), norms  # every step clips
    monkeypatch.setenv("FF_SPARSE_EMB", "0")
    _, b, _, plan0 = _run_model("dlrm", lambda ff: SGDOptimizer(ff, 0.05, clip_norm=clip), ["--no-hip-graphs"], 4)
    assert not plan0
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-5, err_msg=str(k))
