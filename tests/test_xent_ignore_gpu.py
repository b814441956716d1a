"""ignore_index of the loss kernels, element by element (GPU only), by the method of
test_small_kernels_gpu.py, whose helpers and bounds this file imports: fp64 CPU references from the
values the kernel sees, per-element comparison, bf16 bounds 2^-8 / 2^-18, for fp32 the torch-on-device
yardstick with its factor 16, GUARD-surrounded misaligned placements, outputs pre-filled with NaN.

The reference of an ignored row is exact zero, loss and gradient; of every other row the formula of
`_xent_case` there, scaled by the chosen gscale. Then two model-level tests: pad invariance of a
bert-tiny training step and the gradient scale of both reductions against torch.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loss_masking_models as M  # noqa: E402
from test_small_kernels_gpu import (BF16, DEV, DT_IDS, DTYPES, _check, _close, _f32, _gen, _guards_intact,  # noqa: E402
                                    _place, _randn, _scale_of, _yard)

pytestmark = pytest.mark.gpu

IGNS = [-100, 0]
NAN = float("nan")


def _labels(rows, cols, ign, ignored, g):
    """Labels in [1, cols) (0 stays free to be the ignored class) with `ignored` rows set to ign."""
    lab = torch.randint(1, cols, (rows,), generator=g)
    lab[ignored] = ign
    return lab


def _ignore_case(ffC, x, labels, ign, dt, what, place_logits="flat", counted=False, x_dev=None):
    """softmax_xent(ignore_index=ign) on logits x (CPU, dt) against fp64. x_dev: what the kernel gets
    instead of x (poisoned ignored rows); the reference is built from x's valid rows alone.
    counted: the valid_count pointer form (gscale argument unused: 1 / N_valid from the device count)
    against the reference scaled by the host's 1 / N_valid. Returns (dlogits, loss)."""
    rows, cols = x.shape
    keep = labels != ign
    n_valid = int(keep.sum())
    gscale = 1.0 / max(n_valid, 1) if counted else 1.0 / rows
    gs = _f32(gscale)
    xd = _place(x if x_dev is None else x_dev, place_logits)
    lab = labels.to(torch.int32).to(DEV)
    loss = torch.full((rows,), NAN, device=DEV)
    d = torch.full((rows, cols), NAN, dtype=dt, device=DEV)
    acc3 = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    if counted:
        vc = ffC.count_valid_labels(lab, ign)
        assert vc.item() == n_valid
        ffC.softmax_xent(xd, lab, loss, d, rows, cols, 12345.0, acc3, ignore_index=ign, valid_count=vc)
    else:
        ffC.softmax_xent(xd, lab, loss, d, rows, cols, gscale, acc3, ignore_index=ign)
    got_acc = acc3.cpu().double()
    # ignored rows: exactly +0
    dc, lc = d.cpu(), loss.cpu()
    assert bool((lc[~keep] == 0).all()), f"{what}: loss of an ignored row"
    zr = dc[~keep].float()
    assert bool((zr == 0).all()) and not bool(torch.signbit(zr).any()), f"{what}: gradient of an ignored row"
    # valid rows: the formula of _xent_case
    xv, lv = x[keep], labels[keep]
    x64 = xv.double()
    inr = (lv >= 0) & (lv < cols)
    safe = lv.clamp(0, cols - 1).long()
    lse = torch.logsumexp(x64, -1)
    ref_loss = torch.where(inr, lse - x64.gather(1, safe[:, None])[:, 0], torch.zeros(n_valid, dtype=torch.float64))
    onehot = F.one_hot(safe, cols).double() * inr[:, None]
    ref_d = (torch.softmax(x64, -1) - onehot) * gs
    if n_valid:
        xf = xv.to(DEV).float()
        oh_dev, lab_dev, keep_dev = onehot.float().to(DEV), safe.to(DEV), keep.to(DEV)
        _yard(loss[keep_dev], torch.where(inr.to(DEV), torch.logsumexp(xf, -1) - xf.gather(1, lab_dev[:, None])[:, 0],
                                          torch.zeros(n_valid, device=DEV)),
              ref_loss, _scale_of(xv).amax(-1), "loss " + what)
        _check(d[keep_dev], ref_d, dt, True, gs * _scale_of(xv), "dlogits " + what,
               lambda: (torch.softmax(xf, -1) - oh_dev) * gs)
    correct = float((x64.argmax(-1) == lv).sum()) if n_valid else 0.0
    assert got_acc[0] == 1.0 + correct and got_acc[2] == 3.0 + n_valid, (what, got_acc, correct, n_valid)
    _close(got_acc[1:2], 2.0 + ref_loss.sum().reshape(1), 0.0,
           2.0 ** -24 * (2.0 + n_valid * ref_loss.abs().sum()) + 16 * 2.0 ** -24 * ref_loss.abs().sum(),
           "acc3 CE " + what)
    _guards_intact()
    return dc, lc


def _tag(dt, ign):
    return f"{DT_IDS[DTYPES.index(dt)]} ign {ign}"


# ----------------------------------------------------------------------------- softmax_xent
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
@pytest.mark.parametrize("cols", [65, 1001, 4096])
def test_ignore_16byte_paths(ffC, cols, ign, dt):
    """9 rows, rows 0, 3, 4 and 8 ignored (first, last, adjacent): the vector body, the misaligned
    head of odd widths and the tail of the zero fill, next to the gradient pass of the other rows."""
    g = _gen(100 + cols)
    x = _randn((9, cols), dt, g, 3.0)
    labels = _labels(9, cols, ign, [0, 3, 4, 8], g)
    _ignore_case(ffC, x, labels, ign, dt, f"ignore 9x{cols} {_tag(dt, ign)}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
def test_ignore_scalar_branch(ffC, ign, dt):
    """logits one element into their buffer, dlogits aligned: the rows' 16-byte phases differ and the
    zero fill, like the gradient pass, takes its scalar branch."""
    g = _gen(152)
    x = _randn((9, 1001), dt, g, 3.0)
    labels = _labels(9, 1001, ign, [0, 3, 4, 8], g)
    _ignore_case(ffC, x, labels, ign, dt, f"ignore misaligned logits {_tag(dt, ign)}", place_logits="off1")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
@pytest.mark.parametrize("cols", [65, 1001])
def test_ignore_poisoned_logits(ffC, cols, ign, dt):
    """NaN and +inf in the ignored rows' logits: dlogits, loss and acc3 stay finite and equal the
    reference built from the valid rows alone, so the ignored rows were never read."""
    g = _gen(200 + cols)
    x = _randn((9, cols), dt, g, 3.0)
    labels = _labels(9, cols, ign, [0, 3, 4, 8], g)
    bad = x.clone()
    bad[0], bad[3], bad[8] = NAN, math.inf, NAN
    bad[4, ::2], bad[4, 1::2] = math.inf, NAN
    d, loss = _ignore_case(ffC, x, labels, ign, dt, f"ignore poisoned 9x{cols} {_tag(dt, ign)}", x_dev=bad)
    assert bool(torch.isfinite(d.float()).all()) and bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
def test_ignore_wrapping_row_loop(ffC, ign, dt):
    """3100 rows of 65 columns, about 40 % ignored: more rows than the 768 x 4 waves of the capped
    grid, so every wave's row loop wraps and acc3 = {correct, sum CE, N_valid} is gathered over
    several rows per wave."""
    g = _gen(300)
    rows, cols = 3100, 65
    x = _randn((rows, cols), dt, g, 3.0)
    ignored = torch.rand(rows, generator=g) < 0.4
    labels = _labels(rows, cols, ign, ignored, g)
    _ignore_case(ffC, x, labels, ign, dt, f"ignore {rows}x{cols} {_tag(dt, ign)}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
def test_ignore_extremes(ffC, ign, dt):
    """No row ignored with ignore_index set: dlogits and loss bit-equal to the call without it. Every
    row ignored: all zeros, acc3 unchanged, and no NaN from the device count 0."""
    g = _gen(400)
    rows, cols = 9, 1001
    x = _randn((rows, cols), dt, g, 3.0)
    labels = _labels(rows, cols, ign, [], g)
    d, loss = _ignore_case(ffC, x, labels, ign, dt, f"ignore none {_tag(dt, ign)}")
    xd, lab = x.to(DEV), labels.to(torch.int32).to(DEV)
    loss0 = torch.full((rows,), NAN, device=DEV)
    d0 = torch.full((rows, cols), NAN, dtype=dt, device=DEV)
    ffC.softmax_xent(xd, lab, loss0, d0, rows, cols, 1.0 / rows, None)
    assert torch.equal(d0.cpu(), d) and torch.equal(loss0.cpu(), loss)
    every = torch.full((rows,), ign, dtype=torch.int32, device=DEV)
    for counted in (False, True):
        lossz = torch.full((rows,), NAN, device=DEV)
        dz = torch.full((rows, cols), NAN, dtype=dt, device=DEV)
        acc3 = torch.tensor([1.0, 2.0, 3.0], device=DEV)
        vc = ffC.count_valid_labels(every, ign) if counted else None
        assert vc is None or vc.item() == 0.0
        ffC.softmax_xent(xd, every, lossz, dz, rows, cols, 1.0 / rows, acc3, ignore_index=ign, valid_count=vc)
        assert bool((dz.float() == 0).all()) and bool((lossz == 0).all())
        assert acc3.cpu().tolist() == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
def test_ignore_device_count(ffC, ign, dt):
    """The valid_count pointer form: the kernel forms 1 / N_valid itself; gradients against the
    reference scaled by the host's 1 / N_valid, to the same bounds."""
    g = _gen(500)
    x = _randn((9, 1001), dt, g, 3.0)
    labels = _labels(9, 1001, ign, [0, 3, 4, 8], g)
    _ignore_case(ffC, x, labels, ign, dt, f"ignore counted {_tag(dt, ign)}", counted=True)


@pytest.mark.parametrize("ign", IGNS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_count_valid_labels(ffC, n, ign):
    """Exact, and overwritten rather than accumulated (two calls on different labels)."""
    g = _gen(600 + n)
    for frac in (0.4, 0.0):
        lab = torch.randint(1, 1000, (n,), generator=g, dtype=torch.int32)
        lab[torch.rand(n, generator=g) < frac] = ign
        out = ffC.count_valid_labels(lab.to(DEV), ign)
        assert out.dtype == torch.float32 and out.shape == (1,)
        assert out.item() == float((lab != ign).sum())
    from flexflow_amd import kernels as K
    assert K.count_valid_labels(lab.to(DEV).reshape(-1, 1), ign).item() == float((lab != ign).sum())


# ------------------------------------------------------------------ xent_grad / metrics_classify
CLAMP = _f32(1e-12)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ign", IGNS)
def test_xent_grad_and_metrics_ignore(ffC, ign, dt):
    """7 x 130 probabilities, rows 2 and 6 ignored and filled with NaN: zero gradient rows and loss,
    the other rows as test_xent_grad asks, with the host scale and with the device count; the metrics'
    counts and CE over the valid rows only."""
    g = _gen(700)
    rows, cols = 7, 130
    p = torch.softmax(torch.randn(rows, cols, generator=g) * 2, -1).to(dt)
    labels = _labels(rows, cols, ign, [2, 6], g)
    keep = labels != ign
    bad = p.clone()
    bad[~keep] = NAN
    pd, lab = bad.to(DEV), labels.to(torch.int32).to(DEV)
    pv, lv = p[keep], labels[keep]
    p64, t64 = pv.double(), F.one_hot(lv, cols).double()
    ref_loss = -(t64 * torch.log(p64.clamp_min(CLAMP))).sum(-1)
    vc = ffC.count_valid_labels(lab, ign)
    for counted in (False, True):
        gscale = 1.0 / 5 if counted else 1.0 / rows
        gs = _f32(gscale)
        d = torch.full((rows, cols), NAN, dtype=dt, device=DEV)
        loss = torch.full((rows,), NAN, device=DEV)
        if counted:
            ffC.xent_grad(pd, lab, None, d, loss, rows, cols, 12345.0, True, ignore_index=ign, valid_count=vc)
        else:
            ffC.xent_grad(pd, lab, None, d, loss, rows, cols, gscale, True, ignore_index=ign)
        tag = f"xent_grad ignore {'counted ' if counted else ''}{_tag(dt, ign)}"
        zr = d.cpu()[~keep].float()
        assert bool((zr == 0).all()) and not bool(torch.signbit(zr).any()) and bool((loss.cpu()[~keep] == 0).all())
        kd = keep.to(DEV)
        _check(d[kd], (p64 - t64) * gs, dt, False, gs * _scale_of(pv), "dprobs " + tag,
               atol32=2 * 2.0 ** -23 * gs * torch.maximum(p64, t64))
        pvd = pv.to(DEV).float()
        _yard(loss[kd], -(t64.float().to(DEV) * torch.log(pvd.clamp_min(CLAMP))).sum(-1), ref_loss, 1.0, "loss " + tag)
    out = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    ffC.metrics_classify(pd, lab, rows, cols, out, ignore_index=ign)
    got = out.cpu().double()
    correct = float((p64.argmax(-1) == lv).sum())
    assert got[0] == 1.0 + correct and got[2] == 3.0 + 5, got
    ce = ref_loss.sum().item()
    assert math.isfinite(got[1]) and abs(got[1] - 2.0 - ce) <= 2.0 ** -24 * (2.0 + 5 * ce) + 16 * 2.0 ** -24 * ce, got


def test_plain_calls_unchanged(ffC):
    """Positional calls without the new arguments, and ignore_index=None, are the calls they were:
    a label equal to -100 is then an out-of-range label (loss 0, softmax gradient, row counted)."""
    g = _gen(800)
    rows, cols = 6, 130
    x = _randn((rows, cols), BF16, g, 3.0).to(DEV)
    lab = torch.tensor([3, -100, 5, 129, 0, -100], dtype=torch.int32, device=DEV)
    res = []
    for kw in ({}, {"ignore_index": None, "valid_count": None}):
        loss = torch.full((rows,), NAN, device=DEV)
        d = torch.full((rows, cols), NAN, dtype=BF16, device=DEV)
        acc3 = torch.zeros(3, device=DEV)
        ffC.softmax_xent(x, lab, loss, d, rows, cols, 1.0 / rows, acc3, **kw)
        res.append((d.cpu(), loss.cpu(), acc3.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    d, loss, acc3 = res[0]
    assert acc3[2] == rows and loss[1] == 0 and bool((d[1].float() > 0).any())
    with pytest.raises(RuntimeError):
        ffC.softmax_xent(x, lab, loss.to(DEV), d.to(DEV), rows, cols, 1.0, None, valid_count=torch.ones(1, device=DEV))


# ------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("reduction", ["batch", "valid"])
def test_bert_step_is_pad_invariant(reduction):
    """bert-tiny (BertConfig.tiny(32), batch 4, bf16, Adam, key_lengths [32, 17, 5, 1], pad labels
    -100, ignore_index=-100), two train_step()s from the same seed with pad token ids 0 and with
    seeded random ids in the pad positions: updated weights, reported loss and accuracy counts agree
    as closely as two runs with identical inputs do (measured here, expected 0). Without
    ignore_index the same edit moves them."""
    flags = ["--dtype", "bf16"]
    a = M.train_bert(flags, False, M.IGNORE, reduction)
    a2 = M.train_bert(flags, False, M.IGNORE, reduction)
    b = M.train_bert(flags, True, M.IGNORE, reduction)
    d_aa, d_ab = M.run_distance(a, a2), M.run_distance(a, b)
    print("A/A (weights, loss, counts)", d_aa, "pads edited", d_ab)
    assert np.isfinite(a[2]).all() and all(np.isfinite(w).all() for w in a[0])
    n_valid = int(M.BERT_LENS.sum())
    assert a[1][3] == n_valid and a[1][7] == (n_valid if reduction == "valid" else M.BERT_B)
    assert all(x <= y for x, y in zip(d_ab, d_aa)), (d_ab, d_aa)
    c, d = M.train_bert(flags, False, None), M.train_bert(flags, True, None)
    d_without = M.run_distance(c, d)
    print("without ignore_index", d_without)
    assert d_without[0] > max(d_aa[0], 1e-7) and d_without[1] > max(d_aa[1], 1e-7)


def test_valid_reduction_captures_into_step_graph():
    """loss_reduction="valid" under hipGraph step capture (3 eager steps, the capture, 2 replays): the
    device-side count keeps the host out of the step, so the graph exists, and losses and weights
    agree with the eager run as tests/test_runtime_gpu.py::test_graph_captures_adam_update asks of
    captured against eager steps (rtol 1e-5, atol 1e-6)."""
    wg, _, lg = M.train_bert(["--dtype", "bf16", "--hip-graphs"], False, M.IGNORE, "valid", steps=6, capture=True)
    sg = M.train_bert.last._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    we, _, le = M.train_bert(["--dtype", "bf16", "--no-hip-graphs"], False, M.IGNORE, "valid", steps=6)
    print("losses captured", lg, "eager", le)
    assert np.isfinite(lg).all()
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))


@pytest.mark.parametrize("reduction", ["batch", "valid"])
def test_gradient_scale_matches_torch(reduction):
    """dense + dense + softmax on [8, 6, 16] -> 10 classes in bf16, half the labels ignored: the weight
    gradients after one step are torch's F.cross_entropy(ignore_index=-100, reduction="mean") for
    "valid" and reduction="sum" / B for "batch" (torch in fp32 on the bf16-rounded inputs and
    weights; relative Frobenius error below 1e-2, the bf16 bound of tests/test_kernels_gpu.py)."""
    ff, w0, grads = M.mlp_step(["--dtype", "bf16"], reduction)
    ref, tloss, _, y = M.mlp_torch_grads(w0, reduction, round_bf16=True)
    for i, (a, b) in enumerate(zip(grads, ref)):
        rel = ((a - b).norm() / (b.norm() + 1e-12)).item()
        print(f"{reduction} weight {i}: rel {rel:.3e}")
        assert rel < 1e-2, (i, rel)
    pm = ff.get_perf_metrics()
    n_valid = int((y != M.IGNORE).sum())
    assert pm.train_all == n_valid
    # get_loss(): sum CE / N_valid or / B, torch's loss either way. bf16 hidden states and logits
    # (2^-8 relative each, |logit| of order 1) move a row's CE by about 2^-7: 2e-2 of a loss near 2.5
    assert abs(pm.get_loss() - tloss) <= 2e-2 * tloss
