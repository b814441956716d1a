"""ignore_index / loss_reduction of the sparse categorical cross-entropy on the CPU path: the kernel
wrappers' fallbacks against torch's F.cross_entropy, the executor's three sparse routes, compile()'s
errors, Keras' ignore_class, the metric denominators, pad invariance of bert-tiny training steps,
the example, and two gloo ranks with unevenly masked batch shards against one process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flexflow_amd import kernels as K
from flexflow_amd.core import *  # noqa: F401,F403

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loss_masking_models as M  # noqa: E402

RTOL = 1e-5


def _logits_labels(rows, cols, ign, frac, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 3
    lab = torch.randint(1, cols, (rows,), generator=g, dtype=torch.int32)  # 0 is free to be the ignored class
    lab[torch.rand(rows, generator=g) < frac] = ign
    return x, lab


def _torch_ref(x, lab, ign, scale):
    """Gradient and per-row loss from F.cross_entropy(ignore_index, reduction="sum") * scale."""
    xr = x.clone().requires_grad_()
    rows = F.cross_entropy(xr, lab.long(), ignore_index=ign, reduction="none")
    (rows.sum() * scale).backward()
    return xr.grad, rows.detach()


# ------------------------------------------------------------------------------- K.* fallbacks
@pytest.mark.parametrize("ign", [-100, 0])
@pytest.mark.parametrize("frac", [0.4, 0.0, 1.0], ids=["some", "none", "all"])
@pytest.mark.parametrize("reduction", ["batch", "valid"])
def test_softmax_xent_fallback_matches_torch(ign, frac, reduction):
    """Gradient, per-row loss and acc3 = {correct, sum CE, valid rows}; "all": every row ignored, zero
    gradients and loss 0 where torch's mean gives NaN; "none": equal to the call without ignore_index."""
    rows, cols = 37, 65
    x, lab = _logits_labels(rows, cols, ign, frac, 3)
    keep = lab != ign
    n_valid = int(keep.sum())
    vc = K.count_valid_labels(lab, ign)
    assert vc.dtype == torch.float32 and vc.shape == (1,) and vc.item() == n_valid
    acc3 = torch.tensor([1.0, 2.0, 3.0])
    if reduction == "valid":
        d, loss = K.softmax_xent(x, lab, 1.0 / rows, acc3, ignore_index=ign, valid_count=vc)
        scale = 1.0 / max(n_valid, 1)
    else:
        d, loss = K.softmax_xent(x, lab, 1.0 / rows, acc3, ignore_index=ign)
        scale = 1.0 / rows
    gref, lref = _torch_ref(x, lab, ign, scale)
    torch.testing.assert_close(d, gref, rtol=RTOL, atol=1e-7)
    torch.testing.assert_close(loss, lref, rtol=RTOL, atol=1e-6)
    assert bool((d[~keep] == 0).all()) and bool((loss[~keep] == 0).all())
    correct = int(((x.argmax(-1) == lab) & keep).sum())
    assert acc3[0].item() == 1.0 + correct and acc3[2].item() == 3.0 + n_valid
    assert abs(acc3[1].item() - 2.0 - lref.sum().item()) <= RTOL * (2.0 + lref.sum().item())
    if reduction == "valid" and n_valid:
        mean = F.cross_entropy(x, lab.long(), ignore_index=ign, reduction="mean")
        assert abs(loss.sum().item() / n_valid - mean.item()) <= RTOL * mean.item()
    if frac == 0.0 and reduction == "batch":
        d0, l0 = K.softmax_xent(x, lab, 1.0 / rows)
        assert torch.equal(d0, d) and torch.equal(l0, loss)


def test_fallbacks_never_read_ignored_rows():
    """NaN / inf in the ignored rows reach neither gradient, loss nor metrics, through all three
    fallbacks."""
    rows, cols, ign = 9, 33, -100
    x, lab = _logits_labels(rows, cols, ign, 0.0, 5)
    lab[[0, 3, 4, 8]] = ign
    keep = lab != ign
    clean = x.clone()
    x[0], x[3], x[4, ::2], x[8] = float("nan"), float("inf"), float("nan"), float("-inf")
    acc3 = torch.zeros(3)
    d, loss = K.softmax_xent(x, lab, 0.25, acc3, ignore_index=ign)
    acc_ref = torch.zeros(3)
    dref, lref = K.softmax_xent(clean[keep], lab[keep], 0.25, acc_ref)
    assert torch.isfinite(d).all() and torch.isfinite(loss).all() and torch.isfinite(acc3).all()
    assert torch.equal(d[keep], dref) and torch.equal(loss[keep], lref)
    # counts exact; the CE sums add the same terms in another order (fp32: rows * 2^-24 relative)
    assert acc3[0] == acc_ref[0] and acc3[2] == acc_ref[2] == int(keep.sum())
    assert abs(acc3[1].item() - acc_ref[1].item()) <= rows * 2.0 ** -24 * acc_ref[1].item()
    assert bool((d[~keep] == 0).all()) and bool((loss[~keep] == 0).all())
    p = torch.softmax(clean, -1)
    p[~keep] = float("nan")
    d, loss = K.xent_grad(p, lab, None, 0.25, True, ignore_index=ign)
    dref, lref = K.xent_grad(p[keep], lab[keep], None, 0.25, True)
    assert torch.equal(d[keep], dref) and torch.equal(loss[keep], lref)
    assert bool((d[~keep] == 0).all()) and bool((loss[~keep] == 0).all())
    acc3, acc_ref = torch.zeros(3), torch.zeros(3)
    K.metrics_classify(p, lab, acc3, ignore_index=ign)
    K.metrics_classify(p[keep], lab[keep], acc_ref)
    assert acc3[0] == acc_ref[0] and acc3[2] == acc_ref[2] == int(keep.sum())
    assert abs(acc3[1].item() - acc_ref[1].item()) <= rows * 2.0 ** -24 * acc_ref[1].item()


@pytest.mark.parametrize("ign", [-100, 0])
def test_xent_grad_and_metrics_fallbacks(ign):
    """7 x 130 probabilities, two rows ignored: (p - onehot) * scale with zero rows, CE and counts over
    the valid rows; the device-count form scales by 1 / N_valid."""
    rows, cols = 7, 130
    x, lab = _logits_labels(rows, cols, ign, 0.0, 9)
    lab[[2, 6]] = ign
    keep = lab != ign
    p = torch.softmax(x, -1)
    vc = K.count_valid_labels(lab, ign)
    assert vc.item() == 5
    for kw, scale in (({}, 1.0 / rows), ({"valid_count": vc}, 1.0 / 5)):
        d, loss = K.xent_grad(p, lab, None, 1.0 / rows, True, ignore_index=ign, **kw)
        gref, lref = _torch_ref(x, lab, ign, scale)
        torch.testing.assert_close(d, gref, rtol=RTOL, atol=1e-7)
        torch.testing.assert_close(loss, lref, rtol=RTOL, atol=1e-6)
        assert bool((d[~keep] == 0).all())
    acc3 = torch.zeros(3)
    K.metrics_classify(p, lab, acc3, ignore_index=ign)
    assert acc3[0].item() == int(((p.argmax(-1) == lab) & keep).sum()) and acc3[2].item() == 5
    assert abs(acc3[1].item() - lref.sum().item()) <= RTOL * lref.sum().item()
    with pytest.raises(ValueError):
        K.xent_grad(p, None, p, 1.0, False, ignore_index=ign)
    with pytest.raises(ValueError):
        K.softmax_xent(x, lab, 1.0, valid_count=vc)


# ----------------------------------------------------------------------------- executor routes
@pytest.mark.parametrize("reduction", ["batch", "valid"])
@pytest.mark.parametrize("route", ["fused", "probabilities", "no_softmax"])
def test_executor_routes(route, reduction):
    """The loss gradient the executor seeds, and its metrics, on the three sparse routes: fused
    logits (training forward of a model ending in Softmax), probabilities (an evaluation forward:
    the Softmax emits probabilities) and a model without a final Softmax."""
    ff, w0, grads = M.mlp_step([], reduction, softmax=route != "no_softmax")
    ex = ff.executor
    tg, tloss, logits, y = M.mlp_torch_grads(w0, reduction)
    keep = y != M.IGNORE
    n_valid, B = int(keep.sum()), M.MLP_SHAPE[0]
    scale = 1.0 / n_valid if reduction == "valid" else 1.0 / B
    if route == "probabilities":
        ff.reset_metrics()
        ex.forward(training=False)
        assert ex.softmax_fused and not ex._softmax_emitted_logits()
        g = ex.compute_loss_grad().reshape(-1, M.MLP_CLASSES)
        gref, _ = _torch_ref(logits, y.int(), M.IGNORE, scale)
        torch.testing.assert_close(g, gref, rtol=RTOL, atol=1e-7)
        assert bool((g[~keep] == 0).all())
    else:
        assert ex.softmax_fused == (route == "fused")
        for a, b in zip(grads, tg):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    acc = ex.metrics_snapshot()
    ce = F.cross_entropy(logits, y, ignore_index=M.IGNORE, reduction="sum").item()
    correct = int(((logits.argmax(-1) == y) & keep).sum())
    assert acc[1] == correct and acc[3] == n_valid
    assert abs(acc[0] - ce) <= 1e-5 * ce and abs(acc[2] - ce) <= 1e-5 * ce
    assert acc[7] == (n_valid if reduction == "valid" else B)
    pm = ff.get_perf_metrics()
    assert pm.train_all == n_valid and pm.train_correct == correct
    assert abs(pm.get_accuracy() - 100.0 * correct / n_valid) < 1e-9
    want = ce / n_valid if reduction == "valid" else ce / B
    assert abs(pm.get_loss() - want) <= 1e-5 * want
    if reduction == "valid":  # torch's mean
        assert abs(pm.get_loss() - tloss) <= 1e-5 * tloss


def test_no_valid_row_gives_zero_gradients():
    """Every label ignored under "valid": zero weight gradients and loss 0 (torch: NaN)."""
    ff, _, _ = M.mlp_step([], "valid")
    _, lab = M.mlp_data()
    ff.label_tensor.set_tensor(ff, np.full_like(lab, M.IGNORE))
    ff.reset_metrics()
    ff.forward()
    ff.zero_gradients()
    ff.backward()
    for L in ff.layers:
        for w in L.weights:
            g = ff.executor.get_weight_grad(w)
            assert bool((g == 0).all())
    pm = ff.get_perf_metrics()
    assert pm.get_loss() == 0.0 and pm.get_accuracy() == 0.0


# --------------------------------------------------------------------------- compile / Keras
def _tiny_model():
    ff = FFModel(FFConfig(["--no-hip-graphs"]))
    ff.config.batch_size = 4
    x = ff.create_tensor([4, 8], DataType.DT_FLOAT)
    ff.softmax(ff.dense(x, 5))
    ff.optimizer = SGDOptimizer(ff, 0.01)
    return ff


def test_compile_errors():
    sparse = LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY
    with pytest.raises(ValueError, match="ignore_index"):
        _tiny_model().compile(loss_type=LossType.LOSS_CATEGORICAL_CROSSENTROPY, ignore_index=-100)
    with pytest.raises(ValueError, match="ignore_index"):
        _tiny_model().compile(loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, ignore_index=0)
    with pytest.raises(ValueError, match="valid"):
        _tiny_model().compile(loss_type=sparse, loss_reduction="valid")
    with pytest.raises(ValueError, match="loss_reduction"):
        _tiny_model().compile(loss_type=sparse, ignore_index=-100, loss_reduction="mean")
    ff = _tiny_model()
    ff.compile(loss_type=sparse, ignore_index=-100, loss_reduction="valid")
    assert (ff.ignore_index, ff.loss_reduction) == (-100, "valid")
    assert (ff.executor.ignore_index, ff.executor.loss_reduction) == (-100, "valid")
    ff = _tiny_model()
    ff.compile(loss_type=sparse)  # the defaults: as before
    assert (ff.ignore_index, ff.loss_reduction) == (None, "batch")
    assert ff.executor.ignore_index is None


def test_keras_ignore_class():
    from flexflow_amd.keras import losses as klosses
    from flexflow_amd.keras.layers import Dense, Input
    from flexflow_amd.keras.models import Model
    assert klosses.get("sparse_categorical_crossentropy").ignore_class is None
    for loss, want in ((klosses.SparseCategoricalCrossentropy(ignore_class=0), 0),
                       (klosses.SparseCategoricalCrossentropy(), None), ("sparse_categorical_crossentropy", None)):
        inp = Input(shape=(8,))
        out = Dense(5, activation="softmax")(inp)
        m = Model(inp, out)
        m.compile(optimizer="sgd", loss=loss, metrics=["accuracy"], batch_size=4,
                  ffconfig=FFConfig(["--no-hip-graphs"]))
        assert m._ffmodel.ignore_index == want and m._ffmodel.executor.ignore_index == want
        assert m._ffmodel.loss_reduction == "batch"


# ------------------------------------------------------------------------------ pad invariance
@pytest.mark.parametrize("reduction", ["batch", "valid"])
def test_bert_training_is_pad_invariant(reduction):
    """bert-tiny, fp32, two train steps: with the pad labels ignored, what the pad positions hold
    (token 0 or random ids) changes neither the updated weights, the loss nor the accuracy counts,
    any more than a repeat of the identical run does; without ignore_index the same edit does."""
    flags = ["--no-hip-graphs"]
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


def test_varlen_example_ignores_pad_labels():
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", FF_TUNABLEOP="off")
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "python", "native", "bert_varlen.py"), "-b", "4",
                        "--seq-length", "16", "--iterations", "3", "--ignore-pad-labels"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bert-tiny varlen: 3 iterations" in r.stdout and "nan" not in r.stdout.lower(), r.stdout[-500:]
    rng = np.random.default_rng(0)  # the example's corpus
    real = int(rng.integers(8, 17, 12).sum())
    assert f"mean over {real} real tokens" in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------ strategy independence
def test_valid_reduction_two_ranks_match_single():
    """Batch-sharded over 2 gloo ranks with 11 and 2 valid labels in the shards' 24 rows each: the
    weights after two SGD steps under "valid" are the single-process ones, which needs the count of
    the global batch (per-rank counts would scale the shards by 1/11 and 1/2 instead of 1/13)."""
    from test_multirank_cpu import _compare
    ref = M.single("valid")
    par, strat = M.run("valid", 2)
    assert strat["sm"]["degrees"][0] == 2, strat["sm"]
    _compare(par, ref, "loss_reduction valid, batch@2")
    assert ref["__metrics__"][3] == 2 * 13 and ref["__metrics__"][7] == 2 * 13  # two steps accumulated
