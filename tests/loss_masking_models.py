"""Helpers of test_loss_masking_cpu.py and test_xent_ignore_gpu.py: the bert-tiny run behind the
pad-invariance tests, the dense + softmax model of the scale tests, and a two-rank gloo run through
the harness of test_multirank_cpu.py (its _worker / _single / _compare, as attn_lens_dist.py uses
them) with this module's model, strategy and compile() arguments in place of that file's."""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

IGNORE = -100

# ---------------------------------------------------------------------------- bert-tiny, padded
BERT_B, BERT_S = 4, 32
BERT_LENS = np.array([32, 17, 5, 1], dtype=np.int32)


def bert_batch(random_pads):
    """Token ids, labels (IGNORE at the pad positions) and the pad mask of one right-padded batch;
    the pad positions hold token 0 or, with random_pads, seeded random ids. The valid positions are
    the same either way."""
    rng = np.random.default_rng(11)
    tok = rng.integers(1, 1000, (BERT_B, BERT_S)).astype(np.int32)
    lab = rng.integers(0, 1000, (BERT_B, BERT_S, 1)).astype(np.int32)
    pad = np.arange(BERT_S)[None, :] >= BERT_LENS[:, None]
    tok[pad] = rng.integers(1, 1000, int(pad.sum())).astype(np.int32) if random_pads else 0
    lab[pad] = IGNORE
    return tok, lab, pad


def train_bert(flags, random_pads, ignore_index, loss_reduction="batch", steps=2, capture=False):
    """`steps` train_step()s of bert-tiny (BertConfig.tiny(32), batch 4, Adam, key_lengths
    [32, 17, 5, 1]) on the batch above, from seed 0. capture: capture the step into a graph however
    short it is (with --hip-graphs; after the three eager warm-up steps). Returns (weights, the
    metric accumulator after the last step, the loss of every step); train_bert.last is the model."""
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(0)
    bc = BertConfig.tiny(BERT_S)
    cfg = FFConfig(list(flags))
    cfg.batch_size = BERT_B
    if capture:
        cfg.graph_min_step_ms = 1e9
    ff = FFModel(cfg)
    train_bert.last = ff
    kl = ff.create_tensor([BERT_B], DataType.DT_INT32, name="key_lengths")
    ids, pos, _ = build_bert(ff, BERT_B, bc, key_lengths=kl)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    kw = {} if ignore_index is None else dict(ignore_index=ignore_index, loss_reduction=loss_reduction)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY], **kw)
    tok, lab, _ = bert_batch(random_pads)
    ids.set_tensor(ff, tok)
    pos.set_tensor(ff, np.tile(np.arange(BERT_S, dtype=np.int32), (BERT_B, 1)))
    kl.set_tensor(ff, BERT_LENS)
    ff.label_tensor.set_tensor(ff, lab)
    losses = []
    acc = None
    for _ in range(steps):
        ff.reset_metrics()
        ff.train_step()
        acc = ff.executor.metrics_snapshot().astype(np.float64)
        losses.append(ff.get_perf_metrics().get_loss())
    weights = [np.asarray(w.get_weights(ff), dtype=np.float64) for L in ff.layers for w in L.weights]
    return weights, acc, np.asarray(losses, dtype=np.float64)


def run_distance(a, b):
    """Largest absolute difference of two train_bert results: (weights, loss, the accuracy counts
    {correct, rows})."""
    wa, acca, la = a
    wb, accb, lb = b
    dw = max(float(np.abs(x - y).max()) for x, y in zip(wa, wb))
    return dw, float(np.abs(la - lb).max()), float(np.abs(acca[[1, 3]] - accb[[1, 3]]).max())


# ------------------------------------------------------------------------------ dense + softmax
MLP_SHAPE, MLP_CLASSES = (8, 6, 16), 10


def mlp_data():
    """Input and labels (a random half of them IGNORE) of the scale tests' model."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal(MLP_SHAPE).astype(np.float32)
    lab = rng.integers(0, MLP_CLASSES, MLP_SHAPE[:2] + (1,)).astype(np.int32)
    flat = lab.reshape(-1)
    flat[rng.permutation(flat.size)[:flat.size // 2]] = IGNORE
    return x, lab


def mlp_step(flags, loss_reduction, softmax=True):
    """One forward / backward of dense(16 -> 12, relu) -> dense(12 -> 10) [-> softmax] with
    ignore_index on the data above. Returns (ff, initial weights [W1, b1, W2, b2] as the layers hold
    them, their gradients)."""
    from flexflow_amd.core import ActiMode, DataType, FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    torch.manual_seed(0)
    cfg = FFConfig(["--no-hip-graphs"] + list(flags))
    cfg.batch_size = MLP_SHAPE[0]
    ff = FFModel(cfg)
    x = ff.create_tensor(list(MLP_SHAPE), DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 12, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, MLP_CLASSES, name="d2")
    if softmax:
        ff.softmax(t, name="sm")
    ff.optimizer = SGDOptimizer(ff, 0.0)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
               metrics=[MetricsType.METRICS_ACCURACY, MetricsType.METRICS_SPARSE_CATEGORICAL_CROSSENTROPY],
               ignore_index=IGNORE, loss_reduction=loss_reduction)
    xv, lab = mlp_data()
    x.set_tensor(ff, xv)
    ff.label_tensor.set_tensor(ff, lab)
    ws = [w for L in ff.layers for w in L.weights]
    w0 = [torch.from_numpy(np.asarray(w.get_weights(ff), dtype=np.float32)) for w in ws]
    ff.reset_metrics()
    ff.forward()
    ff.zero_gradients()
    ff.backward()
    grads = [torch.as_tensor(np.asarray(ff.executor.get_weight_grad(w).float().cpu())) for w in ws]
    return ff, w0, grads


def mlp_torch_grads(w0, loss_reduction, round_bf16=False):
    """torch's gradients of the same model and data: F.cross_entropy(ignore_index, reduction="mean")
    for "valid", reduction="sum" / B for "batch". round_bf16: inputs and weights rounded to bf16
    first, as the bf16 model sees them."""
    import torch.nn.functional as F
    xv, lab = mlp_data()
    x = torch.from_numpy(xv)
    ws = [w.clone() for w in w0]
    if round_bf16:
        x = x.bfloat16().float()
        ws = [w.bfloat16().float() for w in ws]
    ws = [w.requires_grad_() for w in ws]
    W1, b1, W2, b2 = ws
    # a dense layer's kernel is [out, in] or [in, out]: whichever multiplies
    def lin(h, W, b):
        return h @ (W.t() if W.shape[1] == h.shape[-1] and W.shape[0] == b.numel() else W) + b
    logits = lin(torch.relu(lin(x, W1, b1)), W2, b2).reshape(-1, MLP_CLASSES)
    y = torch.from_numpy(lab.reshape(-1)).long()
    if loss_reduction == "valid":
        loss = F.cross_entropy(logits, y, ignore_index=IGNORE, reduction="mean")
    else:
        loss = F.cross_entropy(logits, y, ignore_index=IGNORE, reduction="sum") / MLP_SHAPE[0]
    return [g.detach() for g in torch.autograd.grad(loss, ws)], loss.item(), logits.detach(), y


# ----------------------------------------------------------------------- two gloo ranks, "valid"
DIST_B, DIST_S = 8, 6  # 48 label rows, 24 per batch shard


def _dist_labels(rng):
    """11 valid labels among the 24 of the batch's first half, 2 among those of the second: a count
    taken per rank would scale the shards' gradients by 1/11 and 1/2 where the global batch asks
    for 1/13."""
    lab = rng.integers(0, 10, (DIST_B * DIST_S,)).astype(np.int32)
    keep = np.zeros(DIST_B * DIST_S, dtype=bool)
    keep[:11] = True
    keep[24:26] = True
    lab[~keep] = IGNORE
    return lab.reshape(DIST_B, DIST_S, 1)


def _build(case, ff):
    from flexflow_amd.core import ActiMode, DataType, LossType
    rng = np.random.default_rng(7)
    x = ff.create_tensor([DIST_B, DIST_S, 16], DataType.DT_FLOAT, name="x")
    t = ff.dense(x, 12, ActiMode.AC_MODE_RELU, name="d1")
    t = ff.dense(t, 10, name="head")
    ff.softmax(t, name="sm")
    feeds = [rng.standard_normal((DIST_B, DIST_S, 16)).astype(np.float32)]
    return [x], feeds, _dist_labels(rng), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY


def _strategy(case, ff, world):
    from flexflow_amd.pcg.strategy import OpConfig
    L = {l.name: l for l in ff.layers}

    def cfg(name):
        n = len(L[name].impl.axis_sizes())
        return OpConfig(tuple([world] + [1] * (n - 1)), tuple(range(world)))

    return {n: cfg(n) for n in ("x", "d1", "head", "sm")}


def _train(case, flags, world, out_file=None):
    """test_multirank_cpu._train with compile(ignore_index, loss_reduction): `case` names the
    reduction."""
    from flexflow_amd.core import FFConfig, FFModel, MetricsType, SGDOptimizer
    cfg = FFConfig(["--no-hip-graphs"] + list(flags))
    cfg.batch_size = DIST_B
    ff = FFModel(cfg)
    inputs, feeds, lab, loss = _build(case, ff)
    ff.optimizer = SGDOptimizer(ff, 0.05)
    ff.compile(loss_type=loss, metrics=[MetricsType.METRICS_ACCURACY], ignore_index=IGNORE, loss_reduction=case)
    for t, v in zip(inputs, feeds):
        t.set_tensor(ff, v)
    ff.label_tensor.set_tensor(ff, lab)
    for _ in range(2):
        ff.forward()
        ff.zero_gradients()
        ff.backward()
        ff.update()
    res = {f"{li}:{l.op_type.name}.{i}": np.asarray(w.get_weights(ff))
           for li, l in enumerate(ff.layers) for i, w in enumerate(l.weights)}
    res["__output__"] = np.asarray(ff._get_tensor_value(ff.output_tensor()), dtype=np.float32)
    res["__metrics__"] = ff.executor.metrics_snapshot().astype(np.float32)
    return ff, res


@contextlib.contextmanager
def _harness():
    import test_multirank_cpu as T
    old = T._build, T._strategy, T._train, T.B
    T._build, T._strategy, T._train, T.B = _build, _strategy, _train, DIST_B
    try:
        yield T
    finally:
        T._build, T._strategy, T._train, T.B = old


def worker(rank, world, port, case, flags, out_dir):
    with _harness() as T:
        T._worker(rank, world, port, case, flags, out_dir)


def run(case, world):
    """(rank 0's weights, output and metrics after the harness's two SGD steps on `world` gloo
    ranks, the strategy that ran)."""
    import torch.multiprocessing as mp

    import test_multirank_cpu as T
    from flexflow_amd.core import FFConfig, FFModel
    from flexflow_amd.pcg.strategy import save_strategy
    tmp = tempfile.mkdtemp()
    ff = FFModel(FFConfig([]))
    ff.config.batch_size = DIST_B
    _build(case, ff)
    sf = os.path.join(tmp, "s.json")
    save_strategy(sf, _strategy(case, ff, world), world)
    mp.start_processes(worker, args=(world, T._free_port(), case, ["--import-strategy", sf], tmp), nprocs=world,
                       join=True, start_method="spawn")
    with open(os.path.join(tmp, "search.json")) as f:
        search = json.load(f)
    return dict(np.load(os.path.join(tmp, "out.npz"))), search["strategy"]


def single(case):
    with _harness() as T:
        return T._single(case)
