"""Attention dropout without a GPU: the Python mirror of the keep-mask (kernels.attn_dropout_keep_ref,
the oracle of every other test), the attention op on the CPU path, bert-tiny training with
checkpoint / resume, and the torch front end.

The statistical checks are conditions on a deterministic function of a fixed seed, not flaky draws:
each compares a kept (or agreeing) fraction over N elements with its expectation, within 4 standard
deviations sqrt(f (1 - f) / N) of a Bernoulli fraction f."""
import math
import zlib

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K
from flexflow_amd.core import *  # noqa: F401,F403
from flexflow_amd.ops import OpCtx

SEED, LAYER, P = 1234, 77, 0.1
P_EFF = 26 / 256  # round(256 * 0.1) / 256


def _sigma(f, n):
    return math.sqrt(f * (1 - f) / n)


def test_threshold_and_effective_rate():
    assert K.attn_dropout_thr(0.1) == 26 and K.attn_dropout_thr(0.0) == 0 and K.attn_dropout_thr(0.001) == 0
    assert K.attn_dropout_thr(0.5) == 128 and K.attn_dropout_thr(0.999) == 255
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            K.attn_dropout_thr(bad)


def test_mirror_statistics():
    B = H = 2
    S = 128
    m = K.attn_dropout_keep_ref(SEED, LAYER, 1, B, H, S, S, P)
    assert m.dtype == torch.bool and tuple(m.shape) == (B, H, S, S)
    f = m.double()
    N = f.numel()
    assert N == 65536
    assert abs(f.mean().item() - (1 - P_EFF)) < 4 * _sigma(P_EFF, N)
    rows = f.mean(-1)  # every query row: N = S
    assert (rows - (1 - P_EFF)).abs().max().item() < 4 * _sigma(P_EFF, S)
    cols = f.mean((0, 1, 2))  # every key column: N = B * H * S
    assert (cols - (1 - P_EFF)).abs().max().item() < 4 * _sigma(P_EFF, B * H * S)
    # independent masks agree where both keep or both drop
    agree = (1 - P_EFF) ** 2 + P_EFF ** 2
    other_step = K.attn_dropout_keep_ref(SEED, LAYER, 2, B, H, S, S, P)
    other_layer = K.attn_dropout_keep_ref(SEED, LAYER + 1, 1, B, H, S, S, P)
    assert abs((m == other_step).double().mean().item() - agree) < 4 * _sigma(agree, N)
    assert abs((m == other_layer).double().mean().item() - agree) < 4 * _sigma(agree, N)
    heads = (m[:, 0] == m[:, 1]).double()
    assert abs(heads.mean().item() - agree) < 4 * _sigma(agree, heads.numel())
    # a pure function of its arguments
    assert torch.equal(m, K.attn_dropout_keep_ref(SEED, LAYER, torch.tensor([1]), B, H, S, S, P))


def test_mirror_shard_invariance():
    """(b0, h0) offsets give the matching slice of the full mask, whatever the shard's own shape;
    so does a shorter Sq / Sk (nothing of the extent enters), odd sizes included."""
    B, H, Sq, Sk = 4, 6, 37, 50
    full = K.attn_dropout_keep_ref(SEED, LAYER, 5, B, H, Sq, Sk, P)
    for b0, nb, h0, nh in ((0, 4, 0, 6), (2, 2, 0, 6), (0, 4, 3, 3), (1, 2, 4, 2), (3, 1, 5, 1)):
        part = K.attn_dropout_keep_ref(SEED, LAYER, 5, nb, nh, Sq, Sk, P, b0=b0, h0=h0, H_total=H)
        assert torch.equal(part, full[b0:b0 + nb, h0:h0 + nh]), (b0, h0)
    small = K.attn_dropout_keep_ref(SEED, LAYER, 5, B, H, 20, 33, P)
    assert torch.equal(small, full[:, :, :20, :33])


# ------------------------------------------------------------------------------------ op level
def _run(build, inputs, training=True, seed=0, step=None):
    """tests/test_ops_cpu.py::run_layer for one attention layer, with the op context's training flag
    and step counter exposed. Returns (layer, ctx, weights, y, dy, dxs)."""
    torch.manual_seed(seed)
    ff = FFModel(FFConfig([]))
    ts = [ff.create_tensor(list(x.shape), DataType.DT_FLOAT) for x in inputs]
    L = build(ff, ts).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n, training=training, seed=SEED)
    if step is not None:
        ctx.rng_step = torch.tensor([step], dtype=torch.int64)
    ws = [torch.randn(w.dims) * 0.3 for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims) for w in L.weights]
    slot = [next(i for i, t in enumerate(ts) if t is u) for u in L.inputs]
    clones = [x.clone() for x in inputs]
    xs = [clones[i] for i in slot]  # self-attention: one tensor in all three slots
    y = L.impl.forward(ctx, xs, ws)[0]
    dy = torch.randn(y.shape)
    dxs = None
    if training:
        dslot = L.impl.backward(ctx, [dy])
        dxs = [None] * len(inputs)
        for i, d in zip(slot, dslot):
            if d is not None:
                dxs[i] = d if dxs[i] is None else dxs[i] + d
    return L, ctx, ws, y, dy, dxs


def _torch_mha(xq, xk, xv, proj, wo, bo, H, D, keep, scale_keep, causal):
    """Plain torch attention with a given keep-mask; proj: [(w, b)] * 3 for q, k, v."""
    B, Sq, Sk = xq.shape[0], xq.shape[1], xk.shape[1]
    qq, kk, vv = ((x @ w.reshape(H * D, -1).t() + b.reshape(-1)).view(B, -1, H, D).transpose(1, 2)
                  for x, (w, b) in zip((xq, xk, xv), proj))
    s = qq @ kk.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(keep, p * scale_keep, torch.zeros_like(p))
    return (p @ vv).transpose(1, 2).reshape(B, Sq, H * D) @ wo.reshape(wo.shape[0], -1).t() + bo


def _close(a, b, tol=2e-4):  # test_ops_cpu.py's attention tolerance
    assert torch.allclose(a, b, atol=tol, rtol=tol), (a - b).abs().max().item()


@pytest.mark.parametrize("kind", ["self", "self_causal", "cross"])
def test_op_matches_torch_with_the_mirrors_mask(kind):
    step = 3
    scale_keep = 1.0 / (1.0 - P_EFF)
    if kind == "cross":
        B, Sq, Sk, E, H, D = 2, 5, 7, 16, 2, 8
        ins = [torch.randn(B, Sq, E), torch.randn(B, Sk, 12), torch.randn(B, Sk, 12)]
        build = lambda ff, t: ff.multihead_attention(t[0], t[1], t[2], E, H, D, D, dropout=P, name="xattn")  # noqa: E731
        name = "xattn"
    else:
        B, Sq, Sk, E, H, D = 2, 6, 6, 16, 4, 4
        ins = [torch.randn(B, Sq, E)]
        build = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, dropout=P,  # noqa: E731
                                                     causal=kind == "self_causal", name="sattn")
        name = "sattn"
    L, ctx, ws, y, dy, dxs = _run(build, ins, step=step)
    assert L.attrs["dropout"] == P
    keep = K.attn_dropout_keep_ref(SEED, zlib.crc32(name.encode()), step, B, H, Sq, Sk, P)
    assert not keep.all() and keep.any()
    xi = [x.clone().requires_grad_() for x in ins]
    wi = [w.clone().requires_grad_() for w in ws]
    if kind == "cross":
        proj = [(wi[0], wi[3]), (wi[1], wi[4]), (wi[2], wi[5])]
        yr = _torch_mha(xi[0], xi[1], xi[2], proj, wi[6], wi[7], H, D, keep, scale_keep, False)
    else:
        proj = [(wi[0][i], wi[1][i]) for i in range(3)]
        yr = _torch_mha(xi[0], xi[0], xi[0], proj, wi[2], wi[3], H, D, keep, scale_keep, kind == "self_causal")
    (yr * dy).sum().backward()
    _close(y, yr.detach())
    for d, x in zip(dxs, xi):
        _close(d, x.grad)
    for g, w in zip(ctx.wgrads, wi):
        _close(g, w.grad)
    y0 = _run(build, ins, step=step + 1)[3]
    assert (y0 - y).abs().max().item() > 1e-3  # another step: another mask


def test_op_differs_from_no_dropout_and_eval_is_exact():
    B, S, E, H = 2, 6, 16, 4
    x = torch.randn(B, S, E)
    drop = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, dropout=P, name="a")  # noqa: E731
    plain = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, name="a")  # noqa: E731
    y_drop = _run(drop, [x])[3]
    y_plain = _run(plain, [x])[3]
    assert (y_drop - y_plain).abs().max().item() > 1e-3
    # evaluation forwards apply nothing
    assert torch.equal(_run(drop, [x], training=False)[3], _run(plain, [x], training=False)[3])
    assert torch.equal(_run(drop, [x], training=False)[3], y_plain)
    # a rate below half a threshold step is no dropout at all
    tiny = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, dropout=0.001, name="a")  # noqa: E731
    assert torch.equal(_run(tiny, [x])[3], y_plain)


@pytest.mark.parametrize("bad", [1.0, 1.5, -0.25])
def test_rate_out_of_range_raises_at_construction(bad):
    ff = FFModel(FFConfig([]))
    t = ff.create_tensor([2, 4, 16], DataType.DT_FLOAT)
    with pytest.raises(ValueError):
        ff.multihead_attention(t, t, t, 16, 4, dropout=bad)


# ------------------------------------------------------------------------------------ training
def _bert(attn_dropout, seed=0, lr=1e-3):
    from flexflow_amd.models.bert import BertConfig, build_bert
    torch.manual_seed(seed)
    B, bc = 2, BertConfig.tiny(16)
    bc.attn_dropout = attn_dropout
    cfg = FFConfig(["--dtype", "fp32"])
    cfg.cpu_only = True  # the CPU path, whatever the machine
    cfg.batch_size = B
    ff = FFModel(cfg)
    ids, pos, _ = build_bert(ff, B, bc)
    ff.optimizer = AdamOptimizer(ff, lr)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    ids.set_tensor(ff, rng.integers(0, bc.vocab, (B, bc.seq), dtype=np.int32))
    pos.set_tensor(ff, np.tile(np.arange(bc.seq, dtype=np.int32), (B, 1)))
    ff.label_tensor.set_tensor(ff, rng.integers(0, bc.vocab, (B, bc.seq, 1), dtype=np.int32))
    return ff


def _steps(ff, n):
    out = []
    for _ in range(n):
        ff.reset_metrics()
        ff.train_step()
        out.append(ff.get_perf_metrics().get_loss())
    return out


def test_bert_training_is_reproducible_and_resumes(tmp_path):
    from flexflow_amd.runtime.checkpoint import load_checkpoint, save_checkpoint
    ff = _bert(P)
    assert ff.executor.rng_step is not None and int(ff.executor.rng_step.item()) == 0
    four = _steps(ff, 4)
    assert int(ff.executor.rng_step.item()) == 4  # advanced once per training forward
    assert np.isfinite(four).all()
    assert four == _steps(_bert(P), 4)  # identical losses: no hidden state, no wall-clock seed
    plain = _bert(0.0)
    assert plain.executor.rng_step is None  # no counter, no extra launch without dropout
    assert _steps(plain, 4) != four
    # 2 steps + checkpoint + resume + 2 steps
    a = _bert(P)
    first = _steps(a, 2)
    save_checkpoint(a, str(tmp_path / "ck"))
    b = _bert(P, seed=1)
    assert load_checkpoint(b, str(tmp_path / "ck")) == 2
    assert int(b.executor.rng_step.item()) == 2
    np.testing.assert_allclose(first + _steps(b, 2), four, rtol=1e-6, atol=1e-7)


def test_consecutive_steps_use_different_masks():
    """The same weights and batch (learning rate 0): the loss of step n + 1 differs from step n's only
    through the mask; an evaluation forward neither drops nor advances the counter."""
    ff = _bert(P, lr=0.0)
    l = _steps(ff, 3)
    assert len({round(v, 9) for v in l}) == 3, l
    before = int(ff.executor.rng_step.item())
    ff.executor.forward(training=False)
    assert int(ff.executor.rng_step.item()) == before


# ------------------------------------------------------------------------------------ front end
def test_torch_frontend_passes_the_rate(tmp_path):
    import torch.nn as nn
    from flexflow_amd.torch.model import PyTorchModel

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.att = nn.MultiheadAttention(16, 4, dropout=0.2, batch_first=True)

        def forward(self, x):
            return self.att(x, x, x)[0]

    pm = PyTorchModel(M())
    ff = FFModel(FFConfig([]))
    t = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    pm.torch_to_ff(ff, [t])
    att = [L for L in ff.layers if L.op_type == OperatorType.OP_MULTIHEAD_ATTENTION]
    assert len(att) == 1 and att[0].attrs["dropout"] == 0.2
    # a .ff file written before the field existed reads as rate 0
    fn = str(tmp_path / "m.ff")
    pm.torch_to_file(fn)
    lines = open(fn).read().splitlines()
    is_att = lambda ln: "MULTIHEAD_ATTENTION" in ln and ln.rstrip().endswith("0.2")  # noqa: E731
    assert sum(map(is_att, lines)) == 1, lines
    old = [ln[:ln.rindex(";")].rstrip() if is_att(ln) else ln for ln in lines]
    ff2 = FFModel(FFConfig([]))
    t2 = ff2.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    PyTorchModel.string_to_ff(old, ff2, [t2])
    att2 = [L for L in ff2.layers if L.op_type == OperatorType.OP_MULTIHEAD_ATTENTION]
    assert len(att2) == 1 and att2[0].attrs["dropout"] == 0.0
    ff3 = FFModel(FFConfig([]))
    PyTorchModel.file_to_ff(fn, ff3, [ff3.create_tensor([2, 6, 16], DataType.DT_FLOAT)])
    assert [L.attrs["dropout"] for L in ff3.layers if L.op_type == OperatorType.OP_MULTIHEAD_ATTENTION] == [0.2]
