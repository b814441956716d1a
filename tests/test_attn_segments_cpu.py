"""Packed sequences through per-token segment ids, on the CPU path: the reference attention with
`segments=` against torch attention run on every sequence alone, the bounds oracles, the builder's
checks, the packer, a packed bert-tiny step against the same sentences right-padded, two gloo ranks
against one process, and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K
from flexflow_amd.core import *  # noqa: F401,F403
from flexflow_amd.ops.attention import _attn_ref
from flexflow_amd.utils.packing import fill_ratio, pack_sequences, packed_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from attn_segments_common import bounds_loop, ids_of, live_of, mask_of, runs_of  # noqa: E402


def p(n):
    return ("p", n)


# a cut row; a leading pad run; a hole between segments and a trailing pad; a reused id around a pad and
# next to another segment (ids_of alternates 0 / 1); single tokens; a row that is all padding
ROWS = [[7, 5, 4], [p(3), 9, 4], [6, p(4), 5, p(1)], [4, 4, p(2), 3, 3], [1, 1, 13, 1], [p(16)]]
S = 16


# ------------------------------------------------------------------------------ reference path
@pytest.mark.parametrize("causal", [False, True])
def test_attn_ref_segments_match_per_sequence_attention(causal):
    """_attn_ref(segments=...) in fp32 against torch's softmax attention run on each sequence alone
    (allclose at 1e-5), outputs and the gradients of q, k, v; padding rows are zeros, not NaN, in both."""
    B, H, D = len(ROWS), 2, 8
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g) for _ in range(4))
    ids = torch.tensor(np.stack([ids_of(r, S) for r in ROWS]))
    scale = 1.0 / np.sqrt(D)
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    out = _attn_ref(qa, ka, va, scale, causal, segments=ids)
    out.backward(do)
    qb, kb, vb = (t.clone().requires_grad_() for t in (q, k, v))
    want = torch.zeros(B, H, S, D)
    pieces = []
    for b, row in enumerate(ROWS):
        for lo, hi, pad in runs_of(row, S):
            if pad:
                continue
            s = torch.einsum("hqd,hkd->hqk", qb[b, :, lo:hi], kb[b, :, lo:hi]) * scale
            if causal:
                s = s.masked_fill(torch.ones(hi - lo, hi - lo, dtype=torch.bool).triu(1), float("-inf"))
            o = torch.einsum("hqk,hkd->hqd", torch.softmax(s, -1), vb[b, :, lo:hi])
            pieces.append((o * do[b, :, lo:hi]).sum())
            want[b, :, lo:hi] = o.detach()
    torch.stack(pieces).sum().backward()
    assert torch.isfinite(out).all()
    assert torch.allclose(out, want, rtol=1e-5, atol=1e-5)
    live = torch.tensor(np.stack([live_of(r, S) for r in ROWS]))
    assert (out[~live[:, None, :].expand(-1, H, -1)] == 0).all()
    for got, ref in ((qa.grad, qb.grad), (ka.grad, kb.grad), (va.grad, vb.grad)):
        assert torch.isfinite(got).all()
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)
        assert (got[~live[:, None, :].expand(-1, H, -1)] == 0).all()


def test_attn_ref_rejects_segments_with_lengths_or_bias():
    q = torch.randn(1, 1, 4, 4)
    ids = torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        _attn_ref(q, q, q, 1.0, False, key_lens=torch.tensor([4]), segments=ids)
    with pytest.raises(ValueError):
        _attn_ref(q, q, q, 1.0, False, bias=torch.zeros(1, 1, 4, 4), segments=ids)


# ------------------------------------------------------------------------------------- bounds
def test_bounds_oracles_agree():
    """bounds_loop (the GPU test's oracle: a plain loop over the ids) against the bounds the run lists
    themselves give, and the tensor-op mirror kernels.attn_seg_bounds_ref against bounds_loop on those
    rows and on random ids (sorted or not, negatives anywhere)."""
    ids = np.stack([ids_of(r, S) for r in ROWS])
    lo, hi = bounds_loop(ids)
    for b, row in enumerate(ROWS):
        for beg, end, pad in runs_of(row, S):
            for i in range(beg, end):
                assert (lo[b, i], hi[b, i]) == ((i, i) if pad else (beg, end)), (b, i)
    rng = np.random.default_rng(0)
    more = [ids, rng.integers(-1, 2, (5, 37)), rng.integers(-3, 4, (4, 1)), np.full((2, 9), 4), np.full((1, 9), -1)]
    for a in more:
        a = a.astype(np.int32)
        wl, wh = bounds_loop(a)
        gl, gh = K.attn_seg_bounds_ref(torch.tensor(a))
        assert gl.dtype == torch.int32 and np.array_equal(gl.numpy(), wl) and np.array_equal(gh.numpy(), wh)
        assert (np.diff(wl, axis=1) >= 0).all() and (np.diff(wh, axis=1) >= 0).all()  # what the kernels rely on
        m = K.segment_mask_ref(torch.tensor(a)).numpy()
        j = np.arange(a.shape[1])
        assert np.array_equal(m, (j[None, None, :] >= wl[:, :, None]) & (j[None, None, :] < wh[:, :, None]))
    for row in ROWS:  # the mask oracle of the GPU test against the bounds
        l1, h1 = bounds_loop(ids_of(row, S)[None])
        j = np.arange(S)
        assert np.array_equal(mask_of(row, S), (j[None, :] >= l1[0][:, None]) & (j[None, :] < h1[0][:, None]))


# ------------------------------------------------------------------------------------ builder
def test_builder_checks_and_unchanged_graphs():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([4, 6, 16], DataType.DT_FLOAT)
    kv = ff.create_tensor([4, 7, 16], DataType.DT_FLOAT)
    sg = ff.create_tensor([4, 6], DataType.DT_INT32)
    kl = ff.create_tensor([4], DataType.DT_INT32)
    bias = ff.create_tensor([1, 1, 6, 6], DataType.DT_FLOAT)
    L = ff.multihead_attention(x, x, x, 16, 4, segment_ids=sg).owner_layer
    assert len(L.inputs) == 4 and L.attrs["segment_ids"] is True
    assert L.impl.input_maps()[3] == (0, None)
    assert [L.impl.needs_input_grad(i) for i in range(4)] == [True, True, True, False]
    with pytest.raises(ValueError):  # Sq != Sk
        ff.multihead_attention(x, kv, kv, 16, 4, segment_ids=sg)
    with pytest.raises(ValueError):  # wrong shape
        ff.multihead_attention(x, x, x, 16, 4, segment_ids=ff.create_tensor([4, 5], DataType.DT_INT32))
    with pytest.raises(ValueError):
        ff.multihead_attention(x, x, x, 16, 4, segment_ids=kl)
    with pytest.raises(ValueError):
        ff.multihead_attention(x, x, x, 16, 4, segment_ids=sg, key_lengths=kl)
    with pytest.raises(ValueError):
        ff.multihead_attention(x, x, x, 16, 4, segment_ids=sg, attn_bias=bias)
    # graphs without the argument are what they were
    L3 = ff.multihead_attention(x, x, x, 16, 4).owner_layer
    L4 = ff.multihead_attention(x, x, x, 16, 4, key_lengths=kl).owner_layer
    assert len(L3.inputs) == 3 and len(L4.inputs) == 4
    assert "segment_ids" not in L3.attrs and "segment_ids" not in L4.attrs
    assert L4.impl.input_maps()[3] == (0,)
    # scaled_dot_product_attention
    q = ff.create_tensor([4, 2, 6, 8], DataType.DT_FLOAT)
    k7 = ff.create_tensor([4, 2, 7, 8], DataType.DT_FLOAT)
    Ls = ff.scaled_dot_product_attention(q, q, q, segment_ids=sg).owner_layer
    assert len(Ls.inputs) == 4 and Ls.attrs["segment_ids"] is True and Ls.impl.input_maps()[3] == (0, None)
    assert not Ls.impl.needs_input_grad(3)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, k7, k7, segment_ids=sg)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, q, q, segment_ids=sg, key_lengths=kl)
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, q, q, segment_ids=sg,
                                        attn_bias=ff.create_tensor([1, 1, 6, 6], DataType.DT_FLOAT))
    L0 = ff.scaled_dot_product_attention(q, q, q).owner_layer
    assert len(L0.inputs) == 3 and "segment_ids" not in L0.attrs


def test_costmodel_fabricates_one_full_segment():
    from flexflow_amd.pcg.costmodel import fabricate_int_input
    from flexflow_amd.pcg.strategy import OpConfig
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([4, 6, 16], DataType.DT_FLOAT)
    sg = ff.create_tensor([4, 6], DataType.DT_INT32)
    L = ff.multihead_attention(x, x, x, 16, 4, segment_ids=sg).owner_layer
    cfg = OpConfig((1,) * len(L.impl.axis_sizes()), (0,))
    t = fabricate_int_input(L, 3, (4, 6), cfg, "cpu")
    assert t.dtype == torch.int32 and t.shape == (4, 6) and (t == 0).all()


def test_mha_op_segments_cpu_matches_masked_reference():
    """The op on the CPU with segment ids against the same layer with the mask given as a 0 / -inf score
    bias (the way to say it before): outputs and every gradient; padding rows give the output bias."""
    from test_ops_cpu import run_layer
    rows = [[3, 2], [p(1), 4], [5], [p(5)]]
    ids = torch.tensor(np.stack([ids_of(r, 5) for r in rows]))
    see = torch.tensor(np.stack([mask_of(r, 5) for r in rows]))
    bias = torch.where(see, 0.0, float("-inf"))[:, None]
    x = torch.randn(4, 5, 16, generator=torch.Generator().manual_seed(1))
    a = run_layer(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4, segment_ids=t[1]), [x, ids],
                  int_inputs=(1,))
    b = run_layer(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], 16, 4, attn_bias=t[1]), [x, bias])
    assert torch.isfinite(a[3][0]).all()
    assert torch.allclose(a[3][0], b[3][0], rtol=1e-5, atol=1e-6)
    assert torch.allclose(a[5][0], b[5][0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------- packer
def test_packer():
    rng = np.random.default_rng(4)
    seq = 64
    lens = rng.integers(1, seq + 1, 50)
    rows = pack_sequences(lens, seq)
    assert rows == pack_sequences(lens.copy(), seq)  # deterministic
    placed = sorted(i for row in rows for i, _ in row)
    assert placed == list(range(len(lens)))  # every sequence exactly once
    for row in rows:
        at = 0
        for i, off in row:
            assert off == at  # back to back, in row order
            at += int(lens[i])
        assert at <= seq  # no row overflows
    assert len(rows) < len(lens) and 0.5 < fill_ratio(rows, lens, seq) <= 1.0
    assert sum(int(n) for n in lens) <= len(rows) * seq
    toks = [rng.integers(1, 100, n).astype(np.int32) for n in lens]
    labs = [t + 1 for t in toks]
    ids, pos, seg, lab = packed_arrays(rows, toks, labs, seq)
    ids2, pos2, seg2, lab2 = packed_arrays(pack_sequences(lens, seq), toks, labs, seq)
    for a, b in ((ids, ids2), (pos, pos2), (seg, seg2), (lab, lab2)):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert ids.shape == pos.shape == seg.shape == (len(rows), seq) and lab.shape == (len(rows), seq, 1)
    for r, row in enumerate(rows):
        end = 0
        for j, (i, off) in enumerate(row):
            n = int(lens[i])
            assert np.array_equal(ids[r, off:off + n], toks[i]) and np.array_equal(lab[r, off:off + n, 0], labs[i])
            assert np.array_equal(pos[r, off:off + n], np.arange(n))  # positions restart at each sequence
            assert (seg[r, off:off + n] == j).all()
            end = off + n
        assert (seg[r, end:] == -1).all() and (lab[r, end:, 0] == -100).all() and (ids[r, end:] == 0).all()
    assert pack_sequences([], seq) == []
    with pytest.raises(ValueError):
        pack_sequences([seq + 1], seq)
    with pytest.raises(ValueError):
        pack_sequences([0], seq)


# --------------------------------------------------------------------- packed equals padded
LENS = [20, 30, 14, 40, 24, 64]


def _bert_step(packed):
    """One SGD step of bert-tiny (BertConfig.tiny(64), fp32, CPU) on six sentences of lengths LENS: as six
    right-padded rows with key_lengths, or packed into rows with segment_ids. Returns (the initial
    weights, the probabilities of every real token in sentence order, the loss, the weights after the step)."""
    from flexflow_amd.models.bert import BertConfig, build_bert
    seq = 64
    bc = BertConfig.tiny(seq)
    rng = np.random.default_rng(7)
    toks = [rng.integers(1, bc.vocab, n).astype(np.int32) for n in LENS]
    labs = [rng.integers(0, bc.vocab, n).astype(np.int32) for n in LENS]
    if packed:
        rows = pack_sequences(LENS, seq)
    else:
        rows = [[(i, 0)] for i in range(len(LENS))]
    ids_a, pos_a, seg_a, lab_a = packed_arrays(rows, toks, labs, seq)
    B = len(rows)
    torch.manual_seed(0)
    cfg = FFConfig(["--no-hip-graphs", "--device", "cpu", "--dtype", "fp32"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    if packed:
        extra = ff.create_tensor([B, seq], DataType.DT_INT32, name="segment_ids")
        ids, pos, out = build_bert(ff, B, bc, segment_ids=extra)
    else:
        extra = ff.create_tensor([B], DataType.DT_INT32, name="key_lengths")
        ids, pos, out = build_bert(ff, B, bc, key_lengths=extra)
    ff.optimizer = SGDOptimizer(ff, 0.1)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY],
               ignore_index=-100, loss_reduction="valid")
    ws = [w for L in ff.layers for w in L.weights]
    w0 = [np.asarray(w.get_weights(ff), dtype=np.float64).copy() for w in ws]
    ids.set_tensor(ff, ids_a)
    pos.set_tensor(ff, pos_a)
    extra.set_tensor(ff, seg_a if packed else np.asarray(LENS, dtype=np.int32))
    ff.label_tensor.set_tensor(ff, lab_a)
    ff.reset_metrics()
    ff.forward()
    probs = np.asarray(ff._get_tensor_value(ff.output_tensor()), dtype=np.float64)
    ff.zero_gradients()
    ff.backward()
    ff.update()
    loss = ff.get_perf_metrics().get_loss()
    per_sentence = {}
    for r, row in enumerate(rows):
        for i, off in row:
            per_sentence[i] = probs[r, off:off + LENS[i]]
    w1 = [np.asarray(w.get_weights(ff), dtype=np.float64) for w in ws]
    return len(rows), w0, [per_sentence[i] for i in range(len(LENS))], loss, w1


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def test_packed_bert_step_equals_padded():
    """The six sentences as six right-padded rows with key_lengths and packed into three rows with
    segment_ids, from the same seeded weights: the output probabilities at every real token, the loss
    and every weight after one SGD step agree within 1e-4, measured as
    test_mha_op_fp32_device_key_lengths measures its fp32 paths (relative Frobenius error per tensor)."""
    na, w0a, pa, la, w1a = _bert_step(False)
    nb, w0b, pb, lb, w1b = _bert_step(True)
    assert (na, nb) == (6, 3)
    for x, y in zip(w0a, w0b):
        assert np.array_equal(x, y)  # the same seeded weights
    assert np.isfinite(la) and np.isfinite(lb)
    e_p = [_rel(x, y) for x, y in zip(pb, pa)]
    e_w = [_rel(x, y) for x, y in zip(w1b, w1a)]
    e_step = [_rel(x - x0, y - y0) for x, y, x0, y0 in zip(w1b, w1a, w0b, w0a) if np.abs(y - y0).max() > 0]
    print("packed against padded: loss", la, lb, "probabilities", max(e_p), "weights", max(e_w),
          "weight updates alone", max(e_step))
    assert all(np.isfinite(x).all() for x in pb)
    assert max(e_p) < 1e-4, e_p
    assert abs(lb - la) <= 1e-4 * abs(la), (la, lb)
    assert max(e_w) < 1e-4, e_w
    assert max(e_step) < 1e-4, e_step  # the updates themselves, not hidden behind the unchanged part of a weight


# -------------------------------------------------------------------------------- distributed
def test_segments_two_ranks_match_single():
    """An attention model with segment ids on 2 gloo ranks, batch-parallel and heads-parallel, gives the
    single-process output and weights after the harness's SGD steps (tests/test_multirank_cpu.py
    tolerance); and the segments matter to that result."""
    import attn_segments_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("batch")
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"attn segment_ids {case}@2")
    dense = A.single("noseg")
    assert np.abs(dense["__output__"] - ref["__output__"]).max() > 1e-4


# ------------------------------------------------------------------------------------ example
def test_varlen_example_runs_packed():
    """examples/python/native/bert_varlen.py --pack runs end to end in its own process and reports rows
    per step, the fill ratio and tokens/s."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", FF_TUNABLEOP="off")
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "python", "native", "bert_varlen.py"), "-b", "4",
                        "--seq-length", "16", "--iterations", "3", "--pack"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "packed: 4 rows per step, fill ratio" in r.stdout and "tokens/s" in r.stdout, r.stdout[-2000:]
