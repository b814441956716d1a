"""Sliding-window (local) attention away from the GPU: the bounds and mask mirrors against loop oracles
(tests/attn_window_common.py), the reference attention path against torch SDPA with the bool mask, the
builders' normalisation and checks, flops(), a small windowed rope decoder on the CPU (packed and not)
against the same model with the window written as a 0 / -inf attn_bias, and two gloo ranks.

Measured once (fp32, CPU, DecoderConfig.tiny(32), sliding_window 8, batch 4): the first-step loss of the
windowed decoder and of the attn_bias decoder, started from the same weights, differ by 0.0 exactly, and
so do the losses of the two steps after it (4.94862366, 3.84171629, 3.06166124 in both). Both run the
reference path of ops/attention.py, where adding a 0 / -inf bias and masked_fill(-inf) leave the same
fp32 scores, so the test demands equality.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from attn_segments_common import bounds_loop, ids_of  # noqa: E402
from attn_window_common import BOUND_CASES, CPU_ROWS, band_mask, bounds_of, p, visible_pairs  # noqa: E402

from flexflow_amd import kernels as K  # noqa: E402
from flexflow_amd.core import (AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType)  # noqa: E402


def _ids(rows, S):
    return None if rows is None else torch.tensor(np.stack([ids_of(r, S) for r in rows]), dtype=torch.int32)


# ------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("S,left,right,rows", BOUND_CASES)
def test_band_bounds_ref_equals_brute_force(S, left, right, rows):
    """attn_band_bounds_ref against first / last visible index per row and per column of the loop mask;
    all four arrays monotone; the key side is the transpose of the query side."""
    ids = _ids(rows, S)
    seg = K.attn_seg_bounds_ref(ids) if ids is not None else (None, None)
    got = [t.numpy() for t in K.attn_band_bounds_ref(S, left, right, *seg)]
    want = bounds_of(band_mask(S, left, right, False, rows))
    for g, w, name in zip(got, want, ("lo", "hi", "klo", "khi")):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
        assert (np.diff(g, axis=1) >= 0).all(), name
    lo, hi, klo, khi = got
    j = np.arange(S)
    q_side = (j[None, None, :] >= lo[:, :, None]) & (j[None, None, :] < hi[:, :, None])  # [b, i, j]
    k_side = (j[None, None, :] >= klo[:, :, None]) & (j[None, None, :] < khi[:, :, None])  # [b, j, i]
    assert np.array_equal(q_side, k_side.transpose(0, 2, 1))
    assert np.array_equal(q_side, band_mask(S, left, right, False, rows))


def test_band_wider_than_every_run_is_the_segment_bounds():
    S = 24
    ids = _ids(CPU_ROWS, S)
    lo, hi = K.attn_seg_bounds_ref(ids)
    longest = 24
    for left, right in ((longest - 1, longest - 1), (longest - 1, -1), (40, 23)):
        got = K.attn_band_bounds_ref(S, left, right, lo, hi)
        for g, w in zip(got, (lo, hi, lo, hi)):
            assert torch.equal(g, w)
    wl, wh = bounds_loop(ids.numpy())
    assert np.array_equal(lo.numpy(), wl) and np.array_equal(hi.numpy(), wh)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S,left,right,rows", BOUND_CASES)
def test_band_mask_ref_equals_loop(S, left, right, rows, causal):
    got = K.band_mask_ref(S, left, right, causal, _ids(rows, S)).numpy()
    assert np.array_equal(got, band_mask(S, left, right, causal, rows))


# ----------------------------------------------------------------------------- reference path
@pytest.mark.parametrize("left,right,causal,packed", [(3, 0, True, False), (5, 2, False, False), (0, 0, False, False),
                                                      (-1, 4, False, True), (4, 0, True, True), (2, 7, False, True)])
def test_reference_path_equals_torch_sdpa(left, right, causal, packed):
    """ops/attention.py's reference attention with window (and segment ids) against
    torch.nn.functional.scaled_dot_product_attention with the loop oracle's bool mask, fp32, forward and
    gradients; rows that see nothing (padding) are zeros in ours and left out of the comparison (torch: NaN)."""
    from flexflow_amd.ops.attention import _attn_ref
    S, H, D = 24, 2, 8
    rows = CPU_ROWS[:4] if packed else None
    B = 4
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, H, S, D, generator=g).requires_grad_() for _ in range(3))
    do = torch.randn(B, H, S, D, generator=g)
    see = torch.tensor(band_mask(S, left, right, causal, rows))[:, None]
    live = see.any(-1)  # [B|1, 1, S]
    out = _attn_ref(q, k, v, D ** -0.5, causal, segments=_ids(rows, S), window=(left, right))
    assert torch.isfinite(out).all()
    lv = live.expand(B, H, S)
    assert (out[~lv] == 0).all()
    w = torch.where(lv[..., None], do, torch.zeros_like(do))
    ga = torch.autograd.grad(out, (q, k, v), w)
    # torch: give dead rows one key so that its softmax stays finite, and no weight in the loss
    see_t = see | (~live[..., None] & torch.eye(S, dtype=torch.bool)[None, None])
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=see_t.expand(B, H, S, S))
    gb = torch.autograd.grad(ref, (q, k, v), w)
    assert torch.allclose(out[lv], ref[lv], rtol=1e-5, atol=1e-6)
    for a, b in zip(ga, gb):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------ builder
def _tensors(ff, B=4, S=6, E=16):
    return (ff.create_tensor([B, S, E], DataType.DT_FLOAT), ff.create_tensor([B, S + 1, E], DataType.DT_FLOAT),
            ff.create_tensor([B, S], DataType.DT_INT32), ff.create_tensor([B], DataType.DT_INT32),
            ff.create_tensor([1, 1, S, S], DataType.DT_FLOAT))


def _sig(L):
    return (len(L.inputs), sorted((k, repr(v)) for k, v in L.attrs.items()))


def test_normalisation():
    """Unbounded and oversized windows leave attributes and inputs those of a call without `window`;
    bounded ones carry window_left / window_right with -1 for an unbounded side."""
    ff = FFModel(FFConfig([]))
    x, kv, sg, kl, bias = _tensors(ff)
    for causal in (False, True):
        base = _sig(ff.multihead_attention(x, x, x, 16, 4, causal=causal).owner_layer)
        for w in (None, -1, (None, None), (-1, -1), 5, 7, (5, 9), (None, 5), (5, None)):
            assert _sig(ff.multihead_attention(x, x, x, 16, 4, causal=causal, window=w).owner_layer) == base, w
    assert _sig(ff.multihead_attention(x, x, x, 16, 4, causal=True, window=(None, 2)).owner_layer) == \
        _sig(ff.multihead_attention(x, x, x, 16, 4, causal=True).owner_layer)
    # a window that bounds nothing goes with key_lengths, attn_bias and Sq != Sk, as before
    assert "window_left" not in ff.multihead_attention(x, x, x, 16, 4, key_lengths=kl, window=(5, 5)).owner_layer.attrs
    assert "window_left" not in ff.multihead_attention(x, x, x, 16, 4, attn_bias=bias, window=None).owner_layer.attrs
    assert "window_left" not in ff.multihead_attention(x, kv, kv, 16, 4, window=(-1, -1)).owner_layer.attrs

    def wl(L):
        return L.attrs["window_left"], L.attrs["window_right"]

    assert wl(ff.multihead_attention(x, x, x, 16, 4, window=2).owner_layer) == (2, 2)
    assert wl(ff.multihead_attention(x, x, x, 16, 4, window=(3, 0)).owner_layer) == (3, 0)
    assert wl(ff.multihead_attention(x, x, x, 16, 4, window=(3, 1), causal=True).owner_layer) == (3, -1)
    assert wl(ff.multihead_attention(x, x, x, 16, 4, window=(5, 1)).owner_layer) == (-1, 1)
    assert wl(ff.multihead_attention(x, x, x, 16, 4, window=(None, 0)).owner_layer) == (-1, 0)
    L = ff.multihead_attention(x, x, x, 16, 4, window=(2, 1), segment_ids=sg).owner_layer
    assert wl(L) == (2, 1) and L.attrs["segment_ids"] is True and len(L.inputs) == 4
    hash(tuple(sorted((k, repr(v)) for k, v in L.attrs.items())))
    q = ff.create_tensor([4, 2, 6, 8], DataType.DT_FLOAT)
    base = _sig(ff.scaled_dot_product_attention(q, q, q, causal=True).owner_layer)
    assert _sig(ff.scaled_dot_product_attention(q, q, q, causal=True, window=(5, 0)).owner_layer) == base
    assert wl(ff.scaled_dot_product_attention(q, q, q, causal=True, window=(4, 0)).owner_layer) == (4, -1)
    assert wl(ff.scaled_dot_product_attention(q, q, q, window=1, segment_ids=sg).owner_layer) == (1, 1)


def test_errors():
    ff = FFModel(FFConfig([]))
    x, kv, sg, kl, bias = _tensors(ff)
    q = ff.create_tensor([4, 2, 6, 8], DataType.DT_FLOAT)
    k7 = ff.create_tensor([4, 2, 7, 8], DataType.DT_FLOAT)
    for kw in (dict(key_lengths=kl), dict(attn_bias=bias)):
        with pytest.raises(ValueError):
            ff.multihead_attention(x, x, x, 16, 4, window=2, **kw)
        with pytest.raises(ValueError):
            ff.scaled_dot_product_attention(q, q, q, window=(2, 0), **kw)
    with pytest.raises(ValueError):
        ff.multihead_attention(x, kv, kv, 16, 4, window=2)  # Sq != Sk
    with pytest.raises(ValueError):
        ff.scaled_dot_product_attention(q, k7, k7, window=2)
    for w in (-2, (-2, 1), (1, -3), (1, 2, 3), 1.5, (1.5, 0)):
        with pytest.raises(ValueError):
            ff.multihead_attention(x, x, x, 16, 4, window=w)
        with pytest.raises(ValueError):
            ff.scaled_dot_product_attention(q, q, q, window=w)
    from flexflow_amd.ops.attention import _attn_ref
    t = torch.zeros(1, 1, 6, 4)
    with pytest.raises(ValueError):
        _attn_ref(t, t, t, 1.0, False, key_lens=torch.tensor([3]), window=(1, 1))
    with pytest.raises(ValueError):
        _attn_ref(t, t, t, 1.0, False, bias=torch.zeros(1, 1, 6, 6), window=(1, 1))


@pytest.mark.parametrize("left,right,causal", [(3, 0, True), (5, 2, False), (0, 0, False), (-1, 4, False),
                                               (7, -1, False), (9, -1, True)])
def test_flops_count_the_band(left, right, causal):
    """flops() of a windowed layer: the projections as ever plus 2 (kd + vd) per visible (query, key) pair,
    head and sample, the pairs counted by the loop oracle."""
    B, S, E, H = 2, 19, 16, 4
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    w = (None if left < 0 else left, None if right < 0 else right)
    L = ff.multihead_attention(x, x, x, E, H, causal=causal, window=w).owner_layer
    L0 = ff.multihead_attention(x, x, x, E, H, causal=causal).owner_layer
    shp = lambda l: ([t.dims for t in l.inputs], [t.dims for t in l.outputs], [t.dims for t in l.weights])  # noqa: E731
    D = E // H
    pairs = visible_pairs(S, left, right, causal)
    assert L.impl.flops(*shp(L)) == L0.impl.flops(*shp(L0)) - 2.0 * B * H * (S * S - pairs) * 2 * D
    q = ff.create_tensor([B, H, S, D], DataType.DT_FLOAT)
    Ls = ff.scaled_dot_product_attention(q, q, q, causal=causal, window=w).owner_layer
    assert Ls.impl.flops(*shp(Ls)) == 2.0 * B * H * pairs * 2 * D


def test_costmodel_keys_differ_by_window():
    from flexflow_amd.pcg.costmodel import cost_params_key
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([4, 64, 16], DataType.DT_FLOAT)
    keys = {cost_params_key(ff.multihead_attention(x, x, x, 16, 4, causal=True, window=w).owner_layer)
            for w in (None, (8, 0), (16, 0))}
    assert len(keys) == 3


# ------------------------------------------------------------------------------ small decoder
def _decoder(window, packed, as_bias=False, steps=3, init=None):
    """DecoderConfig.tiny(32) (what rope_decoder.py --small builds) on the CPU in fp32, `steps` Adam steps:
    (the losses, the initial weights). as_bias: the same model with every layer's window given as a 0 / -inf
    attn_bias. init: initial weights to start from (the extra input tensor of the bias form moves the
    seeds of the initialisers, so the two models are given the same weights explicitly)."""
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    torch.manual_seed(0)
    B, dc = 4, DecoderConfig.tiny(32)
    S = dc.seq
    cfg = FFConfig(["--no-hip-graphs", "--device", "cpu", "--dtype", "fp32"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    seg = pos = bias = None
    if packed:
        seg = ff.create_tensor([B, S], DataType.DT_INT32, name="segment_ids")
        pos = ff.create_tensor([B, S], DataType.DT_INT32, name="rope_position_ids")
    if as_bias:
        bias = ff.create_tensor([1, 1, S, S], DataType.DT_FLOAT, name="band")
        mha = ff.multihead_attention
        ff.multihead_attention = lambda *a, window=None, **kw: mha(*a, attn_bias=bias, **kw)
    else:
        dc.sliding_window = window
    ids, _ = build_rope_decoder(ff, B, dc, segment_ids=seg, position_ids=pos)
    att = [L for L in ff.layers if L.name.endswith("_attn")]
    assert len(att) == dc.layers
    for L in att:
        if as_bias:
            assert L.attrs.get("attn_bias") and "window_left" not in L.attrs
        else:
            assert (L.attrs["window_left"], L.attrs["window_right"]) == (window - 1, -1) and L.attrs["causal"]
    ff.optimizer = AdamOptimizer(ff, 3e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY],
               ignore_index=-100, loss_reduction="valid")
    ws = [w for L in ff.layers for w in L.weights]
    if init is not None:
        assert len(init) == len(ws)
        for w, a in zip(ws, init):
            w.set_weights(ff, a)
    w0 = [np.asarray(w.get_weights(ff)).copy() for w in ws]
    rng = np.random.default_rng(0)
    tok = rng.integers(1, dc.vocab, (B, S)).astype(np.int32)
    lab = ((tok + 1) % dc.vocab)[..., None].astype(np.int32)
    ids.set_tensor(ff, tok)
    if packed:
        rows = [[12, 20], [5, 9, p(18)], [32], [p(3), 29]]
        sid = np.stack([ids_of(r, S) for r in rows])
        lo, _ = bounds_loop(sid)
        seg.set_tensor(ff, sid)
        pos.set_tensor(ff, (np.arange(S)[None, :] - lo).astype(np.int32))
        lab[sid < 0] = -100
    if as_bias:
        bias.set_tensor(ff, np.where(band_mask(S, window - 1, 0, True), 0.0, -np.inf).astype(np.float32)[None])
    ff.label_tensor.set_tensor(ff, lab)
    losses = []
    for _ in range(steps):
        ff.reset_metrics()
        ff.forward()
        ff.zero_gradients()
        ff.backward()
        ff.update()
        losses.append(ff.get_perf_metrics().get_loss())
    return np.asarray(losses, dtype=np.float64), w0


def test_small_decoder_trains_and_equals_the_bias_form():
    """sliding_window = 8 of 32: the windowed decoder trains, packed and unpacked (finite, falling loss);
    unpacked, its losses equal those of the model whose layers take the same band as a 0 / -inf attn_bias
    from the same weights (module docstring: measured difference 0.0, so equality); a wider window gives
    other losses, so the window reaches the scores."""
    W = 8
    win, w0 = _decoder(W, False)
    bias, w0b = _decoder(W, False, as_bias=True, init=w0)
    assert all(np.array_equal(a, b) for a, b in zip(w0, w0b))
    print("windowed", win, "as bias", bias, "difference", np.abs(win - bias).max())
    assert np.isfinite(win).all() and win[-1] < win[0]
    assert np.array_equal(win, bias)
    pk, _ = _decoder(W, True)
    print("windowed, packed", pk)
    assert np.isfinite(pk).all() and pk[-1] < pk[0]
    wide, _ = _decoder(30, False, init=w0)
    assert np.abs(wide - win).max() > 1e-6


def test_example_takes_window(capsys):
    """examples/python/native/rope_decoder.py --small --window 8, packed and not, in this process: it
    reports one windowed attention layer per decoder block, and its losses are not those of the same run
    without --window (the first step's already: the window is in the first forward)."""
    import importlib
    from flexflow_amd.models.decoder import DecoderConfig
    root = os.path.dirname(HERE)
    ex = os.path.join(root, "examples", "python", "native")
    sys.path.insert(0, ex)
    try:
        mod = importlib.import_module("rope_decoder")
        for extra in ([], ["--packed"]):
            argv = ["--small", "--iterations", "3", "-b", "4", "--device", "cpu", "--dtype", "fp32", "--no-hip-graphs"] + extra
            capsys.readouterr()
            losses = np.asarray(mod.top_level_task(argv + ["--window", "8"]))
            out = capsys.readouterr().out
            assert f"sliding window 8: {DecoderConfig.tiny().layers} windowed attention layers" in out, out
            assert "tokens/s" in out
            full = np.asarray(mod.top_level_task(argv))
            out = capsys.readouterr().out
            assert "sliding window" not in out and "tokens/s" in out
            assert np.isfinite(losses).all() and np.isfinite(full).all()
            assert abs(losses[0] - full[0]) > 1e-6, (losses, full)
    finally:
        sys.path.remove(ex)


# -------------------------------------------------------------------------------- distributed
def test_window_two_ranks_match_single():
    """An attention model with a window (and segment ids) on 2 gloo ranks, batch-parallel and
    heads-parallel, gives the single-process output and weights (tests/test_multirank_cpu.py tolerance);
    and the window matters to that result."""
    import attn_window_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("batch")
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"attn window {case}@2")
    dense = A.single("nowin")
    assert np.abs(dense["__output__"] - ref["__output__"]).max() > 1e-4
