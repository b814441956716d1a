"""Sliding-window (local) attention in the flash kernels (AttnArgs.seg_lo / seg_hi / seg_klo / seg_khi as
attn_band_bounds writes them), element by element against the float64 oracle of tests/attn_rows_common.py,
the bounds kernel against brute force, the ops against fp32 torch, and a captured decoder step.

Every element of o, dq, dk and dv must satisfy err <= GPU_FACTOR x the bound attn_rows_common derives
from the kernels' rounding steps (U, ACC as they stand there; with grouped heads the group-sum terms of
test_attn_gqa_gpu.py); lse is held to that file's measured tolerance; where the bound is 0 (padding
positions) that is an exact 0 and lse = +inf. Outputs sit between sentinel rows and start as NaN, the
inputs have NaN behind their last row, the backward workspace has a guard band (the launcher of
test_attn_gqa_gpu.py, which takes Hkv <= H). The mask of the reference is the loop oracle of
tests/attn_window_common.py, written from the definition; the bounds the kernels get are checked against
first / last visible index of that mask before they are used.

Cases, the smallest shapes that reach each path (forward workgroup: 128 rows, 32 per wave, 64-key tiles;
backward: 256 keys per block at D = 64, 128 at D = 128, 64-query tiles):

case  B, H, S, D         mask                          reaches
w1    2, 2, 192, 64      causal, (40, 0)               window < 32 rows of slack: every wave mixed; one key block
w2    2, 2, 300, 64      (70, 25)                      asymmetric; ragged last tile; key block 1 serves the last tiles only
w3a   1, 2, 256, 128     causal, (128, 0)              D = 128 (128-key blocks); edges on tile / block boundaries
w3b   1, 2, 256, 128     causal, (0, 0)                self-only: the common range of every wave is empty
w4    1, 2, 576, 64      causal, (100, 0)              Sq >= 512; three key blocks; a dQ chain that starts past block 0
w5    16, 16, 320, 64    (48, 48) in packed rows       B H = 256: chained backward; window inside runs; padding rows
w6    2, 4 / 2, 192, 64  causal, (40, 0), dropout 1/4  grouped heads and dropout beside the window

Each runs the forward structures 0 (register staging), 1 and 3 (LDS-DMA; 3 has no form of its own here)
and the backward structures 2 (register staging) and 10 (LDS-DMA).

Largest err / tolerance on an MI355X (tolerance = 1.25 x bound; lse: its own tolerance), the same for every
structure of a case; w3b (self-only: P = 1) is exact:

case     o    dv    dq    dk   lse
w1    0.65  0.46  0.16  0.16  0.10
w2    0.60  0.44  0.15  0.15  0.13
w3a   0.64  0.43  0.10  0.09  0.08
w3b   0.00  0.00  0.00  0.00  0.08
w4    0.73  0.47  0.20  0.15  0.08
w5    0.71  0.57  0.20  0.19  0.09
w6    0.65  0.57  0.45  0.15  0.10
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import attn_rows_common as R  # noqa: E402
from attn_segments_common import ids_of, live_of  # noqa: E402
from attn_window_common import band_mask, bounds_of, p  # noqa: E402
from test_attn_gqa_gpu import Launcher, gqa_inputs, gqa_reference  # noqa: E402
from test_attn_segments_gpu import S5, TOL_G, TOL_LSE, TOL_O, _ref_attn, _rel  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
SENTINEL = -7


def _w(B, H, S, D, window, causal=False, rows=None, Hkv=None, thr=0):
    return dict(R._c(S, B=B, H=H, D=D, causal=causal, rows=rows, thr=thr), Hkv=Hkv or H, window=window)


CASES = {
    "w1": _w(2, 2, 192, 64, (40, 0), causal=True),
    "w2": _w(2, 2, 300, 64, (70, 25)),
    "w3a": _w(1, 2, 256, 128, (128, 0), causal=True),
    "w3b": _w(1, 2, 256, 128, (0, 0), causal=True),
    "w4": _w(1, 2, 576, 64, (100, 0), causal=True),
    "w5": _w(16, 16, 320, 64, (48, 48), rows=[S5[i % 5] for i in range(16)]),
    "w6": _w(2, 4, 192, 64, (40, 0), causal=True, Hkv=2, thr=64),
}


def band_bounds(ffC, S, left, right, seg=None, B=1):
    """lo, hi, klo, khi of the device kernel into sentinel-filled buffers."""
    out = [torch.full((B, S), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(4)]
    ffC.attn_band_bounds(left, right, None if seg is None else seg[0], None if seg is None else seg[1], *out)
    return out


def _seg_bounds(ffC, rows, S):
    ids = torch.tensor(np.stack([ids_of(r, S) for r in rows]), dtype=torch.int32, device=DEV)
    lo, hi = torch.full_like(ids, SENTINEL), torch.full_like(ids, SENTINEL)
    ffC.attn_seg_bounds(ids, lo, hi)
    return lo, hi


_cache = {}


def _case(ffC, name):
    """The case on the device, its float64 reference and tolerances, and its bounds, built once. The bounds
    the kernels get are the device kernel's, compared here with the brute-force ones of the loop mask."""
    if name not in _cache:
        c = dict(R.full_case(CASES[name]))
        B, S, rows = c["B"], c["Sq"], c["rows"]
        left, right = c["window"]
        inp = gqa_inputs(name, c)
        drows = rows[:5] if rows is not None else None  # w5 repeats five layouts
        see = band_mask(S, left, right, c["causal"], drows)
        if rows is not None:
            see = see[[i % 5 for i in range(B)]]
        inp["see"] = inp["see"] & torch.from_numpy(see)[:, None]
        ref, tol, fig = gqa_reference(c, inp, DEV)
        L = Launcher(ffC, c, inp, "bhsd")
        seg = _seg_bounds(ffC, rows, S) if rows is not None else None
        got = band_bounds(ffC, S, left, right, seg, B)
        want = bounds_of(band_mask(S, left, right, False, drows))
        for g, w, what in zip(got, want, ("lo", "hi", "klo", "khi")):
            w = w[[i % 5 for i in range(B)]] if rows is not None else np.broadcast_to(w, (B, S))
            assert np.array_equal(g.cpu().numpy(), w), (name, what)
        L.kw.update(seg_lo=got[0], seg_hi=got[1], seg_klo=got[2], seg_khi=got[3])
        live = torch.from_numpy(np.stack([live_of(r, S) for r in rows])) if rows is not None else \
            torch.ones(B, S, dtype=torch.bool)
        _cache[name] = (c, L, ref, tol, fig, live.to(DEV))
    return _cache[name]


def _verdict(tag, res):
    print(f"WINDOW-GPU {tag} {R.ratios(res)}")
    assert not R.fails(res), R.fails(res)


def _padding_is_exact(got, live):
    """Padding positions: exact zeros in o / dq / dk / dv, lse = +inf."""
    for key, t in got.items():
        lv = live[:, None, :].expand(-1, t.shape[1], -1)
        if key == "lse":
            assert (t[~lv] == INF).all() and torch.isfinite(t[lv]).all(), key
        else:
            assert (t[~lv] == 0).all() and torch.isfinite(t).all(), key


@pytest.mark.parametrize("fv", [0, 1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_rows(ffC, name, fv):
    c, L, ref, tol, fig, live = _case(ffC, name)
    got = L.fwd(fv)
    print(f"WINDOW-GPU {name} lse_fig={fig:.2e}")
    _verdict(f"{name} fwd={fv}", R.check(got, ref, tol, R.GPU_FACTOR))
    _padding_is_exact(got, live)


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_backward_rows(ffC, name, variant):
    """dq, dk, dv of backward structure `variant` after the default forward: w5 runs the chained form (one
    launch per key block), the others the slab form; the window kernels leave the fused bias gradient alone."""
    c, L, ref, tol, _, live = _case(ffC, name)
    L.fwd(ffC.attn_fwd_variant())
    got, done = L.bwd(variant)
    assert not done
    _verdict(f"{name} bwd={variant}", R.check(got, ref, tol, R.GPU_FACTOR))
    _padding_is_exact(got, live)


def test_a_window_off_by_one_on_the_device_is_flagged(ffC):
    """w1 run with the bounds of the window (39, 0) against the reference of (40, 0): the checker flags o
    and a gradient, so the comparisons above do not pass for want of looking."""
    c, _, ref, tol, _, _ = _case(ffC, "w1")
    L = Launcher(ffC, c, gqa_inputs("w1", c), "bhsd")
    lo, hi, klo, khi = band_bounds(ffC, c["Sq"], 39, -1, None, c["B"])
    L.kw.update(seg_lo=lo, seg_hi=hi, seg_klo=klo, seg_khi=khi)
    got = L.fwd(ffC.attn_fwd_variant())
    got.update(L.bwd(ffC.attn_bwd_variant())[0])
    res = R.check(got, ref, tol, R.GPU_FACTOR)
    bad = {key: int(res[key][0].sum()) for key in R.OUTS}
    print("WINDOW-GPU w1 with (39, 0): rows flagged", bad)
    assert bad["o"] > 0 and (bad["dq"] > 0 or bad["dk"] > 0 or bad["dv"] > 0)


# ------------------------------------------------------------------------------- bounds kernel
BOUND_ROWS = {255: [[100, p(5), 150], [255], [p(255)]], 257: [[1, 255, p(1)], [128, 129], [p(1), 256]]}


@pytest.mark.parametrize("S", [1, 255, 257, 1000])
def test_band_bounds_kernel(ffC, S):
    """attn_band_bounds against first / last visible index of the loop mask, for bounded, zero, one-sided
    and oversized windows, alone and inside packed rows; the outputs start as a sentinel. S = 1000 (a
    multiple of 4: the int4 form, like the cases' sizes) runs one window without rows: the loop oracle is
    quadratic."""
    wins = [(3, 0), (0, 0), (40, 17), (-1, 5), (6, -1), (S + 3, S + 3)] if S < 1000 else [(130, 61)]
    for left, right in wins:
        for rows in (None, BOUND_ROWS.get(S)):
            if rows is None and S in BOUND_ROWS and (left, right) not in ((40, 17), (-1, 5)):
                continue
            B = 1 if rows is None else len(rows)
            seg = _seg_bounds(ffC, rows, S) if rows is not None else None
            got = band_bounds(ffC, S, left, right, seg, B)
            want = bounds_of(band_mask(S, left, right, False, rows))
            for g, w, what in zip(got, want, ("lo", "hi", "klo", "khi")):
                assert np.array_equal(g.cpu().numpy(), w), (S, left, right, rows is not None, what)
    # the Python entry and its tensor-op mirror agree with the binding
    from flexflow_amd import kernels as K
    a = K.attn_band_bounds(S, 2, 1, B=3, device=DEV)
    b = K.attn_band_bounds_ref(S, 2, 1, B=3, device="cpu")
    assert all(torch.equal(x.cpu(), y) for x, y in zip(a, b))


def test_constant_bounds_are_never_replaced(ffC):
    """kernels.attn_band_bounds_const: a caller that needs more rows gets arrays of its own, and the earlier
    ones stay where they are (a captured graph holds pointers into them) and keep serving smaller callers."""
    from flexflow_amd import kernels as K
    a = K.attn_band_bounds_const(2, 96, 5, 3, DEV)
    ptrs, vals = [t.data_ptr() for t in a], [t.clone() for t in a]
    b = K.attn_band_bounds_const(5, 96, 5, 3, DEV)
    assert all(t.shape == (5, 96) for t in b) and all(t.data_ptr() not in ptrs for t in b)
    c = K.attn_band_bounds_const(2, 96, 5, 3, DEV)
    assert [t.data_ptr() for t in c] == ptrs
    assert all(torch.equal(x, y) for x, y in zip(a, vals))
    want = bounds_of(band_mask(96, 5, 3, False))
    for g, w in zip(b, want):
        assert np.array_equal(g.cpu().numpy(), np.broadcast_to(w, (5, 96)))


def test_key_side_arguments_are_checked(ffC):
    """The backward takes seg_klo / seg_khi as a pair, with the dtype, size and device of seg_lo, and only
    beside seg_lo / seg_hi."""
    c, L, _, _, _, _ = _case(ffC, "w1")
    keep = dict(L.kw)
    klo, khi = keep["seg_klo"], keep["seg_khi"]
    L.fwd(ffC.attn_fwd_variant())
    try:
        for bad in (dict(seg_khi=None), dict(seg_klo=None), dict(seg_klo=klo.long(), seg_khi=khi.long()),
                    dict(seg_klo=klo[:1], seg_khi=khi[:1]), dict(seg_klo=klo.cpu(), seg_khi=khi.cpu()),
                    dict(seg_lo=None, seg_hi=None)):  # the last: a key side without the query side
            L.kw = dict(keep, **bad)
            with pytest.raises(RuntimeError):
                L.bwd(ffC.attn_bwd_variant())
    finally:
        L.kw = keep


# ------------------------------------------------------------------------------------- op level
OP_ROWS = [[50, 46, p(32)], [128], [p(5), 33, 90], [1, 64, p(62), 1]]


def _mha(window, causal, rows, E=128, H=2, S=128, Hkv=None, x=None, ws=None, dy=None):
    """MultiHeadAttention(window=...) through OpCtx on the device in bf16: (layer, y, dx, weight gradients,
    x, weights, dy)."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B = 4
    g = torch.Generator().manual_seed(9)
    ff = FFModel(FFConfig([]))
    tx = ff.create_tensor([B, S, E], DataType.DT_FLOAT)
    ts = ff.create_tensor([B, S], DataType.DT_INT32) if rows is not None else None
    L = ff.multihead_attention(tx, tx, tx, E, H, causal=causal, segment_ids=ts, window=window, num_kv_heads=Hkv).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    if x is None:
        x = torch.randn(B, S, E, generator=g).to(DEV, torch.bfloat16)
        ws = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).to(DEV, torch.bfloat16) for w in L.weights]
        dy = torch.randn(B, S, E, generator=g).to(DEV, torch.bfloat16)
    ctx.wgrads = [torch.zeros(w.dims, device=DEV) for w in L.weights]
    ins = [x, x, x]
    if rows is not None:
        ins.append(torch.tensor(np.stack([ids_of(r, S) for r in rows]), dtype=torch.int32, device=DEV))
    y = L.impl.forward(ctx, ins, ws)[0]
    dxs = L.impl.backward(ctx, [dy])
    torch.cuda.synchronize()
    return L, y, dxs[0], ctx.wgrads, x, ws, dy


@pytest.mark.parametrize("window,causal,packed", [((20, 0), True, False), ((30, 11), False, True)])
def test_mha_op_window(ffC, window, causal, packed):
    """bf16 fused self-attention (E 128, H 2: head dim 64) with a window, with and without packed rows,
    against fp32 torch on the same weights under the loop oracle's mask, at the relative tolerances of the
    segments GPU test."""
    rows = OP_ROWS if packed else None
    B, S, E, H = 4, 128, 128, 2
    L, y, dx, gws, x, ws, dy = _mha(window, causal, rows)
    assert (L.attrs["window_left"], L.attrs["window_right"]) == (window[0], -1 if causal else window[1])
    xf = x.float().requires_grad_()
    wf = [w.float().requires_grad_() for w in ws]
    D = E // H
    W, bb = wf[0].reshape(3, H * D, E), wf[1].reshape(3, H * D)
    qq, kk, vv = ((xf @ W[i].t() + bb[i]).view(B, S, H, D).transpose(1, 2) for i in range(3))
    see = torch.tensor(np.broadcast_to(band_mask(S, window[0], window[1], causal, rows), (B, S, S)).copy(), device=DEV)
    o, _ = _ref_attn(qq, kk, vv, see, 1.0 / math.sqrt(D))
    yr = o.transpose(1, 2).reshape(B, S, H * D) @ wf[2].reshape(E, -1).t() + wf[3]
    yr.backward(dy.float())
    errs = {"y": _rel(y, yr), "dx": _rel(dx, xf.grad)}
    for w, gw, r in zip(L.weights, gws, wf):
        errs["d" + w.short_name] = _rel(gw, r.grad)
    print("mha window", window, causal, packed, {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs.pop("y") < TOL_O, errs
    assert all(e < TOL_G for e in errs.values()), errs


def test_sdpa_op_window(ffC):
    """ScaledDotProductAttention(window=(17, 9)) in packed rows, bf16 [4, 2, 128, 64]."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B, H, S, D = 4, 2, 128, 64
    g = torch.Generator().manual_seed(10)
    ff = FFModel(FFConfig([]))
    tq, tk, tv = (ff.create_tensor([B, H, S, D], DataType.DT_FLOAT) for _ in range(3))
    ts = ff.create_tensor([B, S], DataType.DT_INT32)
    L = ff.scaled_dot_product_attention(tq, tk, tv, segment_ids=ts, window=(17, 9)).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(4))
    ids = torch.tensor(np.stack([ids_of(r, S) for r in OP_ROWS]), dtype=torch.int32, device=DEV)
    o = L.impl.forward(ctx, [q, k, v, ids], [])[0]
    dxs = L.impl.backward(ctx, [do])
    assert len(dxs) == 4 and dxs[3] is None
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    see = torch.tensor(band_mask(S, 17, 9, False, OP_ROWS), device=DEV)
    orf, _ = _ref_attn(qf, kf, vf, see, 1.0 / math.sqrt(D))
    orf.backward(do.float())
    errs = dict(o=_rel(o, orf), dq=_rel(dxs[0], qf.grad), dk=_rel(dxs[1], kf.grad), dv=_rel(dxs[2], vf.grad))
    print("sdpa window relative errors", errs)
    assert errs.pop("o") < TOL_O and all(e < TOL_G for e in errs.values()), errs


@pytest.mark.parametrize("causal", [False, True])
def test_unbounded_window_is_the_call_without_it(ffC, causal):
    """window = (S - 1, S - 1), (None, None) and, with causal, (S - 1, 3): the same attributes, and output,
    input gradient and weight gradients bitwise equal to the call without the keyword."""
    S = 128
    L0, y0, dx0, g0, x, ws, dy = _mha(None, causal, None)
    for w in ((S - 1, S - 1), (None, None)) + (((S - 1, 3),) if causal else ()):
        L1, y1, dx1, g1, _, _, _ = _mha(w, causal, None, x=x, ws=ws, dy=dy)
        assert "window_left" not in L1.attrs and "window_right" not in L1.attrs
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))


# --------------------------------------------------------------------------------- step capture
def _train_decoder(flags, window, steps=6):
    """The rotary decoder of test_rope_gpu.py's capture test (2 blocks, hidden 128, 2 heads of 64 over one KV
    head, batch 4, S 64) with packed rows and sliding_window."""
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    torch.manual_seed(0)
    B = 4
    dc = DecoderConfig(hidden=128, heads=2, kv_heads=1, layers=2, ffn=256, vocab=1000, seq=64, sliding_window=window)
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    seg = ff.create_tensor([B, dc.seq], DataType.DT_INT32, name="segment_ids")
    pos = ff.create_tensor([B, dc.seq], DataType.DT_INT32, name="rope_position_ids")
    ids, _ = build_rope_decoder(ff, B, dc, segment_ids=seg, position_ids=pos)
    assert all(("window_left" in L.attrs) == bool(window) for L in ff.layers if L.name.endswith("_attn"))
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    tok = rng.integers(1, dc.vocab, (N, dc.seq)).astype(np.int32)
    cut = rng.integers(8, dc.seq - 8, N)  # two sequences per row; the cut changes from step to step
    j = np.arange(dc.seq)[None, :]
    loaders = [ff.create_data_loader(ids, tok),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, dc.vocab, (N, dc.seq, 1)).astype(np.int32)),
               ff.create_data_loader(seg, (j >= cut[:, None]).astype(np.int32)),
               ff.create_data_loader(pos, np.where(j >= cut[:, None], j - cut[:, None], j).astype(np.int32))]
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


def test_windowed_packed_decoder_trains_under_step_capture():
    """A windowed (16 of 64), packed decoder step captures into a hipGraph: 6 steps (3 eager, the capture, 2
    replays) with capture on equal 6 eager steps from the same state, losses and weights, as
    test_rope_gpu.py asks of captured against eager steps (rtol 1e-5, atol 1e-6); the per-layer bounds launch
    (segment ids change at every step) is inside the graph, and the losses differ from the run without a
    window."""
    ffg, lg, wg = _train_decoder(["--hip-graphs"], 16)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    _, le, we = _train_decoder(["--no-hip-graphs"], 16)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
    _, ld, _ = _train_decoder(["--no-hip-graphs"], 0)
    print("losses without a window", ld)
    assert np.abs(ld - lg).max() > 1e-6, (ld, lg)
