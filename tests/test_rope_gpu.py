"""Rotary position embeddings on the GPU: rope.hip element by element against the float64 oracle of
tests/rope_common.py (its docstring has the oracle and the derivation of the bound), and the layers that
use it against a test-local fp32 torch attention on the same weights.

Kernel cases (CASES in rope_common.py) are the smallest shapes that reach each branch: the block tail, the
fused [T, 3, H, D] layout with the V third compared bit for bit, grouped heads in separate buffers, the
[B, H, S, D] layout, a partial rotary width, both element-pair paths, interleaved pairs, Sq != Sk, position
ids with restarts / zero rows / the table's last entry, ids outside the table, scaled positions, explicit
frequencies, and the out-of-place form with its pass-through copy. Every case runs forward and inverse.
Outputs start as NaN between sentinel rows; in-place buffers have a sentinel in front and NaN behind.

On an MI355X no element of any case lies outside the bound; the largest |err| / bound is 0.996 on bf16
(the bound's first term is half an ulp of the result, which a correctly rounded result reaches) and 0.44 on
fp32. The inverse after the forward returns the input within 0.95 of 2 u |x| (rope_common.round_trip).
The op tests' relative errors are 2e-3 to 8e-3 in bf16 and below 1e-6 on the fp32 device path.
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

import rope_common as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ffC():
    from flexflow_amd import _C
    return _C


# ------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_rope_kernel_bf16(ffC, name, inverse):
    R.check_case(name, torch.bfloat16, DEV, inverse)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", ["fused_layout", "scalar_path", "out_of_place"])
def test_rope_kernel_fp32(ffC, name, inverse):
    R.check_case(name, torch.float32, DEV, inverse)


@pytest.mark.parametrize("name", ["fused_layout", "gqa", "scalar_path", "interleaved", "ids"])
def test_inverse_undoes_forward(ffC, name):
    w = R.round_trip(name, torch.bfloat16, DEV)
    print(f"rope round trip {name}: worst |back - x| / (2 u |x|) = {w:.3f}")


def test_kernel_matches_reference_path(ffC):
    """kernels.rope on the device and kernels.rope_ref (the CPU path) round the same fp32 values: bf16 results
    differ by at most one rounding step, and almost nowhere."""
    c = R.CASES["fused_layout"]
    gpu, bad = R.run("fused_layout", c, torch.bfloat16, DEV)
    cpu, _ = R.run("fused_layout", c, torch.bfloat16, "cpu")
    assert not bad
    for nm in gpu:
        a, b = gpu[nm][0].float(), cpu[nm][0].float()
        assert float(((a - b).abs() > 2.0 ** -7 * b.abs()).sum()) == 0
        assert float((a != b).float().mean()) < 0.02


def test_arguments_are_checked(ffC):
    from flexflow_amd import kernels as K
    t = K.rope_table(64, 16, device=DEV)
    q = torch.zeros(2 * 16 * 2 * 64, dtype=torch.bfloat16, device=DEV)
    st = [16 * 2 * 64, 64, 2 * 64]
    ffC.rope(q, q, st, 2, 16, None, None, [0, 0, 0], 0, 0, 2, 64, 64, t)
    with pytest.raises(RuntimeError):  # the strides reach past the buffer
        ffC.rope(q[:-8], q[:-8], st, 2, 16, None, None, [0, 0, 0], 0, 0, 2, 64, 64, t)
    with pytest.raises(RuntimeError):  # odd rotary width
        ffC.rope(q, q, st, 2, 16, None, None, [0, 0, 0], 0, 0, 2, 64, 63, t)
    with pytest.raises(RuntimeError):  # a table for another width
        ffC.rope(q, q, st, 2, 16, None, None, [0, 0, 0], 0, 0, 2, 64, 32, t)
    with pytest.raises(RuntimeError):  # ids of another shape
        ffC.rope(q, q, st, 2, 16, None, None, [0, 0, 0], 0, 0, 2, 64, 64, t, torch.zeros(2, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):  # ids with different query and key lengths
        ffC.rope(q, q, st, 2, 16, q, q, st, 2, 8, 2, 64, 64, t, torch.zeros(2, 16, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- op level
MHA = {
    # fused QKV with a bias: qkv_bias's gradient must come from linear_bwd, not from the flash kernel's column sums
    "fused_bias": dict(D=64, kw=dict(bias=True), fused=True),
    "kv1": dict(D=64, kw=dict(num_kv_heads=1, bias=True), Hkv=1),
    "causal": dict(D=64, kw=dict(causal=True, bias=False), fused=True),
    "padded": dict(D=32, kw=dict(bias=True, rotary=dict(dim=16)), fused=True),  # head dim 32 zero-padded to 64
    "fp32": dict(D=64, kw=dict(bias=True, causal=True), fused=True, dtype=torch.float32),
}


@pytest.mark.parametrize("name", list(MHA))
def test_mha_rotary_op(ffC, name):
    """One training step of multihead_attention(rotary=...) with B2 S128 H4 on the device against a fp32 torch
    attention that rotates q and k by the definition, on the same weights: output, input gradient and every
    weight gradient."""
    m = MHA[name]
    B, S, H, D = 2, 128, 4, m["D"]
    Hkv, E = m.get("Hkv", H), H * D
    dtype = m.get("dtype", torch.bfloat16)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, S, E, generator=g).bfloat16().float()
    dy = torch.randn(B, S, E, generator=g).bfloat16().float()
    kw = dict(m["kw"])
    rotary = kw.pop("rotary", True)
    build = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, rotary=rotary, **kw)  # noqa: E731
    ws = R.make_weights(E, 32)
    L, got = R.layer_step(build, [x], (), ws, dy, DEV, dtype)
    torch.cuda.synchronize()
    assert bool(L.attrs["fused_qkv"]) == bool(m.get("fused", False))
    W = {w.short_name: t for w, t in zip(L.weights, ws(L))}
    c = R.rope_cfg(L.attrs["rope_dim"], S)
    want = R.mha_torch([x], W, H, Hkv, c, None, dy, torch.float32, causal=bool(kw.get("causal")))
    assert set(got) == set(want), (sorted(got), sorted(want))
    errs = {n: R.rel(got[n], want[n]) for n in got}
    print("mha rotary relative errors", name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(torch.isfinite(t).all() for t in got.values())
    assert errs.pop("y") < R.TOL_O and all(e < R.TOL_G for e in errs.values()), errs
    # the rotation matters: without it the same weights give another output
    _, plain = R.layer_step(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, **kw), [x], (), ws, dy, DEV, dtype)
    assert R.rel(plain["y"], want["y"]) > 5 * R.TOL_O


def test_rotary_embedding_and_sdpa_equal_the_mha_core(ffC):
    """rotary_embedding on q and k, then scaled_dot_product_attention(enable_gqa=True, causal), in bf16 on the
    device against fp32 torch (rotate, repeat K / V, softmax): the output and the gradients that come back
    through both ops."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    B, H, Hkv, S, D = 2, 4, 2, 128, 64
    g = torch.Generator().manual_seed(33)
    q, do = (torch.randn(B, H, S, D, generator=g).bfloat16().float() for _ in range(2))
    k, v = (torch.randn(B, Hkv, S, D, generator=g).bfloat16().float() for _ in range(2))
    ff = FFModel(FFConfig([]))
    tq, tk, tv = (ff.create_tensor(list(t.shape), DataType.DT_FLOAT) for t in (q, k, v))
    rq, rk = ff.rotary_embedding(tq, dim=32, base=500.0), ff.rotary_embedding(tk, dim=32, base=500.0)
    att = ff.scaled_dot_product_attention(rq, rk, tv, causal=True, enable_gqa=True)
    Lq, Lk, La = rq.owner_layer, rk.owner_layer, att.owner_layer
    ctxs = {}
    for L in (Lq, Lk, La):
        n = len(L.impl.axis_sizes())
        ctxs[L] = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    dq_, dk_, dv_ = (t.to(DEV, torch.bfloat16) for t in (q, k, v))
    yq = Lq.impl.forward(ctxs[Lq], [dq_], [])[0]
    yk = Lk.impl.forward(ctxs[Lk], [dk_], [])[0]
    assert yq.data_ptr() != dq_.data_ptr() and yq.shape == dq_.shape and yq.dtype == dq_.dtype  # out of place
    o = La.impl.forward(ctxs[La], [yq, yk, dv_], [])[0]
    gq, gk, gv = La.impl.backward(ctxs[La], [do.to(DEV, torch.bfloat16)])[:3]
    gq = Lq.impl.backward(ctxs[Lq], [gq])[0]
    gk = Lk.impl.backward(ctxs[Lk], [gk])[0]
    torch.cuda.synchronize()
    c = R.rope_cfg(32, S, base=500.0)
    qi, ki, vi = (t.clone().requires_grad_() for t in (q, k, v))
    qr, kr = R.rotate(qi, c, rd=32), R.rotate(ki, c, rd=32)
    s = qr @ kr.repeat_interleave(H // Hkv, 1).transpose(-1, -2) / math.sqrt(D)
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    ref = torch.softmax(s, -1) @ vi.repeat_interleave(H // Hkv, 1)
    (ref * do).sum().backward()
    errs = {n: R.rel(a, b) for n, a, b in (("o", o, ref.detach()), ("dq", gq, qi.grad), ("dk", gk, ki.grad), ("dv", gv, vi.grad))}
    print("rotary_embedding + sdpa relative errors", {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs.pop("o") < R.TOL_O and all(e < R.TOL_G for e in errs.values()), errs


def test_packed_rows_equal_their_sequences(ffC):
    """Rows packed by utils/packing.py, fed with segment_ids and rope_position_ids, give sequence by sequence
    the outputs and input gradients of the same sequences run one per row without ids (and the same weight
    gradients in sum), at the op bounds: a sequence rotates by its own positions wherever it sits in a row."""
    from flexflow_amd.utils.packing import pack_sequences, packed_arrays
    S, H, Hkv, D = 128, 4, 2, 64
    E = H * D
    lens = [70, 50, 128, 33, 58, 20]
    rows = pack_sequences(lens, S)
    _, pos, seg, _ = packed_arrays(rows, [np.zeros(n) for n in lens], [np.zeros(n) for n in lens], S)
    Bp, Bs = len(rows), len(lens)
    g = torch.Generator().manual_seed(35)
    xs = [torch.randn(n, E, generator=g).bfloat16().float() for n in lens]
    dys = [torch.randn(n, E, generator=g).bfloat16().float() for n in lens]
    xp, dyp = torch.zeros(Bp, S, E), torch.zeros(Bp, S, E)
    xo, dyo = torch.zeros(Bs, S, E), torch.zeros(Bs, S, E)
    for r, row in enumerate(rows):
        for i, off in row:
            xp[r, off:off + lens[i]], dyp[r, off:off + lens[i]] = xs[i], dys[i]
    for i, n in enumerate(lens):
        xo[i, :n], dyo[i, :n] = xs[i], dys[i]
    ws = R.make_weights(E, 36)
    kw = dict(causal=True, num_kv_heads=Hkv, bias=False, rotary=dict(max_positions=2 * S))
    packed = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, segment_ids=t[1], rope_position_ids=t[2], **kw)  # noqa: E731
    single = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, segment_ids=t[1], **kw)  # noqa: E731
    _, gp = R.layer_step(packed, [xp, torch.tensor(seg), torch.tensor(pos)], (1, 2), ws, dyp, DEV, torch.bfloat16)
    seg1 = torch.full((Bs, S), -1, dtype=torch.int32)
    for i, n in enumerate(lens):
        seg1[i, :n] = 0
    _, g1 = R.layer_step(single, [xo, seg1], (1,), ws, dyo, DEV, torch.bfloat16)
    torch.cuda.synchronize()
    for key, tol in (("y", R.TOL_O), ("dx0", R.TOL_G)):
        a = torch.cat([gp[key][r, off:off + lens[i]].float().cpu() for r, row in enumerate(rows) for i, off in row])
        b = torch.cat([g1[key][i, :lens[i]].float().cpu() for r, row in enumerate(rows) for i, off in row])
        e = R.rel(a, b)
        print("packed against one sequence per row", key, f"{e:.2e}")
        assert torch.isfinite(a).all() and e < tol, (key, e)
    for key in gp:
        if key.startswith("d") and key != "dx0":
            e = R.rel(gp[key], g1[key])
            print("packed against one sequence per row", key, f"{e:.2e}")
            assert e < R.TOL_G, (key, e)
    # the ids are read: a shift of a whole sequence would change nothing (the scores depend on position
    # differences alone), ids twice as far apart do
    _, gw = R.layer_step(packed, [xp, torch.tensor(seg), torch.tensor(2 * pos)], (1, 2), ws, dyp, DEV, torch.bfloat16)
    assert R.rel(gw["y"], gp["y"]) > 5 * R.TOL_O


# ------------------------------------------------------------------------------------- training
def _train_decoder(flags, spread, steps=6):
    """spread: the position ids of a sample are its in-sequence indices times 1, 2 or 3 (drawn per sample, so
    they change from step to step and, unlike a shift, change the scores); else times 1."""
    from flexflow_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    torch.manual_seed(0)
    B = 4
    dc = DecoderConfig(hidden=128, heads=2, kv_heads=1, layers=2, ffn=256, vocab=1000, seq=64, max_positions=192)
    cfg = FFConfig(["--dtype", "bf16"] + flags)
    cfg.graph_min_step_ms = 1e9  # capture whatever the step length
    cfg.batch_size = B
    ff = FFModel(cfg)
    seg = ff.create_tensor([B, dc.seq], DataType.DT_INT32, name="segment_ids")
    pos = ff.create_tensor([B, dc.seq], DataType.DT_INT32, name="rope_position_ids")
    ids, _ = build_rope_decoder(ff, B, dc, segment_ids=seg, position_ids=pos)
    ff.optimizer = AdamOptimizer(ff, 1e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    N = B * steps
    tok = rng.integers(1, dc.vocab, (N, dc.seq)).astype(np.int32)
    loaders = [ff.create_data_loader(ids, tok),
               ff.create_data_loader(ff.label_tensor, rng.integers(0, dc.vocab, (N, dc.seq, 1)).astype(np.int32))]
    # every row: two sequences; the cut and the spread, and so the ids, change from step to step
    cut = rng.integers(8, dc.seq - 8, N)
    mul = rng.integers(1, 4, N)[:, None] if spread else 1
    j = np.arange(dc.seq)[None, :]
    loaders.append(ff.create_data_loader(seg, (j >= cut[:, None]).astype(np.int32)))
    loaders.append(ff.create_data_loader(pos, (np.where(j >= cut[:, None], j - cut[:, None], j) * mul).astype(np.int32)))
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


def test_decoder_position_ids_train_under_step_capture():
    """The rotary decoder (2 blocks, hidden 128, batch 4, S 64) with segment and position ids fed by data
    loaders, hipGraph step capture on and off: 6 steps (3 eager, the capture, 2 replays), the graph must
    exist, losses and weights agree as test_attn_key_lengths_gpu.py asks of captured against eager steps
    (rtol 1e-5, atol 1e-6). The ids change at every step, and the losses differ from the same run with
    every spread equal to 1, so the replays read them on the device."""
    ffg, lg, wg = _train_decoder(["--hip-graphs"], True)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    _, le, we = _train_decoder(["--no-hip-graphs"], True)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
    _, ld, _ = _train_decoder(["--hip-graphs"], False)
    print("losses with every spread 1", ld)
    assert np.abs(ld[3:] - lg[3:]).max() > 1e-6, (ld, lg)
