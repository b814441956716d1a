"""Grouped-query and multi-query attention without a GPU: the builder and its checks, both ops on the CPU
path against float64 torch with K / V repeat_interleave'd, the proof that the GPU test's inputs tell the
right head map from a wrong one, the search's heads degrees, two gloo ranks against one process, and the
torch.export importer."""
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K
from flexflow_amd.core import DataType, FFConfig, FFModel
from flexflow_amd.ops import OpCtx
from flexflow_amd.type import OperatorType

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from attn_segments_common import ids_of, mask_of  # noqa: E402

SEED, P = 11, 0.25
P_EFF = K.attn_dropout_thr(P) / 256.0


# ------------------------------------------------------------------------------------ builder
def _weights(L):
    return {w.short_name: tuple(w.dims) for w in L.weights}


@pytest.mark.parametrize("Hkv", [2, 1])
def test_builder_weight_names_and_shapes(Hkv):
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    kv = ff.create_tensor([2, 7, 12], DataType.DT_FLOAT)
    L = ff.multihead_attention(x, x, x, 16, 4, num_kv_heads=Hkv).owner_layer
    assert L.attrs["num_kv_heads"] == Hkv and L.attrs["fused_qkv"] is False
    assert _weights(L) == dict(q_weight=(4, 4, 16), k_weight=(Hkv, 4, 16), v_weight=(Hkv, 4, 16), q_bias=(4, 4),
                               k_bias=(Hkv, 4), v_bias=(Hkv, 4), o_weight=(16, 4, 4), o_bias=(16,))
    assert tuple(L.outputs[0].dims) == (2, 6, 16)
    L = ff.multihead_attention(x, kv, kv, 16, 4, 8, 6, bias=False, num_kv_heads=Hkv).owner_layer
    assert _weights(L) == dict(q_weight=(4, 8, 16), k_weight=(Hkv, 8, 12), v_weight=(Hkv, 6, 12), o_weight=(16, 4, 6))
    # the heads axis splits dim 0 of every projection weight, as it always did
    assert L.impl.weight_maps() == [(3, None, None)] * 3 + [(None, 3, None)]
    full = L.impl.flops([(2, 6, 16), (2, 7, 12), (2, 7, 12)], None, [tuple(w.dims) for w in L.weights])
    L4 = ff.multihead_attention(x, kv, kv, 16, 4, 8, 6, bias=False).owner_layer
    mha = L4.impl.flops([(2, 6, 16), (2, 7, 12), (2, 7, 12)], None, [tuple(w.dims) for w in L4.weights])
    assert full == mha - 2.0 * 2 * (4 - Hkv) * 7 * (8 + 6) * 16  # the smaller K / V projections


def test_builder_without_gqa_is_unchanged():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    base = ff.multihead_attention(x, x, x, 16, 4).owner_layer
    for Hkv in (None, 4):
        L = ff.multihead_attention(x, x, x, 16, 4, num_kv_heads=Hkv).owner_layer
        assert L.attrs == base.attrs and "num_kv_heads" not in L.attrs and L.attrs["fused_qkv"] is True
        assert [(w.short_name, tuple(w.dims)) for w in L.weights] == [(w.short_name, tuple(w.dims)) for w in base.weights]
    q = ff.create_tensor([2, 4, 6, 8], DataType.DT_FLOAT)
    assert "enable_gqa" not in ff.scaled_dot_product_attention(q, q, q).owner_layer.attrs


def test_builder_rejects_bad_head_counts():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    for bad in (3, 0, 8):
        with pytest.raises(ValueError):
            ff.multihead_attention(x, x, x, 16, 4, num_kv_heads=bad)
    q = ff.create_tensor([2, 4, 6, 8], DataType.DT_FLOAT)
    k2, k1, k3 = (ff.create_tensor([2, h, 6, 8], DataType.DT_FLOAT) for h in (2, 1, 3))
    with pytest.raises(ValueError):  # k and v head counts differ
        ff.scaled_dot_product_attention(q, k2, k1, enable_gqa=True)
    with pytest.raises(ValueError):  # 3 does not divide 4
        ff.scaled_dot_product_attention(q, k3, k3, enable_gqa=True)
    with pytest.raises(ValueError):  # mismatched heads without enable_gqa
        ff.scaled_dot_product_attention(q, k2, k2)
    L = ff.scaled_dot_product_attention(q, k2, k2, enable_gqa=True).owner_layer
    assert L.attrs["enable_gqa"] is True and tuple(L.outputs[0].dims) == (2, 4, 6, 8)
    assert tuple(ff.scaled_dot_product_attention(q, q, q, enable_gqa=True).dims) == (2, 4, 6, 8)
    with pytest.raises(ValueError):
        K.attn_kv_heads(4, 3)
    assert K.attn_kv_heads(4, None) == 4 and K.attn_kv_heads(4, 1) == 1


# ------------------------------------------------------------------------------------ numerics
def _run(build, inputs, int_inputs=(), step=3):
    """One training forward and backward of an attention layer through OpCtx on the CPU (tests/test_ops_cpu.py's
    run_layer with the dropout seed and step set): layer, weights, y, dy, input gradients, weight gradients."""
    torch.manual_seed(0)
    ff = FFModel(FFConfig([]))
    ts = [ff.create_tensor(list(x.shape), DataType.DT_INT32 if i in int_inputs else DataType.DT_FLOAT)
          for i, x in enumerate(inputs)]
    L = build(ff, ts).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n, training=True, seed=SEED)
    ctx.rng_step = torch.tensor([step], dtype=torch.int64)
    ws = [torch.randn(w.dims) * 0.3 for w in L.weights]
    ctx.wgrads = [torch.zeros(w.dims) for w in L.weights]
    slot = [next(i for i, t in enumerate(ts) if t is u) for u in L.inputs]
    clones = [x.clone() for x in inputs]
    y = L.impl.forward(ctx, [clones[i] for i in slot], ws)[0]
    dy = torch.randn(y.shape)
    dslot = L.impl.backward(ctx, [dy])
    dxs = [None] * len(inputs)
    for i, d in zip(slot, dslot):
        if d is not None:
            dxs[i] = d if dxs[i] is None else dxs[i] + d
    return L, ws, y, dy, dxs, ctx.wgrads


def _attn64(q, k, v, G, scale, see=None, bias=None, keep=None):
    """float64 attention from its definition with K / V repeated over the groups; q [B, H, Sq, D], k / v [B,
    Hkv, Sk, D]; see bool [B, 1|H, Sq, Sk]; a row that sees no key gives zeros."""
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double()
    if see is not None:
        s = s.masked_fill(~see, float("-inf"))
    dead = torch.isneginf(s).all(-1, keepdim=True)
    p = torch.where(dead, torch.zeros_like(s), torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1))
    if keep is not None:
        p = torch.where(keep, p / (1.0 - P_EFF), torch.zeros_like(p))
    return p @ v


B, SQ, H, D = 3, 6, 4, 4
KINDS = ["plain", "causal", "lens", "bias", "segments", "dropout"]
LENS = [6, 3, 0]
SEG = [[3, 3], [("p", 1), 2, 3], [2, ("p", 2), 2]]


def _variant(kind, name, Sq, Sk):
    """(extra inputs, their int positions offset, builder kwargs as a function of the extra tensors, see, bias, keep)."""
    see = bias = keep = None
    extra, ints, kw = [], (), (lambda t: {})
    if kind == "causal":
        see = ~torch.ones(Sq, Sk, dtype=torch.bool).triu(1)[None, None]
        kw = lambda t: dict(causal=True)  # noqa: E731
    elif kind == "lens":
        extra, ints = [torch.tensor(LENS, dtype=torch.int32)], (0,)
        see = (torch.arange(Sk)[None, :] < torch.tensor(LENS)[:, None])[:, None, None, :].expand(B, 1, Sq, Sk)
        kw = lambda t: dict(key_lengths=t[0])  # noqa: E731
    elif kind == "bias":
        b = torch.randn(B, H, Sq, Sk, generator=torch.Generator().manual_seed(5))
        b[:, :, :, 1] = float("-inf")
        b[1, 2, 4] = float("-inf")  # a row with no key left
        extra, bias = [b], b
        kw = lambda t: dict(attn_bias=t[0])  # noqa: E731
    elif kind == "segments":
        extra, ints = [torch.tensor(np.stack([ids_of(r, Sq) for r in SEG]), dtype=torch.int32)], (0,)
        see = torch.tensor(np.stack([mask_of(r, Sq) for r in SEG]))[:, None]
        kw = lambda t: dict(segment_ids=t[0])  # noqa: E731
    elif kind == "dropout":
        keep = K.attn_dropout_keep_ref(SEED, zlib.crc32(name.encode()), 3, B, H, Sq, Sk, P)
        assert keep.any() and not keep.all()
        kw = lambda t: dict(dropout=P)  # noqa: E731
    return extra, ints, kw, see, bias, keep


def _close(a, b):
    from test_ops_cpu import close
    close(a, b.float(), 2e-4)  # test_ops_cpu.py's attention tolerance


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_mha_op_cpu_matches_float64(kind, Hkv):
    """multihead_attention(num_kv_heads=Hkv): output, input gradients and every weight / bias gradient
    against float64 torch on the same weights with K / V repeat_interleave'd."""
    E, G = H * D, H // Hkv
    cross = kind in ("plain", "bias", "lens", "dropout")  # Sq != Sk where the variant allows it
    Sk = 7 if cross else SQ
    g = torch.Generator().manual_seed(1)
    xq, xk, xv = torch.randn(B, SQ, E, generator=g), torch.randn(B, Sk, 12, generator=g), torch.randn(B, Sk, 12, generator=g)
    extra, ints, kw, see, bias, keep = _variant(kind, "gqa", SQ, Sk)
    ins = ([xq, xk, xv] if cross else [xq]) + extra
    n0 = len(ins) - len(extra)
    if cross:
        build = lambda ff, t: ff.multihead_attention(t[0], t[1], t[2], E, H, name="gqa", num_kv_heads=Hkv, **kw(t[3:]))  # noqa: E731
    else:
        build = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, name="gqa", num_kv_heads=Hkv, **kw(t[1:]))  # noqa: E731
    L, ws, y, dy, dxs, wg = _run(build, ins, int_inputs=tuple(n0 + i for i in ints))
    assert [w.short_name for w in L.weights] == ["q_weight", "k_weight", "v_weight", "q_bias", "k_bias", "v_bias",
                                                 "o_weight", "o_bias"]
    xi = [x.double().requires_grad_() for x in ins[:n0]]
    wi = [w.double().requires_grad_() for w in ws]
    srcs = xi if cross else [xi[0]] * 3
    q, k, v = ((x @ w.reshape(-1, w.shape[-1]).t() + b.reshape(-1)).view(B, x.shape[1], -1, D).transpose(1, 2)
               for x, w, b in zip(srcs, wi[:3], wi[3:6]))
    assert q.shape[1] == H and k.shape[1] == Hkv
    o = _attn64(q, k, v, G, 1.0 / math.sqrt(D), see, bias, keep)
    yr = o.transpose(1, 2).reshape(B, SQ, E) @ wi[6].reshape(E, -1).t() + wi[7]
    (yr * dy.double()).sum().backward()
    assert torch.isfinite(y).all()
    _close(y, yr.detach())
    for d, x in zip(dxs, xi):
        _close(d, x.grad)
    assert all(d is None for d in dxs[n0:])
    for gw, w in zip(wg, wi):
        _close(gw, w.grad)


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_sdpa_op_cpu_matches_float64(kind, Hkv):
    """scaled_dot_product_attention(enable_gqa=True): o, dq, dk, dv (dk / dv in the K / V shapes)."""
    G = H // Hkv
    Sk, Dv = (7, 5) if kind in ("plain", "bias", "lens", "dropout") else (SQ, D)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(B, H, SQ, D, generator=g)
    k, v = torch.randn(B, Hkv, Sk, D, generator=g), torch.randn(B, Hkv, Sk, Dv, generator=g)
    extra, ints, kw, see, bias, keep = _variant(kind, "gsdpa", SQ, Sk)
    build = lambda ff, t: ff.scaled_dot_product_attention(t[0], t[1], t[2], name="gsdpa", enable_gqa=True, **kw(t[3:]))  # noqa: E731
    L, _, o, do, dxs, _ = _run(build, [q, k, v] + extra, int_inputs=tuple(3 + i for i in ints))
    qi, ki, vi = (t.double().requires_grad_() for t in (q, k, v))
    orf = _attn64(qi, ki, vi, G, 1.0 / math.sqrt(D), see, bias, keep)
    (orf * do.double()).sum().backward()
    assert dxs[1].shape == k.shape and dxs[2].shape == v.shape and all(d is None for d in dxs[3:])
    _close(o, orf.detach())
    for d, x in zip(dxs, (qi, ki, vi)):
        _close(d, x.grad)


# --------------------------------------------------------------------------- the grouping is observable
@pytest.mark.parametrize("name", ["gqa_plain", "gqa_cross", "gqa_two_blocks", "gqa_d128_causal", "gqa_chain",
                                  "gqa_chain_causal", "gqa_lens", "gqa_drop", "gqa_bias", "gqa_seg"])
def test_the_grouping_is_observable(name):
    """On the GPU test's inputs the reference under the wrong head map h % Hkv differs from the right one
    (h // G) by more than the GPU test's tolerance: in o, and in dk of every KV head. A kernel with the wrong
    map cannot pass test_attn_gqa_gpu.py. (MQA has one map only; of the B = 16 cases the first sample, whose
    inputs are seeded per (sample, head) and so are the GPU test's.)"""
    import attn_rows_common as R
    import test_attn_gqa_gpu as T
    case = T.CASES[name]
    c = dict(R.full_case(dict(case, B=1 if case["B"] == 16 else case["B"])))
    Hkv, G = c["Hkv"], c["H"] // c["Hkv"]
    inp = T.gqa_inputs(name, c)
    ref, tol, _ = T.gqa_reference(c, inp, "cpu")
    wrong_k, wrong_v = (inp[key][:, [h % Hkv for h in range(c["H"])]] for key in ("k", "v"))
    bad, _, _ = R.reference(dict(inp, k=wrong_k, v=wrong_v), "cpu")
    # what a kernel with the wrong map would hand back for KV head j: the sum over the query heads it sent there
    bad_dk = torch.stack([bad["dk"][:, [h for h in range(c["H"]) if h % Hkv == j]].sum(1) for j in range(Hkv)], 1)
    res = R.check(dict(o=bad["o"], dk=bad_dk), ref, tol, R.GPU_FACTOR)
    assert res["o"][2] is not None and res["o"][1] > 10.0, res["o"][1:]
    rows = res["dk"][0]  # bool [B, Hkv, Sk]: rows with an element outside the tolerance
    assert rows.any(-1).any(0).all(), rows.any(-1)
    assert res["dk"][1] > 10.0


# -------------------------------------------------------------------------------------- search
def _heads_degrees(L, axis, devices=4):
    from flexflow_amd.pcg.strategy import enumerate_configs
    return sorted({cfg.degrees[axis] for cfg in enumerate_configs(L, devices, max_configs=10 ** 6)})


def test_search_offers_only_heads_degrees_that_divide_hkv():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([8, 6, 64], DataType.DT_FLOAT)
    q = ff.create_tensor([8, 8, 6, 8], DataType.DT_FLOAT)
    k2, k1 = (ff.create_tensor([8, h, 6, 8], DataType.DT_FLOAT) for h in (2, 1))
    assert _heads_degrees(ff.multihead_attention(x, x, x, 64, 8).owner_layer, 3) == [1, 2, 4]
    assert _heads_degrees(ff.multihead_attention(x, x, x, 64, 8, num_kv_heads=2).owner_layer, 3) == [1, 2]
    assert _heads_degrees(ff.multihead_attention(x, x, x, 64, 8, num_kv_heads=1).owner_layer, 3) == [1]
    assert _heads_degrees(ff.scaled_dot_product_attention(q, q, q).owner_layer, 1) == [1, 2, 4]
    assert _heads_degrees(ff.scaled_dot_product_attention(q, k2, k2, enable_gqa=True).owner_layer, 1) == [1, 2]
    assert _heads_degrees(ff.scaled_dot_product_attention(q, k1, k1, enable_gqa=True).owner_layer, 1) == [1]


# -------------------------------------------------------------------------------- distributed
def test_gqa_two_ranks_match_single():
    """A grouped-query attention model (H = 4, Hkv = 2) on 2 gloo ranks, batch-parallel and heads-parallel
    (each rank two query heads over one KV head), gives the single-process output and weights after the
    harness's SGD steps (tests/test_multirank_cpu.py tolerance); and the KV head count matters to it."""
    import attn_gqa_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("batch")
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"attn gqa {case}@2")
    mha = A.single("mha")
    assert np.abs(mha["__output__"] - ref["__output__"]).max() > 1e-4


# ------------------------------------------------------------------------------------ importer
class _Gqa(torch.nn.Module):
    def forward(self, q, k, v):
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, enable_gqa=True)


def _import(fuse):
    from flexflow_amd.torch.export import ExportImporter
    g = torch.Generator().manual_seed(4)
    q = torch.randn(2, 4, 6, 8, generator=g)
    k, v = torch.randn(2, 2, 6, 8, generator=g), torch.randn(2, 2, 6, 8, generator=g)
    imp = ExportImporter(_Gqa(), ["q", "k", "v"], fuse_sdpa=fuse)
    imp.ep = torch.export.export(_Gqa(), (q, k, v))
    ff = FFModel(FFConfig(["--device", "cpu"]))
    ts = [ff.create_tensor(list(t.shape), DataType.DT_FLOAT) for t in (q, k, v)]
    return ff, imp.to_ff(ff, ts), (q, k, v)


def test_importer_passes_enable_gqa_on():
    ff, outs, (q, k, v) = _import(True)
    sdpa = [L for L in ff.layers if L.op_type == OperatorType.OP_SDPA]
    assert len(sdpa) == 1 and sdpa[0].attrs["enable_gqa"] is True
    assert outs[0].owner_layer is sdpa[0] and tuple(outs[0].dims) == (2, 4, 6, 8)
    L = sdpa[0]
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n, training=False)
    o = L.impl.forward(ctx, [q, k, v], [])[0]
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, enable_gqa=True)
    assert torch.allclose(o, want, rtol=1e-5, atol=1e-6)


def test_importer_unfused_form_names_fuse_sdpa():
    with pytest.raises(NotImplementedError, match="fuse_sdpa"):
        _import(False)
