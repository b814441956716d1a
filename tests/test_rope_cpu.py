"""Rotary position embeddings without a GPU: the kernel's cases through the plain-torch reference path
(kernels.rope_ref, what the wrappers run on the CPU) against the float64 oracle of tests/rope_common.py, the
proof that the cases tell a wrong convention from the right one, the host table, the builder and its
checks, multihead_attention(rotary=...) and rotary_embedding against float64 torch, packed rows against
their sequences, the cost model's view of the new input, two gloo ranks against one process, and the
example."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from flexflow_amd import kernels as K
from flexflow_amd.core import DataType, FFConfig, FFModel
from flexflow_amd.type import OperatorType

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import rope_common as R  # noqa: E402


# ------------------------------------------------------------------------------------ reference path
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_path_bf16(name, inverse):
    R.check_case(name, torch.bfloat16, "cpu", inverse)


@pytest.mark.parametrize("name", ["fused_layout", "scalar_path", "out_of_place"])
def test_reference_path_fp32(name):
    R.check_case(name, torch.float32, "cpu")


@pytest.mark.parametrize("name", ["fused_layout", "gqa", "interleaved", "ids"])
def test_inverse_undoes_forward(name):
    assert R.round_trip(name, torch.bfloat16, "cpu") <= 1.0


@pytest.mark.parametrize("name", ["fused_layout", "partial", "interleaved", "ids", "scaled"])
def test_the_convention_is_observable(name):
    """On the GPU test's inputs a wrong convention lies outside the tolerance in most rotated elements: the
    other pairing (interleaved for half-split and the reverse), and +sin for -sin (the forward where the
    inverse is asked). A kernel with either mistake cannot pass test_rope_gpu.py."""
    c = R.CASES[name]
    bufs = R.make_inputs(name, c, torch.bfloat16)
    x4 = R.view4(bufs["q"], R._layout(c, "q")[1], c["B"], c["H"], c["Sq"], c["D"])
    ids = R.make_ids(c)
    ref, tol = R.oracle(x4, c, ids, R.U[torch.bfloat16])
    rot = tol[..., :c["rd"]] > 0  # rotated elements with a non-zero pair
    if ids is not None:
        rot = rot & (ids.clamp(0, c["maxp"] - 1) > 0)[:, None, :, None]  # position 0 rotates by nothing
    else:
        rot = rot & (torch.arange(c["Sq"]) > 0)[None, None, :, None]
    for what, wrong in (("pairing", R.oracle(x4, c, ids, 0.0, interleaved=not c["interleaved"])[0]),
                        ("sign", R.oracle(x4, c, ids, 0.0, inverse=True)[0])):
        out = ((wrong - ref).abs() > tol)[..., :c["rd"]]
        frac = float(out[rot].float().mean())
        print(f"{name}: wrong {what} outside the bound in {frac:.3f} of the rotated elements")
        assert frac > 0.5, (name, what, frac)


def test_table_is_built_in_float64_and_cached():
    t = K.rope_table(64, 4096)
    assert t.dtype == torch.float32 and tuple(t.shape) == (4096, 32, 2) and K.rope_table(64, 4096) is t
    p, i = 4095, 1
    ang = p * 10000.0 ** (-2.0 * i / 64)
    assert abs(float(t[p, i, 0]) - math.cos(ang)) <= 2.0 ** -24 and abs(float(t[p, i, 1]) - math.sin(ang)) <= 2.0 ** -24
    # the angle formed in fp32 would be off by about 2e-4 there, far outside the kernel's bound
    a32 = torch.tensor(float(p), dtype=torch.float32) * torch.tensor(10000.0 ** (-2.0 * i / 64), dtype=torch.float32)
    assert abs(float(a32.double()) - ang) > 2e-5
    s = K.rope_table(8, 4, scale=4.0)
    assert torch.allclose(s[3, 0], torch.tensor([math.cos(0.75), math.sin(0.75)]))
    f = K.rope_table(4, 3, inv_freq=[0.5, 0.25])
    assert torch.allclose(f[2, :, 1], torch.tensor([math.sin(1.0), math.sin(0.5)]))
    with pytest.raises(ValueError):
        K.rope_table(4, 3, inv_freq=[0.5])
    with pytest.raises(ValueError):
        K.rope_table(5, 3)


# ------------------------------------------------------------------------------------ builder
def _mha_layers(**kw):
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    return ff, x, ff.multihead_attention(x, x, x, 16, 4, **kw).owner_layer


def test_builder_without_rotary_is_unchanged():
    _, _, base = _mha_layers()
    for off in (None, False):
        _, _, L = _mha_layers(rotary=off)
        assert L.attrs == base.attrs and not any(k.startswith("rope") or k == "rotary" for k in L.attrs)
        assert len(L.inputs) == 3 and [(w.short_name, tuple(w.dims)) for w in L.weights] == \
            [(w.short_name, tuple(w.dims)) for w in base.weights]
        assert L.impl.input_maps() == base.impl.input_maps()


def test_builder_stores_plain_hashable_attributes():
    _, _, L = _mha_layers(rotary=True)
    assert (L.attrs["rope_dim"], L.attrs["rope_base"], L.attrs["rope_interleaved"], L.attrs["rope_scale"],
            L.attrs["rope_inv_freq"], L.attrs["rope_max_positions"]) == (4, 10000.0, False, 1.0, None, 6)
    assert "rope_positions" not in L.attrs and L.attrs["fused_qkv"] is True
    _, _, L = _mha_layers(rotary=dict(dim=2, base=500.0, interleaved=True, scale=2.0, inv_freq=[0.5], max_positions=64))
    assert (L.attrs["rope_dim"], L.attrs["rope_base"], L.attrs["rope_interleaved"], L.attrs["rope_scale"],
            L.attrs["rope_inv_freq"], L.attrs["rope_max_positions"]) == (2, 500.0, True, 2.0, (0.5,), 64)
    hash(tuple(sorted((k, v) for k, v in L.attrs.items() if k.startswith("rope"))))
    # cross attention: max_positions defaults to the longer side
    ff = FFModel(FFConfig([]))
    q, kv = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT), ff.create_tensor([2, 9, 16], DataType.DT_FLOAT)
    assert ff.multihead_attention(q, kv, kv, 16, 4, rotary=True).owner_layer.attrs["rope_max_positions"] == 9


def test_builder_places_the_position_ids():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    pos = ff.create_tensor([2, 6], DataType.DT_INT32)
    seg = ff.create_tensor([2, 6], DataType.DT_INT32)
    kl = ff.create_tensor([2], DataType.DT_INT32)
    bias = ff.create_tensor([1, 4, 6, 6], DataType.DT_FLOAT)
    L = ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=pos, key_lengths=kl, attn_bias=bias).owner_layer
    assert L.attrs["rope_positions"] is True and [t.guid for t in L.inputs] == [x.guid] * 3 + [kl.guid, pos.guid, bias.guid]
    # the ids' map is the key lengths': sharded with the batch, replicated over the heads
    assert L.impl.input_maps()[3:] == [(0,), (0, None), (None, 3, None, None)]
    assert [L.impl.needs_input_grad(i) for i in range(6)] == [True] * 3 + [False] * 3
    L = ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=pos, segment_ids=seg).owner_layer
    assert [t.guid for t in L.inputs][3:] == [seg.guid, pos.guid] and L.impl._has_key_lens()
    L = ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=pos).owner_layer
    assert len(L.inputs) == 4 and not L.impl._has_key_lens() and L.impl.input_maps()[3] == (0, None)


def test_builder_rejects_bad_arguments():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    kv = ff.create_tensor([2, 9, 16], DataType.DT_FLOAT)
    pos = ff.create_tensor([2, 6], DataType.DT_INT32)
    for bad in (dict(dim=3), dict(dim=6), dict(dim=0.5), dict(inv_freq=[1.0]), dict(dim=4, inv_freq=[1.0, 0.5, 0.25]),
                dict(max_positions=5), dict(base=-1.0), dict(scale=0.0), dict(dims=4)):
        with pytest.raises(ValueError):
            ff.multihead_attention(x, x, x, 16, 4, rotary=bad)
    with pytest.raises(ValueError):  # ids need one length for queries and keys
        ff.multihead_attention(x, kv, kv, 16, 4, rotary=True, rope_position_ids=pos)
    with pytest.raises(ValueError):  # ids without rotary
        ff.multihead_attention(x, x, x, 16, 4, rope_position_ids=pos)
    with pytest.raises(ValueError):  # wrong shape
        ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=ff.create_tensor([2, 5], DataType.DT_INT32))
    with pytest.raises(ValueError):  # wrong dtype
        ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=ff.create_tensor([2, 6], DataType.DT_FLOAT))
    h = ff.create_tensor([2, 4, 6, 8], DataType.DT_FLOAT)
    for bad in (dict(dim=10), dict(dim=3), dict(seq_dim=3), dict(max_positions=4)):
        with pytest.raises(ValueError):
            ff.rotary_embedding(h, **bad)
    with pytest.raises(ValueError):
        ff.rotary_embedding(h, position_ids=ff.create_tensor([2, 4], DataType.DT_INT32))  # [B, H], not [B, S]
    L = ff.rotary_embedding(h, dim=4).owner_layer
    assert L.op_type == OperatorType.OP_ROPE and int(OperatorType.OP_ROPE.value) == 103 and not L.weights
    assert tuple(L.outputs[0].dims) == (2, 4, 6, 8) and L.attrs["rope_max_positions"] == 6
    assert L.impl.flops([(2, 4, 6, 8)], None, []) == 3.0 * 2 * 4 * 6 * 4 and not L.impl.uses_mfma()
    assert L.impl.supports_axis(0) and L.impl.supports_axis(1) and not L.impl.supports_axis(2)
    L1 = ff.rotary_embedding(ff.create_tensor([2, 6, 4, 8], DataType.DT_FLOAT), seq_dim=1).owner_layer
    assert L1.impl.supports_axis(2) and not L1.impl.supports_axis(1) and L1.attrs["rope_max_positions"] == 6


def test_cost_model_sees_the_rotation_and_the_ids():
    from flexflow_amd.pcg.costmodel import cost_key, fabricate_int_input, is_rope_ids_input, is_score_bias_input
    from flexflow_amd.pcg.strategy import OpConfig
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    pos = ff.create_tensor([2, 6], DataType.DT_INT32)
    kl = ff.create_tensor([2], DataType.DT_INT32)
    bias = ff.create_tensor([1, 4, 6, 6], DataType.DT_FLOAT)
    plain = ff.multihead_attention(x, x, x, 16, 4).owner_layer
    rot = ff.multihead_attention(x, x, x, 16, 4, rotary=True).owner_layer
    rot2 = ff.multihead_attention(x, x, x, 16, 4, rotary=dict(base=500.0)).owner_layer
    cfg = OpConfig((1,) * len(plain.impl.axis_sizes()), (0,))
    keys = [cost_key(L, cfg, DataType.DT_FLOAT) for L in (plain, rot, rot2)]
    assert len(set(keys)) == 3
    full = ff.multihead_attention(x, x, x, 16, 4, rotary=True, key_lengths=kl, rope_position_ids=pos, attn_bias=bias).owner_layer
    assert [is_rope_ids_input(full, i) for i in range(6)] == [False] * 4 + [True, False]
    assert [is_score_bias_input(full, i) for i in range(6)] == [False] * 5 + [True]
    ids = fabricate_int_input(full, 4, (2, 6), cfg, "cpu")  # positions are timed as arange(S), not as key lengths
    assert ids.dtype == torch.int32 and torch.equal(ids, torch.arange(6, dtype=torch.int32).repeat(2, 1))
    assert torch.equal(fabricate_int_input(full, 3, (2,), cfg, "cpu"), torch.full((2,), 6, dtype=torch.int32))
    only = ff.multihead_attention(x, x, x, 16, 4, rotary=True, rope_position_ids=pos).owner_layer
    assert torch.equal(fabricate_int_input(only, 3, (2, 6), cfg, "cpu"), ids)
    op = ff.rotary_embedding(ff.create_tensor([2, 4, 6, 8], DataType.DT_FLOAT), position_ids=pos).owner_layer
    assert torch.equal(fabricate_int_input(op, 1, (2, 6), cfg, "cpu"), ids)


# ------------------------------------------------------------------------------------ numerics
def _close(a, b, what):
    from test_ops_cpu import close
    close(a.float(), b.float(), 2e-4)  # test_ops_cpu.py's attention tolerance


B, S, H, D = 3, 6, 4, 8
VARIANTS = {
    "fused_bias": dict(kw=dict(bias=True)),
    "kv1": dict(kw=dict(bias=True, num_kv_heads=1), Hkv=1),
    "causal_kv2": dict(kw=dict(bias=False, causal=True, num_kv_heads=2), Hkv=2),
    "cross": dict(kw=dict(bias=True), cross=9),
    "partial_interleaved": dict(kw=dict(bias=True), rotary=dict(dim=4, interleaved=True, base=100.0)),
    "scaled_inv_freq": dict(kw=dict(bias=True), rotary=dict(scale=2.0, inv_freq=[1.0, 0.5, 0.25, 0.125])),
    "ids": dict(kw=dict(bias=True, causal=True), ids=True, rotary=dict(max_positions=32)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_mha_rotary_cpu_matches_float64(name):
    """multihead_attention(rotary=...) on the CPU path: output, input gradients and every weight and bias
    gradient against float64 torch that rotates q and k by the definition, on the same weights."""
    v = VARIANTS[name]
    E, Hkv, Sk = H * D, v.get("Hkv", H), v.get("cross", S)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(B, S, E, generator=g)]
    if "cross" in v:
        xs += [torch.randn(B, Sk, 12, generator=g), torch.randn(B, Sk, 12, generator=g)]
    ids = torch.randint(-2, 36, (B, S), generator=g, dtype=torch.int32) if v.get("ids") else None  # some outside the table
    rotary = v.get("rotary", True)
    dy = torch.randn(B, S, E, generator=g)

    def build(ff, t):
        src = t[:3] if "cross" in v else [t[0]] * 3
        extra = dict(rope_position_ids=t[-1]) if ids is not None else {}
        return ff.multihead_attention(*src, E, H, rotary=rotary, **v["kw"], **extra)

    ins = xs + ([ids] if ids is not None else [])
    ws = R.make_weights(E, 4)
    L, got = R.layer_step(build, ins, (len(ins) - 1,) if ids is not None else (), ws, dy, "cpu", torch.float32)
    assert L.attrs["fused_qkv"] == (Hkv == H and "cross" not in v)
    W = {w.short_name: t for w, t in zip(L.weights, ws(L))}
    rc = R.rope_cfg(L.attrs["rope_dim"], max(S, Sk), **(rotary if isinstance(rotary, dict) else {}))
    want = R.mha_torch(xs, W, H, Hkv, rc, ids, dy, torch.float64, causal=bool(v["kw"].get("causal")))
    assert set(got) == set(want), (sorted(got), sorted(want))
    for n in got:
        assert torch.isfinite(got[n]).all(), n
        _close(got[n], want[n], n)
    plain = R.mha_torch(xs, W, H, Hkv, None, None, dy, torch.float64, causal=bool(v["kw"].get("causal")))
    assert R.rel(plain["y"], want["y"]) > 1e-2  # the rotation matters


@pytest.mark.parametrize("seq_dim", [2, 1])
def test_rotary_embedding_op_cpu(seq_dim):
    """The op against the float64 oracle element by element (fp32 storage), with ids, both layouts; its
    backward is the inverse rotation of dy; the ids take no gradient."""
    Bx, Hx, Sx, Dx, rd = 2, 3, 7, 12, 8
    g = torch.Generator().manual_seed(5)
    x4 = torch.randn(Bx, Hx, Sx, Dx, generator=g)
    dy4 = torch.randn(Bx, Hx, Sx, Dx, generator=g)
    ids = torch.randint(0, 20, (Bx, Sx), generator=g, dtype=torch.int32)
    to = (lambda t: t) if seq_dim == 2 else (lambda t: t.transpose(1, 2).contiguous())
    build = lambda ff, t: ff.rotary_embedding(t[0], position_ids=t[1], seq_dim=seq_dim, dim=rd, max_positions=20)  # noqa: E731
    L, got = R.layer_step(build, [to(x4), ids], (1,), lambda L: [], to(dy4), "cpu", torch.float32)
    assert set(got) == {"y", "dx0"} and got["y"].shape == to(x4).shape
    c = R._c(B=Bx, Sq=Sx, H=Hx, D=Dx, rd=rd, maxp=20)
    for key, src, inverse in (("y", x4, False), ("dx0", dy4, True)):
        ref, tol = R.oracle(src, c, ids, R.U[torch.float32], inverse)
        miss, worst = R.check(to(got[key]) if seq_dim == 1 else got[key], ref, tol)
        assert miss == 0, (key, miss, worst)


def test_rotary_embedding_and_sdpa_equal_the_mha_core_cpu():
    """rotary_embedding on q and k, then scaled_dot_product_attention(enable_gqa=True) equals, on the heads a
    multihead_attention(rotary=True, num_kv_heads=2) layer projects, that layer's attention core."""
    from flexflow_amd.ops import OpCtx
    E, Hkv = H * D, 2
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, S, E, generator=g)
    ws = R.make_weights(E, 8)
    build = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, rotary=True, num_kv_heads=Hkv, causal=True, bias=False)  # noqa: E731
    L, got = R.layer_step(build, [x], (), ws, torch.zeros(B, S, E), "cpu", torch.float32)
    W = {w.short_name: t for w, t in zip(L.weights, ws(L))}
    q, k, v = ((x @ W[f"{n}_weight"].reshape(-1, E).t()).view(B, S, -1, D).transpose(1, 2).contiguous() for n in "qkv")
    ff = FFModel(FFConfig([]))
    tq, tk, tv = (ff.create_tensor(list(t.shape), DataType.DT_FLOAT) for t in (q, k, v))
    rq, rk = ff.rotary_embedding(tq), ff.rotary_embedding(tk)
    att = ff.scaled_dot_product_attention(rq, rk, tv, causal=True, enable_gqa=True)
    outs = {}
    for Lx, xs in ((rq.owner_layer, [q]), (rk.owner_layer, [k])):
        n = len(Lx.impl.axis_sizes())
        outs[Lx] = Lx.impl.forward(OpCtx(layer=Lx, part_coords=(0,) * n, degrees=(1,) * n, training=False), xs, [])[0]
    La = att.owner_layer
    n = len(La.impl.axis_sizes())
    o = La.impl.forward(OpCtx(layer=La, part_coords=(0,) * n, degrees=(1,) * n, training=False),
                        [outs[rq.owner_layer], outs[rk.owner_layer], v], [])[0]
    y = o.transpose(1, 2).reshape(B, S, E) @ W["o_weight"].reshape(E, -1).t()
    _close(y, got["y"], "y")


def test_packed_rows_equal_their_sequences_cpu():
    """Rows packed by utils/packing.py with segment_ids + rope_position_ids give, sequence by sequence, the
    outputs and input gradients of the same sequences run one per row without ids, and the same weight
    gradients in sum."""
    from flexflow_amd.utils.packing import pack_sequences, packed_arrays
    Sx, E, Hkv = 16, H * D, 2
    lens = [9, 6, 16, 4, 7, 3]
    rows = pack_sequences(lens, Sx)
    _, pos, seg, _ = packed_arrays(rows, [np.zeros(n) for n in lens], [np.zeros(n) for n in lens], Sx)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(n, E, generator=g) for n in lens]
    dys = [torch.randn(n, E, generator=g) for n in lens]
    xp, dyp = torch.zeros(len(rows), Sx, E), torch.zeros(len(rows), Sx, E)
    xo, dyo = torch.zeros(len(lens), Sx, E), torch.zeros(len(lens), Sx, E)
    seg1 = torch.full((len(lens), Sx), -1, dtype=torch.int32)
    for r, row in enumerate(rows):
        for i, off in row:
            xp[r, off:off + lens[i]], dyp[r, off:off + lens[i]] = xs[i], dys[i]
    for i, n in enumerate(lens):
        xo[i, :n], dyo[i, :n], seg1[i, :n] = xs[i], dys[i], 0
    assert any(len(row) > 1 for row in rows)
    ws = R.make_weights(E, 10)
    kw = dict(causal=True, num_kv_heads=Hkv, bias=True, rotary=dict(max_positions=2 * Sx))
    packed = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, segment_ids=t[1], rope_position_ids=t[2], **kw)  # noqa: E731
    single = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, segment_ids=t[1], **kw)  # noqa: E731
    _, gp = R.layer_step(packed, [xp, torch.tensor(seg), torch.tensor(pos)], (1, 2), ws, dyp, "cpu", torch.float32)
    _, g1 = R.layer_step(single, [xo, seg1], (1,), ws, dyo, "cpu", torch.float32)
    places = [(r, i, off) for r, row in enumerate(rows) for i, off in row]
    for key in ("y", "dx0"):
        a = torch.cat([gp[key][r, off:off + lens[i]] for r, i, off in places])
        b = torch.cat([g1[key][i, :lens[i]] for r, i, off in places])
        _close(a, b, key)
    for key in gp:
        if key.startswith("d") and key != "dx0":
            _close(gp[key], g1[key], key)
    # the ids are read: ids twice as far apart change the scores (a shift of a whole sequence would not)
    _, gw = R.layer_step(packed, [xp, torch.tensor(seg), torch.tensor(2 * pos)], (1, 2), ws, dyp, "cpu", torch.float32)
    assert R.rel(gw["y"], gp["y"]) > 1e-2


# ------------------------------------------------------------------------------------ distributed
def test_two_ranks_match_one_process():
    """Two gloo ranks, split over the batch (every rank rotates by its rows of the ids) and over the heads
    (num_kv_heads = 2: one KV head per rank), against one process."""
    import rope_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("batch")
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"rope {case}@2")
    plain = A.single("plain")
    assert np.abs(plain["__output__"] - ref["__output__"]).max() > 1e-4


# ------------------------------------------------------------------------------------ example
@pytest.mark.parametrize("packed", [False, True])
def test_rope_decoder_example_learns(packed):
    """examples/python/native/rope_decoder.py --small [--packed] runs end to end in its own process on the CPU
    and its loss falls over a few steps."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", FF_TUNABLEOP="off")
    cmd = [sys.executable, os.path.join(root, "examples", "python", "native", "rope_decoder.py"), "--small", "-b", "4",
           "--iterations", "6"] + (["--packed"] if packed else [])
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("loss first")]
    assert line and "nan" not in r.stdout.lower(), r.stdout[-500:]
    first, last = float(line[0].split()[2]), float(line[0].split()[4])
    assert last < first - 0.1, line
    if packed:
        assert "fill ratio" in r.stdout
