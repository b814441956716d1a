"""Grouped-query and multi-query attention in the flash kernels, element by element against the float64
oracle of tests/attn_rows_common.py.

Query head h reads KV head h // G, G = H / Hkv. Inputs are attn_rows_common.make_inputs of the H-head
case with k[:, ::G] and v[:, ::G] as the KV tensors; the reference is reference() on those K / V repeated
G times (repeat_interleave over the heads), and

    dk_ref[hkv] = sum_g dk_ref[hkv G + g]                                        (dv likewise)
    tol_dk[hkv] = sum_g tol_dk[hkv G + g] + U |dk_ref[hkv]| + ACC sum_g |dk_ref[hkv G + g]|

Each query head's partial dK / dV is what the kernels computed before (its bound holds its own bf16
store); attn_kv_group_sum_kernel then adds the G partials in fp32 (the ACC term) and rounds once to bf16
(the U term). o, dq and lse keep their bounds unchanged. Every bound is applied at GPU_FACTOR; where it is
0 (dk / dv rows past a length, padding positions) the output must be an exact 0. Outputs sit between
sentinel rows and start as NaN, the inputs have NaN behind their last row, the workspace has a guard band.

Every case runs in the [B, S, heads, D] layout of the MultiHeadAttention projections ("bshd") and in the
[B, heads, S, D] layout of ScaledDotProductAttention ("bhsd"), with the forward structures 0, 1, 3 and the
backward structures 2, 10 as test_attn_rows_gpu.py selects them.

test_attn_gqa_cpu.py::test_the_grouping_is_observable shows on these inputs that the wrong map h % Hkv
lies outside these tolerances in o and in dk of every KV head.

Largest err / tolerance on an MI355X over both layouts and all structures (tolerance = 1.25 x bound; lse:
its own tolerance):

case              shape                              |   o    dv    dq    dk   lse
-----------------------------------------------------------------------------------
gqa_plain         S128 H4 Hkv2                       | 0.65  0.44  0.14  0.15  0.13
mqa_ragged        S200 H4 Hkv1                       | 0.59  0.35  0.14  0.10  0.13
gqa_cross         Sq577 Sk130 H4 Hkv2                | 0.61  0.35  0.17  0.06  0.14
gqa_two_blocks    S512 H4 Hkv2                       | 0.64  0.43  0.15  0.12  0.15
gqa_d128_causal   S320 D128 H4 Hkv2 causal           | 0.62  0.54  0.13  0.16  0.14
gqa_chain         B16 H16 Hkv4 S320                  | 0.72  0.46  0.19  0.13  0.14
gqa_chain_causal  B16 H16 Hkv4 S320 causal           | 0.68  0.65  0.27  0.27  0.12
gqa_lens          B5 H4 Hkv2 S320 lens5              | 0.67  0.47  0.16  0.18  0.14
gqa_drop          S200 H4 Hkv2 thr64                 | 0.67  0.48  0.19  0.12  0.15
gqa_bias          B2 H4 Hkv2 S128 bias full          | 0.63  0.51  0.14  0.14  0.13
gqa_seg           B2 H4 Hkv2 S320 segments           | 0.64  0.47  0.20  0.16  0.09
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

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL_O, TOL_G = 2e-2, 3e-2  # the sibling GPU op tests' relative Frobenius bounds


def _g(Hkv, Sq, Sk=None, H=4, **kw):
    return dict(R._c(Sq, Sk, H=H, **kw), Hkv=Hkv)


# the smallest shapes that reach each branch
CASES = {
    "gqa_plain": _g(2, 128),                                  # slab form, one key block
    "mqa_ragged": _g(1, 200),                                 # MQA, ragged
    "gqa_cross": _g(2, 577, 130),
    "gqa_two_blocks": _g(2, 512),                             # attn_fwd2_kernel; two key blocks + attn_dq_finish_kernel
    "gqa_d128_causal": _g(2, 320, D=128, causal=True),
    "gqa_chain": _g(4, 320, B=16, H=16),                      # chained form, attn_bwd1b_kernel
    "gqa_chain_causal": _g(4, 320, B=16, H=16, causal=True),
    "gqa_lens": _g(2, 320, B=5, lens=R.LENS5),
    "gqa_drop": _g(2, 200, thr=64),
    "gqa_bias": _g(2, 128, B=2, bias="full"),
    "gqa_seg": _g(2, 320, B=2, rows=R.SEG_ROWS),
}
LAYOUTS = ("bshd", "bhsd")


def gqa_inputs(name, c):
    """make_inputs of the H-head case with every group sharing its first head's K / V: `k` / `v` are the
    [B, Hkv, Sk, D] KV tensors, `k_rep` / `v_rep` their repeat over the groups (what the reference sees)."""
    inp = R.make_inputs(name, c)
    G = c["H"] // c["Hkv"]
    kv = {key: inp[key][:, ::G].contiguous() for key in ("k", "v")}
    return dict(inp, k=kv["k"], v=kv["v"], k_rep=kv["k"].repeat_interleave(G, 1), v_rep=kv["v"].repeat_interleave(G, 1))


def gqa_reference(c, inp, device):
    """Reference and tolerances of the module docstring: o, lse, dq as [B, H, ..], dk, dv as [B, Hkv, ..]."""
    ref, tol, fig = R.reference(dict(inp, k=inp["k_rep"], v=inp["v_rep"]), device)
    B, H, Hkv = c["B"], c["H"], c["Hkv"]
    for key in ("dk", "dv"):
        r = ref[key].unflatten(1, (Hkv, H // Hkv))
        t = tol[key].unflatten(1, (Hkv, H // Hkv))
        ref[key] = r.sum(2)
        tol[key] = t.sum(2) + R.U * ref[key].abs() + R.ACC * r.abs().sum(2)
    return ref, tol, fig


class Launcher:
    """attn_rows_common.Launcher for Hkv <= H KV heads and either layout; hkv_arg=False leaves the Hkv
    argument out of the calls (the passthrough test, Hkv == H)."""

    def __init__(self, ffC, c, inp, layout, hkv_arg=True):
        from flexflow_amd import kernels as K
        self.X, self.c, self.layout, self.scale = ffC, c, layout, inp["scale"]
        B, H, Hkv, Sq, Sk, D = (c[key] for key in ("B", "H", "Hkv", "Sq", "Sk", "D"))
        put = (lambda t: t.permute(0, 2, 1, 3)) if layout == "bshd" else (lambda t: t)
        self.q, self.k, self.v, self.do = (R._nan_tail(put(inp[key]), R.GUARD_ROWS, DEV) for key in ("q", "k", "v", "do"))
        if layout == "bshd":
            self.sq, self.sk = [Sq * H * D, D, H * D], [Sk * Hkv * D, D, Hkv * D]
        else:
            self.sq, self.sk = [H * Sq * D, Sq * D, D], [Hkv * Sk * D, Sk * D, D]
        self.kw = dict(Hkv=Hkv) if hkv_arg else {}
        if c["lens"] is not None:
            self.kw["key_lens"] = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
        if c["thr"]:
            self.kw.update(K._drop_kw((c["thr"], torch.tensor([R.DROP_STEP], dtype=torch.int64, device=DEV),
                                       K.attn_dropout_seed(R.DROP_SEED, R.DROP_LAYER), 0, 0, H)))
        if inp["bias"] is not None:
            bias = inp["bias"].to(DEV).contiguous()
            self.kw.update(sbias=bias, sbias_sb=H * Sq * Sk if bias.shape[0] > 1 else 0, sbias_sh=Sq * Sk)
        if c["rows"] is not None:
            from attn_segments_common import ids_of
            ids = torch.tensor(np.stack([ids_of(r, Sq) for r in c["rows"]]), dtype=torch.int32, device=DEV)
            lo, hi = torch.full_like(ids, -7), torch.full_like(ids, -7)
            ffC.attn_seg_bounds(ids, lo, hi)
            self.kw.update(seg_lo=lo, seg_hi=hi)

    def _bhsd(self, flat, heads, S):
        D = self.c["D"]
        if self.layout == "bshd":
            return flat.view(self.c["B"], S, heads, D).permute(0, 2, 1, 3)
        return flat.view(self.c["B"], heads, S, D)

    def fwd(self, variant):
        c, X = self.c, self.X
        B, H, Sq, Sk, D = (c[key] for key in ("B", "H", "Sq", "Sk", "D"))
        n = B * H * Sq
        obuf, o = R._guarded(n, D, torch.bfloat16, DEV)
        lbuf, lse = R._guarded(n, 1, torch.float32, DEV)
        prev = X.attn_fwd_variant()
        X.attn_set_fwd_variant(variant)
        try:
            X.attn_fwd(self.q, self.sq, self.k, self.sk, self.v, self.sk, o, self.sq, lse, B, H, Sq, Sk, D,
                       self.scale, c["causal"], **self.kw)
        finally:
            X.attn_set_fwd_variant(prev)
        assert R._guards_intact(obuf, n, D), "attn_fwd wrote outside o"
        assert R._guards_intact(lbuf, n, 1), "attn_fwd wrote outside lse"
        self.o, self.lse = o, lse
        return dict(o=self._bhsd(o, H, Sq), lse=lse.view(B, H, Sq))

    def grad_buffers(self):
        c = self.c
        return [R._guarded(c["B"] * heads * S, c["D"], torch.bfloat16, DEV)
                for heads, S in ((c["H"], c["Sq"]), (c["Hkv"], c["Sk"]), (c["Hkv"], c["Sk"]))]

    def bwd(self, variant, shift=0):
        """Backward of the last fwd(): dq [B, H, Sq, D], dk and dv [B, Hkv, Sk, D], and what attn_bwd returned.
        shift: dk and dv start that many elements into their NaN interior (shift * 2 bytes off 16-B alignment);
        the interior must then be one row longer than the gradient, and what lies outside stays NaN."""
        c, X = self.c, self.X
        B, H, Hkv, Sq, Sk, D = (c[key] for key in ("B", "H", "Hkv", "Sq", "Sk", "D"))
        nws = X.attn_bwd_ws(B, H, Sq, Sk, D, **({"Hkv": Hkv} if "Hkv" in self.kw else {}))
        ws = torch.full((nws + 65536,), R.SENT, device=DEV)
        (qb, dq), (kb, dk), (vb, dv) = self.grad_buffers()
        if shift:
            nkv = B * Hkv * Sk * D
            (kb, kin), (vb, vin) = (R._guarded(B * Hkv * Sk + 1, D, torch.bfloat16, DEV) for _ in range(2))
            dk, dv = kin[shift:shift + nkv], vin[shift:shift + nkv]
        prev = X.attn_bwd_variant()
        X.attn_set_bwd_variant(variant)
        try:
            done = X.attn_bwd(self.q, self.sq, self.k, self.sk, self.v, self.sk, self.o, self.sq, self.do, self.sq,
                              self.lse, dq, self.sq, dk, self.sk, dv, self.sk, ws[:nws], B, H, Sq, Sk, D,
                              self.scale, c["causal"], **self.kw)
        finally:
            X.attn_set_bwd_variant(prev)
        assert bool((ws[nws:] == R.SENT).all()), "attn_bwd wrote past its workspace"
        extra = 1 if shift else 0
        for buf, n in ((qb, B * H * Sq), (kb, B * Hkv * Sk + extra), (vb, B * Hkv * Sk + extra)):
            assert R._guards_intact(buf, n, D), "attn_bwd wrote outside dq / dk / dv"
        if shift:
            for inner in (kin, vin):
                assert torch.isnan(inner[:shift]).all() and torch.isnan(inner[shift + nkv:]).all(), "wrote outside dk / dv"
        return dict(dq=self._bhsd(dq, H, Sq), dk=self._bhsd(dk, Hkv, Sk), dv=self._bhsd(dv, Hkv, Sk)), bool(done)


_cache = {}


def _case(ffC, name, layout):
    """The case on the device in one layout; its inputs, float64 reference and tolerances are built once."""
    if name not in _cache:
        c = dict(R.full_case(CASES[name]))
        inp = gqa_inputs(name, c)
        _cache[name] = (c, inp) + gqa_reference(c, inp, DEV)
    c, inp, ref, tol, fig = _cache[name]
    if (name, layout) not in _cache:
        _cache[name, layout] = Launcher(ffC, c, inp, layout)
    return c, _cache[name, layout], ref, tol, fig


def _verdict(tag, res):
    print(f"GQA-GPU {tag} {R.ratios(res)}")
    assert not R.fails(res), R.fails(res)


@pytest.mark.parametrize("fv", [0, 1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_rows(ffC, name, layout, fv):
    """o and lse of forward structure fv with Hkv < H KV heads: every element within its unchanged bound."""
    c, L, ref, tol, fig = _case(ffC, name, layout)
    got = L.fwd(fv)
    _verdict(f"{name} {layout} fwd={fv}", R.check(got, ref, tol, R.GPU_FACTOR))


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_backward_rows(ffC, name, layout, variant):
    """dq per query head and dk / dv per KV head (the group sums) of backward structure `variant` after
    the default forward; no fused bias gradient."""
    c, L, ref, tol, _ = _case(ffC, name, layout)
    L.fwd(ffC.attn_fwd_variant())
    got, done = L.bwd(variant)
    assert not done
    _verdict(f"{name} {layout} bwd={variant}", R.check(got, ref, tol, R.GPU_FACTOR))


@pytest.mark.parametrize("name", ["gqa_chain", "gqa_chain_causal"])
def test_dbias_is_declined_and_left_alone(ffC, name):
    """kernels.flash_attn_bwd with a dbias tensor on the chained GQA case: it returns False, the tensor is
    untouched, and the gradients are those of the call without it."""
    from flexflow_amd import kernels as K
    c, L, ref, tol, _ = _case(ffC, name, "bshd")
    B, H, Hkv, Sq, Sk, D = (c[key] for key in ("B", "H", "Hkv", "Sq", "Sk", "D"))
    L.fwd(ffC.attn_fwd_variant())
    (_, dq), (_, dk), (_, dv) = L.grad_buffers()
    dbias = torch.full((3 * H * D,), 0.5, device=DEV)
    done = K.flash_attn_bwd(L.q, L.sq, L.k, L.sk, L.v, L.sk, L.o, L.sq, L.do, L.sq, L.lse, dq, L.sq, dk, L.sk, dv, L.sk,
                            B, H, Sq, Sk, D, L.scale, c["causal"], dbias=dbias, Hkv=Hkv)
    assert done is False
    assert torch.equal(dbias, torch.full_like(dbias, 0.5))
    got = dict(dq=L._bhsd(dq, H, Sq), dk=L._bhsd(dk, Hkv, Sk), dv=L._bhsd(dv, Hkv, Sk))
    _verdict(f"{name} dbias", R.check(got, ref, tol, R.GPU_FACTOR))


@pytest.mark.parametrize("name", ["plain", "chain_s320"])
@pytest.mark.parametrize("variant", [2, 10])
def test_hkv_equal_h_is_the_call_without_it(ffC, name, variant):
    """Hkv = H gives o, lse, dq, dk and dv bit-identical to the call without the argument (S 128 and the
    B 16, H 16, S 320 case of attn_rows_common)."""
    c = dict(R.full_case(R.CASES[name]))
    c["Hkv"] = c["H"]
    inp = R.make_inputs(name, c)
    outs = []
    for hkv_arg in (False, True):
        L = Launcher(ffC, c, inp, "bhsd", hkv_arg=hkv_arg)
        got = L.fwd(ffC.attn_fwd_variant())
        got.update(L.bwd(variant)[0])
        outs.append(got)
    for key in ("o", "lse", "dq", "dk", "dv"):
        a, b = outs[0][key], outs[1][key]
        assert not torch.isnan(a.float()).any(), key
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), key


@pytest.mark.parametrize("variant", [2, 10])
def test_backward_is_deterministic(ffC, variant):
    """Two backward runs of the chained GQA case give equal bits (the group sum has no atomics)."""
    c, L, _, _, _ = _case(ffC, "gqa_chain", "bshd")
    L.fwd(ffC.attn_fwd_variant())
    a, _ = L.bwd(variant)
    a = {key: t.clone() for key, t in a.items()}
    b, _ = L.bwd(variant)
    for key in a:
        assert torch.equal(a[key].contiguous().view(torch.int16), b[key].contiguous().view(torch.int16)), key


@pytest.mark.parametrize("name", ["gqa_plain", "gqa_lens"])
def test_group_sum_without_16_byte_stores(ffC, name):
    """dk / dv 8 bytes off 16-byte alignment: attn_kv_group_sum_kernel takes its 2-byte stores and gives the
    bits of the aligned call, within its bounds, nothing written outside."""
    c, L, ref, tol, _ = _case(ffC, name, "bhsd")
    L.fwd(ffC.attn_fwd_variant())
    a, _ = L.bwd(10)
    b, _ = L.bwd(10, shift=4)
    _verdict(f"{name} shift=4", R.check(b, ref, tol, R.GPU_FACTOR))
    for key in ("dq", "dk", "dv"):
        assert torch.equal(a[key].contiguous().view(torch.int16), b[key].contiguous().view(torch.int16)), key


def test_arguments_are_checked(ffC):
    c, L, _, _, _ = _case(ffC, "gqa_plain", "bhsd")
    B, H, Sq, Sk, D = (c[key] for key in ("B", "H", "Sq", "Sk", "D"))
    o = torch.empty(B * H * Sq * D, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * H * Sq, device=DEV)
    with pytest.raises(RuntimeError):  # 3 does not divide 4
        ffC.attn_fwd(L.q, L.sq, L.k, L.sk, L.v, L.sk, o, L.sq, lse, B, H, Sq, Sk, D, L.scale, False, Hkv=3)
    short = L.k[:Sk * D]  # one KV head where the strides address two
    with pytest.raises(RuntimeError):
        ffC.attn_fwd(L.q, L.sq, short, L.sk, L.v, L.sk, o, L.sq, lse, B, H, Sq, Sk, D, L.scale, False, Hkv=2)
    assert ffC.attn_bwd_ws(B, H, Sq, Sk, D) == ffC.attn_bwd_ws(B, H, Sq, Sk, D, H)
    assert ffC.attn_bwd_ws(B, H, Sq, Sk, D, 2) >= ffC.attn_bwd_ws(B, H, Sq, Sk, D) + B * H * Sk * D


# ------------------------------------------------------------------------------------- op level
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _step(build, inputs, ws, dy, device, dtype):
    """One training step (forward, backward) of a layer through OpCtx on `device`: y, input and weight gradients."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    ff = FFModel(FFConfig([]))
    ts = [ff.create_tensor(list(x.shape), DataType.DT_FLOAT) for x in inputs]
    L = build(ff, ts).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    xs = [x.to(device, dtype) for x in inputs]
    slot = [next(i for i, t in enumerate(ts) if t is u) for u in L.inputs]
    w = [t.to(device, dtype) for t in ws(L)]
    ctx.wgrads = [torch.zeros(t.shape, device=device) for t in w]
    y = L.impl.forward(ctx, [xs[i] for i in slot], w)[0]
    dslot = L.impl.backward(ctx, [dy.to(device, dtype)])
    dxs = [None] * len(inputs)
    for i, d in zip(slot, dslot):
        if d is not None:
            dxs[i] = d if dxs[i] is None else dxs[i] + d
    return L, [y] + dxs + ctx.wgrads


@pytest.mark.parametrize("D", [64, 32])
def test_mha_op_bf16_gqa(ffC, D):
    """One training step of multihead_attention(num_kv_heads=2) with H = 4, S = 128 on the device in bf16
    (head dim 64: the flash kernels; 32: zero-padded to 64) against the same layer on the CPU reference path."""
    B, S, H, Hkv = 2, 128, 4, 2
    E = H * D
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, S, E, generator=g).bfloat16().float()
    dy = torch.randn(B, S, E, generator=g).bfloat16().float()
    store = {}

    def ws(L):
        if "w" not in store:
            store["w"] = [(torch.randn(w.dims, generator=g) / math.sqrt(E)).bfloat16().float() for w in L.weights]
        return store["w"]

    build = lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, num_kv_heads=Hkv)  # noqa: E731
    L, got = _step(build, [x], ws, dy, DEV, torch.bfloat16)
    assert not L.attrs["fused_qkv"] and [tuple(w.dims)[0] for w in L.weights[:3]] == [H, Hkv, Hkv]
    torch.cuda.synchronize()
    _, want = _step(build, [x], ws, dy, "cpu", torch.float32)
    names = ["y", "dx"] + ["d" + w.short_name for w in L.weights]
    got, want = dict(zip(names, got)), dict(zip(names, want))
    # the K bias shifts every score of a row alike, so its gradient is 0 but for rounding and has no relative
    # error of its own: the three projection biases are measured as one tensor, as the sibling tests' fused
    # qkv_bias gradient is
    for d in (got, want):
        d["dqkv_bias"] = torch.cat([d.pop(n).reshape(-1).float().cpu() for n in ("dq_bias", "dk_bias", "dv_bias")])
    errs = {n: _rel(got[n], want[n]) for n in got}
    got = list(got.values())
    print("mha gqa relative errors", D, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(torch.isfinite(t).all() for t in got)
    assert errs.pop("y") < TOL_O and all(e < TOL_G for e in errs.values()), errs


@pytest.mark.parametrize("Hkv", [2, 1])
def test_sdpa_op_fp32_device_gqa(ffC, Hkv):
    """The fp32 device path (f32 MFMA GEMMs on K / V expanded per sample, the gradients summed per group)
    against the CPU reference path, at the 1e-4 of the sibling fp32 device tests; cross shapes, key lengths."""
    B, H, Sq, Sk, D = 3, 4, 96, 136, 32
    g = torch.Generator().manual_seed(23)
    q, do = (torch.randn(B, H, Sq, D, generator=g) for _ in range(2))
    k, v = (torch.randn(B, Hkv, Sk, D, generator=g) for _ in range(2))
    lens = torch.tensor([136, 64, 1], dtype=torch.int32)

    def run(device):
        from flexflow_amd.core import DataType, FFConfig, FFModel
        from flexflow_amd.ops import OpCtx
        ff = FFModel(FFConfig([]))
        ts = [ff.create_tensor(list(t.shape), DataType.DT_FLOAT) for t in (q, k, v)]
        tl = ff.create_tensor([B], DataType.DT_INT32)
        L = ff.scaled_dot_product_attention(*ts, key_lengths=tl, enable_gqa=True).owner_layer
        n = len(L.impl.axis_sizes())
        ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
        o = L.impl.forward(ctx, [t.to(device) for t in (q, k, v, lens)], [])[0]
        if device != "cpu":
            assert "P" in ctx.saved  # the fp32 device kernels ran, not the reference
        return [o] + L.impl.backward(ctx, [do.to(device)])[:3]

    got, want = run(DEV), run("cpu")
    torch.cuda.synchronize()
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv"), got, want)}
    print("sdpa gqa fp32 relative errors", Hkv, errs)
    assert got[2].shape == k.shape and all(e < 1e-4 for e in errs.values()), errs


@pytest.mark.parametrize("D", [64, 32])
def test_sdpa_op_bf16_gqa(ffC, D):
    """One training step of scaled_dot_product_attention(enable_gqa=True), q [2, 4, 128, D], k / v [2, 2, 128,
    D], causal, on the device in bf16 against the CPU reference path; dk / dv come back in the K / V shapes."""
    B, S, H, Hkv = 2, 128, 4, 2
    g = torch.Generator().manual_seed(22)
    q, do = (torch.randn(B, H, S, D, generator=g).bfloat16().float() for _ in range(2))
    k, v = (torch.randn(B, Hkv, S, D, generator=g).bfloat16().float() for _ in range(2))
    build = lambda ff, t: ff.scaled_dot_product_attention(t[0], t[1], t[2], causal=True, enable_gqa=True)  # noqa: E731
    _, got = _step(build, [q, k, v], lambda L: [], do, DEV, torch.bfloat16)
    torch.cuda.synchronize()
    _, want = _step(build, [q, k, v], lambda L: [], do, "cpu", torch.float32)
    assert got[2].shape == k.shape and got[3].shape == v.shape
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv"), got, want)}
    print("sdpa gqa relative errors", D, {k_: f"{e:.2e}" for k_, e in errs.items()})
    assert errs.pop("o") < TOL_O and all(e < TOL_G for e in errs.values()), errs
