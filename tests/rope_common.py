"""Shared by test_rope_cpu.py and test_rope_gpu.py: the rotary kernel's cases, a float64 oracle written
from the definition, the derived per-element bound, and a runner that calls kernels.rope on guarded buffers
(on the CPU that is the plain-torch reference path, on a GPU the HIP kernel).

Oracle: theta[p][i] = (p / scale) * inv_freq[i], inv_freq[i] = base^(-2i / rd) in float64 (or the explicit
list), applied to the exact stored input values: y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin over the pairs
(i, i + rd/2) (half-split) or (2i, 2i + 1) (interleaved); `inverse` negates sin. Ids are clamped to
[0, max_positions - 1].

Bound per element, derived and not tuned:  tol = u |ref| + 4 * 2^-24 (|x1 c| + |x2 s|)  with u = 2^-8 for
bf16 storage (round to nearest: half an ulp of 2^-7) and 2^-24 for fp32. The second term covers the
table's rounding to fp32, the two products and the sum. Where tol is 0 (both inputs of the pair are zero)
the result must equal the reference exactly (a rotated zero may carry either sign, so this is a value
comparison); columns [rd, D) and every buffer the launch must not touch are compared bit for bit.
"""
import math

import torch

from flexflow_amd import kernels as K

U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
F32 = 2.0 ** -24
GUARD = 512  # elements of sentinel in front of / NaN behind every buffer (a multiple of 16 bytes)
SENT = 7.0


def _c(B=2, Sq=67, Sk=None, H=3, Hkv=None, D=64, rd=None, layout="bshd", interleaved=False, ids=None, maxp=None,
       scale=1.0, inv_freq=None, base=10000.0, out_of_place=False, k=True):
    Sk = Sq if Sk is None else Sk
    return dict(B=B, Sq=Sq, Sk=Sk, H=H, Hkv=H if Hkv is None else Hkv, D=D, rd=D if rd is None else rd, layout=layout,
                interleaved=interleaved, ids=ids, maxp=maxp or max(Sq, Sk), scale=scale, inv_freq=inv_freq, base=base,
                out_of_place=out_of_place, k=k)


# the smallest shapes that reach each branch of rope.hip (S = 67 tokens x chunks is no multiple of a block)
CASES = {
    "plain": _c(B=1, Sq=5, H=2, Hkv=2),  # less than one block: the tail
    "fused_layout": _c(layout="fused"),  # Q and K thirds of [T, 3, H, D] in one launch, V untouched
    "gqa": _c(H=4, Hkv=1, D=128),
    "bhsd": _c(layout="bhsd"),
    "partial": _c(rd=32),
    "scalar_path": _c(D=80, rd=20),  # rd / 2 = 10 is no multiple of a 16-byte vector
    "scalar_path_interleaved": _c(D=20, rd=20, interleaved=True),  # strides of 20 elements
    "interleaved": _c(interleaved=True),
    "many_heads": _c(B=1, Sq=9, H=9, Hkv=2),  # 11 head rows: more than one lane's share, and its tail
    "cross": _c(Sq=33, Sk=70),
    "ids": _c(B=3, Sq=40, ids="restarts", maxp=4096),
    "ids_out_of_range": _c(B=3, Sq=40, ids="out_of_range", maxp=50),
    "scaled": _c(scale=4.0),
    "inv_freq": _c(rd=32, inv_freq=[1.0 / (1.7 ** i) for i in range(16)]),
    "out_of_place": _c(layout="bhsd", rd=32, out_of_place=True, k=False),
    "out_of_place_odd_tail": _c(layout="bhsd", D=76, rd=64, out_of_place=True, k=False),  # 12 pass-through columns
}


def make_ids(c):
    B, S, maxp = c["B"], c["Sq"], c["maxp"]
    if c["ids"] is None:
        return None
    ids = torch.arange(S, dtype=torch.int32).repeat(B, 1)
    if c["ids"] == "restarts":  # packed rows: positions restart; a row of zeros; the table's last entry, where
        ids[0, 17:] = torch.arange(S - 17, dtype=torch.int32)  # fp32 angle arithmetic would be off by ~2e-4
        ids[1] = 0
        ids[2, 5:] = torch.arange(maxp - (S - 5), maxp, dtype=torch.int32)
        assert int(ids.max()) == maxp - 1
    else:
        ids[0, 3], ids[1, 7], ids[2, 0] = -3, maxp + 5, 2 ** 31 - 1
    return ids


def _layout(c, which):
    """(flat element count, (batch, head, row) strides, offset of this tensor in its buffer)."""
    B, D = c["B"], c["D"]
    H, S = (c["H"], c["Sq"]) if which == "q" else (c["Hkv"], c["Sk"])
    if c["layout"] == "fused":
        assert c["H"] == c["Hkv"] and c["Sq"] == c["Sk"]
        return B * S * 3 * H * D, [S * 3 * H * D, D, 3 * H * D], (0 if which == "q" else H * D)
    if c["layout"] == "bhsd":
        return B * H * S * D, [H * S * D, S * D, D], 0
    return B * S * H * D, [S * H * D, D, H * D], 0


def view4(flat, st, B, H, S, D):
    return flat.as_strided((B, H, S, D), (st[0], st[1], st[2], 1), flat.storage_offset())


def make_inputs(name, c, dtype):
    """Random stored values in the case's layout; some pairs are zeroed (tol = 0 there)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n, qs, _ = _layout(c, "q")
    bufs = {"q": torch.randn(n, generator=g).to(dtype)}
    if c["k"] and c["layout"] != "fused":
        bufs["k"] = torch.randn(_layout(c, "k")[0], generator=g).to(dtype)
    q4 = view4(bufs["q"], qs, c["B"], c["H"], c["Sq"], c["D"])
    q4[:, 0, 1::7, :] = 0  # zero rows
    return bufs


def inv_freq64(c):
    if c["inv_freq"] is not None:
        return torch.tensor(c["inv_freq"], dtype=torch.float64)
    return c["base"] ** (-torch.arange(0, c["rd"], 2, dtype=torch.float64) / c["rd"])


def oracle(x4, c, ids, u, inverse=False, interleaved=None):
    """(ref, tol) float64 [B, H, S, D] of the stored values x4 rotated by the definition."""
    B, H, S_, D = x4.shape
    rd, half = c["rd"], c["rd"] // 2
    inter = c["interleaved"] if interleaved is None else interleaved
    p = (torch.arange(S_).repeat(B, 1) if ids is None else ids.long()).clamp(0, c["maxp"] - 1).double()
    ang = (p / c["scale"])[:, :, None] * inv_freq64(c)[None, None, :]  # [B, S, half]
    cs, sn = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
    if inverse:
        sn = -sn
    x = x4.double()
    ref, mag = x.clone(), torch.zeros_like(x)
    i1, i2 = (slice(0, rd, 2), slice(1, rd, 2)) if inter else (slice(0, half), slice(half, rd))
    x1, x2 = x[..., i1], x[..., i2]
    ref[..., i1], ref[..., i2] = x1 * cs - x2 * sn, x2 * cs + x1 * sn
    mag[..., i1] = (x1 * cs).abs() + (x2 * sn).abs()
    mag[..., i2] = (x2 * cs).abs() + (x1 * sn).abs()
    return ref, u * ref.abs() + 4 * F32 * mag


def _guarded(data, dev):
    """[sentinel | data | NaN] on `dev`, the data region as a flat view."""
    buf = torch.cat([torch.full((GUARD,), SENT, dtype=data.dtype), data,
                     torch.full((GUARD,), float("nan"), dtype=data.dtype)]).to(dev)
    return buf, buf[GUARD:]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def guards_intact(buf, n):
    head, tail = buf[:GUARD].cpu(), buf[GUARD + n:].cpu()
    return bool((head == SENT).all()) and bool(torch.isnan(tail).all()) and tail.numel() == GUARD


def run(name, c, dtype, device, inverse=False, inputs=None):
    """The case through kernels.rope: per tensor (got [B, H, S, D] on the CPU, stored input x4, ids) plus
    the list of integrity failures (guards, untouched buffers, pass-through bits)."""
    dev = torch.device(device)
    bufs = inputs if inputs is not None else make_inputs(name, c, dtype)
    ids = make_ids(c)
    table = K.rope_table(c["rd"], c["maxp"], c["base"], c["scale"], c["inv_freq"], dev)
    B, H, Hkv, Sq, Sk, D, rd = (c[k] for k in ("B", "H", "Hkv", "Sq", "Sk", "D", "rd"))
    nq, qs, _ = _layout(c, "q")
    nk, ks, koff = _layout(c, "k")
    qbuf, qflat = _guarded(bufs["q"], dev)
    if not c["k"]:
        kflat = kbuf = None
    elif c["layout"] == "fused":
        kbuf, kflat = qbuf, qflat[koff:]
    else:
        kbuf, kflat = _guarded(bufs["k"], dev)
    bad = []
    outs = {}
    pos = None if ids is None else ids.to(dev)
    if c["out_of_place"]:
        obuf = torch.cat([torch.full((GUARD,), SENT, dtype=dtype), torch.full((nq,), float("nan"), dtype=dtype),
                          torch.full((GUARD,), SENT, dtype=dtype)]).to(dev)
        K.rope(qflat, qs, None, None, B, H, 0, Sq, 0, D, rd, table, pos=pos, interleaved=c["interleaved"],
               inverse=inverse, q_out=obuf[GUARD:])
        o = obuf.cpu()
        if not (bool((o[:GUARD] == SENT).all()) and bool((o[GUARD + nq:] == SENT).all())):
            bad.append("output sentinels overwritten")
        if not torch.equal(_bits(qbuf.cpu()[GUARD:GUARD + nq]), _bits(bufs["q"])):
            bad.append("out of place: the input changed")
        outs["q"] = view4(o[GUARD:GUARD + nq], qs, B, H, Sq, D)
    else:
        K.rope(qflat, qs, kflat, ks, B, H, Hkv, Sq, Sk, D, rd, table, pos=pos, interleaved=c["interleaved"],
               inverse=inverse)
        outs["q"] = view4(qbuf.cpu()[GUARD:GUARD + nq], qs, B, H, Sq, D)
        if c["k"]:
            kc = kbuf.cpu()
            outs["k"] = view4(kc[GUARD + (koff if c["layout"] == "fused" else 0):GUARD + (nq if c["layout"] == "fused" else nk)],
                              ks, B, Hkv, Sk, D)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for nm, b, n in (("q", qbuf, nq),) + ((("k", kbuf, nk),) if c["k"] and c["layout"] != "fused" else ()):
        if not guards_intact(b, n):
            bad.append(f"{nm}: guard rows changed")
    res = {}
    for nm in outs:
        src = bufs["q"] if (nm == "q" or c["layout"] == "fused") else bufs["k"]
        H_, S_ = (H, Sq) if nm == "q" else (Hkv, Sk)
        st = qs if nm == "q" else ks
        x4 = view4(src[(koff if nm == "k" and c["layout"] == "fused" else 0):], st, B, H_, S_, D)
        res[nm] = (outs[nm], x4, ids)
        if rd < D and not torch.equal(_bits(outs[nm][..., rd:]), _bits(x4[..., rd:])):
            bad.append(f"{nm}: pass-through columns differ in bits")
    if c["layout"] == "fused":  # the V third of every token
        got = qbuf.cpu()[GUARD:GUARD + nq].view(B * Sq, 3, H, D)[:, 2]
        if not torch.equal(_bits(got), _bits(bufs["q"].view(B * Sq, 3, H, D)[:, 2])):
            bad.append("fused: the V third changed")
    return res, bad


def check(got, ref, tol):
    """(number of elements outside the bound, largest |got - ref| / tol over elements with tol > 0)."""
    err = (got.double() - ref).abs()
    miss = int((~(err <= tol)).sum())  # NaN counts as a miss
    pos = tol > 0
    worst = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    return miss, worst


def check_case(name, dtype, device, inverse=False):
    """Asserts the case; returns the worst ratio to the bound."""
    c = CASES[name]
    res, bad = run(name, c, dtype, device, inverse)
    assert not bad, (name, bad)
    worst = 0.0
    for nm, (got, x4, ids) in res.items():
        ref, tol = oracle(x4, c, ids, U[dtype], inverse)
        miss, w = check(got, ref, tol)
        print(f"rope {name} {nm} {dtype} inverse={inverse}: {miss} of {got.numel()} outside, worst ratio {w:.3f}")
        assert miss == 0, (name, nm, miss, w)
        worst = max(worst, w)
    return worst


def pair_norm(x4, c):
    """|x| of the rotated 2-vector every element belongs to (its own magnitude behind column rd)."""
    rd, half = c["rd"], c["rd"] // 2
    x = x4.double()
    n = x.abs().clone()
    i1, i2 = (slice(0, rd, 2), slice(1, rd, 2)) if c["interleaved"] else (slice(0, half), slice(half, rd))
    n[..., i1] = n[..., i2] = torch.sqrt(x[..., i1] ** 2 + x[..., i2] ** 2)
    return n


def round_trip(name, dtype, device):
    """inverse(forward(x)) against x within 2 u |x|, |x| the norm of the pair (x1, x2) that is rotated: each of
    the two launches rounds a component of a vector of that norm once (u |x| each; a rotation keeps the
    norm of the first launch's error). An element-wise |x| could not hold: a small x1 beside a large x2
    comes back with the large one's rounding error. Returns the worst ratio to the bound."""
    c = CASES[name]
    bufs = make_inputs(name, c, dtype)
    res, bad = run(name, c, dtype, device, False, inputs={k: v.clone() for k, v in bufs.items()})
    assert not bad, bad
    mid = {k: v.clone() for k, v in bufs.items()}  # the rotated buffers become the inverse launch's inputs
    for nm, (got, _, _) in res.items():
        fused_k = nm == "k" and c["layout"] == "fused"
        H_, S_ = (c["H"], c["Sq"]) if nm == "q" else (c["Hkv"], c["Sk"])
        _, st, off = _layout(c, nm)
        view4(mid["q" if fused_k else nm][off:], st, c["B"], H_, S_, c["D"]).copy_(got)
    back, bad = run(name, c, dtype, device, True, inputs=mid)
    assert not bad, bad
    worst = 0.0
    for nm, (got, _, _) in back.items():
        x4 = res[nm][1]
        err = (got.double() - x4.double()).abs()
        lim = 2 * U[dtype] * pair_norm(x4, c)
        assert bool((err <= lim).all()), (name, nm, float((err - lim).max()))
        nz = lim > 0
        worst = max(worst, float((err[nz] / lim[nz]).max()))
    return worst


# ------------------------------------------------------------------------------------------ op level
TOL_O, TOL_G = 2e-2, 3e-2  # the sibling GPU op tests' relative Frobenius bounds (bf16 against fp32)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def rope_cfg(rd, S, **kw):
    """A CASES-style dict for `oracle` / `rotate` from a builder's rotary dict."""
    return _c(Sq=S, D=rd, rd=rd, interleaved=kw.get("interleaved", False), scale=kw.get("scale", 1.0),
              inv_freq=kw.get("inv_freq"), base=kw.get("base", 10000.0), maxp=kw.get("max_positions") or S)


def rotate(x, c, ids=None, rd=None):
    """Differentiable rotation of x [B, H, S, D] in x's dtype, from the definition (angles in float64)."""
    B, H, S, D = x.shape
    rd = c["rd"] if rd is None else rd
    half = rd // 2
    p = (torch.arange(S).repeat(B, 1) if ids is None else ids.long().cpu()).clamp(0, c["maxp"] - 1).double()
    ang = (p / c["scale"])[:, :, None] * inv_freq64(c)[None, None, :]
    cs, sn = (t[:, None].to(device=x.device, dtype=x.dtype) for t in (torch.cos(ang), torch.sin(ang)))
    xr, rest = x[..., :rd], x[..., rd:]
    if c["interleaved"]:
        x1, x2 = xr[..., 0::2], xr[..., 1::2]
        y = torch.stack((x1 * cs - x2 * sn, x2 * cs + x1 * sn), -1).flatten(-2)
    else:
        x1, x2 = xr[..., :half], xr[..., half:]
        y = torch.cat((x1 * cs - x2 * sn, x2 * cs + x1 * sn), -1)
    return torch.cat((y, rest), -1)


def mha_torch(xs, W, H, Hkv, c, ids, dy, dtype, causal=False, see=None):
    """Test-local torch multi-head attention with rotary q / k on the layer's weights W (name -> tensor),
    in `dtype` with autograd: {"y", "dx0".., "d<weight>"}. xs: [x] (self-attention) or [xq, xk, xv];
    see: optional bool [B, 1, Sq, Sk] mask (packed rows)."""
    xi = [x.to(dtype).requires_grad_() for x in xs]
    Wd = {n: w.to(dtype).requires_grad_() for n, w in W.items()}
    src = xi * 3 if len(xi) == 1 else xi
    B, Sq, Sk = src[0].shape[0], src[0].shape[1], src[1].shape[1]
    if "qkv_weight" in Wd:
        ws = [Wd["qkv_weight"][i] for i in range(3)]
        bs = [Wd["qkv_bias"][i] for i in range(3)] if "qkv_bias" in Wd else [None] * 3
    else:
        ws = [Wd[f"{n}_weight"] for n in "qkv"]
        bs = [Wd.get(f"{n}_bias") for n in "qkv"]
    heads = []
    for x, w, b in zip(src, ws, bs):
        y = x @ w.reshape(-1, w.shape[-1]).t()
        if b is not None:
            y = y + b.reshape(-1)
        heads.append(y.view(B, x.shape[1], w.shape[0], w.shape[1]).transpose(1, 2))
    q, k, v = heads
    kd = q.shape[-1]
    if c is not None:
        q, k = rotate(q, c, ids), rotate(k, c, ids)
    G = H // Hkv
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = q @ k.transpose(-1, -2) / math.sqrt(kd)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), float("-inf"))
    if see is not None:
        s = s.masked_fill(~see, float("-inf"))
    dead = torch.isneginf(s).all(-1, keepdim=True)
    p = torch.where(dead, torch.zeros_like(s), torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1))
    o = (p @ v).transpose(1, 2).reshape(B, Sq, -1)
    wo = Wd["o_weight"]
    y = o @ wo.reshape(wo.shape[0], -1).t()
    if "o_bias" in Wd:
        y = y + Wd["o_bias"]
    (y * dy.to(dtype)).sum().backward()
    out = {"y": y.detach()}
    for i, x in enumerate(xi):
        out[f"dx{i}"] = x.grad
    for n, w in Wd.items():
        out["d" + n] = w.grad
    return out


def layer_step(build, inputs, int_inputs, weights, dy, device, dtype):
    """One training forward and backward of a layer through OpCtx on `device` in `dtype`: the layer and
    {"y", "dx<i>", "d<weight>"}. weights(L) -> list of fp32 tensors (made once, shared between runs)."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    ff = FFModel(FFConfig([]))
    ts = [ff.create_tensor(list(x.shape), DataType.DT_INT32 if i in int_inputs else DataType.DT_FLOAT)
          for i, x in enumerate(inputs)]
    L = build(ff, ts).owner_layer
    n = len(L.impl.axis_sizes())
    ctx = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
    xs = [x.to(device) if i in int_inputs else x.to(device, dtype) for i, x in enumerate(inputs)]
    slot = [next(i for i, t in enumerate(ts) if t is u) for u in L.inputs]
    w = [t.to(device, dtype) for t in weights(L)]
    ctx.wgrads = [torch.zeros(t.shape, device=device) for t in w]
    y = L.impl.forward(ctx, [xs[i] for i in slot], w)[0]
    dslot = L.impl.backward(ctx, [dy.to(device, dtype)])
    out = {"y": y}
    for i, d in zip(slot, dslot):
        if d is not None:
            out[f"dx{i}"] = d if f"dx{i}" not in out else out[f"dx{i}"] + d
    for wt, gacc in zip(L.weights, ctx.wgrads):
        out["d" + wt.short_name] = gacc
    return L, out


def make_weights(E, seed):
    """weights(L) for layer_step: bf16-representable values, drawn once per test."""
    store = {}
    g = torch.Generator().manual_seed(seed)

    def ws(L):
        if "w" not in store:
            store["w"] = [(torch.randn(w.dims, generator=g) * (0.5 if w.short_name.endswith("bias") else 1 / math.sqrt(E)))
                          .bfloat16().float() for w in L.weights]
        return store["w"]
    return ws
