"""Shared by test_attn_rows_cpu.py and test_attn_rows_gpu.py: a float64 oracle of attention written
from its definition, per-element error bounds derived from the rounding steps of
csrc/kernels/attention.hip, an fp32 emulation of those steps, the case table, the inputs (peaked
softmax, hot padding, NaN / sentinel guards) and the launch helpers. Nothing here calls flexflow_amd
except the Python mirror of the dropout hash (kernels.attn_dropout_keep_ref) and, in the launch
helpers, the bindings under test.

Notation: P0 = softmax over the keys a query sees, P = P0 * keep * drop_scale (P = P0 without
dropout), s = scale, u = 2^-8 (bf16 round-to-nearest-even).

Rounding steps of the kernels (attention.hip): unnormalised p is packed to bf16 before the PV MFMA
(pack8 in the tile body of attn_fwd_kernel), the row sum is taken in fp32 from the unrounded p, o is
stored as bf16 (f2bf in the epilogue), delta is summed from the stored bf16 o (attn_bwd_pre_kernel),
the recomputed P is packed to bf16 for dV and dS is packed to bf16 for dQ / dK (pack8 in
attn_bwd_kernel), and dq / dk / dv are stored as bf16 (pack_bf2 / f2bf). Hence

    tol_o [i,d] = u ( sum_j P_ij |v_jd|  + |o_id| )
    eps_i       = sum_d tol_o[i,d] |dO_id|                     (error of delta_i)
    tol_dv[j,d] = u ( sum_i P_ij |dO_id| + |dv_jd| )
    e_ij        = u |dS_ij| + P_ij eps_i
    tol_dq[i,d] = s sum_j e_ij |k_jd| + u |dq_id|
    tol_dk[j,d] = s sum_i e_ij |q_id| + u |dk_jd|

One term was added to these after the CPU emulation exceeded them with dropout (dq at 1.47 x the bound
in case bias_drop, 0.70 in drop_d128): attention.hip:1116 forms
dS = P0 * ((keep ? dP * drop_scale : 0) - delta) with the UNDROPPED P0, so the error eps_i of delta_i
(attn_bwd_pre_kernel, attention.hip:652, sums it from the stored bf16 o) also enters where the
element was dropped and P_ij = 0:

    e_ij       += [keep_ij = 0] P0_ij eps_i

With it the emulation's dq stays below 0.31 x the bound in the dropout cases. Every tolerance gets
2^-12 of its absolute-sum term (sum P |v|, sum P |dO|, s sum |dS| |k|, s sum |dS| |q|) for the fp32
accumulation and the hardware exp2 / log2. Where a bound is 0 (rows past a length, padding positions,
rows that see no key) the comparison err <= tol demands an exact 0.
"""
import math
import zlib

import numpy as np
import torch

from attn_segments_common import mask_of

U = 2.0 ** -8
ACC = 2.0 ** -12
GPU_FACTOR = 1.25  # the GPU accumulates in another order than the emulation the bounds were tried on
INF = float("inf")
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
GUARD_ROWS = 256  # rows of NaN behind the inputs, of sentinel around the outputs
SENT = 7.0
DROP_SEED, DROP_LAYER, DROP_STEP = 1234, 77, 3
OUTS = ("o", "dq", "dk", "dv")


def pad_run(n):
    """A padding run of n positions in a packed row (attn_segments_common)."""
    return ("p", n)


SEG_ROWS = [[63, 1, 65, pad_run(2), 127, 62], [320]]  # run edges one key either side of 64 and 128; a row of one run
LENS5 = [320, 257, 256, 1, 0]  # edge, mid-tile, block edge, single key, empty sample


def _c(Sq, Sk=None, B=1, H=2, D=64, causal=False, lens=None, thr=0, bias=None, rows=None, fused=False, heads=None):
    """A case: bias is None, "bcast" ([1, H, Sq, Sk]) or "full" ([B, H, Sq, Sk]); rows are packed-row
    run lists per sample; heads are the (b, h) pairs the CPU test keeps of a B * H = 256 case."""
    return dict(B=B, H=H, Sq=Sq, Sk=Sq if Sk is None else Sk, D=D, causal=causal, lens=lens, thr=thr, bias=bias,
                rows=rows, fused=fused, heads=heads)


CASES = {
    "plain": _c(128),
    "ragged": _c(200),
    "causal": _c(192, causal=True),
    "two_blocks": _c(512),
    "cross": _c(577, 130),
    "causal_long": _c(576, causal=True),
    "d128": _c(128, D=128),
    "d128_causal": _c(200, D=128, causal=True),
    "d128_s320": _c(320, D=128),
    "chain_s320": _c(320, B=16, H=16, heads=[(0, 0), (15, 15)]),
    "chain_s320_causal": _c(320, B=16, H=16, causal=True, heads=[(0, 1), (15, 15)]),
    "chain_s512": _c(512, B=16, H=16, heads=[(3, 2), (15, 15)]),
    "chain_d128": _c(192, B=16, H=16, D=128, heads=[(0, 0), (15, 15)]),
    "fused_layout": _c(320, B=16, H=16, fused=True, heads=[(7, 9), (15, 15)]),
    "lens": _c(320, B=5, lens=LENS5),
    "lens_causal": _c(320, B=5, lens=LENS5, causal=True),
    "lens_d128": _c(200, B=3, D=128, lens=[200, 129, 64]),
    "chain_lens": _c(320, B=16, H=16, lens=[LENS5[b % 5] for b in range(16)], heads=[(0, 3), (1, 3), (12, 0), (8, 15), (4, 4)]),
    "drop_ragged": _c(200, thr=64),
    "drop_d128": _c(320, D=128, thr=64),
    "drop_chain": _c(320, B=16, H=16, thr=64, heads=[(0, 0), (15, 15)]),
    "bias_bcast": _c(200, 137, B=2, bias="bcast"),
    "bias_full": _c(256, B=2, D=128, causal=True, bias="full"),
    "bias_lens": _c(256, 320, B=2, bias="full", lens=[320, 65]),
    "bias_drop": _c(128, B=2, bias="full", thr=64),
    "seg": _c(320, B=2, rows=SEG_ROWS),
    "seg_causal": _c(320, B=2, rows=SEG_ROWS, causal=True),
    "seg_drop": _c(320, B=2, rows=SEG_ROWS, thr=64),
}


def cpu_case(c):
    """The case the CPU test runs: a B * H = 256 case cut to its listed heads, each a sample of one head
    (`origin` keeps the (b, h) it came from: its seed, its length and its dropout stream)."""
    if c["heads"] is None:
        return dict(c, origin=[(b, h) for b in range(c["B"]) for h in range(c["H"])], H_total=c["H"])
    hs = c["heads"]
    return dict(c, B=len(hs), H=1, origin=list(hs), H_total=c["H"],
                lens=None if c["lens"] is None else [c["lens"][b] for b, _ in hs],
                rows=None if c["rows"] is None else [c["rows"][b] for b, _ in hs])


def full_case(c):
    return dict(c, origin=[(b, h) for b in range(c["B"]) for h in range(c["H"])], H_total=c["H"])


# ---------------------------------------------------------------------------------------- inputs
def make_bias(name, c):
    """fp32 [Bb, H, Sq, Sk]: unit normal, -inf outside a band |i - j| <= 72 (shifted by 3 per sample), a
    -inf stripe of 7 key columns and three query rows wholly -inf."""
    if c["bias"] is None:
        return None
    Bb = c["B"] if c["bias"] == "full" else 1
    Sq, Sk = c["Sq"], c["Sk"]
    g = torch.Generator().manual_seed(zlib.crc32(("bias" + name).encode()))
    b = torch.randn(Bb, c["H"], Sq, Sk, generator=g)
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    for bb in range(Bb):
        b[bb].masked_fill_(((i - j - 3 * bb).abs() > 72)[None], -INF)
    b[:, :, :, 100:107] = -INF
    for r in (5, 64, Sq - 2):
        b[:, :, r] = -INF
    return b


def see_of(c, bias=None, diag=0, lens=None, rows=None):
    """bool numpy [B, H or 1, Sq, Sk]: query i of (b, h) sees key j. From the case description alone;
    diag / lens / rows override the causal diagonal (j <= i + diag), the lengths and the run lists."""
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    lens = c["lens"] if lens is None else lens
    rows = c["rows"] if rows is None else rows
    see = np.ones((B, 1, Sq, Sk), dtype=bool)
    if c["causal"]:
        see &= (np.arange(Sk)[None, :] <= np.arange(Sq)[:, None] + diag)[None, None]
    if lens is not None:
        for b in range(B):
            see[b, :, :, min(max(lens[b], 0), Sk):] = False
    if rows is not None:
        for b in range(B):
            see[b, 0] &= mask_of(rows[b], Sq)
    if bias is not None:
        see = see & ~np.isneginf(bias.numpy())
    return see


def _bf(t):
    return t.bfloat16()


def make_inputs(name, c):
    """CPU tensors of a case (cpu_case / full_case): q, k, v, do as bf16 [B, H, S, D], seeded per
    (case, origin head); bias; see; keep. q and k at 1.7 x a unit normal (scores of std ~3: a peaked
    softmax), v and dO unit normal. Hot padding: a key row no query sees gets k at 3 x and v = +-64, a
    query row that sees no key gets dO = +-64, all finite. Under a causal mask k leans towards its own
    query (below)."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    bias = make_bias(name, c)
    see = see_of(c, bias)
    q, k, v, do = (torch.empty(B, H, S, D) for S in (Sq, Sk, Sk, Sq))
    for g, (ob, oh) in enumerate(c["origin"]):
        b, h = divmod(g, H)
        gen = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * (ob * c["H_total"] + oh)) % (1 << 62))
        q[b, h] = 1.7 * torch.randn(Sq, D, generator=gen)
        k[b, h] = 1.7 * torch.randn(Sk, D, generator=gen)
        if c["causal"] and Sq == Sk:
            # under a causal mask the last key of a stretch is seen by few rows (key Sk - 1 by one row
            # alone): every key leans towards its own query, so the diagonal carries weight and a key
            # dropped or added at a boundary shows
            k[b, h] += 0.5 * q[b, h]
        v[b, h] = torch.randn(Sk, D, generator=gen)
        do[b, h] = torch.randn(Sq, D, generator=gen)
        khot = 3.0 * torch.randn(Sk, D, generator=gen)
        vhot = 128.0 * torch.randint(0, 2, (Sk, D), generator=gen) - 64.0
        dhot = 128.0 * torch.randint(0, 2, (Sq, D), generator=gen) - 64.0
        sm = torch.from_numpy(see[b, h if see.shape[1] > 1 else 0])
        unseen, blind = ~sm.any(0), ~sm.any(1)
        k[b, h][unseen] = khot[unseen]
        v[b, h][unseen] = vhot[unseen]
        do[b, h][blind] = dhot[blind]
    keep = None
    if c["thr"]:
        from flexflow_amd import kernels as K
        keep = torch.empty(B, H, Sq, Sk, dtype=torch.bool)
        for g, (ob, oh) in enumerate(c["origin"]):
            b, h = divmod(g, H)
            keep[b, h] = K.attn_dropout_keep_ref(DROP_SEED, DROP_LAYER, DROP_STEP, 1, 1, Sq, Sk, c["thr"] / 256.0,
                                                 b0=ob, h0=oh, H_total=c["H_total"])[0, 0]
    return dict(q=_bf(q), k=_bf(k), v=_bf(v), do=_bf(do), bias=bias, see=torch.from_numpy(see), keep=keep,
                scale=1.0 / math.sqrt(D), drop_scale=256.0 / (256 - c["thr"]))


# ---------------------------------------------------------------------------------------- oracle
def oracle(q, k, v, do, see, scale, bias=None, keep=None, drop_scale=1.0):
    """Attention from its definition in float64. q, do [G, Sq, D], k, v [G, Sk, D] (any float dtype), see
    bool [G or 1, Sq, Sk], bias fp32 [G or 1, Sq, Sk] or None, keep bool [G, Sq, Sk] or None. Returns o,
    lse, dq, dk, dv and the intermediates P0, P, dS, dP (dP is dO.V^T, the gradient of P). A row that sees
    no key: o = 0, lse = +inf, zero gradients."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = torch.einsum("gqd,gkd->gqk", q, k) * scale
    if bias is not None:
        s = s + torch.where(torch.isneginf(bias), torch.zeros_like(bias), bias).double()
    see = see.expand(s.shape)
    s = s.masked_fill(~see, -INF)
    live = see.any(-1)
    m = torch.where(live, s.amax(-1), torch.zeros_like(s[..., 0]))
    e = torch.exp(s - m[..., None])  # exp(-inf) = 0 exactly
    l = e.sum(-1)
    P0 = torch.where(live[..., None], e / torch.where(live, l, torch.ones_like(l))[..., None], torch.zeros_like(e))
    lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, INF))
    P = P0 if keep is None else torch.where(keep, P0 * drop_scale, torch.zeros_like(P0))
    o = torch.einsum("gqk,gkd->gqd", P, v)
    dP = torch.einsum("gqd,gkd->gqk", do, v)
    dP0 = dP if keep is None else torch.where(keep, dP * drop_scale, torch.zeros_like(dP))
    delta = (P0 * dP0).sum(-1)
    dS = P0 * (dP0 - delta[..., None])
    return dict(o=o, lse=lse, dq=torch.einsum("gqk,gkd->gqd", dS, k) * scale,
                dk=torch.einsum("gqk,gqd->gkd", dS, q) * scale, dv=torch.einsum("gqk,gqd->gkd", P, do),
                P0=P0, P=P, dS=dS, dP=dP)


def bounds(r, q, k, v, do, scale):
    """The per-element bounds of the module docstring (factor 1) from an oracle result r."""
    q, k, v, do = (t.double().abs() for t in (q, k, v, do))
    P, dS = r["P"], r["dS"].abs()
    a_o = torch.einsum("gqk,gkd->gqd", P, v)
    tol_o = U * (a_o + r["o"].abs()) + ACC * a_o
    eps = (tol_o * do).sum(-1)
    a_dv = torch.einsum("gqk,gqd->gkd", P, do)
    e = U * dS + (P + torch.where(P == 0, r["P0"], torch.zeros_like(P))) * eps[..., None]
    a_dq = torch.einsum("gqk,gkd->gqd", dS, k) * scale
    a_dk = torch.einsum("gqk,gqd->gkd", dS, q) * scale
    return dict(o=tol_o, dv=U * (a_dv + r["dv"].abs()) + ACC * a_dv,
                dq=scale * torch.einsum("gqk,gkd->gqd", e, k) + U * r["dq"].abs() + ACC * a_dq,
                dk=scale * torch.einsum("gqk,gqd->gkd", e, q) + U * r["dk"].abs() + ACC * a_dk)


def lse_fp32(q, k, see, scale, bias=None):
    """Plain fp32 torch.logsumexp of the masked scores; +inf for a row that sees no key."""
    s = torch.einsum("gqd,gkd->gqk", q.float(), k.float()) * scale
    if bias is not None:
        s = s + torch.where(torch.isneginf(bias), torch.zeros_like(bias), bias)
    see = see.expand(s.shape)
    live = see.any(-1)
    s = s.masked_fill(~see, -INF)
    s = torch.where(live[..., None], s, torch.zeros_like(s))
    return torch.where(live, torch.logsumexp(s, -1), torch.full_like(s[..., 0], INF))


def _flat(t, lo, hi, B, H):
    """Heads lo..hi-1 (flat b * H + h) of a [B or 1, H or 1, ...] tensor as [n or 1, ...]."""
    if t is None:
        return None
    if t.shape[0] == 1 and t.shape[1] == 1:
        return t[0]
    g = torch.arange(lo, hi, device=t.device)
    batch = g // H if t.shape[0] > 1 else torch.zeros_like(g)
    head = g % H if t.shape[1] > 1 else torch.zeros_like(g)
    return t[batch, head]


def reference(inp, device="cpu", chunk=16, **over):
    """Oracle, bounds and the lse tolerance of a whole case, evaluated on `device` in chunks of heads (an
    [Sq, Sk] float64 matrix per head is small, 256 of them at once are not). `over` replaces inputs
    (see, keep, bias, k, v): the boundary mutants. Returns ref and tol, dicts of [B, H, S, D] float64
    (lse: [B, H, Sq]) on the device, and lse_fig, the largest error of fp32 torch.logsumexp against the
    float64 lse: tol["lse"] = max(8 lse_fig, 2^-20 max(1, |lse|))."""
    x = dict(inp, **over)
    B, H = x["q"].shape[:2]
    G = B * H
    ref, tol, fig = {}, {}, 0.0
    dev = {key: (x[key].to(device) if x[key] is not None else None) for key in ("q", "k", "v", "do", "see", "bias", "keep")}
    parts = []
    for lo in range(0, G, chunk):
        hi = min(G, lo + chunk)
        q, k, v, do = (dev[key].flatten(0, 1)[lo:hi] for key in ("q", "k", "v", "do"))
        see, bias, keep = (_flat(dev[key], lo, hi, B, H) for key in ("see", "bias", "keep"))
        r = oracle(q, k, v, do, see, x["scale"], bias, keep, x["drop_scale"])
        t = bounds(r, q, k, v, do, x["scale"])
        l32 = lse_fp32(q, k, see, x["scale"], bias)
        fin = torch.isfinite(r["lse"])
        assert torch.equal(fin, torch.isfinite(l32))
        if fin.any():
            fig = max(fig, (l32.double() - r["lse"])[fin].abs().max().item())
        parts.append(({key: r[key] for key in OUTS + ("lse",)}, t))
    for key in OUTS + ("lse",):
        ref[key] = torch.cat([a[key] for a, _ in parts]).unflatten(0, (B, H))
    for key in OUTS:
        tol[key] = torch.cat([t[key] for _, t in parts]).unflatten(0, (B, H))
    tol["lse"] = torch.clamp(2.0 ** -20 * ref["lse"].abs().clamp(min=1.0), min=8 * fig)
    return ref, tol, fig


# --------------------------------------------------------------------------------------- checker
def check(got, ref, tol, factor):
    """Per element err <= factor * tol, NaN failing. `factor` scales the derived bounds only: lse is held
    to its measured tolerance as it stands, and lse = +inf must match exactly. Returns
    {output: (bad rows as bool [B, H, S], largest err / applied tolerance over elements where that is
    > 0, description of the worst failing element or None)}."""
    out = {}
    for key in got:
        g, r = got[key].double().to(ref[key].device), ref[key]
        t = tol[key] if key == "lse" else factor * tol[key]
        if key == "lse":
            inf = torch.isinf(r)
            ok = torch.where(inf, g == r, (g - r).abs() <= t)
            err = torch.where(inf, torch.zeros_like(r), (g - r).abs())
        else:
            err = (g - r).abs()
            ok = err <= t
        ratio = torch.where(t > 0, err / torch.where(t > 0, t, torch.ones_like(t)), torch.zeros_like(t))
        ratio = torch.nan_to_num(ratio, nan=INF)
        bad = ~ok
        what = None
        if bad.any():
            sc = torch.where(bad, torch.nan_to_num(err, nan=INF) / (t + 1e-300), torch.zeros_like(t))
            w = np.unravel_index(int(sc.argmax()), sc.shape)
            what = (f"{key}{list(w)}: got {g[w].item():.6g}, reference {r[w].item():.6g}, tolerance {t[w].item():.3g}; "
                    f"{int(bad.sum())} elements fail")
        out[key] = (bad if key == "lse" else bad.any(-1), ratio.max().item() if ratio.numel() else 0.0, what)
    return out


def fails(res):
    return {key: v[2] for key, v in res.items() if v[2] is not None}


def ratios(res):
    return " ".join(f"{key}={v[1]:.3f}" for key, v in res.items())


# ------------------------------------------------------------------------------------- emulation
def emulate(inp, see=None):
    """fp32 torch emulation of the kernels' rounding steps (module docstring), dropout and bias included:
    dict of o, dq, dk, dv (bf16) and lse (fp32) as [B, H, S, D] / [B, H, Sq]."""
    B, H = inp["q"].shape[:2]
    q, k, v, do = (inp[key].float().flatten(0, 1) for key in ("q", "k", "v", "do"))
    see = _flat(inp["see"] if see is None else see, 0, B * H, B, H)
    bias, keep = _flat(inp["bias"], 0, B * H, B, H), _flat(inp["keep"], 0, B * H, B, H)
    scale, ds = inp["scale"], inp["drop_scale"]
    t = torch.einsum("gqd,gkd->gqk", q, k) * (scale * LOG2E)
    if bias is not None:
        t = t + torch.where(torch.isneginf(bias), torch.zeros_like(bias), bias) * LOG2E
    see = see.expand(t.shape)
    live = see.any(-1)
    t = t.masked_fill(~see, -INF)
    m = torch.where(live, t.amax(-1), torch.zeros_like(t[..., 0]))
    pe = torch.exp2(t - m[..., None])
    lsum = pe.sum(-1)
    pd = pe if keep is None else torch.where(keep, pe, torch.zeros_like(pe))
    inv = torch.where(live, 1.0 / torch.where(live, lsum, torch.ones_like(lsum)), torch.zeros_like(lsum)) * ds
    o = (torch.einsum("gqk,gkd->gqd", pd.bfloat16().float(), v) * inv[..., None]).bfloat16()
    lse = torch.where(live, m * LN2 + torch.log(torch.where(live, lsum, torch.ones_like(lsum))), torch.full_like(m, INF))
    lse2 = torch.where(live, lse * LOG2E, torch.zeros_like(lse))
    P0 = torch.where(see, torch.exp2(t - lse2[..., None]), torch.zeros_like(t))
    delta = (o.float() * do).sum(-1)
    dP = torch.einsum("gqd,gkd->gqk", do, v)
    if keep is not None:
        dP = torch.where(keep, dP * ds, torch.zeros_like(dP))
    dS = (P0 * (dP - delta[..., None])).bfloat16().float()
    Pb = (P0 if keep is None else torch.where(keep, P0, torch.zeros_like(P0))).bfloat16().float()
    out = dict(o=o, lse=lse, dq=(torch.einsum("gqk,gkd->gqd", dS, k) * scale).bfloat16(),
               dk=(torch.einsum("gqk,gqd->gkd", dS, q) * scale).bfloat16(),
               dv=(torch.einsum("gqk,gqd->gkd", Pb, do) * ds).bfloat16())
    return {key: val.unflatten(0, (B, H)) for key, val in out.items()}


# -------------------------------------------------------------------------------- launch helpers
def _nan_tail(t, rows, dev):
    """t [.., D] flattened to rows of D inside a larger allocation whose last `rows` rows hold NaN."""
    D = t.shape[-1]
    buf = torch.full((t.numel() + rows * D,), float("nan"), dtype=t.dtype, device=dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf


def _guarded(n, D, dtype, dev):
    """n rows of D inside a sentinel-filled allocation, GUARD_ROWS rows before and after; the interior
    starts as NaN. Returns (buffer, interior view)."""
    buf = torch.full(((n + 2 * GUARD_ROWS) * D,), SENT, dtype=dtype, device=dev)
    view = buf[GUARD_ROWS * D:(GUARD_ROWS + n) * D]
    view.fill_(float("nan"))
    return buf, view


def _guards_intact(buf, n, D):
    g = GUARD_ROWS * D
    return bool((buf[:g] == SENT).all()) and bool((buf[g + n * D:] == SENT).all())


class Launcher:
    """A case on the device: inputs inside NaN-tailed allocations in [B, H, S, D] order, or as one fused
    [B, S, 3, H, D] buffer; every output inside a sentinel-guarded, NaN-filled allocation; a guard band
    behind the backward workspace."""

    def __init__(self, ffC, c, inp, dev="cuda"):
        from flexflow_amd import kernels as K
        self.X, self.c, self.dev, self.scale = ffC, c, dev, inp["scale"]
        B, H, Sq, Sk, D = (c[key] for key in ("B", "H", "Sq", "Sk", "D"))
        self.fused = c["fused"]
        if self.fused:
            qkv = torch.stack([inp[key].permute(0, 2, 1, 3) for key in ("q", "k", "v")], dim=2)  # [B, S, 3, H, D]
            base = _nan_tail(qkv, GUARD_ROWS, dev)
            self.q, self.k, self.v = base, base[H * D:], base[2 * H * D:]
            self.sq = self.sk = [Sq * 3 * H * D, D, 3 * H * D]
            self.so = [Sq * H * D, D, H * D]
            self.do = _nan_tail(inp["do"].permute(0, 2, 1, 3), GUARD_ROWS, dev)
        else:
            self.q, self.k, self.v, self.do = (_nan_tail(inp[key], GUARD_ROWS, dev) for key in ("q", "k", "v", "do"))
            self.sq = self.so = [H * Sq * D, Sq * D, D]
            self.sk = [H * Sk * D, Sk * D, D]
        self.kw = {}
        if c["lens"] is not None:
            self.kw["key_lens"] = torch.tensor(c["lens"], dtype=torch.int32, device=dev)
        if c["thr"]:
            self.kw.update(K._drop_kw((c["thr"], torch.tensor([DROP_STEP], dtype=torch.int64, device=dev),
                                       K.attn_dropout_seed(DROP_SEED, DROP_LAYER), 0, 0, H)))
        if inp["bias"] is not None:
            bias = inp["bias"].to(dev).contiguous()
            self.kw.update(sbias=bias, sbias_sb=H * Sq * Sk if bias.shape[0] > 1 else 0, sbias_sh=Sq * Sk)
        if c["rows"] is not None:
            from attn_segments_common import ids_of
            ids = torch.tensor(np.stack([ids_of(r, Sq) for r in c["rows"]]), dtype=torch.int32, device=dev)
            lo, hi = torch.full_like(ids, -7), torch.full_like(ids, -7)
            ffC.attn_seg_bounds(ids, lo, hi)
            self.kw.update(seg_lo=lo, seg_hi=hi)

    def _bhsd(self, flat, S):
        """An output interior as [B, H, S, D] whatever the layout."""
        c = self.c
        if self.fused:
            return flat.view(c["B"], S, c["H"], c["D"]).permute(0, 2, 1, 3)
        return flat.view(c["B"], c["H"], S, c["D"])

    def fwd(self, variant):
        c, X = self.c, self.X
        B, H, Sq, Sk, D = (c[key] for key in ("B", "H", "Sq", "Sk", "D"))
        n = B * H * Sq
        obuf, o = _guarded(n, D, torch.bfloat16, self.dev)
        lbuf, lse = _guarded(n, 1, torch.float32, self.dev)
        prev = X.attn_fwd_variant()
        X.attn_set_fwd_variant(variant)
        try:
            X.attn_fwd(self.q, self.sq, self.k, self.sk, self.v, self.sk, o, self.so, lse, B, H, Sq, Sk, D,
                       self.scale, c["causal"], **self.kw)
        finally:
            X.attn_set_fwd_variant(prev)
        assert _guards_intact(obuf, n, D), "attn_fwd wrote outside o"
        assert _guards_intact(lbuf, n, 1), "attn_fwd wrote outside lse"
        self.o, self.lse = o, lse
        return dict(o=self._bhsd(o, Sq), lse=lse.view(B, H, Sq))

    def bwd(self, variant, want_dbias=False):
        """Backward of the last fwd(). Returns dq, dk, dv as [B, H, S, D], whether the kernel added the
        fused bias gradient, and dbias (fp32 [3, H, D], started at 0.5) or None."""
        c, X = self.c, self.X
        B, H, Sq, Sk, D = (c[key] for key in ("B", "H", "Sq", "Sk", "D"))
        nws = X.attn_bwd_ws(B, H, Sq, Sk, D)
        ws = torch.full((nws + 65536,), SENT, device=self.dev)
        dbias = torch.full((3 * H * D,), 0.5, device=self.dev) if want_dbias else None
        if self.fused:
            gbuf, g = _guarded(B * Sq * 3 * H, D, torch.bfloat16, self.dev)
            dq, dk, dv = g, g[H * D:], g[2 * H * D:]
            bufs = [(gbuf, B * Sq * 3 * H)]
        else:
            (qb, dq), (kb, dk), (vb, dv) = (_guarded(B * H * S, D, torch.bfloat16, self.dev) for S in (Sq, Sk, Sk))
            bufs = [(qb, B * H * Sq), (kb, B * H * Sk), (vb, B * H * Sk)]
        prev = X.attn_bwd_variant()
        X.attn_set_bwd_variant(variant)
        try:
            done = X.attn_bwd(self.q, self.sq, self.k, self.sk, self.v, self.sk, self.o, self.so, self.do, self.so,
                              self.lse, dq, self.sq, dk, self.sk, dv, self.sk, ws[:nws], B, H, Sq, Sk, D,
                              self.scale, c["causal"], dbias=dbias, **self.kw)
        finally:
            X.attn_set_bwd_variant(prev)
        assert bool((ws[nws:] == SENT).all()), "attn_bwd wrote past its workspace"
        for buf, n in bufs:
            assert _guards_intact(buf, n, D), "attn_bwd wrote outside dq / dk / dv"
        if self.fused:
            g5 = g.view(B, Sq, 3, H, D)
            out = {key: g5[:, :, i].permute(0, 2, 1, 3) for i, key in enumerate(("dq", "dk", "dv"))}
        else:
            out = dict(dq=self._bhsd(dq, Sq), dk=self._bhsd(dk, Sk), dv=self._bhsd(dv, Sk))
        return out, bool(done), dbias

