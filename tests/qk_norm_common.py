"""Shared by test_qk_norm_cpu.py and test_qk_norm_gpu.py: the cases of the fused QK-norm + rotary launches, a
float64 oracle written from the definition, the derived per-element bounds, and a runner that calls
kernels.qk_norm_rope / qk_norm_rope_bwd on guarded buffers (on the CPU the plain-torch path, on a GPU qknorm.hip).

Oracle (float64, on the exact stored values): rstd = 1 / sqrt(mean_d(x^2) + eps), yhat = x rstd w, y = R yhat
with R the rotation of rope_common.oracle over the first rd columns (identity behind them and for rd = 0).
Backward: g = R^-1 dz, xhat = x rstd, dw = sum_rows g xhat, dx = rstd (g w - xhat mean_d(g w xhat)).

Bounds, derived and not tuned, with u = 2^-8 (bf16 storage, half an ulp) or 2^-24 (fp32) and f = 2^-24:
  rstd  (D/2 + 5) f |rstd|: D squares summed in fp32 in any order (D f), the mean, eps and the rounding
        of 1/D (4 f), all halved by the square root; rsqrt within 2 ulp; the fp32 store.
  y     u |y| + (D/2 + 10) f mag: rstd's D/2 + 4, two products, and the rotation's 4 f of rope_common
        on mag = |yhat1 c| + |yhat2 s| (mag = |yhat| where nothing rotates).
  dx    u |dx| + f ((D/2 + 12) A + (5D/2 + 26) M), A = rstd |w| mag_g the first term's magnitude (rotation 4,
        w, rstd, the subtraction, rstd's own D/2 + 4) and M = rstd |xhat| mean_d(|w| mag_g |xhat|) the second's
        (each summand D/2 + 11, D of them summed, 1/D, then xhat D/2 + 6 and rstd D/2 + 5, the subtraction).
  dw    (D/2 + 11 + N) f sum_rows(mag_g |xhat|) over the N = B S H rows: each term D/2 + 10, N terms summed in
        fp32 in any order, the fp32 store; relative to the sum of the terms' magnitudes, not to |dw|.
Where a bound is 0 the result must equal the reference. Inputs, the V third of a fused gradient buffer and
the guard rows around every buffer are compared bit for bit with what they held.
"""
import torch

import rope_common as R
from flexflow_amd import kernels as K

F32, EPS, GUARD, SENT = 2.0 ** -24, 1e-6, 512, 7.0


def _c(B=2, Sq=37, Sk=None, H=3, Hkv=None, D=64, rd=None, fused=False, interleaved=False, ids=False, maxp=None, off=0,
       dtype=None, wdtype=None):
    Sk = Sq if Sk is None else Sk
    return dict(B=B, Sq=Sq, Sk=Sk, H=H, Hkv=H if Hkv is None else Hkv, D=D, rd=D if rd is None else rd, fused=fused,
                interleaved=interleaved, ids=ids, maxp=maxp or max(Sq, Sk), off=off, dtype=dtype, wdtype=wdtype)


# the smallest shapes that reach each branch of qknorm.hip
CASES = {
    "fused_layout": _c(fused=True),  # x and dz [T, 3, H, D], out [T, 2, H, D]; 74 tokens: a ragged workgroup
    "gqa": _c(H=4, Hkv=1, D=128, Sq=40, Sk=24),  # separate buffers, the shorter tensor's rows bounds-checked
    "norm_only": _c(rd=0),
    "partial": _c(rd=32),
    "interleaved": _c(interleaved=True),
    "interleaved_partial": _c(rd=32, interleaved=True),
    "ids": _c(B=3, Sq=40, ids=True, maxp=50),  # restarts, a row of zeros, ids outside the table
    "d32": _c(D=32),
    "d256_f32w": _c(B=1, H=5, Hkv=2, D=256, wdtype=torch.float32),  # 16 lanes a row; 5 rows: a ragged row batch
    "d80_fp32": _c(D=80, rd=40, dtype=torch.float32),  # the general form: 40 pairs, 20 of them rotated
    "d48_interleaved": _c(D=48, rd=20, interleaved=True),  # the general form in bf16
    "misaligned": _c(off=1),  # every base pointer off by one element: no 16-byte access fits
    "multi_wg": _c(B=1, Sq=150, H=2, Hkv=1),  # 64 tokens a workgroup: three of them, the last with 22
}


def _lay(c, which, thirds):
    """(flat element count, (batch, head, row) strides, this tensor's offset in its buffer)."""
    B, D = c["B"], c["D"]
    H, S = (c["H"], c["Sq"]) if which == "q" else (c["Hkv"], c["Sk"])
    if c["fused"]:
        return B * S * thirds * H * D, [S * thirds * H * D, D, thirds * H * D], (0 if which == "q" else H * D)
    return B * S * H * D, [S * H * D, D, H * D], 0


def _guard(data, dev, off):
    """[sentinel | off pad | data | sentinel] on `dev` and the data region as a flat view."""
    pad = torch.full((GUARD + off,), SENT, dtype=data.dtype)
    buf = torch.cat([pad, data, pad[:GUARD]]).to(dev)
    return buf, buf[GUARD + off:GUARD + off + data.numel()]


def _same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.cpu().contiguous().view(v), b.cpu().contiguous().view(v))


def make(name, c, dtype):
    """Stored inputs of the case: x and dz per buffer, the two weights (drawn around 1), the ids. Some head
    rows of x are zero, one of them with a zero dz row as well."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    wdt = c["wdtype"] or dtype
    d = {"w": {n: (1 + 0.25 * torch.randn(c["D"], generator=g)).to(wdt) for n in "qk"}, "x": {}, "dz": {}}
    for nm in ("q",) if c["fused"] else ("q", "k"):
        n = _lay(c, nm, 3)[0]
        d["x"][nm], d["dz"][nm] = torch.randn(n, generator=g).to(dtype), torch.randn(n, generator=g).to(dtype)
    _, st, _ = _lay(c, "q", 3)
    R.view4(d["x"]["q"], st, c["B"], c["H"], c["Sq"], c["D"])[:, 0, 1::7, :] = 0
    R.view4(d["dz"]["q"], st, c["B"], c["H"], c["Sq"], c["D"])[:, 0, 1, :] = 0
    d["ids"] = None
    if c["ids"]:
        ids = torch.arange(c["Sq"], dtype=torch.int32).repeat(c["B"], 1)
        ids[0, 17:] = torch.arange(c["Sq"] - 17, dtype=torch.int32)
        ids[1] = 0
        ids[2, 3], ids[2, 7], ids[2, 0] = -3, c["maxp"] + 5, 2 ** 31 - 1
        d["ids"] = ids
    return d


def oracle(x4, w, dz4, c, ids, u):
    """{name: (reference, bound)} in float64 for y, rstd [B, S, H], dx and this tensor's dw."""
    D, rd = c["D"], c["rd"]
    rc = R._c(B=c["B"], Sq=x4.shape[2], H=x4.shape[1], D=D, rd=rd, interleaved=c["interleaved"], maxp=c["maxp"])

    def rot(t, inverse):  # (R t, the magnitude the rotation's 4 f refers to)
        ref, tol = R.oracle(t, rc, ids, 0.0, inverse)
        mag = tol / (4 * F32)
        mag[..., rd:] = t[..., rd:].abs()
        return ref, mag

    x, w = x4.double(), w.double()
    rstd = 1 / torch.sqrt((x * x).mean(-1, keepdim=True) + EPS)
    y, mag = rot(x * rstd * w, False)
    g, mag_g = rot(dz4.double(), True)
    xh, gw = x * rstd, g * w
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    A = rstd * w.abs() * mag_g
    M = rstd * xh.abs() * (w.abs() * mag_g * xh.abs()).mean(-1, keepdim=True)
    N = x[..., 0].numel()
    return {"y": (y, u * y.abs() + (D / 2 + 10) * F32 * mag),
            "rstd": (rstd[..., 0].transpose(1, 2), (D / 2 + 5) * F32 * rstd[..., 0].transpose(1, 2)),
            "dx": (dx, u * dx.abs() + F32 * ((D / 2 + 12) * A + (5 * D / 2 + 26) * M)),
            "dw": ((g * xh).sum((0, 1, 2)), (D / 2 + 11 + N) * F32 * (mag_g * xh.abs()).sum((0, 1, 2)))}


def run(name, dtype, device, frozen=False):
    """The case through kernels.qk_norm_rope and qk_norm_rope_bwd: ({tensor: {y, rstd, dx, dw}} on the CPU, the
    stored inputs, the list of integrity failures). frozen: no dw is asked for."""
    c = CASES[name]
    dtype = c["dtype"] or dtype
    dev, d = torch.device(device), make(name, c, dtype)
    B, H, Hkv, Sq, Sk, D, rd, off = (c[k] for k in ("B", "H", "Hkv", "Sq", "Sk", "D", "rd", "off"))
    table = K.rope_table(rd, c["maxp"], device=dev) if rd else None
    pos = None if d["ids"] is None else d["ids"].to(dev)
    names = ("q",) if c["fused"] else ("q", "k")
    xb = {n: _guard(d["x"][n], dev, off) for n in names}
    gb = {n: _guard(d["dz"][n], dev, off) for n in names}
    ob = {n: _guard(torch.full((_lay(c, n, 2)[0],), float("nan"), dtype=dtype), dev, off) for n in names}
    flat = lambda bufs, n, thirds: bufs["q" if c["fused"] else n][1][_lay(c, n, thirds)[2]:]  # noqa: E731
    (_, xqs, _), (_, xks, _), (_, oqs, _), (_, oks, _) = (_lay(c, n, t) for t in (3, 2) for n in "qk")
    w = {n: t.to(dev) for n, t in d["w"].items()}
    rq, rk = K.qk_norm_rope(flat(xb, "q", 3), xqs, flat(ob, "q", 2), oqs, w["q"], flat(xb, "k", 3), xks, flat(ob, "k", 2), oks,
                            w["k"], B, H, Hkv, Sq, Sk, D, EPS, rd=rd, table=table, pos=pos, interleaved=c["interleaved"])
    dw = {n: None if frozen else torch.zeros(D, device=dev) for n in "qk"}
    K.qk_norm_rope_bwd(flat(xb, "q", 3), xqs, flat(gb, "q", 3), xqs, w["q"], rq, dw["q"], flat(xb, "k", 3), xks,
                       flat(gb, "k", 3), xks, w["k"], rk, dw["k"], B, H, Hkv, Sq, Sk, D, rd=rd, table=table, pos=pos,
                       interleaved=c["interleaved"])
    if dev.type == "cuda":
        torch.cuda.synchronize()
    bad = []
    for n in names:
        lo, hi = GUARD + off, GUARD + off + d["x"][n].numel()
        if not _same_bits(xb[n][0], _guard(d["x"][n], "cpu", off)[0]):
            bad.append(f"{n}: the input or its guard rows changed")
        for what, b, end in (("output", ob[n][0], GUARD + off + ob[n][1].numel()), ("gradient", gb[n][0], hi)):
            if not (bool((b[:lo] == SENT).all()) and bool((b[end:] == SENT).all())):
                bad.append(f"{n}: {what} guard rows changed")
    if c["fused"] and not _same_bits(gb["q"][1].view(-1, 3, H * D)[:, 2], d["dz"]["q"].view(-1, 3, H * D)[:, 2]):
        bad.append("fused: the V third of the gradient buffer changed")
    res = {}
    for n, H_, S_, r in (("q", H, Sq, rq), ("k", Hkv, Sk, rk)):
        v = lambda t, thirds: R.view4(t[_lay(c, n, thirds)[2]:], _lay(c, n, thirds)[1], B, H_, S_, D)  # noqa: E731
        src = "q" if c["fused"] else n
        res[n] = dict(y=v(ob[src][1].cpu(), 2), rstd=r.cpu(), dx=v(gb[src][1].cpu(), 3), dw=None if frozen else dw[n].cpu(),
                      x=v(d["x"][src], 3), dz=v(d["dz"][src], 3), w=d["w"][n])
    return res, d, bad


def check_case(name, dtype, device):
    """Asserts the case element by element; returns the worst |err| / bound."""
    res, d, bad = run(name, dtype, device)
    assert not bad, (name, bad)
    c, worst = CASES[name], 0.0
    for n, r in res.items():
        want = oracle(r["x"], r["w"], r["dz"], c, d["ids"], R.U[c["dtype"] or dtype])
        for key, (ref, tol) in want.items():
            miss, wr = R.check(r[key], ref, tol)
            print(f"qk_norm {name} {n} {key}: {miss} of {ref.numel()} outside, worst ratio {wr:.3f}")
            assert miss == 0, (name, n, key, miss, wr)
            worst = max(worst, wr)
    zero = res["q"]["dx"][:, 0, 1]  # an all-zero head row with a zero gradient row: finite and exactly zero
    assert bool(torch.isfinite(res["q"]["y"]).all()) and bool((zero == 0).all())
    return worst
