"""Shared by test_glu_cpu.py and test_glu_gpu.py: the gated-linear-unit kernel's cases, a float64 oracle
written from the definition, the per-element bounds, and a runner that calls kernels.glu_fwd / glu_bwd on
guarded buffers (on the CPU that is the plain-torch reference path, on a GPU the HIP kernel glu.hip).

Definition:  y = act(g) u,  dg = dy u act'(g),  du = dy act(g)  with act one of
  silu       x expit(x)                       act' = s + x s (1 - s),  s = expit(x)
  gelu       0.5 x (1 + erf(x / sqrt 2))      act' = Phi(x) + x phi(x)
  gelu_tanh  0.5 x (1 + tanh z)               act' = 0.5 (1 + t) + 0.5 x (1 - t^2) c (1 + 3 k x^2),
             z = c (x + k x^3), c = sqrt(2 / pi), k = 0.044715, t = tanh z
  relu       max(x, 0)                        act' = [x > 0]
  sigmoid    expit(x)                         act' = s (1 - s)

Oracle: float64 on the CPU from exactly the stored input values (bf16 values are rounded first, then
widened), torch.special.expit / torch.erf / torch.tanh in float64 and the closed forms above (1 - s is
taken as expit(-x)); no autograd.

bf16 storage: the project's per-element bound (tests/test_small_kernels_gpu.py, 'Bounds'):
  |err| <= 2^-8 |ref| + 2^-18 s
with s the magnitude of the largest intermediate of the element. |act(x)| <= max(1, |x|) for all five
activations (|silu|, |gelu|, |relu| <= |x|, sigmoid <= 1) and |act'(x)| < 1.13 with its own intermediates
(x phi(x), x s (1 - s), the tanh form's x (1 - t^2) z') bounded by a constant, so
  y:   s = max(1, |g|) |u|        (act(g), then one product)
  du:  s = max(1, |g|) |dy|       (act(g), then one product)
  dg:  s = max(1, |g|) |u| |dy|   (the two products; act' priced like act)
The first term is the one rounding to bf16 (half an ulp of 2^-7 of the computed value, with room for that
value's own error); the second covers the fp32 arithmetic in front of it: exp2 / rcp (1 ulp each), the
erf polynomial (1.5e-7 ~ 2^-22.7 absolute on Phi, times |x|) and the products (2^-24 each) stay below
2^-21 s. Where every factor is zero (u == 0 for y and dg, dy == 0 for dg and du) s is 0 and so is ref: the
result must then equal the reference by value (either sign of zero). Written down before any run and not
tuned.

fp32 storage: the activations use fast intrinsics (v_exp_f32, v_rcp_f32, an erf polynomial), so there is
no constant; torch's own fp32 composition on the same device and inputs (F.silu(g) * u, F.gelu(g,
approximate=..) * u, ... and their autograd gradients) is the yardstick, by that file's rule (copied here):
with e = max |err| / (|ref| + 2^-10 s) for the kernel (e_k) and for torch (e_t, floored at 2^-25: no fp32
result is better than half an ulp), the kernel passes if e_k <= 16 e_t; and where s == 0 it equals ref.

Untouched memory: every buffer lies between GUARD sentinels in front and GUARD NaNs behind; the guards,
the gaps between the rows of strided outputs and every input buffer are compared bit for bit after the
launches.

Measured on an MI355X (every case, activation and output passes; per activation and direction the case
with the worst ratio; every `yardstick` line a run prints feeds this table):

  bf16, worst |err| / tol over every case, activation and output: 0.992 (both grid_stride cases; a correctly rounded
  bf16 result reaches 1 of the first term); unary silu 0.936 forward, 0.974 backward.

  fp32 yardstick    e_t       e_k       e_k / e_t   case
  silu       fwd    1.28e-07  3.35e-07    2.61      packed
             bwd    4.93e-06  1.28e-05    2.60      grid_stride
  gelu       fwd    5.53e-06  3.53e-05    6.38      vec_and_tail   (1)
             bwd    3.09e-06  3.27e-05   10.58      packed         (1)
  gelu_tanh  fwd    7.56e-08  1.31e-07    1.74      tail_only      (2)
             bwd    3.20e-08  1.12e-07    3.51      tail_only      (2)
  relu       fwd    4.61e-08  4.61e-08    1.00      vec_and_tail
             bwd    5.36e-08  5.36e-08    1.00      tail_only
  sigmoid    fwd    1.33e-07  2.84e-07    2.14      rows_aligned
             bwd    1.31e-07  3.13e-07    2.39      rows_aligned
  unary silu fwd    1.39e-07  2.85e-07    2.05      4099 elements (tests/test_glu_gpu.py)
             bwd    5.55e-06  1.27e-05    2.28

  (1) both err where 1 + erf(x / sqrt 2) cancels (x < -2); the kernel's erf polynomial (1.5e-7 absolute) is
      several times torch's erff there, as for the unary gelu (tests/test_small_kernels_gpu.py, note 2).
  (2) on the larger cases torch's own tanh form errs by e_t 1e-05 to 1e-04 and the kernel, which takes
      0.5 (1 + tanh z) as one sigmoid, by 4e-07 to 4e-05: ratios 0.01 to 0.34.
"""
import math

import torch
import torch.nn.functional as F

from flexflow_amd import kernels as K

BF16, F32 = torch.bfloat16, torch.float32
ACTS = ["silu", "gelu", "gelu_tanh", "relu", "sigmoid"]
RT_BF16, AT_BF16 = 2.0 ** -8, 2.0 ** -18
YARD_FACTOR = 16.0
GUARD = 512  # elements of sentinel in front of / NaN behind every buffer (a multiple of 16 bytes)
SENT = 7.0
FILL = 3.0  # what output buffers hold before the launch (rows' gaps must still hold it afterwards)
OPERANDS = ("g", "u", "y", "dy", "dg", "du")
OUTPUTS = ("y", "dg", "du")


def _case(rows, F_, stride=None, off=0, packed=False, strides=None, max_blocks=0, extremes=False):
    """place[operand] = (buffer name, offset in elements, row stride in elements)."""
    def place(F1):
        if packed:  # gate | up halves of one [rows, 2F] buffer; dg | du likewise; y and dy on their own
            return {"g": ("x", 0, 2 * F1), "u": ("x", F1, 2 * F1), "y": ("y", 0, F1), "dy": ("dy", 0, F1),
                    "dg": ("dx", 0, 2 * F1), "du": ("dx", F1, 2 * F1)}
        return {o: (o, off, (strides or {}).get(o, stride or F1)) for o in OPERANDS}
    return dict(rows=rows, F=F_, place=place, max_blocks=max_blocks, extremes=extremes)


# the smallest shapes that reach each branch of glu.hip (a 16-byte vector is 8 bf16 / 4 fp32 elements)
CASES = {
    "tail_only": _case(1, 5),  # fewer elements than one vector
    "vec_and_tail": _case(3, 11),  # contiguous: the flat path, vectors plus a scalar tail
    "rows_aligned": _case(5, 64, stride=72),  # strided vector path, gaps untouched
    "rows_misaligned": _case(5, 64, stride=67),  # scalar path chosen from a stride
    "base_misaligned": _case(4, 32, off=1),  # scalar path chosen from a pointer
    "packed": _case(7, 64, packed=True),  # both halves of one [7, 128] buffer, dg / du into one [7, 128]
    "packed_misaligned": _case(7, {BF16: 12, F32: 6}, packed=True),  # the second half starts 24 bytes in
    "grid_stride": _case(40, 136, max_blocks=1),  # one block: every thread loops several times
    # the same on strided rows (no flat collapse): a thread's steps carry from one row into the next
    "packed_grid_stride": _case(40, 136, packed=True, max_blocks=1),
    "mixed_strides": _case(6, 40, strides=dict(g=40, u=48, y=56, dy=64, dg=72, du=80)),
    "extremes": _case(2, 16, extremes=True),
}
EXTREME_G = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4, 1e4, -1e4, 20.0, -20.0, 0.0, -0.0]


def width(c, dtype):
    return c["F"][dtype] if isinstance(c["F"], dict) else c["F"]


def layout(c, dtype):
    """(place, {buffer name: elements})."""
    rows, F_ = c["rows"], width(c, dtype)
    place = c["place"](F_)
    size = {}
    for o, (b, off, st) in place.items():
        size[b] = max(size.get(b, 0), off + (rows - 1) * st + F_)
    return place, size


def view2(flat, off, st, rows, F_):
    return flat.as_strided((rows, F_), (st, 1), flat.storage_offset() + off)


_INPUTS = {}


def make_inputs(name, dtype):
    """CPU buffers of the case, made once per (case, dtype) and shared by every activation and test (never
    written: runs work on copies). Inputs are randn * 2 in the whole buffer (the gaps too); output buffers
    hold FILL."""
    key = (name, dtype)
    if key in _INPUTS:
        return _INPUTS[key]
    c = CASES[name]
    rows, F_ = c["rows"], width(c, dtype)
    place, size = layout(c, dtype)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    out_bufs = {place[o][0] for o in OUTPUTS}
    bufs = {}
    for b in sorted(size):
        bufs[b] = (torch.full((size[b],), FILL) if b in out_bufs else torch.randn(size[b], generator=g) * 2).to(dtype)
    if c["extremes"]:
        gv, uv, dv = (view2(bufs[place[o][0]], place[o][1], place[o][2], rows, F_) for o in ("g", "u", "dy"))
        gv.copy_(torch.tensor(EXTREME_G).to(dtype).repeat(rows, 1))
        uv[:, 2::5] = 0  # some u == 0: y and dg exactly zero there
        dv[1] = 0  # one dy row of zeros: dg and du exactly zero there
    _INPUTS[key] = bufs
    return bufs


# ------------------------------------------------------------------------------------------ oracle
_C, _K = math.sqrt(2.0 / math.pi), 0.044715


def act64(x, act):
    """(act(x), act'(x)) in float64 from the closed forms."""
    s, oms = torch.special.expit(x), torch.special.expit(-x)
    if act == "silu":
        return x * s, s + x * s * oms
    if act == "gelu":
        cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
        return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == "gelu_tanh":
        t = torch.tanh(_C * (x + _K * x ** 3))
        return 0.5 * x * (1 + t), 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * _C * (1 + 3 * _K * x * x)
    if act == "relu":
        return torch.relu(x), (x > 0).double()
    if act == "sigmoid":
        return s, s * oms
    raise KeyError(act)


def oracle(g, u, dy, act):
    """{output: (ref, s)} float64 from the stored values g, u, dy."""
    g, u, dy = g.double(), u.double(), dy.double()
    f, d = act64(g, act)
    m = g.abs().clamp(min=1.0)
    return {"y": (f * u, m * u.abs()), "dg": (dy * u * d, m * u.abs() * dy.abs()), "du": (dy * f, m * dy.abs())}


def torch32(g, u, dy, act):
    """torch's own fp32 composition and its autograd gradients on the tensors' device."""
    gr, ur = g.detach().clone().requires_grad_(), u.detach().clone().requires_grad_()
    a = {"silu": F.silu, "gelu": F.gelu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "relu": torch.relu,
         "sigmoid": torch.sigmoid}[act](gr)
    y = a * ur
    dg, du = torch.autograd.grad(y, (gr, ur), dy)
    return {"y": y.detach(), "dg": dg, "du": du}


def bf16_check(got, ref, s):
    """(elements outside |err| <= 2^-8 |ref| + 2^-18 s, worst |err| / tol over elements with tol > 0)."""
    err = (got.double().cpu() - ref).abs()
    tol = RT_BF16 * ref.abs() + AT_BF16 * s
    miss = int((~(err <= tol)).sum())  # NaN counts as a miss; tol == 0: by value
    pos = tol > 0
    worst = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    return miss, worst


def yard_err(got, ref, s):
    """max |err| / (|ref| + 2^-10 s) over the elements with s > 0; elements with s == 0 must equal ref."""
    got = got.double().cpu()
    zero = s == 0
    assert bool((got[zero] == ref[zero]).all()), "an element whose factors are all zero is not zero"
    if bool(zero.all()):
        return 0.0
    e = (got - ref).abs()[~zero] / (ref.abs() + (AT_BF16 / RT_BF16) * s)[~zero]
    return float(torch.nan_to_num(e, nan=math.inf).max())


YARD_LOG = {}  # (act, direction) -> (e_t, e_k) of the worst ratio seen in this process


def yardstick(got, t32, ref, s, act, direction, what):
    e_k = yard_err(got, ref, s)
    e_t = max(yard_err(t32, ref, s), 2.0 ** -25)
    print(f"yardstick {what}: e_t {e_t:.3e} e_k {e_k:.3e} ratio {e_k / e_t:.2f}")
    old = YARD_LOG.get((act, direction))
    if old is None or e_k / e_t > old[1] / old[0]:
        YARD_LOG[(act, direction)] = (e_t, e_k)
    assert e_k <= YARD_FACTOR * e_t, f"{what}: e_k {e_k:.3e} > {YARD_FACTOR} * e_t {e_t:.3e}"


# ------------------------------------------------------------------------------------------ runner
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(name, act, dtype, device):
    """Forward and backward of the case through kernels.glu_fwd / glu_bwd on guarded copies of the shared
    buffers: ({operand: CPU [rows, F] tensor}, list of integrity failures)."""
    c = CASES[name]
    rows, F_ = c["rows"], width(c, dtype)
    place, size = layout(c, dtype)
    src = make_inputs(name, dtype)
    dev = torch.device(device)
    full, flat = {}, {}
    for b, data in src.items():
        full[b] = torch.cat([torch.full((GUARD,), SENT, dtype=dtype), data,
                             torch.full((GUARD,), float("nan"), dtype=dtype)]).to(dev)
        flat[b] = full[b][GUARD:GUARD + size[b]]
    v = {o: view2(flat[b], off, st, rows, F_) for o, (b, off, st) in place.items()}
    if c["place"](F_)["g"][1] == 1:
        assert v["g"].data_ptr() % 16 != 0
    out = K.glu_fwd(v["g"], v["u"], act, out=v["y"], max_blocks=c["max_blocks"])
    assert out.data_ptr() == v["y"].data_ptr()
    K.glu_bwd(v["g"], v["u"], v["dy"], act, dg=v["dg"], du=v["du"], max_blocks=c["max_blocks"])
    if dev.type == "cuda":
        torch.cuda.synchronize()
    bad = []
    after = {b: t.cpu() for b, t in full.items()}
    out_bufs = {place[o][0] for o in OUTPUTS}
    for b, t in after.items():
        if not (bool((t[:GUARD] == SENT).all()) and bool(torch.isnan(t[GUARD + size[b]:]).all())):
            bad.append(f"{b}: guards changed")
        data = t[GUARD:GUARD + size[b]]
        if b not in out_bufs:
            if not torch.equal(_bits(data), _bits(src[b])):
                bad.append(f"{b}: an input buffer changed")
            continue
        written = torch.zeros(size[b], dtype=torch.bool)
        for o in OUTPUTS:
            if place[o][0] == b:
                view2(written, place[o][1], place[o][2], rows, F_).fill_(True)
        if not torch.equal(_bits(data[~written]), _bits(src[b][~written])):
            bad.append(f"{b}: elements outside the output's rows and columns changed")
    res = {o: view2(after[b][GUARD:GUARD + size[b]], off, st, rows, F_).clone() for o, (b, off, st) in place.items()}
    return res, bad


def check_case(name, dtype, device, acts=ACTS):
    """Asserts the case for every activation, forward and backward; returns the worst bf16 ratio (0 for
    fp32 storage on a GPU, which goes by the yardstick)."""
    worst = 0.0
    for act in acts:
        res, bad = run(name, act, dtype, device)
        assert not bad, (name, act, bad)
        refs = oracle(res["g"], res["u"], res["dy"], act)
        for o in OUTPUTS:
            assert torch.isfinite(res[o]).all(), (name, act, o, "not finite")
        if dtype == F32 and torch.device(device).type == "cuda":
            t32 = torch32(res["g"].to(device), res["u"].to(device), res["dy"].to(device), act)
            for o in OUTPUTS:
                yardstick(res[o], t32[o], *refs[o], act, "fwd" if o == "y" else "bwd", f"glu {name} {act} {o}")
        else:
            for o in OUTPUTS:
                miss, w = bf16_check(res[o], *refs[o])
                print(f"glu {name} {act} {o} {dtype}: {miss} of {res[o].numel()} outside, worst ratio {w:.3f}")
                assert miss == 0, (name, act, o, miss, w)
                worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------ op level
TOL_O, TOL_G = 2e-2, 3e-2  # the sibling GPU op tests' relative Frobenius bounds (bf16 against fp32)
HID, FFN, BATCH = 16, 24, 4


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def ffn_weights(seed=11):
    """bf16-representable gate / up / down weights [out, in] of the tiny gated FFN."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda o, i: (torch.randn(o, i, generator=g) / math.sqrt(i)).bfloat16().float()  # noqa: E731
    return {"gate": mk(FFN, HID), "up": mk(FFN, HID), "down": mk(HID, FFN)}


def ffn_torch(x, W, dy, act="silu", dtype=torch.float32):
    """down(act(gate(x)) * up(x)) in torch with autograd: y, dx and the three weight gradients."""
    xr = x.to(dtype).requires_grad_()
    Wd = {n: w.to(dtype).requires_grad_() for n, w in W.items()}
    a = {"silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh")}[act]
    y = (a(xr @ Wd["gate"].t()) * (xr @ Wd["up"].t())) @ Wd["down"].t()
    (y * dy.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": xr.grad, "dgate": Wd["gate"].grad, "dup": Wd["up"].grad, "ddown": Wd["down"].grad}


def ffn_step(x, W, dy, device, dtype, fused=False, act="silu", need_dx=True):
    """One training forward and backward of FFModel.gated_ffn's layers through OpCtx on `device` in `dtype`,
    on the weights W (the fused form's gate_up weight is their concatenation, gate rows first): the layers
    by name and {"y", "dx", "dgate", "dup", "ddown"} (the fused weight gradient split back into its halves).
    need_dx=False: the layers that read x are told that x needs no gradient, as the executor tells a layer
    fed by a model input."""
    from flexflow_amd.core import DataType, FFConfig, FFModel
    from flexflow_amd.ops import OpCtx
    ff = FFModel(FFConfig([]))
    t = ff.create_tensor(list(x.shape), DataType.DT_FLOAT)
    out = ff.gated_ffn(t, FFN, activation=act, fused_gate_up=fused, name="ffn")
    layers = [L for L in ff.layers if L.inputs]
    byname = {L.name: L for L in layers}
    wof = {"ffn_gate": [W["gate"]], "ffn_up": [W["up"]], "ffn_down": [W["down"]], "ffn_glu": [],
           "ffn_gate_up": [torch.cat([W["gate"], W["up"]], 0)]}
    val = {id(t): x.to(device, dtype)}
    ctxs = {}
    for L in layers:
        n = len(L.impl.axis_sizes())
        ctx = ctxs[L.name] = OpCtx(layer=L, part_coords=(0,) * n, degrees=(1,) * n)
        w = [v.to(device, dtype) for v in wof[L.name]]
        assert [tuple(v.shape) for v in w] == [tuple(s.dims) for s in L.weights], L.name
        ctx.wgrads = [torch.zeros(v.shape, device=device) for v in w]
        if L.inputs[0] is t:
            ctx.extra["need_dx0"] = need_dx
        val[id(L.outputs[0])] = L.impl.forward(ctx, [val[id(i)] for i in L.inputs], w)[0]
    grad = {id(out): dy.to(device, dtype)}
    for L in reversed(layers):
        ds = L.impl.backward(ctxs[L.name], [grad[id(L.outputs[0])]])
        for i, d in zip(L.inputs, ds):
            if d is not None:
                grad[id(i)] = d if id(i) not in grad else grad[id(i)] + d
    res = {"y": val[id(out)], "ddown": ctxs["ffn_down"].wgrads[0]}
    if id(t) in grad:
        res["dx"] = grad[id(t)]
    if fused:
        res["dgate"], res["dup"] = ctxs["ffn_gate_up"].wgrads[0][:FFN], ctxs["ffn_gate_up"].wgrads[0][FFN:]
    else:
        res["dgate"], res["dup"] = ctxs["ffn_gate"].wgrads[0], ctxs["ffn_up"].wgrads[0]
    return byname, res
