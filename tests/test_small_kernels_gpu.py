"""The small kernels, element by element, against fp64 references (GPU only).

Elementwise (unary / binary / cast / dropout), softmax and the losses, metrics, reductions, the
optimizers, embedding and the initialisers. Every reference is computed in fp64 on the CPU from
exactly the values the kernel sees (bf16 inputs are rounded first, then widened) and the comparison
is per element: `_close` reports the worst element, its index and both values.

Bounds
  bf16 outputs           rtol 2^-8 (one bf16 ulp), atol 2^-18 * max(1, |operands|)
  fp32, exact ops        rtol 2^-22, atol 0 (add / sub / scalar_sub: 2 fp32 ulps of the larger operand)
  fp32, fast intrinsics  no constant: torch's own fp32 op on the same device and inputs is the
                         yardstick. With e = max |err| / (|ref| + 2^-10 * max(1, |operands|)) for the
                         kernel (e_k) and for torch (e_t, floored at 2^-25: no fp32 result is better
                         than half an ulp), the kernel passes if e_k <= 16 * e_t.

Measured on an MI355X (fp32; per op the case with the worst ratio over every size, layout and
accumulate setting that the tests below run; every `yardstick` line a run prints feeds this table):

  op                      e_t       e_k       e_k/e_t  inputs
  sigmoid      fwd        1.08e-07  2.34e-07   2.17    randn * 2
               bwd        2.07e-07  2.13e-07   1.03
  tanh         fwd        1.14e-07  1.14e-07   1.00    randn * 2
               bwd        3.74e-08  4.64e-08   1.24
  elu          fwd        4.14e-08  4.14e-08   1.00    randn * 2, some x == 0   (1)
               bwd        5.44e-08  5.44e-08   1.00
  gelu         fwd        1.65e-06  1.45e-05   8.82    randn * 2   (2)
               bwd        7.53e-07  4.86e-06   6.45
  exp          fwd        5.81e-08  2.34e-07   4.03    [-4, 4]
               bwd        3.18e-08  3.18e-08   1.00
  sin          fwd        3.39e-08  3.39e-08   1.00    [-4, 4], zero crossings included   (3)
               bwd        4.69e-08  5.36e-08   1.14
  cos          fwd        5.92e-08  5.92e-08   1.00    [-4, 4], zero crossings included   (3)
               bwd        3.83e-08  3.83e-08   1.00
  rsqrt        fwd        5.68e-08  8.53e-08   1.50    [0.1, 8]
               bwd        7.78e-07  9.88e-07   1.27
  pow 2.0      fwd        5.42e-08  1.11e-07   2.06    [0.1, 8]
               bwd        5.79e-08  1.64e-07   2.83
  pow 0.5      fwd        5.84e-08  1.05e-07   1.81    [0.1, 8]
               bwd        9.92e-08  1.32e-07   1.33
  pow -1.5     fwd        4.81e-08  4.81e-08   1.00    [0.1, 8]
               bwd        3.70e-08  3.70e-08   1.00
  log          fwd        1.23e-07  1.59e-07   1.29    [0.1, 8]
               bwd        4.22e-08  4.22e-08   1.00
  sqrt         fwd        4.54e-08  4.54e-08   1.00    [0.1, 8]
               bwd        5.42e-08  5.42e-08   1.00
  softmax      fwd        8.07e-08  2.25e-07   2.79    randn * 3, scale 1 / 0.125 / 2
               bwd        2.86e-07  1.02e-06   3.55
               +-1e4      4.93e-08  2.19e-07   4.45    uniform in [-1e4, 1e4], error scale 1
               -inf fwd   1.91e-07  3.28e-07   1.72    causal / prefix / isolated / full-row masks
               -inf bwd   1.90e-07  2.98e-07   1.56
  softmax_xent loss       3.46e-08  7.91e-08   2.29    randn * 3, -inf off the label
               dlogits    1.04e-07  5.40e-07   5.17
  xent_grad    loss       8.28e-08  1.26e-07   1.52    softmax of randn * 2
  init_normal             7.44e-05  1.59e-04   2.14    yardstick: the CPU evaluation in fp32 torch ops   (4)

  (1) with `__expf(x) - 1` the forward measured e_k 1.27e-05, 172 x e_t: the subtraction cancels for
      small |x|. The kernel now calls expm1f; the input range was not narrowed.
  (2) both err where 1 + erf(x / sqrt 2) cancels (x < -2); the kernel's erf polynomial (1.5e-7
      absolute) is 9 x torch's erff there.
  (3) with the hardware `__sinf` / `__cosf` the kernels measured e_k 5.8e-05 .. 1.1e-04, 500 .. 750 x
      e_t: an absolute error near 1e-6 everywhere, which no input range makes relative. The kernels
      now call sinf / cosf; the input range was not narrowed.
  (4) cos(2 pi b) is ill-conditioned in b for either evaluation, hence the large e_t.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [BF16, F32]
DT_IDS = ["bf16", "fp32"]
RT_BF16, AT_BF16 = 2.0 ** -8, 2.0 ** -18
RT_F32 = 2.0 ** -22
ULP32 = 2.0 ** -23
_YARD_FACTOR = 16.0
_YARD_LOG = []  # (what, e_t, e_k): the figures behind the table above
GUARD = 4096.0  # exact in bf16: written around misaligned views to catch a store outside them


def _vec(dt):
    return 8 if dt == BF16 else 4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, dt, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dt)


def _uni(shape, dt, g, lo, hi):
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(dt)


def _d(t):
    return t.detach().cpu().double()


def _f32(v):
    """A Python float as the kernel receives it (its `float` argument)."""
    return float(np.float32(v))


def _scale_of(*ts):
    """max(1, |operands|) per element, fp64; non-finite operands (masked logits) count as 1."""
    s = torch.ones_like(_d(ts[0]))
    for t in ts:
        a = _d(t).abs()
        s = torch.maximum(s, torch.where(torch.isfinite(a), a, torch.ones_like(a)))
    return s


def _close(got, ref64, rtol, atol=0.0, what=""):
    """Per-element |got - ref| <= rtol * |ref| + atol (atol a float or a per-element tensor); where the
    reference is inf / NaN the result must be the same inf / NaN. Reports the worst element."""
    g, r = _d(got).reshape(-1), _d(ref64).reshape(-1)
    assert g.numel() == r.numel(), f"{what}: {tuple(got.shape)} vs {tuple(ref64.shape)}"
    if g.numel() == 0:
        return
    a = _d(atol).reshape(-1) if torch.is_tensor(atol) else torch.full_like(r, float(atol))
    excess = (g - r).abs() - (rtol * r.abs() + a)
    special = ~torch.isfinite(r)
    same = (g == r) | (torch.isnan(g) & torch.isnan(r))
    excess = torch.where(special, torch.where(same, -torch.ones_like(r), torch.full_like(r, math.inf)), excess)
    excess = torch.nan_to_num(excess, nan=math.inf)
    i = int(excess.argmax())
    assert excess[i] <= 0, (f"{what}: worst element {i} of {g.numel()}: got {g[i].item()!r}, ref {r[i].item()!r}, "
                            f"|err| {abs(g[i].item() - r[i].item()):.3e}, allowed "
                            f"{(rtol * r[i].abs() + a[i]).item():.3e}")


def _err(got, ref64, scale64):
    g, r = _d(got).reshape(-1), _d(ref64).reshape(-1)
    s = _d(scale64).reshape(-1) if torch.is_tensor(scale64) else torch.full_like(r, float(scale64))
    fin = torch.isfinite(r)
    same = (g == r) | (torch.isnan(g) & torch.isnan(r))
    assert bool(same[~fin].all()), "inf / NaN of the reference not reproduced"
    if not bool(fin.any()):
        return 0.0
    e = ((g - r).abs() / (r.abs() + (AT_BF16 / RT_BF16) * s))[fin]
    e = torch.nan_to_num(e, nan=math.inf)
    return float(e.max())


def _yard(got, torch32, ref64, scale64, what):
    """The fast-intrinsic rule: the kernel's worst error against 16 x torch's own fp32 error."""
    e_k = _err(got, ref64, scale64)
    e_t = max(_err(torch32, ref64, scale64), 2.0 ** -25)
    _YARD_LOG.append((what, e_t, e_k))
    print(f"yardstick {what}: e_t {e_t:.3e} e_k {e_k:.3e} ratio {e_k / e_t:.2f}")
    assert e_k <= _YARD_FACTOR * e_t, f"{what}: e_k {e_k:.3e} > {_YARD_FACTOR} * e_t {e_t:.3e}"


def _check(got, ref64, dt, fast, scale64, what, torch32=None, atol32=0.0, extra=0.0):
    """bf16: the bf16 bound; fp32: the yardstick (fast) or the exact-op bound. `extra` is added to atol
    (an accumulated term's own error, which does not shrink when the sum cancels)."""
    if dt == BF16:
        _close(got, ref64, RT_BF16, AT_BF16 * scale64 + extra, what)
    elif fast:
        _yard(got, torch32(), ref64, scale64, what)
    else:
        _close(got, ref64, RT_F32, atol32 + extra, what)


_GUARDED = []


def _place(t, mode="flat"):
    """t on the device: as it is, as a contiguous view one element into its buffer ('off1': off a
    16-byte boundary), or channel-last ('nhwc')."""
    t = t.to(DEV)
    if mode == "off1":
        buf = torch.full((t.numel() + 2,), GUARD, dtype=t.dtype, device=DEV)
        v = buf[1:-1].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        _GUARDED.append(buf)
        return v
    if mode == "nhwc":
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def _guards_intact():
    while _GUARDED:
        buf = _GUARDED.pop()
        assert buf[0].item() == GUARD and buf[-1].item() == GUARD, "a kernel wrote outside a misaligned view"


# ------------------------------------------------------------------------------------ unary
FAST_UNARY = {"sigmoid", "tanh", "elu", "gelu", "exp", "sin", "cos", "rsqrt", "pow", "log", "sqrt"}
UNARY_CASES = [("relu", 0.0), ("sigmoid", 0.0), ("tanh", 0.0), ("elu", 0.0), ("gelu", 0.0), ("exp", 0.0),
               ("sin", 0.0), ("cos", 0.0), ("rsqrt", 0.0), ("pow", 2.0), ("pow", 0.5), ("pow", -1.5),
               ("identity", 0.0), ("scalar_multiply", 1.5), ("scalar_add", 0.75), ("scalar_sub", 0.75),
               ("scalar_true_divide", 3.0), ("scalar_floor_divide", 0.5), ("scalar_floor_divide", 3.0),
               ("log", 0.0), ("sqrt", 0.0), ("neg", 0.0), ("leaky_relu", 0.125)]
assert {n for n, _ in UNARY_CASES} == set(K.U)


def _uf(name, x, s):
    """y = f(x) with torch's own ops: the fp64 reference on a CPU double tensor, the fp32 yardstick on
    a device float tensor."""
    return {
        "relu": lambda: torch.relu(x), "sigmoid": lambda: torch.sigmoid(x), "tanh": lambda: torch.tanh(x),
        "elu": lambda: F.elu(x), "gelu": lambda: F.gelu(x), "exp": lambda: torch.exp(x),
        "sin": lambda: torch.sin(x), "cos": lambda: torch.cos(x), "rsqrt": lambda: torch.rsqrt(x),
        "pow": lambda: torch.pow(x, s), "identity": lambda: x.clone(), "scalar_multiply": lambda: x * s,
        "scalar_add": lambda: x + s, "scalar_sub": lambda: x - s, "scalar_true_divide": lambda: x / s,
        "scalar_floor_divide": lambda: torch.floor(x / s), "log": lambda: torch.log(x),
        "sqrt": lambda: torch.sqrt(x), "neg": lambda: -x, "leaky_relu": lambda: torch.where(x > 0, x, x * s),
    }[name]()


def _udf(name, x, y, s):
    """d f / d x from the input x and the output y, as the backward kernel is given them."""
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    return {
        "relu": lambda: torch.where(x > 0, one, zero), "sigmoid": lambda: y * (1 - y),
        "tanh": lambda: 1 - y * y, "elu": lambda: torch.where(x > 0, one, y + 1),
        "gelu": lambda: 0.5 * (1 + torch.erf(x * 0.7071067811865476))
        + x * 0.3989422804014327 * torch.exp(-0.5 * x * x),
        "exp": lambda: y.clone(), "sin": lambda: torch.cos(x), "cos": lambda: -torch.sin(x),
        "rsqrt": lambda: -0.5 * y * y * y, "pow": lambda: s * torch.pow(x, s - 1), "identity": lambda: one,
        "scalar_multiply": lambda: one * s, "scalar_add": lambda: one, "scalar_sub": lambda: one,
        "scalar_true_divide": lambda: one / s, "scalar_floor_divide": lambda: zero, "log": lambda: 1 / x,
        "sqrt": lambda: 0.5 / y, "neg": lambda: -one, "leaky_relu": lambda: torch.where(x > 0, one, one * s),
    }[name]()


def _unary_input(name, s, shape, dt, g):
    if name in ("rsqrt", "log", "sqrt", "pow"):
        return _uni(shape, dt, g, 0.1, 8.0)
    if name in ("exp", "sin", "cos"):
        return _uni(shape, dt, g, -4.0, 4.0)
    if name == "scalar_floor_divide":  # x = s * (k + u): the quotient never sits on a rounding edge
        k = torch.randint(-20, 21, shape, generator=g).double()
        u = torch.rand(shape, generator=g).double() * 0.5 + 0.25
        x = (s * (k + u)).to(dt)
        assert torch.equal(torch.floor(x.float() / s).double(), torch.floor(x.double() / s))
        return x
    x = _randn(shape, dt, g, 2.0)
    if name in ("relu", "leaky_relu", "elu"):
        x.view(-1)[1::5] = 0.0  # x == 0: the gradient's branch point
    return x


def _unary_case(ffC, name, s, dt, shape, mode, seed):
    g = _gen(seed)
    sf = _f32(s)
    tag = f"{name}({s}) {DT_IDS[DTYPES.index(dt)]} {tuple(shape)} {mode}"
    x = _unary_input(name, sf, shape, dt, g)
    x64 = x.double()
    ref = _uf(name, x64, sf)
    xd = _place(x, mode)
    yd = _place(torch.full(shape, GUARD, dtype=dt), mode)
    ffC.unary_fwd(xd, yd, K.U[name], s)
    if name == "scalar_floor_divide":
        assert torch.equal(_d(yd), ref), f"{tag}: floor(x / s) must be exact"
    else:
        atol32 = 2 * ULP32 * torch.maximum(x64.abs(), torch.full_like(x64, abs(sf))) \
            if name in ("scalar_sub", "scalar_add") else 0.0
        _check(yd, ref, dt, name in FAST_UNARY, _scale_of(x), "fwd " + tag, lambda: _uf(name, xd, sf), atol32)
    # backward: y as the forward would have left it (the rounded reference), a random dy
    y = ref.to(dt)
    dy = _randn(shape, dt, g)
    dx0 = _randn(shape, dt, g)
    yd2, dyd = _place(y, mode), _place(dy, mode)
    d64 = dy.double() * _udf(name, x64, y.double(), sf)
    rt = RT_BF16 if dt == BF16 else RT_F32
    for acc in (False, True):
        dxd = _place(dx0, mode).clone() if mode == "flat" else _place(dx0, mode)
        ffC.unary_bwd(xd, yd2, dyd, dxd, K.U[name], s, acc)
        ref_dx = d64 + dx0.double() if acc else d64
        scale = _scale_of(x, y, dy, dx0) if acc else _scale_of(x, y, dy)
        _check(dxd, ref_dx, dt, name in FAST_UNARY, scale, f"bwd acc={acc} " + tag,
               lambda: dyd * _udf(name, xd, yd2, sf) + (_place(dx0, "flat") if acc else 0.0),
               extra=rt * d64.abs() if acc else 0.0)
    _guards_intact()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name,s", UNARY_CASES)
def test_unary(ffC, name, s, dt):
    """Every unary op, forward and backward (accumulate off / on): sizes around the vector width,
    a multi-block size with a tail, and for three ops the size at which the capped 2048-block grid
    takes a second stride."""
    v = _vec(dt)
    sizes = [1, v - 1, v, v + 1, 4099]
    if (name, s) in (("relu", 0.0), ("gelu", 0.0), ("scalar_multiply", 1.5)):
        sizes.append(2048 * 256 * v + 256 * v + 5)
    for i, n in enumerate(sizes):
        _unary_case(ffC, name, s, dt, (n,), "flat", 100 + i)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["nhwc", "off1"])
def test_unary_layouts(ffC, mode, dt):
    """Channel-last 4-D tensors (indexed flat in memory order) and contiguous views that start one
    element into their buffer (x, y, dy and dx all off a 16-byte boundary: the scalar kernels)."""
    for i, (name, s) in enumerate(UNARY_CASES):
        _unary_case(ffC, name, s, dt, (2, 8, 3, 5), mode, 200 + i)
        if mode == "off1":
            _unary_case(ffC, name, s, dt, (4099,), mode, 300 + i)


def test_unary_misaligned_mixed(ffC):
    """One misaligned pointer among aligned ones is enough to need the scalar form."""
    x = _randn((4099,), F32, _gen(5))
    ref = torch.relu(x.double())
    for x_mode, y_mode in (("off1", "flat"), ("flat", "off1")):
        xd, yd = _place(x, x_mode), _place(torch.zeros_like(x), y_mode)
        ffC.unary_fwd(xd, yd, K.U["relu"], 0.0)
        _close(yd, ref, 0.0, 0.0, f"relu x {x_mode} y {y_mode}")
    _guards_intact()


def test_unary_wrapper_channels_last():
    """K.unary_fwd / K.unary_bwd keep a channel-last tensor channel-last and give its logical values."""
    g = _gen(6)
    x = _randn((2, 8, 3, 5), BF16, g, 2.0)
    dy = _randn((2, 8, 3, 5), BF16, g)
    xd = _place(x, "nhwc")
    y = K.unary_fwd("gelu", xd)
    assert K.is_nhwc(y)
    ref = F.gelu(x.double())
    _close(y, ref, RT_BF16, AT_BF16 * _scale_of(x), "K.unary_fwd gelu nhwc")
    dx = K.unary_bwd("gelu", xd, y, _place(dy, "flat"))
    _close(dx, dy.double() * _udf("gelu", x.double(), _d(y), 0.0), RT_BF16, AT_BF16 * _scale_of(x, dy),
           "K.unary_bwd gelu nhwc")


# ----------------------------------------------------------------------------------- binary
BIN = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b,
       "div": lambda a, b: a / b, "max": torch.maximum, "min": torch.minimum}
assert set(BIN) == set(K.B)


def _bin_grads(name, a, b, g):
    """fp64 (da, db) at full output shape; max / min without ties."""
    if name == "add":
        return g, g
    if name == "sub":
        return g, -g
    if name == "mul":
        return g * b, g * a
    if name == "div":
        return g / b, -g * a / (b * b)
    first = (a > b) if name == "max" else (a < b)
    z = torch.zeros_like(g)
    return torch.where(first, g, z), torch.where(first, z, g)


def _bin_inputs(name, n, dt, g):
    a = _randn((n,), dt, g, 2.0)
    if name in ("max", "min"):  # b = a + sign * delta, |delta| >= |a| / 8 + 1 / 8: no tie survives bf16 rounding
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        delta = (a.double().abs() / 8 + 0.125) * (1 + torch.rand(n, generator=g).double())
        b = (a.double() + sign * delta).to(dt)
        assert not bool((a == b).any())
    elif name == "div":
        b = _uni((n,), dt, g, 0.5, 4.0) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).to(dt)
    else:
        b = _randn((n,), dt, g, 2.0)
    return a, b


def _bin_atol32(name, a64, b64):
    return 2 * ULP32 * torch.maximum(a64.abs(), b64.abs()) if name in ("add", "sub") else 0.0


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(BIN))
def test_binary_same_shape(ffC, name, dt):
    """Same-shape binary ops: the sizes of test_unary, with and without the fused ReLU, aligned
    (16-byte kernel) and one element into the buffers (the indexed kernel); backward with each of
    da / db switched off once."""
    v = _vec(dt)
    for i, n in enumerate([1, v - 1, v, v + 1, 4099]):
        for mode in ("flat", "off1"):
            g = _gen(400 + i)
            a, b = _bin_inputs(name, n, dt, g)
            dc = _randn((n,), dt, g)
            a64, b64 = a.double(), b.double()
            ad, bd, dcd = _place(a, mode), _place(b, mode), _place(dc, mode)
            tag = f"{name} {DT_IDS[DTYPES.index(dt)]} n={n} {mode}"
            for relu in (False, True):
                cd = _place(torch.full((n,), GUARD, dtype=dt), mode)
                ffC.binary_fwd(ad, bd, cd, K.B[name] | (0x100 if relu else 0), [n], [1], [1], True)
                ref = BIN[name](a64, b64)
                _check(cd, torch.relu(ref) if relu else ref, dt, False, _scale_of(a, b), f"fwd relu={relu} " + tag,
                       atol32=_bin_atol32(name, a64, b64))
            ra, rb = _bin_grads(name, a64, b64, dc.double())
            rt32 = 2.0 ** -21 if name == "div" else RT_F32  # db of div: three multiplies and a divide
            for need_a, need_b in ((True, True), (False, True), (True, False)):
                da = _place(torch.full((n,), GUARD, dtype=dt), mode) if need_a else None
                db = _place(torch.full((n,), GUARD, dtype=dt), mode) if need_b else None
                ffC.binary_bwd(ad, bd, dcd, da, db, K.B[name], [n], [1], [1], True)
                for got, r, nm in ((da, ra, "da"), (db, rb, "db")):
                    if got is None:
                        continue
                    if dt == BF16:
                        _close(got, r, RT_BF16, AT_BF16 * _scale_of(a, b, dc), f"bwd {nm} " + tag)
                    else:
                        _close(got, r, rt32, 0.0, f"bwd {nm} " + tag)
            _guards_intact()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", ["max", "min"])
def test_binary_minmax_ties(ffC, name, dt):
    """a == b everywhere: the kernel gives the whole gradient to one side (torch halves it). The
    contract is that the gradient is conserved: da + db == dc exactly, each of them 0 or dc."""
    g = _gen(9)
    n = 4099
    a = _randn((n,), dt, g)
    dc = _randn((n,), dt, g)
    ad, dcd = _place(a), _place(dc)
    da, db = torch.empty_like(ad), torch.empty_like(ad)
    ffC.binary_bwd(ad, ad.clone(), dcd, da, db, K.B[name], [n], [1], [1], True)
    da, db, dc64 = _d(da), _d(db), dc.double()
    assert torch.equal(da + db, dc64)
    assert bool(((da == 0) | (da == dc64)).all()) and bool(((db == 0) | (db == dc64)).all())


BCAST = [((4, 1, 5), (3, 1)), ((2, 3, 4, 5), (5,)), ((7,), (1,)), ((2, 1, 3, 1, 2, 1), (1, 4, 1, 5, 1, 3)),
         ((1,), (2, 3))]


def _grid_values(shape, g, frac, dt):
    """integer + frac in [-8, 8]: exact in bf16, never zero, and two operands built with different
    fractions never tie."""
    return (torch.randint(-8, 8, shape, generator=g).double() + frac).to(dt)


def _sum_to(t, shape):
    nd = t.dim()
    shp = [1] * (nd - len(shape)) + list(shape)
    dims = [i for i in range(nd) if shp[i] == 1 and t.shape[i] != 1]
    return (t.sum(dim=dims, keepdim=True) if dims else t).reshape(shape)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sa,sb", BCAST, ids=[f"{a}x{b}".replace(" ", "") for a, b in BCAST])
@pytest.mark.parametrize("name", list(BIN))
def test_binary_broadcast(name, sa, sb, dt):
    """Broadcast forward (with and without ReLU) and backward through K.binary_fwd / K.binary_bwd:
    the reduced gradients against the fp64 sums, the bound scaled by what was summed."""
    g = _gen(11)
    a, b = _grid_values(sa, g, 0.25, dt), _grid_values(sb, g, 0.5, dt)
    a64, b64 = a.double(), b.double()
    out_shape = torch.broadcast_shapes(sa, sb)
    dc = _randn(out_shape, dt, g)
    ad, bd, dcd = _place(a), _place(b), _place(dc)
    tag = f"{name} {sa}x{sb} {DT_IDS[DTYPES.index(dt)]}"
    ref = BIN[name](a64, b64)
    full = lambda t: t.expand(out_shape)  # noqa: E731
    for relu in (False, True):
        c = K.binary_fwd(name, ad, bd, relu=relu)
        assert tuple(c.shape) == tuple(out_shape)
        _check(c, torch.relu(ref) if relu else ref, dt, False, _scale_of(full(a), full(b)), f"fwd relu={relu} " + tag,
               atol32=_bin_atol32(name, full(a64), full(b64)))
    ra, rb = _bin_grads(name, full(a64), full(b64), dc.double())
    rt = RT_BF16 if dt == BF16 else (2.0 ** -21 if name == "div" else RT_F32)
    for need_a, need_b in ((True, True), (False, True), (True, False)):
        da, db = K.binary_bwd(name, ad, bd, dcd, need_a=need_a, need_b=need_b)
        assert (da is None) == (not need_a) and (db is None) == (not need_b)
        for got, r, shp, nm in ((da, ra, sa, "da"), (db, rb, sb, "db")):
            if got is None:
                continue
            assert tuple(got.shape) == tuple(shp)
            k = r.numel() // max(1, math.prod(shp))  # terms summed per element
            # every term carries one rounding of its own (stored in dt at full shape), the fp32 sum of
            # k terms k more at the sum's scale, the result one more
            atol = rt * _sum_to(r.abs(), shp) * (1 + k * 2.0 ** -24 / rt)
            if dt == BF16:
                atol = atol + AT_BF16 * _sum_to(_scale_of(full(a), full(b), dc), shp)
            _close(got, _sum_to(r, shp), rt, atol, f"bwd {nm} (k={k}) " + tag)


# ------------------------------------------------------------------------------------- cast
def _cast_specials():
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # halfway ties: to even down / up, both signs
            0x3F807FFF, 0x3F808001,  # one fp32 ulp either side of a tie
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
            0x7F7FFFFF, 0xFF7FFFFF,  # the largest finite fp32: rounds to inf
            0x00010000, 0x00018000, 0x80028000, 0x007F8000,  # bf16 subnormals, two of them ties
            0x7FC00000]  # NaN
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


@pytest.mark.parametrize("n", [1, 255, 257])
def test_cast(ffC, n):
    """fp32 -> bf16 equals round-to-nearest-even bit for bit (ties, signed zeros, infinities, overflow
    to inf, subnormals; NaN stays NaN); bf16 -> fp32 and the same-type copies are exact."""
    sp = _cast_specials()
    cases = [torch.cat([sp, _randn((300,), F32, _gen(n), 50.0)])[:n]]
    if n == 1:
        cases += [sp[i:i + 1] for i in range(sp.numel())]
    for x in cases:
        xd = x.to(DEV)
        y = torch.empty(x.numel(), dtype=BF16, device=DEV)
        ffC.cast(xd, y)
        want = x.bfloat16()
        nan = torch.isnan(x)
        assert torch.equal(torch.isnan(y.cpu()), nan)
        assert torch.equal(y.cpu().view(torch.int16)[~nan], want.view(torch.int16)[~nan]), (x, y.cpu(), want)
        back = torch.empty(x.numel(), dtype=F32, device=DEV)
        ffC.cast(y, back)
        assert torch.equal(back.cpu()[~nan], want.float()[~nan]) and bool(torch.isnan(back.cpu()[nan]).all())
        for src in (xd, y):
            dst = torch.empty_like(src)
            ffC.cast(src, dst)
            bits = torch.int32 if src.dtype == F32 else torch.int16
            assert torch.equal(dst.view(bits)[~nan.to(DEV)], src.view(bits)[~nan.to(DEV)])
            assert bool(torch.isnan(dst[nan.to(DEV)]).all())


# ---------------------------------------------------------------------------------- dropout
def _dropout(ffC, x, rate, seed, offset):
    y = torch.full_like(x, GUARD)
    mask = torch.full((x.numel(),), 7, dtype=torch.uint8, device=DEV)
    ffC.dropout_fwd(x, y, mask, rate, seed, offset)
    return y, mask


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rate", [0.0, 0.25, 0.9])
def test_dropout(ffC, rate, dt):
    n = 1 << 16
    g = _gen(21)
    x = _randn((n,), dt, g, 2.0)
    xd = x.to(DEV)
    y, mask = _dropout(ffC, xd, rate, 1234, 0)
    m = mask.cpu()
    assert bool(((m == 0) | (m == 1)).all())
    keep = m.bool()
    # y = x / (1 - rate) where kept (the kernel multiplies by the fp32 reciprocal: two roundings), else 0
    assert bool((y.cpu()[~keep] == 0).all())
    ref = x.double() / (1.0 - _f32(rate))
    if rate == 0.0:
        assert torch.equal(y.cpu(), x)
    _check(y.cpu()[keep], ref[keep], dt, False, _scale_of(x)[keep], f"dropout rate={rate}")
    # kept fraction: within 5 binomial standard deviations
    p = 1.0 - rate
    assert abs(int(keep.sum()) - n * p) <= 5 * math.sqrt(n * p * (1 - p)), int(keep.sum())
    # same (seed, offset): same mask; another seed: another mask
    _, mask2 = _dropout(ffC, xd, rate, 1234, 0)
    assert torch.equal(mask, mask2)
    if rate > 0:
        _, mask3 = _dropout(ffC, xd, rate, 1235, 0)
        assert not torch.equal(mask, mask3)
    # the sharding promise: the mask at offset k is the offset-0 mask shifted by k
    k, ns = 1000, 5000
    _, m0 = _dropout(ffC, xd[:ns].contiguous(), rate, 77, 0)
    _, mk = _dropout(ffC, xd[:ns].contiguous(), rate, 77, k)
    assert torch.equal(mk[:ns - k], m0[k:])
    # backward, accumulate off / on
    dy = _randn((n,), dt, g)
    dx0 = _randn((n,), dt, g)
    d64 = torch.where(keep, dy.double() / (1.0 - _f32(rate)), torch.zeros(n, dtype=torch.float64))
    rt = RT_BF16 if dt == BF16 else RT_F32
    for acc in (False, True):
        dx = dx0.to(DEV)
        ffC.dropout_bwd(dy.to(DEV), mask, dx, rate, acc)
        _check(dx, d64 + dx0.double() if acc else d64, dt, False, _scale_of(dy, dx0) if acc else _scale_of(dy),
               f"dropout_bwd rate={rate} acc={acc}", extra=rt * d64.abs() if acc else 0.0)


# ---------------------------------------------------------------------------------- softmax
def _softmax_check(ffC, x, scale, dt, what, scale64=None):
    """softmax_fwd of x (CPU, dt) against torch.softmax in fp64; returns the device output."""
    rows, cols = x.shape
    xd = x.to(DEV)
    y = torch.full_like(xd, GUARD)
    ffC.softmax_fwd(xd, y, rows, cols, scale)
    sf = _f32(scale)
    ref = torch.softmax(x.double() * sf, -1)
    _check(y, ref, dt, True, _scale_of(x) if scale64 is None else scale64, what,
           lambda: torch.softmax(xd * sf, -1))
    return y


def _softmax_bwd_check(ffC, y, dy, scale, dt, what):
    """softmax_bwd from the probabilities y and dy (CPU, dt): dx = scale * y * (dy - sum(y * dy))."""
    rows, cols = y.shape
    sf = _f32(scale)
    y64, dy64 = y.double(), dy.double()
    d64 = sf * y64 * (dy64 - (y64 * dy64).sum(-1, keepdim=True))
    dx0 = _randn((rows, cols), dt, _gen(31))
    yd, dyd = y.to(DEV), dy.to(DEV)
    rt = RT_BF16 if dt == BF16 else RT_F32
    # operand scale of the row: dy - sum(y dy) is at most 2 max|dy|
    rs = (sf * dy64.abs().amax(-1, keepdim=True)).clamp_min(1.0).expand(rows, cols)
    out = None
    for acc in (False, True):
        dx = dx0.to(DEV)
        ffC.softmax_bwd(yd, dyd, dx, rows, cols, scale, acc)
        ydf, dydf = yd.float(), dyd.float()
        _check(dx, d64 + dx0.double() if acc else d64, dt, True, torch.maximum(rs, _scale_of(dx0)) if acc else rs,
               f"{what} acc={acc}",
               lambda: (sf * ydf * (dydf - (ydf * dydf).sum(-1, keepdim=True)) + (dx0.to(DEV) if acc else 0.0)),
               extra=rt * d64.abs() if acc else 0.0)
        if not acc:
            out = dx
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 127, 1000])
def test_softmax(ffC, cols, dt):
    """Row softmax forward / backward: one row, a few rows, and more rows than the capped grid has
    waves (a wave takes a second row); widths around the 64-lane wave; three scales."""
    for rows in (1, 5, 3077):
        for scale in (1.0, 0.125, 2.0):
            g = _gen(rows * 7 + cols)
            x = _randn((rows, cols), dt, g, 3.0)
            tag = f"softmax {rows}x{cols} scale={scale} {DT_IDS[DTYPES.index(dt)]}"
            _softmax_check(ffC, x, scale, dt, "fwd " + tag)
            y = torch.softmax(x.double() * _f32(scale), -1).to(dt)
            _softmax_bwd_check(ffC, y, _randn((rows, cols), dt, g), scale, dt, "bwd " + tag)


def test_softmax_wide_logits(ffC):
    """fp32 logits spread over +-1e4: no overflow, and as close to the fp64 softmax as torch's own
    (the error scale is 1 here, not |x|: stricter than the general rule)."""
    g = _gen(41)
    x = _uni((5, 1000), F32, g, -1e4, 1e4)
    x[0, :3] = 1e4  # a three-way tie at the top
    y = _softmax_check(ffC, x, 1.0, F32, "softmax +-1e4", scale64=1.0)
    assert bool(torch.isfinite(y).all())
    _close(y.double().sum(-1), torch.ones(5, dtype=torch.float64), 0.0, 1000 * 2.0 ** -24, "row sums")


def _masked_patterns():
    g = _gen(43)
    pats = {}
    for c in (24, 33, 64, 65, 200):
        pats[f"causal{c}"] = torch.randn(c, c, generator=g).masked_fill(torch.ones(c, c).triu(1).bool(), -math.inf)
    for first in (64, 130):  # a lane sees -inf before its finite values
        x = torch.randn(5, 200, generator=g)
        x[:, :first] = -math.inf
        pats[f"prefix{first}"] = x
    x = torch.randn(9, 200, generator=g)
    x[torch.rand(9, 200, generator=g) < 0.1] = -math.inf
    x[:, 77] = 0.5  # no row entirely masked
    pats["isolated"] = x
    x = torch.randn(6, 130, generator=g)
    x[2] = -math.inf
    x[4, 64:] = -math.inf
    pats["full_row"] = x
    return pats


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("pat", ["causal24", "causal33", "causal64", "causal65", "causal200", "prefix64",
                                 "prefix130", "isolated", "full_row"])
def test_softmax_masked(ffC, pat, dt):
    """-inf logits contribute 0: causal and prefix masks, isolated entries, and one row entirely
    -inf, which is NaN exactly where torch's is while the other rows are unaffected. The backward on
    the masked outputs (y = 0) gives 0 there and no NaN."""
    x = _masked_patterns()[pat].to(dt)
    y = _softmax_check(ffC, x, 1.0, dt, f"softmax {pat}")
    ref = torch.softmax(x.double(), -1)
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(ref))
    rows_ok = ~torch.isnan(ref).any(-1)
    assert bool((y.cpu()[rows_ok][torch.isinf(x[rows_ok])] == 0).all())
    yk = ref[rows_ok].to(dt)
    dy = _randn(tuple(yk.shape), dt, _gen(44))
    dx = _softmax_bwd_check(ffC, yk, dy, 1.0, dt, f"softmax_bwd {pat}").cpu()
    assert bool(torch.isfinite(dx).all()) and bool((dx[yk == 0] == 0).all())


# ----------------------------------------------------------------------------- softmax_xent
def _xent_case(ffC, x, labels, dt, what, place_logits="flat"):
    """Fused softmax + sparse cross-entropy of the logits x (CPU, dt) against fp64: loss, gradient,
    acc3 = {correct, sum CE, rows}."""
    rows, cols = x.shape
    gscale = 1.0 / rows
    gs = _f32(gscale)
    xd = _place(x, place_logits)
    lab = labels.to(torch.int32).to(DEV)
    loss = torch.full((rows,), GUARD, device=DEV)
    d = torch.full((rows, cols), GUARD, dtype=dt, device=DEV)
    acc3 = torch.tensor([1.0, 2.0, 3.0], device=DEV)  # accumulated into, not overwritten
    ffC.softmax_xent(xd, lab, loss, d, rows, cols, gscale, acc3)
    x64 = x.double()
    valid = (labels >= 0) & (labels < cols)
    safe = labels.clamp(0, cols - 1).long()
    lse = torch.logsumexp(x64, -1)
    ref_loss = torch.where(valid, lse - x64.gather(1, safe[:, None])[:, 0], torch.zeros(rows, dtype=torch.float64))
    onehot = F.one_hot(safe, cols).double() * valid[:, None]
    ref_d = (torch.softmax(x64, -1) - onehot) * gs
    xf = xd.float()
    oh_dev = onehot.float().to(DEV)
    lab_dev = safe.to(DEV)
    _yard(loss, torch.where(valid.to(DEV), torch.logsumexp(xf, -1) - xf.gather(1, lab_dev[:, None])[:, 0],
                            torch.zeros(rows, device=DEV)),
          ref_loss, _scale_of(x).amax(-1), "loss " + what)
    _check(d, ref_d, dt, True, gs * _scale_of(x), "dlogits " + what, lambda: (torch.softmax(xf, -1) - oh_dev) * gs)
    correct = float((x64.argmax(-1) == labels).sum())  # torch's argmax returns the first maximum
    got = acc3.cpu().double()
    assert got[0] == 1.0 + correct and got[2] == 3.0 + rows, (got, correct)
    _close(got[1:2], 2.0 + ref_loss.sum().reshape(1), 0.0,
           2.0 ** -24 * (2.0 + rows * ref_loss.abs().sum()) + 16 * 2.0 ** -24 * ref_loss.abs().sum(), "acc3 CE " + what)
    _guards_intact()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cols", [65, 1001, 4096])
def test_softmax_xent_masked(ffC, cols, dt):
    """-inf logits in columns that are not the label (the two-pass kernel; 4096 bf16 columns would take
    the register-resident kernel only under FF_XENT_REG, which is left unset)."""
    g = _gen(cols)
    rows = 7
    x = _randn((rows, cols), dt, g, 3.0)
    labels = torch.randint(0, cols, (rows,), generator=g)
    mask = torch.rand(rows, cols, generator=g) < 0.3
    mask[torch.arange(rows), labels] = False
    mask[1, :min(cols, 200)] = True  # a masked prefix: lanes that see -inf first
    mask[1, labels[1]] = False
    x[mask] = -math.inf
    _xent_case(ffC, x, labels, dt, f"xent masked {rows}x{cols} {DT_IDS[DTYPES.index(dt)]}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_softmax_xent_label_out_of_range(ffC, dt):
    """A label outside [0, cols): loss 0, the row still counted, the gradient the plain softmax."""
    g = _gen(51)
    x = _randn((6, 130), dt, g, 3.0)
    labels = torch.tensor([3, -1, 130, 129, 0, 1000])
    _xent_case(ffC, x, labels, dt, f"xent labels out of range {DT_IDS[DTYPES.index(dt)]}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_softmax_xent_row_phase(ffC, dt):
    """logits one element into their buffer, dlogits aligned: the rows of the two have different
    16-byte phases and the gradient pass takes its scalar branch."""
    g = _gen(52)
    x = _randn((5, 1001), dt, g, 3.0)
    labels = torch.randint(0, 1001, (5,), generator=g)
    _xent_case(ffC, x, labels, dt, f"xent misaligned logits {DT_IDS[DTYPES.index(dt)]}", place_logits="off1")


# -------------------------------------------------------------- xent_grad / mse_grad / metrics
CLAMP = _f32(1e-12)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sparse", [True, False], ids=["sparse", "onehot"])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
def test_xent_grad(ffC, cols, sparse, dt):
    """(p - t) * gscale and the per-row CE from probabilities; a probability of exactly 0 at the
    label gives -log(1e-12) by the clamp."""
    g = _gen(60 + cols)
    rows = 6
    gscale = 1.0 / rows
    gs = _f32(gscale)
    p = torch.softmax(torch.randn(rows, cols, generator=g) * 2, -1).to(dt)
    labels = torch.randint(0, cols, (rows,), generator=g)
    p[0, labels[0]] = 0.0
    t = F.one_hot(labels, cols).to(dt)
    pd, td = p.to(DEV), t.to(DEV)
    d = torch.full((rows, cols), GUARD, dtype=dt, device=DEV)
    loss = torch.full((rows,), GUARD, device=DEV)
    ffC.xent_grad(pd, labels.to(torch.int32).to(DEV) if sparse else None, None if sparse else td, d, loss, rows, cols,
                  gscale, sparse)
    p64, t64 = p.double(), t.double()
    tag = f"xent_grad {rows}x{cols} {'sparse' if sparse else 'onehot'} {DT_IDS[DTYPES.index(dt)]}"
    _check(d, (p64 - t64) * gs, dt, False, gs * _scale_of(p), "dprobs " + tag,
           atol32=2 * ULP32 * gs * torch.maximum(p64, t64))
    ref_loss = -(t64 * torch.log(p64.clamp_min(CLAMP))).sum(-1)
    assert abs(loss[0].item() + math.log(CLAMP)) <= 16 * ULP32 * abs(math.log(CLAMP))  # 16 fp32 ulps of the value
    _yard(loss, -(td.float() * torch.log(pd.float().clamp_min(CLAMP))).sum(-1), ref_loss, 1.0, "loss " + tag)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_mse_grad(ffC, n, dt):
    """Gradient per element; the loss against the fp64 sum. The inputs are multiples of 2^-6 in
    [-4, 4], so every (pred - label)^2 is exact in fp32 and only the unordered fp32 sum of n terms
    errs: n * 2^-24 relative to the sum of the terms' magnitudes."""
    g = _gen(70)
    pred = (torch.randint(-256, 257, (n,), generator=g).double() / 64).to(dt)
    label = (torch.randint(-256, 257, (n,), generator=g).double() / 64).to(dt)
    gscale = 2.0 / n
    d = torch.full((n,), GUARD, dtype=dt, device=DEV)
    loss = torch.zeros(1, device=DEV)
    ffC.mse_grad(pred.to(DEV), label.to(DEV), d, loss, gscale)
    diff = pred.double() - label.double()
    _check(d, diff * _f32(gscale), dt, False, _f32(gscale) * _scale_of(pred, label), f"mse_grad n={n}",
           atol32=2 * ULP32 * _f32(gscale) * torch.maximum(pred.double().abs(), label.double().abs()))
    terms = diff * diff
    assert torch.equal(terms.float().double(), terms)
    _close(loss, terms.sum().reshape(1), 0.0, n * 2.0 ** -24 * terms.sum().item(), f"mse loss n={n}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_metrics_classify(ffC, dt):
    """argmax with ties (the lowest index wins, within a lane and across lanes), a label out of
    range (never correct, no CE, still counted), and accumulation over two calls."""
    cols = 130
    #        tied maxima at        expected argmax   label
    spec = [((5, 70), 5, 5),       # lanes 5 and 6: the lower index, from the other lane
            ((3, 67), 3, 67),      # the same lane twice: the first one seen; label is the loser
            ((64, 1), 1, 1),       # lane 0 (index 64) against lane 1 (index 1)
            ((129,), 129, 129),    # the last column
            ((0, 63, 64, 128), 0, -1),    # label out of range
            ((10,), 10, 130)]      # label out of range
    rows = len(spec)
    p = torch.full((rows, cols), 0.125, dtype=torch.float64)
    for r, (idx, _, _) in enumerate(spec):
        p[r, list(idx)] = 0.5
    p = p.to(dt)
    labels = torch.tensor([s[2] for s in spec], dtype=torch.int32)
    want_correct = sum(1 for _, am, lab in spec if am == lab)
    ce = sum(-math.log(p[r, lab].double().item()) for r, (_, _, lab) in enumerate(spec) if 0 <= lab < cols)
    out = torch.zeros(3, device=DEV)
    for call in (1, 2):
        ffC.metrics_classify(p.to(DEV), labels.to(DEV), rows, cols, out)
        got = out.cpu().double()
        assert got[0] == call * want_correct and got[2] == call * rows, got
        # probabilities are powers of two: the fast log is exact up to a few ulps of log 2
        assert abs(got[1] - call * ce) <= 16 * 2.0 ** -24 * call * ce, (got, ce)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("outer,red,inner", [(1, 1, 1), (3, 7, 1), (1, 5, 9), (4, 33, 65)])
def test_reduce_rows(ffC, outer, red, inner, mean, dt):
    x = _randn((outer, red, inner), dt, _gen(80), 2.0)
    y = torch.full((outer, inner), GUARD, dtype=dt, device=DEV)
    ffC.reduce_rows(x.to(DEV), y, outer, red, inner, mean)
    x64 = x.double()
    ref = x64.mean(1) if mean else x64.sum(1)
    # a sequential fp32 sum of `red` terms (+ the division): (red + 2) half-ulps at the terms' scale
    atol = (red + 2) * 2.0 ** -24 * x64.abs().sum(1) / (red if mean else 1)
    _close(y, ref, RT_BF16 if dt == BF16 else 0.0, atol, f"reduce_rows {(outer, red, inner)} mean={mean}")


# ------------------------------------------------------------------------------- optimizers
def _opt_tol(ref64, step):
    """16 fp32 ulps of max(1, |value|) per step taken (at most 8 roundings per element and step, doubled)."""
    return 16 * step * ULP32 * ref64.abs().clamp_min(1.0)


@pytest.mark.parametrize("max_blocks", [0, 2, -1, -8])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 10001])
def test_sgd_update(ffC, n, max_blocks):
    """Three SGD steps with fresh gradients against the fp64 recurrence: momentum, Nesterov, weight
    decay, gradient scale, with and without the bf16 copy; capped and short-lived grids."""
    lr = 0.1
    for momentum in (0.0, 0.9):
        for nesterov in (False, True):
            for wd in (0.0, 0.01):
                for gscale in (1.0, 0.5):
                    for with_lowp in (False, True):
                        g = _gen(90)
                        w0 = _randn((n,), F32, g)
                        w = w0.to(DEV)
                        mom = torch.zeros(n, device=DEV) if momentum > 0 else None
                        lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV) if with_lowp else None
                        w64, v64 = w0.double(), torch.zeros(n, dtype=torch.float64)
                        tag = f"sgd n={n} mb={max_blocks} mom={momentum} nest={nesterov} wd={wd} gs={gscale}"
                        for step in (1, 2, 3):
                            grad = _randn((n,), F32, g)
                            ffC.sgd_update(w, grad.to(DEV), mom, lowp, lr, momentum, nesterov, wd, gscale, max_blocks)
                            gt = grad.double() * _f32(gscale) + _f32(wd) * w64
                            if momentum > 0:
                                v64 = v64 * _f32(momentum) + gt
                                gt = gt + _f32(momentum) * v64 if nesterov else v64
                            w64 = w64 - _f32(lr) * gt
                            _close(w, w64, 0.0, _opt_tol(w64, step), f"w step {step} " + tag)
                            if mom is not None:
                                _close(mom, v64, 0.0, _opt_tol(v64, step), f"mom step {step} " + tag)
                            if lowp is not None:
                                assert torch.equal(lowp, w.bfloat16()), f"lowp step {step} " + tag


@pytest.mark.parametrize("max_blocks", [0, 2, -1, -8])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 10001])
def test_adam_update(ffC, n, max_blocks):
    """Three Adam steps (alpha_t changing per step) against the fp64 recurrence; once with the step
    size read from device memory and a deliberately wrong alpha_t argument."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    one = np.float32(1.0)
    c1, c2 = float(one - np.float32(b1)), float(one - np.float32(b2))  # 1 - beta as the kernel forms it
    for wd in (0.0, 0.01):
        for gscale in (1.0, 0.5):
            for use_dev in (False, True):
                g = _gen(91)
                w0 = _randn((n,), F32, g)
                w = w0.to(DEV)
                m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
                lowp = torch.full((n,), GUARD, dtype=BF16, device=DEV)
                alpha_dev = torch.zeros(1, device=DEV) if use_dev else None
                w64 = w0.double()
                m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
                tag = f"adam n={n} mb={max_blocks} wd={wd} gs={gscale} alpha_dev={use_dev}"
                for step in (1, 2, 3):
                    alpha_t = 1e-2 * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
                    grad = _randn((n,), F32, g)
                    if use_dev:
                        alpha_dev.fill_(alpha_t)
                        ffC.adam_update(w, grad.to(DEV), m, v, lowp, 123.0, b1, b2, wd, eps, gscale, max_blocks, alpha_dev)
                    else:
                        ffC.adam_update(w, grad.to(DEV), m, v, lowp, alpha_t, b1, b2, wd, eps, gscale, max_blocks)
                    gt = grad.double() * _f32(gscale) + _f32(wd) * w64
                    m64 = _f32(b1) * m64 + c1 * gt
                    v64 = _f32(b2) * v64 + c2 * gt * gt
                    w64 = w64 - _f32(alpha_t) * m64 / (v64.sqrt() + _f32(eps))
                    _close(w, w64, 0.0, _opt_tol(w64, step), f"w step {step} " + tag)
                    _close(m, m64, 0.0, _opt_tol(m64, step), f"m step {step} " + tag)
                    _close(v, v64, 0.0, _opt_tol(v64, step), f"v step {step} " + tag)
                    assert torch.equal(lowp, w.bfloat16()), f"lowp step {step} " + tag


# -------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("bag", [1, 3])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 200])
def test_embedding(ffC, dim, bag, idt, dt):
    """Bag lookup (sum / avg) and its scatter-add backward: ids -1 and num_rows contribute nothing,
    duplicates within a bag and across rows accumulate, dtable starts non-zero."""
    n_out, n_tab = 37, 50
    g = _gen(95)
    idx = torch.randint(0, n_tab, (n_out, bag), generator=g)
    idx[0, 0], idx[1, -1] = -1, n_tab  # out of range: another shard's rows
    idx[2, :] = 7  # a duplicate within the bag ...
    idx[3, 0], idx[5, -1] = 7, 7  # ... and across rows
    table = _randn((n_tab, dim), dt, g)
    dout = _randn((n_out, dim), dt, g)
    valid = ((idx >= 0) & (idx < n_tab)).double()
    rows64 = table.double()[idx.clamp(0, n_tab - 1)] * valid[..., None]  # [n_out, bag, dim]
    idxd = idx.to(idt).to(DEV)
    for avg in (False, True):
        sc = float(np.float32(1.0) / np.float32(bag)) if avg else 1.0
        tag = f"embedding dim={dim} bag={bag} avg={avg} {DT_IDS[DTYPES.index(dt)]}"
        out = torch.full((n_out, dim), GUARD, dtype=dt, device=DEV)
        ffC.embedding_fwd(idxd, table.to(DEV), out, n_out, bag, dim, avg)
        # an fp32 sum of `bag` terms and the scaling: (bag + 1) half-ulps at the terms' scale
        _close(out, rows64.sum(1) * sc, RT_BF16 if dt == BF16 else 0.0,
               (bag + 1) * 2.0 ** -24 * rows64.abs().sum(1) * sc, "fwd " + tag)
        dt0 = _randn((n_tab, dim), F32, _gen(96))
        dtable = dt0.to(DEV)
        ffC.embedding_bwd(idxd, dout.to(DEV), dtable, n_out, bag, dim, avg)
        ref = dt0.double().clone()
        mag = dt0.double().abs()
        cnt = torch.ones(n_tab, dtype=torch.float64)  # the initial value is a term as well
        for r in range(n_out):
            for b in range(bag):
                i = int(idx[r, b])
                if 0 <= i < n_tab:
                    ref[i] += dout[r].double() * sc
                    mag[i] += dout[r].double().abs() * sc
                    cnt[i] += 1
        # k accumulated terms in an unordered atomic sum: k * 2^-23 * sum |terms| per table element
        _close(dtable, ref, 0.0, cnt[:, None] * ULP32 * mag, "bwd " + tag)


# ----------------------------------------------------------------------------- initialisers
SEEDS = [7, 2 ** 31 + 5]


def test_cpu_hash_open_interval():
    """The CPU hash the device is compared with stays strictly inside (0, 1)."""
    idx = torch.arange(6000, dtype=torch.int64)
    for seed in SEEDS:
        for stream in (0, 1):
            u = K._u01_ref(seed, idx, stream)
            assert bool((u > 0).all()) and bool((u < 1).all())


@pytest.mark.parametrize("seed", SEEDS)
def test_init_uniform(ffC, seed):
    """The device hash equals flexflow_amd.kernels' CPU evaluation of it; a shard launched with its
    global offset gets exactly the unpartitioned tensor's values; bf16 is the fp32 value rounded."""
    n, k = 5000, 777
    lo, hi = -0.375, 1.5  # hi - lo is exact in fp32
    dev = torch.empty(n, device=DEV)
    ffC.init_uniform(dev, lo, hi, seed, 0)
    cpu = torch.empty(n)
    K.init_uniform(cpu, lo, hi, seed)
    # lo + (hi - lo) * u: the device may contract the multiply-add
    _close(dev, cpu.double(), 0.0, ULP32 * max(abs(lo), abs(hi)), f"init_uniform seed={seed}")
    assert bool((dev >= _f32(lo)).all()) and bool((dev <= _f32(hi)).all())
    assert dev.unique().numel() > n // 2
    shard = torch.empty(n - k, device=DEV)
    ffC.init_uniform(shard, lo, hi, seed, k)
    assert torch.equal(shard, dev[k:])
    low = torch.empty(n, dtype=BF16, device=DEV)
    ffC.init_uniform(low, lo, hi, seed, 0)
    assert torch.equal(low, dev.bfloat16())


@pytest.mark.parametrize("seed", SEEDS)
def test_init_normal(ffC, seed):
    """Box-Muller on the hash values against fp64, by the yardstick rule (the yardstick is the CPU
    evaluation in fp32 torch ops); the offset property bit for bit."""
    n, k = 5000, 777
    mean, std = 0.5, 2.0
    dev = torch.empty(n, device=DEV)
    ffC.init_normal(dev, mean, std, seed, 0)
    cpu = torch.empty(n)
    K.init_normal(cpu, mean, std, seed)
    idx = torch.arange(n, dtype=torch.int64)
    a, b = K._u01_ref(seed, idx, 0).double(), K._u01_ref(seed, idx, 1).double()
    ref = mean + std * torch.sqrt(-2 * torch.log(a)) * torch.cos(_f32(2 * math.pi) * b)
    _yard(dev, cpu, ref, max(1.0, abs(mean), abs(std)), f"init_normal seed={seed}")
    shard = torch.empty(n - k, device=DEV)
    ffC.init_normal(shard, mean, std, seed, k)
    assert torch.equal(shard, dev[k:])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 257])
def test_fill(ffC, n, dt):
    for v in (0.0, -1.5, 0.1):
        t = torch.full((n,), GUARD, dtype=dt, device=DEV)
        ffC.fill(t, v)
        assert torch.equal(t.cpu(), torch.full((n,), _f32(v)).to(dt))


# -------------------------------------------------------------------------- layout contract
def _transposed(dt, g, positive=False):
    """A dense but non-contiguous (10, 6) tensor (CPU): the transpose of a (6, 10) one."""
    t = _randn((6, 10), dt, g)
    if positive:
        t = torch.softmax(t.float(), 0).to(dt)
    t = t.t()
    assert not t.is_contiguous() and t.shape == (10, 6)
    return t


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_wrappers_take_transposed_inputs(dt):
    """The functional layer gives the same logical result for a transposed-dense input as for its
    contiguous copy (outputs used to inherit the transpose's strides and were written row-major)."""
    g = _gen(99)
    x, dy = _transposed(dt, g), _transposed(dt, g)
    p = _transposed(dt, g, positive=True)
    labels = torch.randint(0, 6, (10,), generator=g).to(torch.int32).to(DEV)
    xt, dyt, pt = x.to(DEV), dy.to(DEV), p.to(DEV)
    assert not xt.is_contiguous()
    xc, dyc, pc = xt.contiguous(), dyt.contiguous(), pt.contiguous()

    def same(a, b, what):
        a = a if isinstance(a, tuple) else (a,)
        b = b if isinstance(b, tuple) else (b,)
        for u, w in zip(a, b):
            assert u.shape == w.shape and torch.equal(u.contiguous(), w.contiguous()), what

    _, mask = K.dropout_fwd(xc, 0.25, 5, 0)
    same(K.dropout_bwd(dyt, mask, 0.25), K.dropout_bwd(dyc, mask, 0.25), "dropout_bwd")
    same(K.mse_grad(xt, dyt, 0.5), K.mse_grad(xc, dyc, 0.5), "mse_grad")
    same(K.softmax_fwd(xt), K.softmax_fwd(xc), "softmax_fwd")
    same(K.softmax_bwd(pt, dyt), K.softmax_bwd(pc, dyc), "softmax_bwd")
    same(K.xent_grad(pt, labels, None, 0.1, True), K.xent_grad(pc, labels, None, 0.1, True), "xent_grad")
    same(K.softmax_xent(xt, labels, 0.1), K.softmax_xent(xc, labels, 0.1), "softmax_xent")
    # and the logical values are right, not merely consistent
    _check(K.softmax_fwd(xt), torch.softmax(x.double(), -1), dt, True, _scale_of(x), "softmax_fwd of a transpose",
           lambda: torch.softmax(xt.float(), -1))
    keep = mask.view(10, 6).cpu().bool()
    _close(K.dropout_bwd(dyt, mask, 0.25), torch.where(keep, dy.double() / 0.75, torch.zeros(10, 6, dtype=torch.float64)),
           RT_BF16 if dt == BF16 else RT_F32, 0.0, "dropout_bwd of a transpose")


def test_bindings_reject_non_contiguous(ffC):
    """The raw entry points index their tensors flat: a non-contiguous one raises (a host-side check,
    nothing is launched) instead of producing a permuted result."""
    def t(dt=F32):
        return torch.zeros(6, 10, dtype=dt, device=DEV).t()

    def c(dt=F32):
        return torch.zeros(10, 6, dtype=dt, device=DEV)

    mask = torch.zeros(60, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(10, dtype=torch.int32, device=DEV)
    lab_nc = torch.zeros(20, dtype=torch.int32, device=DEV)[::2]
    loss = torch.zeros(10, device=DEV)
    acc3 = torch.zeros(3, device=DEV)
    flat, flat_nc = torch.zeros(60, device=DEV), torch.zeros(120, device=DEV)[::2]
    low_nc = torch.zeros(120, dtype=BF16, device=DEV)[::2]
    idx = torch.zeros(10, dtype=torch.int64, device=DEV)
    idx_nc = torch.zeros(20, dtype=torch.int64, device=DEV)[::2]
    calls = {
        "cast x": lambda: ffC.cast(t(), c(BF16)), "cast y": lambda: ffC.cast(c(), t(BF16)),
        "dropout_fwd x": lambda: ffC.dropout_fwd(t(), c(), mask, 0.5, 1, 0),
        "dropout_fwd y": lambda: ffC.dropout_fwd(c(), t(), mask, 0.5, 1, 0),
        "dropout_bwd dy": lambda: ffC.dropout_bwd(t(), mask, c(), 0.5, False),
        "dropout_bwd dx": lambda: ffC.dropout_bwd(c(), mask, t(), 0.5, False),
        "softmax_fwd x": lambda: ffC.softmax_fwd(t(), c(), 10, 6, 1.0),
        "softmax_fwd y": lambda: ffC.softmax_fwd(c(), t(), 10, 6, 1.0),
        "softmax_bwd y": lambda: ffC.softmax_bwd(t(), c(), c(), 10, 6, 1.0, False),
        "softmax_bwd dy": lambda: ffC.softmax_bwd(c(), t(), c(), 10, 6, 1.0, False),
        "softmax_bwd dx": lambda: ffC.softmax_bwd(c(), c(), t(), 10, 6, 1.0, False),
        "softmax_xent logits": lambda: ffC.softmax_xent(t(), lab, loss, c(), 10, 6, 1.0, acc3),
        "softmax_xent dlogits": lambda: ffC.softmax_xent(c(), lab, loss, t(), 10, 6, 1.0, acc3),
        "softmax_xent labels": lambda: ffC.softmax_xent(c(), lab_nc, loss, c(), 10, 6, 1.0, acc3),
        "xent_grad probs": lambda: ffC.xent_grad(t(), lab, None, c(), loss, 10, 6, 1.0, True),
        "xent_grad dprobs": lambda: ffC.xent_grad(c(), lab, None, t(), loss, 10, 6, 1.0, True),
        "xent_grad onehot": lambda: ffC.xent_grad(c(), None, t(), c(), loss, 10, 6, 1.0, False),
        "mse_grad pred": lambda: ffC.mse_grad(t(), c(), c(), acc3, 1.0),
        "mse_grad label": lambda: ffC.mse_grad(c(), t(), c(), acc3, 1.0),
        "mse_grad dpred": lambda: ffC.mse_grad(c(), c(), t(), acc3, 1.0),
        "metrics_classify probs": lambda: ffC.metrics_classify(t(), lab, 10, 6, acc3),
        "metrics_classify labels": lambda: ffC.metrics_classify(c(), lab_nc, 10, 6, acc3),
        "reduce_rows x": lambda: ffC.reduce_rows(t(), torch.zeros(10, device=DEV), 10, 6, 1, False),
        "reduce_rows y": lambda: ffC.reduce_rows(c(), torch.zeros(20, device=DEV)[::2], 10, 6, 1, False),
        "embedding_fwd idx": lambda: ffC.embedding_fwd(idx_nc, c(), c(), 10, 1, 6, False),
        "embedding_fwd table": lambda: ffC.embedding_fwd(idx, torch.zeros(6, 10, device=DEV).t(), c(), 10, 1, 6, False),
        "embedding_fwd out": lambda: ffC.embedding_fwd(idx, c(), t(), 10, 1, 6, False),
        "embedding_bwd dout": lambda: ffC.embedding_bwd(idx, t(), c(), 10, 1, 6, False),
        "embedding_bwd dtable": lambda: ffC.embedding_bwd(idx, c(), t(), 10, 1, 6, False),
        "init_uniform": lambda: ffC.init_uniform(t(), 0.0, 1.0, 1, 0),
        "init_normal": lambda: ffC.init_normal(t(), 0.0, 1.0, 1, 0),
        "fill": lambda: ffC.fill(t(), 1.0),
        "sgd_update master": lambda: ffC.sgd_update(flat_nc, flat, None, None, 0.1, 0.0, False, 0.0, 1.0),
        "sgd_update grad": lambda: ffC.sgd_update(flat, flat_nc, None, None, 0.1, 0.0, False, 0.0, 1.0),
        "sgd_update mom": lambda: ffC.sgd_update(flat, flat, flat_nc, None, 0.1, 0.9, False, 0.0, 1.0),
        "sgd_update lowp": lambda: ffC.sgd_update(flat, flat, None, low_nc, 0.1, 0.0, False, 0.0, 1.0),
        "adam_update m": lambda: ffC.adam_update(flat, flat, flat_nc, flat, None, 1e-3, 0.9, 0.999, 0.0, 1e-8, 1.0),
        "adam_update v": lambda: ffC.adam_update(flat, flat, flat, flat_nc, None, 1e-3, 0.9, 0.999, 0.0, 1e-8, 1.0),
    }
    for what, call in calls.items():
        with pytest.raises(RuntimeError, match="contiguous"):
            call()
            pytest.fail(f"{what}: a non-contiguous tensor was accepted")


def test_optimizer_bindings_reject_misaligned(ffC):
    """The optimizer kernels use 16-byte accesses of master / grad / m / v and 8-byte ones of the
    bf16 copy; the arenas are aligned by construction, anything else raises."""
    def f(off):
        return torch.zeros(64 + off, device=DEV)[off:]

    def lowp(off):
        return torch.zeros(64 + off, dtype=BF16, device=DEV)[off:]

    sgd = lambda w, g, m, l: ffC.sgd_update(w, g, m, l, 0.1, 0.9, False, 0.0, 1.0)  # noqa: E731
    adam = lambda w, g, m, v, l: ffC.adam_update(w, g, m, v, l, 1e-3, 0.9, 0.999, 0.0, 1e-8, 1.0)  # noqa: E731
    sgd(f(0), f(0), f(0), lowp(0))
    sgd(f(4), f(4), f(4), lowp(4))  # a 16-byte aligned range inside an arena is fine
    adam(f(0), f(0), f(0), f(0), lowp(0))
    bad = [lambda: sgd(f(1), f(0), f(0), None), lambda: sgd(f(0), f(1), f(0), None),
           lambda: sgd(f(0), f(0), f(1), None), lambda: sgd(f(0), f(0), f(0), lowp(1)),
           lambda: sgd(f(0), f(0), f(0), lowp(2)),
           lambda: adam(f(1), f(0), f(0), f(0), None), lambda: adam(f(0), f(2), f(0), f(0), None),
           lambda: adam(f(0), f(0), f(3), f(0), None), lambda: adam(f(0), f(0), f(0), f(1), None),
           lambda: adam(f(0), f(0), f(0), f(0), lowp(1))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="aligned"):
            call()
            pytest.fail(f"misaligned case {i} was accepted")
