"""K.add_rmsnorm_fwd / K.add_rmsnorm_bwd (csrc/kernels/add_rmsnorm.hip), element by element against fp64
references computed from the same bf16 / fp32 inputs (GPU only).

Bounds, from the kernel's rounding steps alone (u = 2^-24, one fp32 rounding; U = 2^-8 for bf16 outputs,
2^-24 for fp32 ones: one rounding of the stored value). L is the longest chain of fp32 adds a row sum
passes through: a lane's own terms (at most 32 in the register forms, ceil(d / 64) in the element form),
6 butterfly steps, at most 8 partial sums of the waves that share a row.

  s     bit for bit: one fp32 add of two exactly widened values, one rounding.
  rstd  mean(s^2) + eps: every square rounded (1), L adds, times 1/d (2: the reciprocal and the product),
        plus eps (1): (L + 4) u relative, all terms being positive. rsqrt halves a relative error and
        adds its own 2 ulp = 4 u:  |rstd - ref| <= ((L + 4) / 2 + 4) u ref.
  y     s * rstd (1), * w (1), the stored rounding, and 1 u for the products of these small terms:
        |y - ref| <= (U + ((L + 4) / 2 + 7) u) |ref|.
  dx    = A - B + ds, A = r g, B = r^3 s mean(g s), g = dy w, with r the fp32 rstd the kernel is given (the
        reference uses the same value). g (1) and r g (1): 2 u |A|. The dot: g (1), g s (1), L adds:
        (L + 2) u r^3 |s| mean|g s|; times 1/d (2), r r r (3), times s (1): 6 u |B|. The subtraction and the
        add of ds round at most at |A| + |B| + |ds| each (2 u). With scale = |A| + |B| + |ds|, since the
        terms cancel:  |dx - ref| <= U scale + u ((L + 2) r^3 |s| mean|g s| + 8 scale).
  dw    += sum over rows of t = dy s r: two roundings a term, at most `rows` adds on any path through the
        wave partials and the fold, one add into the gradient that is already there (pre):
        |dw - (pre + ref)| <= (rows + 3) u (sum|t| + |pre|) per column.
"""
import pytest
import torch

from add_rmsnorm_common import decoder, reference64, step, weights
from flexflow_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-6
u = 2.0 ** -24
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# d: the issue's widths, and either side of the one-wave / shared-row cut (4 chunks of 64 lanes x 16 bytes)
WIDTHS = {"bf16": [8, 512, 520, 100, 2048, 2056, 4096, 8192], "fp32": [8, 512, 520, 100, 1024, 1028, 4096, 8192]}
# rows: 1; one fewer than a workgroup's waves (4, or 8 for fp32 rows past 4096 columns); 5, the smallest count
# at which one group takes two rows and another one (groups = ceil(rows / 4), whole workgroups of 4 waves)
ROWS = [1, 3, 5, 7]
CASES = [(dt, d, rows, 0) for dt in DTYPES for d in WIDTHS[dt] for rows in ROWS]
CASES += [(dt, 8, 8197, 0) for dt in DTYPES]  # past the cap of 2048 waves: 4 or 5 rows a wave, a 2048-row fold
# every operand a view one element into its buffer, at a width the 16-byte forms would serve: the element form
CASES += [(dt, 520, 5, 1) for dt in DTYPES]


def _inputs(dt, rows, d, offset, seed):
    """x, res, w, dy, ds, dw_pre; with offset = 1 each is a view one element into its buffer."""
    g = torch.Generator().manual_seed(seed)

    def mk(n, scale=1.0, shift=0.0, dtype=dt):
        buf = (torch.randn(n + offset, generator=g) * scale + shift).to(dtype).to(DEV)
        return buf[offset:]
    x, res, dy, ds = (mk(rows * d).view(rows, d) for _ in range(4))
    return x, res, mk(d, 0.5, 1.0), dy, ds, mk(d, dtype=torch.float32)


def _le(got, ref, bound, what):
    excess = (got.double().cpu() - ref).abs() - bound
    i = int(excess.argmax())
    assert excess.reshape(-1)[i] <= 0, (f"{what}: worst element {i}: got {got.reshape(-1)[i].item()!r}, ref "
                                        f"{ref.reshape(-1)[i].item()!r}, allowed {bound.reshape(-1)[i].item():.3e}")


def _check(dt_name, d, rows, offset=0):
    dt = DTYPES[dt_name]
    U = 2.0 ** -8 if dt == torch.bfloat16 else u
    elem_form = bool(offset) or d % (16 // torch.empty(0, dtype=dt).element_size()) != 0
    L = (-(-d // 64) if elem_form else 32) + 6 + 8  # the longest chain of adds (module docstring)
    x, res, w, dy, ds, pre = _inputs(dt, rows, d, offset, 1000 * d + rows)
    s, y, rstd = K.add_rmsnorm_fwd(x, res, w, EPS)
    s_ref = (x.float() + res.float()).to(dt)
    assert torch.equal(s, s_ref), "s is not the rounded fp32 sum"
    s64, w64 = s_ref.double().cpu(), w.double().cpu()
    r64 = 1.0 / torch.sqrt((s64 * s64).mean(-1) + EPS)
    _le(rstd, r64, ((L + 4) / 2 + 4) * u * r64, "rstd")
    y64 = s64 * r64[:, None] * w64
    _le(y, y64, (U + ((L + 4) / 2 + 7) * u) * y64.abs(), "y")

    r = rstd.double().cpu()[:, None]  # the backward's own input
    dy64, ds64 = dy.double().cpu(), ds.double().cpu()
    g64 = dy64 * w64
    A, m = r * g64, (g64 * s64).mean(-1, keepdim=True)
    B = r ** 3 * s64 * m
    t = dy64 * s64 * r
    for with_ds in (False, True):
        dw = pre.clone()
        dx = K.add_rmsnorm_bwd(s, w, rstd, dy, ds if with_ds else None, dw)
        extra = ds64 if with_ds else torch.zeros_like(ds64)
        scale = A.abs() + B.abs() + extra.abs()
        chain = (L + 2) * r ** 3 * s64.abs() * (g64 * s64).abs().mean(-1, keepdim=True) + 8 * scale
        _le(dx, A - B + extra, U * scale + u * chain, f"dx ds={with_ds}")
        pre64 = pre.double().cpu()
        _le(dw, pre64 + t.sum(0), (rows + 3) * u * (t.abs().sum(0) + pre64.abs()), f"dw ds={with_ds}")
    assert torch.equal(K.add_rmsnorm_bwd(s, w, rstd, dy, None, None), K.add_rmsnorm_bwd(s, w, rstd, dy, None, pre.clone()))


@pytest.mark.parametrize("dt,d,rows,offset", CASES, ids=[f"{dt}-d{d}-r{r}-off{o}" for dt, d, r, o in CASES])
def test_against_fp64(dt, d, rows, offset):
    _check(dt, d, rows, offset)


@pytest.mark.parametrize("dt,rows,d", [("bf16", 37, 520), ("bf16", 9, 4096), ("fp32", 37, 101)])
def test_backward_has_the_same_bits_every_run(dt, rows, d):
    """Several rows a wave (one-wave form, shared-row form, element form): two runs on fresh zeroed dw."""
    x, res, w, dy, ds, _ = _inputs(DTYPES[dt], rows, d, 0, 7)
    s, _, rstd = K.add_rmsnorm_fwd(x, res, w, EPS)
    runs = []
    for _ in range(2):
        dw = torch.zeros(d, device=DEV)
        runs.append((K.add_rmsnorm_bwd(s, w, rstd, dy, ds, dw), dw))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().sum()) > 0


def test_fused_decoder_is_as_close_to_float64_as_the_unfused_one():
    """DecoderConfig.tiny() in bf16 from one seed, fused_norm off and on, one training step each (final_norm
    runs without ds, the other fused norms with the next block's). Both start from the same weights, so one
    float64 run of the model on those bf16 values (reference64) is the reference of both. The yardstick is
    the unfused model's measured distance from it, |loss - ref| and |g - ref|_F / |ref|_F for every weight
    gradient; the fused model's may be at most twice that."""
    flags = ["--no-hip-graphs", "--dtype", "bf16"]
    (plain, dc, tok, lab), fused = decoder(False, flags, seq=32), decoder(True, flags, seq=32)[0]
    W = weights(plain)
    assert list(W) == [w.name for L in fused.layers for w in L.weights]
    assert all((W[k] == v).all() for k, v in weights(fused).items())
    ref_loss, ref = reference64(W, dc, tok, lab)
    (lp, gp), (lf, gf) = step(plain), step(fused)
    dist = {"loss": (abs(lp - ref_loss), abs(lf - ref_loss))}
    dist.update({k: tuple(float((g[k] - ref[k]).norm() / ref[k].norm()) for g in (gp, gf)) for k in ref})
    for k, (unfused, fus) in dist.items():
        print(f"{k}: unfused {unfused:.3e} fused {fus:.3e}")
    assert not [k for k, (unfused, fus) in dist.items() if not fus <= 2 * unfused]
