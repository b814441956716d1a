"""The flash-attention kernels element by element against a float64 oracle (tests/attn_rows_common.py).

The other attention tests take one relative Frobenius error over a whole tensor (o < 2e-2, gradients
< 3e-2): about ten times the error the kernels' own rounding makes, and blind to a fault confined to a
few rows (a mask test on the wrong 32 x 32 block, a tile edge, a key-block loop bound off by one). Here
every element of o, dq, dk and dv must satisfy err <= 1.25 x the bound derived from the kernels'
rounding steps (attn_rows_common's docstring), no element exempt; where the bound is 0 (dk / dv rows
past a length, padding positions, rows that see no key) that is an exact 0. The factor 1.25: the bounds
were tried against an fp32 emulation of the rounding steps (test_attn_rows_cpu.py, largest err / bound
0.89), and the GPU accumulates in another order than that emulation (32-wide MFMA partial sums, an online
softmax whose running maximum moves late, key blocks summed through fp32 slabs or a carried fp32 dQ).

lse has no bound derived tightly, so it is measured: per case the largest error of plain fp32
torch.logsumexp against the float64 oracle on the same inputs (`lse fig` below), and the tolerance is
8 x that figure, floored at 2^-20 max(1, |lse|): the kernel adds three fp32 roundings torch does not
have (scale * log2(e) times the score, the running maximum times ln 2, the fast log). +inf must match
exactly.

Inputs (attn_rows_common.make_inputs): q and k at 1.7 x a unit normal, so the softmax is peaked; key
rows no query sees hold k at 3 x and v = +-64, query rows that see no key hold dO = +-64, so a key that
leaks across a length, a run edge, a -inf bias column or the sequence end dominates its row. q, k, v and
dO sit in allocations whose rows behind the last head hold NaN (memory bounds stay on Sq / Sk, so these
never reach arithmetic); o, lse, dq, dk and dv sit inside sentinel-filled allocations whose guard rows
must keep the sentinel and whose interior starts as NaN; the backward workspace has a guard band.

Cases (B = 1, H = 2, D = 64 unless stated; the table is attn_rows_common.CASES). Each runs the forward
structures 0, 1 and 3 and the backward structures 2 and 10. Combinations the bindings reject are left
out: segments with key lengths or with a score bias. Columns: largest err / bound of the CPU emulation
(bound x 1.0; B * H = 256 cases cut to a few heads), largest err / tolerance on an MI355X over all
structures (tolerance = 1.25 x bound; lse: its own tolerance, 8 x the figure with the floor and without
the factor 1.25), and the lse figure measured on the GPU.

One test goes beyond the per-case comparison, as a positive control on the device:
test_a_length_off_by_one_on_the_device_is_flagged runs the kernels with one key length moved by one
(still inside Sk) and demands that the checker flags rows of that sample and of no other.

case              shape                             | emu  o    dv    dq    dk  | gpu  o    dv    dq    dk   lse  | lse fig
---------------------------------------------------------------------------------------------------------------------------
plain             S128                              |   0.61  0.69  0.17  0.19 |   0.49  0.55  0.14  0.16  0.14 | 1.02e-06
ragged            S200                              |   0.58  0.64  0.18  0.15 |   0.59  0.52  0.11  0.13  0.12 | 1.25e-06
causal            S192 causal                       |   0.75  0.81  0.21  0.25 |   0.51  0.65  0.17  0.20  0.12 | 2.89e-06
two_blocks        S512                              |   0.55  0.66  0.18  0.16 |   0.57  0.53  0.12  0.13  0.13 | 1.25e-06
cross             Sq577 Sk130                       |   0.63  0.53  0.19  0.07 |   0.62  0.43  0.16  0.06  0.07 | 2.28e-06
causal_long       S576 causal                       |   0.69  0.89  0.16  0.25 |   0.61  0.71  0.13  0.20  0.11 | 3.25e-06
d128              S128 D128                         |   0.73  0.72  0.13  0.18 |   0.60  0.58  0.10  0.14  0.07 | 2.52e-06
d128_causal       S200 D128 causal                  |   0.55  0.73  0.12  0.10 |   0.44  0.58  0.10  0.12  0.08 | 6.33e-06
d128_s320         S320 D128                         |   0.60  0.66  0.13  0.14 |   0.58  0.53  0.12  0.11  0.12 | 1.60e-06
chain_s320        B16 H16 S320                      |   0.56  0.70  0.15  0.16 |   0.69  0.64  0.21  0.22  0.12 | 2.53e-06
chain_s320_causal B16 H16 S320 causal               |   0.62  0.83  0.22  0.23 |   0.68  0.72  0.26  0.27  0.10 | 5.21e-06
chain_s512        B16 H16 S512                      |   0.58  0.77  0.20  0.20 |   0.69  0.62  0.22  0.21  0.14 | 2.29e-06
chain_d128        B16 H16 S192 D128                 |   0.56  0.74  0.12  0.16 |   0.72  0.64  0.18  0.20  0.08 | 3.53e-06
fused_layout      B16 H16 S320 [B,S,3,H,D]+dbias    |   0.64  0.62  0.15  0.19 |   0.70  0.64  0.21  0.23  0.12 | 2.56e-06  dbias 0.01
lens              B5 H2 S320 lens5                  |   0.61  0.68  0.21  0.17 |   0.61  0.55  0.20  0.17  0.15 | 1.56e-06
lens_causal       B5 H2 S320 causal lens5           |   0.70  0.80  0.22  0.26 |   0.68  0.64  0.18  0.21  0.08 | 4.80e-06
lens_d128         B3 H2 S200 D128 lens 200,129,64   |   0.67  0.80  0.18  0.13 |   0.62  0.64  0.14  0.10  0.10 | 2.21e-06
chain_lens        B16 H16 S320 lens                 |   0.56  0.70  0.17  0.15 |   0.70  0.62  0.19  0.21  0.14 | 2.04e-06
drop_ragged       S200 thr64                        |   0.73  0.64  0.22  0.19 |   0.58  0.51  0.16  0.13  0.15 | 1.16e-06
drop_d128         S320 D128 thr64                   |   0.61  0.70  0.21  0.12 |   0.72  0.56  0.17  0.11  0.15 | 1.96e-06
drop_chain        B16 H16 S320 thr64                |   0.66  0.70  0.31  0.15 |   0.70  0.63  0.33  0.23  0.14 | 2.24e-06
bias_bcast        B2 H2 Sq200 Sk137 bias bcast      |   0.70  0.76  0.18  0.20 |   0.67  0.61  0.18  0.16  0.14 | 1.71e-06
bias_full         B2 H2 S256 D128 causal bias full  |   0.70  0.81  0.19  0.19 |   0.53  0.65  0.15  0.15  0.09 | 7.29e-06
bias_lens         B2 H2 Sq256 Sk320 lens 320,65 full|   0.66  0.80  0.24  0.25 |   0.62  0.64  0.19  0.15  0.08 | 2.05e-06
bias_drop         B2 H2 S128 thr64 bias full        |   0.69  0.72  0.27  0.18 |   0.54  0.57  0.22  0.15  0.15 | 1.57e-06
seg               B2 H2 S320 segments               |   0.61  0.74  0.21  0.24 |   0.61  0.59  0.17  0.19  0.14 | 1.33e-06
seg_causal        B2 H2 S320 causal segments        |   0.64  0.86  0.22  0.33 |   0.71  0.69  0.17  0.26  0.10 | 3.17e-06
seg_drop          B2 H2 S320 thr64 segments         |   0.75  0.73  0.31  0.18 |   0.67  0.59  0.25  0.15  0.15 | 1.40e-06

lens5 = [320, 257, 256, 1, 0] (edge, mid-tile, block edge, single key, empty sample); chain_lens cycles it
over its 16 samples. dbias of fused_layout: 0.01 of its tolerance.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import attn_rows_common as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
_cache = {}


def _case(ffC, name):
    """The case on the device, its float64 reference and tolerances, built once."""
    if name not in _cache:
        c = R.full_case(R.CASES[name])
        inp = R.make_inputs(name, c)
        ref, tol, fig = R.reference(inp, DEV)
        _cache[name] = (c, R.Launcher(ffC, c, inp, DEV), ref, tol, fig)
    return _cache[name]


def _verdict(tag, res):
    print(f"ROWS-GPU {tag} {R.ratios(res)}")
    assert not R.fails(res), R.fails(res)


@pytest.mark.parametrize("fv", [0, 1, 3])
@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_rows(ffC, name, fv):
    """o and lse of forward structure fv (a structure the shape cannot reach runs the one it falls back
    to): every element within tolerance, lse = +inf exactly where a row sees no key, guards intact."""
    c, L, ref, tol, fig = _case(ffC, name)
    got = L.fwd(fv)
    print(f"ROWS-GPU {name} lse_fig={fig:.2e}")
    _verdict(f"{name} fwd={fv}", R.check(got, ref, tol, R.GPU_FACTOR))


@pytest.mark.parametrize("variant", [2, 10])
@pytest.mark.parametrize("name", list(R.CASES))
def test_backward_rows(ffC, name, variant):
    """dq, dk and dv of backward structure `variant` after the default forward. The fused layout also
    asks for the QKV projection's bias gradient: the chained attn_bwd1b_kernel (structure 10) adds it,
    checked per element against the float64 column sums with the column sums of the per-element
    tolerances; structure 2 declines and leaves dbias alone."""
    c, L, ref, tol, _ = _case(ffC, name)
    L.fwd(ffC.attn_fwd_variant())
    got, done, dbias = L.bwd(variant, want_dbias=c["fused"])
    res = R.check(got, ref, tol, R.GPU_FACTOR)
    _verdict(f"{name} bwd={variant}", res)
    if c["fused"]:
        assert done == (variant == 10)
        if done:
            want = {"dbias": torch.stack([ref[key].sum(dim=(0, 2)) for key in ("dq", "dk", "dv")])}
            wtol = {"dbias": torch.stack([tol[key].sum(dim=(0, 2)) for key in ("dq", "dk", "dv")])}
            have = {"dbias": dbias.view(3, c["H"], c["D"]).double() - 0.5}
            _verdict(f"{name} bwd={variant}", R.check(have, want, wtol, R.GPU_FACTOR))
        else:
            assert torch.equal(dbias, torch.full_like(dbias, 0.5))
    else:
        assert not done


@pytest.mark.parametrize("name,lens", [("lens", [320, 258, 256, 1, 0]), ("lens_d128", [200, 129, 63])])
def test_a_length_off_by_one_on_the_device_is_flagged(ffC, name, lens):
    """The kernels run with one key length moved by one (the reference keeps the case's own): the checker
    must flag rows of o and of a gradient in that sample and in no other, so the comparison above is
    not passing for want of looking."""
    c, _, ref, tol, _ = _case(ffC, name)
    b = [x != y for x, y in zip(lens, c["lens"])].index(True)
    L = R.Launcher(ffC, dict(c, lens=lens), R.make_inputs(name, c), DEV)
    got = L.fwd(ffC.attn_fwd_variant())
    got.update(L.bwd(ffC.attn_bwd_variant())[0])
    res = R.check(got, ref, tol, R.GPU_FACTOR)
    rows = {key: res[key][0] for key in R.OUTS}
    print(f"ROWS-GPU {name} lens {lens}: rows flagged", {key: int(r.sum()) for key, r in rows.items()})
    assert rows["o"][b].any() and (rows["dq"][b].any() or rows["dk"][b].any() or rows["dv"][b].any())
    for key, r in rows.items():
        assert int(r.sum()) == int(r[b].sum()), key
