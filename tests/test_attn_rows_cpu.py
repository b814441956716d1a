"""The per-element attention checker of tests/attn_rows_common.py has teeth, shown without a GPU.

For every case of the table (B * H = 256 cases cut to their listed heads):

* an fp32 torch emulation of the kernels' rounding steps (dropout and bias included) stays within
  1.0 x the derived bounds, so the bounds are not tighter than the arithmetic allows;
* the float64 oracle with one boundary moved by one key (causal diagonal, a key length, a segment run
  edge, Sk, a flipped quad of the dropout mask, the bias shifted by one key) fails the checker, at the
  1.25 x the GPU test uses, in at least one row of o and in at least one of dq / dk / dv. The kernel is
  never mutated. A mutant that passes would mean the case's inputs are too tame;
* a fault confined to one 32-row block of the emulated output (the block scaled by 1.15; the block
  given the diagonal j <= i + 1) is flagged in every row it moved by more than the tolerance plus the
  emulation's own error there (such a row cannot pass), and in no row outside the block. The relative
  Frobenius error is printed beside it: the j <= i + 1 block stays far below the 2e-2 / 3e-2 of the
  whole-tensor tests.

The largest err / bound of the emulation per case is in the table of test_attn_rows_gpu.py.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import attn_rows_common as R  # noqa: E402
from attn_segments_common import runs_of  # noqa: E402

_cache = {}


def _case(name):
    if name not in _cache:
        c = R.cpu_case(R.CASES[name])
        inp = R.make_inputs(name, c)
        ref, tol, fig = R.reference(inp)
        _cache[name] = (c, inp, ref, tol, fig, R.emulate(inp))
    return _cache[name]


def _frob(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulation_stays_inside_the_bounds(name):
    c, inp, ref, tol, fig, emu = _case(name)
    res = R.check(emu, ref, tol, 1.0)
    print(f"ROWS-EMU {name} {R.ratios(res)} lse_fig={fig:.2e} max|lse|={ref['lse'][torch.isfinite(ref['lse'])].abs().max():.1f}")
    assert not R.fails(res), R.fails(res)
    for key in R.OUTS:  # exact zeros where the bound is 0, and the inputs do produce such places where promised
        assert (emu[key].double()[tol[key] == 0] == 0).all(), key
    blind = ~inp["see"].any(-1).expand(c["B"], c["H"], c["Sq"])
    assert (ref["lse"][blind] == R.INF).all() and (tol["dq"][blind] == 0).all() and (tol["o"][blind] == 0).all()
    unseen = ~inp["see"].any(-2).expand(c["B"], c["H"], c["Sk"])
    assert (tol["dk"][unseen] == 0).all() and (tol["dv"][unseen] == 0).all()


def _mutants(c, inp):
    """(label, overrides of reference()) of every boundary mutant the case has."""
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    bias = inp["bias"]

    def see(**kw):
        return torch.from_numpy(R.see_of(c, bias, **kw))

    if c["causal"]:
        for d in (1, -1):
            yield f"diagonal {d:+d}", dict(see=see(diag=d))
    if c["lens"] is not None:
        for b, L in enumerate(c["lens"]):
            for d in (1, -1):
                if 0 <= L + d <= Sk:
                    yield f"L[{b}] {L}{d:+d}", dict(see=see(lens=[L + d if i == b else x for i, x in enumerate(c["lens"])]))
    if c["rows"] is not None:
        for b, row in enumerate(c["rows"]):
            for e in range(len(row) - 1):  # the edge between run e and run e + 1
                for d in (1, -1):
                    n = [list(r) if isinstance(r, tuple) else r for r in row]

                    def grow(i, by):
                        if isinstance(n[i], list):
                            n[i][1] += by
                            return n[i][1]
                        n[i] += by
                        return n[i]

                    if grow(e, d) < 0 or grow(e + 1, -d) < 0:
                        continue
                    new = [tuple(r) if isinstance(r, list) else r for r in n]
                    yield f"row {b} edge {e} {d:+d}", dict(see=see(rows=[new if i == b else x for i, x in enumerate(c["rows"])]))
    # Sk - 1: the last key is seen by nobody
    s = inp["see"].clone()
    s[..., Sk - 1] = False
    yield "Sk - 1", dict(see=s)
    # Sk + 1: the next row in memory is a key too. Under a causal mask with Sq <= Sk, or with key
    # lengths (clamped to Sk), no query would see it: no such mutant there.
    if not (c["causal"] and Sq <= Sk) and c["lens"] is None:
        ext = {}
        for key in ("k", "v"):
            flat = torch.cat([inp[key].flatten(0, 2), torch.full((R.GUARD_ROWS, c["D"]), float("nan")).bfloat16()])
            ext[key] = torch.stack([flat[g * Sk:g * Sk + Sk + 1] for g in range(B * H)]).unflatten(0, (B, H))
        s = inp["see"]
        col = s.any(-1, keepdim=True)  # every query that sees anything
        if c["rows"] is not None:
            col = torch.zeros_like(col)
            for b, row in enumerate(c["rows"]):
                lo, hi, pad = runs_of(row, Sq)[-1]
                if not pad:
                    col[b, :, lo:hi] = True
        ext["see"] = torch.cat([s, col], -1)
        if bias is not None:
            ext["bias"] = torch.cat([bias, torch.zeros_like(bias[..., :1])], -1)
        if inp["keep"] is not None:
            from flexflow_amd import kernels as K
            ext["keep"] = torch.stack([K.attn_dropout_keep_ref(R.DROP_SEED, R.DROP_LAYER, R.DROP_STEP, 1, 1, Sq, Sk + 1,
                                                               c["thr"] / 256.0, b0=ob, h0=oh, H_total=c["H_total"])[0, 0]
                                       for ob, oh in c["origin"]]).unflatten(0, (B, H))
        yield "Sk + 1", ext
    if inp["keep"] is not None:  # the quad of the dropout mask that holds the heaviest probability of a middle row
        r = R.oracle(inp["q"][0, 0][None], inp["k"][0, 0][None], inp["v"][0, 0][None], inp["do"][0, 0][None],
                     inp["see"][0, 0][None], inp["scale"], None if bias is None else bias[0, 0][None])
        i = Sq // 2
        while not bool(inp["see"][0, 0, i].any()):
            i += 1
        j = int(r["P0"][0, i].argmax()) // 4 * 4
        keep = inp["keep"].clone()
        keep[0, 0, i, j:j + 4] ^= True
        yield f"dropout quad ({i}, {j}..{j + 3})", dict(keep=keep)
    if bias is not None:
        rolled = torch.roll(bias, 1, -1)
        yield "bias shifted by one key", dict(bias=rolled, see=torch.from_numpy(R.see_of(c, rolled)))


@pytest.mark.parametrize("name", list(R.CASES))
def test_boundary_mutants_are_flagged(name):
    c, inp, ref, tol, _, _ = _case(name)
    n = 0
    for label, over in _mutants(c, inp):
        # a mutant that moves no key any query sees would be no mutant: the case must be changed then
        assert "see" not in over or over["see"].shape != inp["see"].shape or not torch.equal(over["see"], inp["see"]), label
        mref, _, _ = R.reference(inp, **over)
        got = {key: mref[key][:, :, :ref[key].shape[2]] for key in R.OUTS}
        res = R.check(got, ref, tol, R.GPU_FACTOR)
        rows = {key: int(res[key][0].sum()) for key in R.OUTS}
        print(f"{name}: {label}: rows flagged {rows}")
        assert rows["o"] >= 1, (label, "passes in o: the inputs are too tame")
        assert rows["dq"] + rows["dk"] + rows["dv"] >= 1, (label, "passes in dq, dk and dv: the inputs are too tame")
        n += 1
    assert n >= 1


def _must_flag(mut, emu, ref, tol):
    """Rows the fault moved, in some element, by more than the tolerance plus the emulation's own error
    there: by the triangle inequality such a row cannot pass."""
    moved = (mut.double() - emu.double()).abs() - (emu.double() - ref).abs()
    return (moved > R.GPU_FACTOR * tol).any(-1)


def _fault_head(tol):
    """(b, h) of the last head among those with the most rows that hold anything."""
    n = (tol["o"] > 0).any(-1).sum(-1) + (tol["dk"] > 0).any(-1).sum(-1)
    g = n.numel() - 1 - int(n.flatten().flip(0).argmax())
    return divmod(g, n.shape[1])


@pytest.mark.parametrize("name", list(R.CASES))
def test_localised_faults_are_flagged(name):
    c, inp, ref, tol, _, emu = _case(name)
    b, h = _fault_head(tol)
    for key in R.OUTS:  # one 32-row block of one head scaled by 1.15
        S = emu[key].shape[2]
        lo = max(0, min(S - 32, 64))
        while lo > 0 and not bool((tol[key][b, h, lo:lo + 32] > 0).any()):
            lo -= 32  # a block that holds something
        mut = emu[key].clone()
        mut[b, h, lo:lo + 32] = (mut[b, h, lo:lo + 32].float() * 1.15).bfloat16()
        res = R.check({key: mut}, ref, tol, R.GPU_FACTOR)
        must = _must_flag(mut, emu[key], ref[key], tol[key])
        print(f"{name}: {key} rows {lo}..{lo + 31} x 1.15: {int(res[key][0].sum())} rows flagged, {int(must.sum())} "
              f"moved past the tolerance, Frobenius error {_frob(mut, ref[key]):.2e}")
        assert bool((res[key][0] | ~must).all()), key
        if bool((tol[key][b, h, lo:lo + 32] > 0).any()):
            flagged = res[key][0]
            assert int(flagged.sum()) >= 1 and int(flagged[b, h, lo:lo + 32].sum()) == int(flagged.sum()), key
    if c["causal"]:  # one 32-row block of that head given the diagonal j <= i + 1
        lo = min(c["Sq"] - 32, 64)
        see = inp["see"].expand(c["B"], -1, -1, -1).clone()
        wrong = torch.from_numpy(R.see_of(c, inp["bias"], diag=1))
        if see.shape[1] == 1 and c["H"] > 1:
            see = see.expand(-1, c["H"], -1, -1).clone()
            wrong = wrong.expand(-1, c["H"], -1, -1)
        see[b, h, lo:lo + 32] = wrong[b, h if wrong.shape[1] > 1 else 0, lo:lo + 32]
        mut = R.emulate(inp, see)
        res = R.check({key: mut[key] for key in R.OUTS}, ref, tol, R.GPU_FACTOR)
        for key in R.OUTS:
            must = _must_flag(mut[key], emu[key], ref[key], tol[key])
            print(f"{name}: {key} rows {lo}..{lo + 31} with j <= i + 1: {int(res[key][0].sum())} rows flagged, "
                  f"{int(must.sum())} moved past the tolerance, Frobenius error {_frob(mut[key], ref[key]):.2e}")
            assert bool((res[key][0] | ~must).all()), key
        assert int(res["o"][0].sum()) >= 1 and int(res["o"][0][b, h, lo:lo + 32].sum()) == int(res["o"][0].sum())
