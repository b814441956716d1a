"""QK-norm fused with rotary on the GPU: qknorm.hip element by element against the float64 oracle of
tests/qk_norm_common.py (its docstring has the oracle and the derivation of the bounds), and the attention layer
that uses it against a test-local fp32 torch attention that norms and rotates by the definition.

Kernel cases (CASES in qk_norm_common.py) are the smallest shapes that reach each branch: the fused [T, 3, H, D]
layout with another stride set for the output and the V third of the gradient buffer compared bit for bit,
grouped heads in separate buffers with Sq != Sk, the norm alone, a partial rotary width, interleaved pairs,
position ids (restarts, a zero row, ids outside the table), head dims 32 and 256, fp32 weights, the general form
(D 80 in fp32, D 48 in bf16, every base pointer off by one element), and three workgroups with a ragged last one.
Every case has all-zero head rows (finite output; with a zero gradient row, an exactly zero dx: with a non-zero
one the definition gives dx = g w / sqrt(eps), which the oracle checks). Outputs start as NaN between sentinel rows.

On an MI355X no element of any case lies outside the bound; the largest |err| / bound is 0.995 for y and 0.994
for dx in bf16 (the bound's first term is half an ulp of the result, which a correctly rounded result reaches),
0.097 for rstd and 0.010 for dw; in fp32 storage 0.076 (y), 0.054 (rstd), 0.078 (dx), 0.003 (dw). The layer
tests' relative errors are 2.2e-3 to 4.1e-3 (output) and up to 1.1e-2 (gradients) in bf16, below 1e-6 in fp32.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import qk_norm_common as Q  # noqa: E402
import rope_common as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ffC():
    from flexflow_amd import _C
    return _C


@pytest.mark.parametrize("name", list(Q.CASES))
def test_kernel_against_float64(ffC, name):
    Q.check_case(name, torch.bfloat16, DEV)


def test_each_weight_goes_to_its_own_tensor(ffC):
    """wq != wk, both far from ones: swapping them in the oracle puts most elements outside the bound."""
    res, d, bad = Q.run("gqa", torch.bfloat16, DEV)
    assert not bad and not torch.equal(d["w"]["q"], d["w"]["k"])
    for n, other in (("q", "k"), ("k", "q")):
        r = res[n]
        ref, tol = Q.oracle(r["x"], d["w"][other], r["dz"], Q.CASES["gqa"], None, R.U[torch.bfloat16])["y"]
        assert R.check(r["y"], ref, tol)[0] > r["y"].numel() // 2


def test_weight_gradient_is_reproducible_and_optional(ffC):
    a, _, _ = Q.run("multi_wg", torch.bfloat16, DEV)
    b, _, _ = Q.run("multi_wg", torch.bfloat16, DEV)
    f, _, bad = Q.run("multi_wg", torch.bfloat16, DEV, frozen=True)  # dw = None: the same dx, nothing else written
    assert not bad
    for n in "qk":
        assert torch.equal(a[n]["dw"].view(torch.int32), b[n]["dw"].view(torch.int32)) and float(a[n]["dw"].abs().max()) > 0
        assert torch.equal(a[n]["dx"], f[n]["dx"])


def test_arguments_are_checked(ffC):
    from flexflow_amd import kernels as K
    B, S, H, D = 2, 16, 2, 64
    t = K.rope_table(64, S, device=DEV)
    x, y = (torch.zeros(B * S * H * D, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    w, r = torch.ones(D, dtype=torch.bfloat16, device=DEV), torch.zeros(B, S, H, device=DEV)
    st, no = [S * H * D, D, H * D], [0, 0, 0]
    fwd = lambda x=x, y=y, st=st, w=w, r=r, rd=64, t=t, pos=None: ffC.qk_norm_rope_fwd(  # noqa: E731
        x, y, st, st, H, S, w, r, None, None, no, no, 0, 0, None, None, B, D, rd, 1e-6, t, pos)
    fwd()
    for bad in (dict(x=x[:-8]), dict(y=y[:-8]), dict(y=x), dict(rd=63), dict(rd=32), dict(w=w[:-1]), dict(r=r[:, :, :1]),
                dict(pos=torch.zeros(B, 8, dtype=torch.int32, device=DEV)), dict(t=None)):
        with pytest.raises(RuntimeError):
            fwd(**bad)
    dw = torch.zeros(D, device=DEV)
    with pytest.raises(RuntimeError):  # a slab too small for the partials
        ffC.qk_norm_rope_bwd(x, y, st, st, H, S, w, r, dw, None, None, no, no, 0, 0, None, None, None, B, D, 64, t, None, False,
                             torch.zeros(8, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- the layer
def mha_qk_norm_torch(x, W, H, Hkv, c, dy, causal):
    """fp32 torch attention on the layer's weights W that norms q and k by the definition, then rotates them
    (c: a rope_common config or None): {"y", "dx0", "d<weight>"}."""
    x = x.clone().requires_grad_()
    Wd = {n: w.clone().requires_grad_() for n, w in W.items()}
    B, S, _ = x.shape
    ws = [Wd["qkv_weight"][i] for i in range(3)] if "qkv_weight" in Wd else [Wd[f"{n}_weight"] for n in "qkv"]
    bs = ([Wd["qkv_bias"][i] for i in range(3)] if "qkv_bias" in Wd else [Wd.get(f"{n}_bias") for n in "qkv"])
    q, k, v = ((x @ w.reshape(-1, w.shape[-1]).t() + (0 if b is None else b.reshape(-1))).view(B, S, w.shape[0], -1)
               .transpose(1, 2) for w, b in zip(ws, bs))
    norm = lambda t, g: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6) * g  # noqa: E731
    q, k = norm(q, Wd["q_norm_weight"]), norm(k, Wd["k_norm_weight"])
    if c is not None:
        q, k = R.rotate(q, c), R.rotate(k, c)
    k, v = k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1)
    s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, -1)
    y = o @ Wd["o_weight"].reshape(Wd["o_weight"].shape[0], -1).t() + (Wd["o_bias"] if "o_bias" in Wd else 0)
    (y * dy).sum().backward()
    return {"y": y.detach(), "dx0": x.grad, **{"d" + n: w.grad for n, w in Wd.items()}}


MHA = {
    "fused_bias_rotary": dict(D=64, kw=dict(bias=True, rotary=True)),
    "kv1": dict(D=64, kw=dict(num_kv_heads=1, bias=True, rotary=True), Hkv=1),
    "causal_no_rotary": dict(D=64, kw=dict(causal=True, bias=False)),
    "padded": dict(D=32, kw=dict(bias=True, rotary=dict(dim=16))),  # head dim 32 zero-padded to 64 by the core
    "fp32": dict(D=64, kw=dict(bias=True, causal=True, rotary=True), dtype=torch.float32),
}


@pytest.mark.parametrize("name", list(MHA))
def test_mha_qk_norm_op(ffC, name):
    """One training step of multihead_attention(qk_norm=True) with B2 S128 H4 on the device against fp32 torch
    on the same weights: output, input gradient and every weight gradient, the two norm weights included."""
    m = MHA[name]
    B, S, H, D = 2, 128, 4, m["D"]
    Hkv, E, dtype = m.get("Hkv", H), H * D, m.get("dtype", torch.bfloat16)
    g = torch.Generator().manual_seed(41)
    x, dy = (torch.randn(B, S, E, generator=g).bfloat16().float() for _ in range(2))
    base = R.make_weights(E, 42)  # the two norm weights drawn around 1 instead of around 0
    ws = lambda L: [(1 + 4 * t).bfloat16().float() if w.short_name.endswith("norm_weight") else t  # noqa: E731
                    for w, t in zip(L.weights, base(L))]
    L, got = R.layer_step(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, qk_norm=True, **m["kw"]), [x], (), ws,
                          dy, DEV, dtype)
    torch.cuda.synchronize()
    W = {w.short_name: t for w, t in zip(L.weights, ws(L))}
    assert [w.short_name for w in L.weights][-2:] == ["q_norm_weight", "k_norm_weight"]
    assert float((W["q_norm_weight"] - 1).abs().max()) > 0.1
    c = R.rope_cfg(L.attrs["rope_dim"], S) if L.attrs.get("rope_dim") else None
    want = mha_qk_norm_torch(x, W, H, Hkv, c, dy, bool(m["kw"].get("causal")))
    assert set(got) == set(want), (sorted(got), sorted(want))
    errs = {n: R.rel(got[n], want[n]) for n in got}
    print("mha qk_norm relative errors", name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(torch.isfinite(t).all() for t in got.values())
    assert errs.pop("y") < R.TOL_O and all(e < R.TOL_G for e in errs.values()), errs
    ws0 = lambda L0: ws(L)[:len(L0.weights)]  # noqa: E731  the same weights without the norm
    _, plain = R.layer_step(lambda ff, t: ff.multihead_attention(t[0], t[0], t[0], E, H, **m["kw"]), [x], (), ws0, dy, DEV, dtype)
    assert R.rel(plain["y"], want["y"]) > 5 * R.TOL_O


def test_decoder_qk_norm_trains_under_step_capture(monkeypatch):
    """test_rope_gpu.py's tiny decoder with qk_norm=True, hipGraph step capture on and off: 6 steps, the graph
    exists, losses and weights agree at that test's rtol 1e-5, atol 1e-6."""
    import test_rope_gpu as T
    from flexflow_amd.models import decoder
    real = decoder.build_rope_decoder

    def with_qk_norm(ff, batch, cfg, **kw):
        cfg.qk_norm = True
        return real(ff, batch, cfg, **kw)
    monkeypatch.setattr(decoder, "build_rope_decoder", with_qk_norm)
    ffg, lg, wg = T._train_decoder(["--hip-graphs"], True)
    assert any(w.short_name == "q_norm_weight" for L in ffg.layers for w in L.weights)
    sg = ffg._step_graph
    assert sg is not None and sg.graph is not None and not sg.failed
    _, le, we = T._train_decoder(["--no-hip-graphs"], True)
    assert np.isfinite(lg).all() and np.isfinite(le).all()
    print("losses captured", lg, "eager", le)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for i, (a, b) in enumerate(zip(wg, we)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=str(i))
