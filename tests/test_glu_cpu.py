"""Gated linear units without a GPU: the reference path (kernels.glu_ref and the CPU side of glu_fwd /
glu_bwd) against the float64 oracle of tests/glu_common.py on every kernel case, the builder and its
errors, the axes the search is offered, a tiny gated FFN against torch, the torch.export importer (silu,
fuse_glu), two gloo ranks with the ffn axis split, and the decoder model and example with a SwiGLU MLP."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import glu_common as G  # noqa: E402

from flexflow_amd import kernels as K  # noqa: E402
from flexflow_amd.core import DataType, FFConfig, FFModel  # noqa: E402
from flexflow_amd.ops import OpCtx  # noqa: E402
from flexflow_amd.type import OperatorType  # noqa: E402


# ------------------------------------------------------------------------------------ reference path
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(G.CASES))
def test_reference_path_within_the_bf16_bound(name, dtype):
    """glu_fwd / glu_bwd on the CPU (glu_ref's arithmetic, written through the same strided views the kernel
    gets) pass the bf16 bound on every case, with the guards, gaps and inputs untouched: the reference alone
    stays within the bound."""
    G.check_case(name, dtype, "cpu")


@pytest.mark.parametrize("act", G.ACTS)
def test_glu_ref_is_the_definition(act):
    g = torch.Generator().manual_seed(2)
    a, b = (torch.randn(9, 13, generator=g) * 2).bfloat16(), (torch.randn(9, 13, generator=g) * 2).bfloat16()
    y = K.glu_ref(a, b, act)
    assert y.dtype == torch.bfloat16 and y.shape == a.shape
    ref, s = G.oracle(a, b, torch.zeros_like(a), act)["y"]
    assert G.bf16_check(y, ref, s)[0] == 0
    assert torch.equal(K.glu_fwd(a, b, act), y)
    x = torch.cat([a, b], -1)  # the packed halves are views, not copies
    assert torch.equal(K.glu_fwd(x[:, :13], x[:, 13:], act), y)
    assert torch.equal(K.unary_ref("silu", a, 0.0), F.silu(a.float()).bfloat16())


def test_kernel_wrappers_check_their_arguments():
    a = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="swish"):
        K.glu_fwd(a, a, "swish")
    with pytest.raises(ValueError, match="shape"):
        K.glu_fwd(a, torch.zeros(4, 5), "silu")
    with pytest.raises(ValueError, match="dtype"):
        K.glu_bwd(a, a, a.bfloat16(), "silu")
    with pytest.raises(ValueError, match="output"):
        K.glu_fwd(a, a, "silu", out=torch.zeros(6, 4).t())  # no contiguous last dim: it would be a copy
    assert "silu" not in K.U and K.unary_code("silu") == 20 and K.unary_code("relu") == K.U["relu"]


# ------------------------------------------------------------------------------------------- builder
def test_builder_shapes_values_and_errors():
    ff = FFModel(FFConfig([]))
    a = ff.create_tensor([4, 6, 24], DataType.DT_FLOAT)
    b = ff.create_tensor([4, 6, 24], DataType.DT_FLOAT)
    y = ff.glu(a, b, activation="gelu_tanh")
    L = y.owner_layer
    assert int(OperatorType.OP_GLU.value) == 105 and int(OperatorType.OP_SILU.value) == 104
    assert L.op_type == OperatorType.OP_GLU and tuple(y.dims) == (4, 6, 24) and y.data_type == DataType.DT_FLOAT
    assert not L.weights and L.attrs["activation"] == "gelu_tanh" and not L.impl.saves_output()
    assert not L.impl.uses_mfma() and L.impl.flops([(4, 6, 24)] * 2, [(4, 6, 24)], []) > 0
    p = ff.glu(a)
    Lp = p.owner_layer
    assert tuple(p.dims) == (4, 6, 12) and Lp.attrs["packed"] and Lp.attrs["activation"] == "silu" and not Lp.weights
    s = ff.silu(a)
    assert s.owner_layer.op_type == OperatorType.OP_SILU and tuple(s.dims) == (4, 6, 24)
    assert not s.owner_layer.impl.can_inplace()  # its gradient needs x
    i32 = ff.create_tensor([4, 6, 24], DataType.DT_INT32)
    for bad, match in ((lambda: ff.glu(a, b, activation="swish"), "swish"),
                       (lambda: ff.glu(a, ff.create_tensor([4, 6, 12], DataType.DT_FLOAT)), r"\[4, 6, 12\]"),
                       (lambda: ff.glu(ff.create_tensor([4, 6, 25], DataType.DT_FLOAT)), r"25"),
                       (lambda: ff.glu(a, i32), "INT32"),
                       (lambda: ff.gated_ffn(a, 8, activation="tanh"), "tanh")):
        with pytest.raises(ValueError, match=match) as e:
            bad()
        assert "glu" in str(e.value) or "gated_ffn" in str(e.value)


def test_gated_ffn_layer_names():
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([4, 16], DataType.DT_FLOAT, name="x")
    y = ff.gated_ffn(x, 24, name="mlp")
    assert [L.name for L in ff.layers] == ["x", "mlp_gate", "mlp_up", "mlp_glu", "mlp_down"]
    assert tuple(y.dims) == (4, 16) and all(len(L.weights) == 1 for L in ff.layers[1:] if L.name != "mlp_glu")
    z = ff.gated_ffn(x, 24, out_dim=10, use_bias=True, fused_gate_up=True, activation="gelu_tanh", name="f")
    names = [L.name for L in ff.layers][5:]
    assert names == ["f_gate_up", "f_glu", "f_down"] and tuple(z.dims) == (4, 10)
    by = {L.name: L for L in ff.layers}
    assert tuple(by["f_gate_up"].outputs[0].dims) == (4, 48) and len(by["f_gate_up"].weights) == 2
    assert by["f_glu"].attrs["packed"] and by["f_glu"].attrs["activation"] == "gelu_tanh"


def _degrees(L, axis, devices=4):
    from flexflow_amd.pcg.strategy import enumerate_configs
    return sorted({cfg.degrees[axis] for cfg in enumerate_configs(L, devices, max_configs=10 ** 6)})


def test_search_is_offered_the_right_axes():
    """Two inputs: every axis, with identity input maps (column-parallel gate / up feed it shard by shard).
    Packed: every axis but the last, whose split would separate a gate from its up."""
    ff = FFModel(FFConfig([]))
    a, b = (ff.create_tensor([8, 4, 16], DataType.DT_FLOAT) for _ in range(2))
    L2 = ff.glu(a, b).owner_layer
    Lp = ff.glu(ff.create_tensor([8, 4, 32], DataType.DT_FLOAT)).owner_layer
    assert all(L2.impl.supports_axis(i) for i in range(3))
    assert L2.impl.input_maps() == [(0, 1, 2), (0, 1, 2)] and L2.impl.output_maps() == [(0, 1, 2)]
    assert [_degrees(L2, i) for i in range(3)] == [[1, 2, 4]] * 3
    assert [Lp.impl.supports_axis(i) for i in range(3)] == [True, True, False]
    assert [_degrees(Lp, i) for i in range(3)] == [[1, 2, 4], [1, 2, 4], [1]]


# ------------------------------------------------------------------------------- numerics in the model
def _close(a, b):
    from test_ops_cpu import close
    close(a.float(), b.float(), 2e-4)  # test_rope_cpu.py's layer-vs-torch tolerance


@pytest.mark.parametrize("fused", [False, True], ids=["two_gemms", "fused_gate_up"])
def test_gated_ffn_matches_torch_cpu(fused):
    """hidden 16, ffn 24, batch 4 in fp32 on the CPU against down(F.silu(gate(x)) * up(x)) on the same
    weights (the fused form's weight is their concatenation): output, input gradient, all three weight
    gradients."""
    g = torch.Generator().manual_seed(13)
    x, dy = torch.randn(G.BATCH, G.HID, generator=g), torch.randn(G.BATCH, G.HID, generator=g)
    W = G.ffn_weights()
    layers, got = G.ffn_step(x, W, dy, "cpu", torch.float32, fused=fused)
    assert sorted(layers) == (["ffn_down", "ffn_gate_up", "ffn_glu"] if fused else
                              ["ffn_down", "ffn_gate", "ffn_glu", "ffn_up"])
    want = G.ffn_torch(x, W, dy)
    assert set(got) == set(want)
    for n in want:
        _close(got[n], want[n])
    other = G.ffn_torch(x, W, dy, act="gelu_tanh")
    assert G.rel(other["y"], want["y"]) > 1e-2  # the activation matters


def test_one_sgd_step_of_the_model_matches_torch():
    """The same FFN through compile / forward / backward / update: after one SGD step the three weights
    equal torch's w - lr * grad under a mean-squared-error loss."""
    from flexflow_amd.core import LossType, MetricsType, SGDOptimizer
    cfg = FFConfig(["--device", "cpu", "--no-hip-graphs"])
    cfg.batch_size = G.BATCH
    ff = FFModel(cfg)
    x = ff.create_tensor([G.BATCH, G.HID], DataType.DT_FLOAT, name="x")
    ff.gated_ffn(x, G.FFN, name="ffn")
    ff.optimizer = SGDOptimizer(ff, 0.1)
    ff.compile(loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, metrics=[MetricsType.METRICS_MEAN_SQUARED_ERROR])
    W = G.ffn_weights()
    by = {L.name: L for L in ff.layers}
    for n in ("gate", "up", "down"):
        by[f"ffn_{n}"].weights[0].set_weights(ff, W[n].numpy())
    g = torch.Generator().manual_seed(14)
    xv, lab = torch.randn(G.BATCH, G.HID, generator=g), torch.randn(G.BATCH, G.HID, generator=g)
    x.set_tensor(ff, xv.numpy())
    ff.label_tensor.set_tensor(ff, lab.numpy())
    ff.forward()
    y0 = torch.as_tensor(np.asarray(ff._get_tensor_value(ff.output_tensor()), dtype=np.float32))
    ff.zero_gradients()
    ff.backward()
    ff.update()
    Wt = {n: w.clone().requires_grad_() for n, w in W.items()}
    y = (F.silu(xv @ Wt["gate"].t()) * (xv @ Wt["up"].t())) @ Wt["down"].t()
    _close(y0, y.detach())
    new = {n: torch.as_tensor(np.asarray(by[f"ffn_{n}"].weights[0].get_weights(ff))) for n in W}
    moved = {n: (new[n] - W[n]) / -0.1 for n in W}  # the gradient the step applied
    # the loss gradient's scale is the executor's; fix it from one weight and ask the others to agree
    (y * (y.detach() - lab)).sum().backward()
    k = float((moved["down"] * Wt["down"].grad).sum() / (Wt["down"].grad ** 2).sum())
    assert k > 0
    for n in W:
        _close(moved[n], k * Wt[n].grad)


# ------------------------------------------------------------------------------------------ importer
class _Ffn(torch.nn.Module):
    def __init__(self, act="silu", twice=False, swap=False):
        super().__init__()
        torch.manual_seed(5)
        self.gate, self.up = torch.nn.Linear(16, 24, bias=False), torch.nn.Linear(16, 24, bias=False)
        self.down = torch.nn.Linear(24, 16, bias=False)
        self.act, self.twice, self.swap = act, twice, swap

    def forward(self, x):
        a = {"silu": F.silu, "gelu": F.gelu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "relu": F.relu,
             "sigmoid": torch.sigmoid}[self.act](self.gate(x))
        u = self.up(x)
        h = u * a if self.swap else a * u
        if self.twice:  # the activation has a second user
            h = h + a
        return self.down(h)


def _import(m, fuse):
    from flexflow_amd.torch.export import ExportImporter
    x = torch.randn(4, 16, generator=torch.Generator().manual_seed(6))
    imp = ExportImporter(m, ["x"], fuse_glu=fuse)
    imp.ep = torch.export.export(m, (x,))
    cfg = FFConfig(["--device", "cpu"])
    cfg.batch_size = 4
    ff = FFModel(cfg)
    t = ff.create_tensor([4, 16], DataType.DT_FLOAT)
    outs = imp.to_ff(ff, [t])
    return ff, t, outs, x


def _ops(ff):
    return [L.op_type for L in ff.layers if L.op_type != OperatorType.OP_INPUT]


def _run_imported(ff, t, outs, x):
    from flexflow_amd.core import LossType, MetricsType, SGDOptimizer
    ff.optimizer = SGDOptimizer(ff, 0.01)
    ff.compile(loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, metrics=[MetricsType.METRICS_MEAN_SQUARED_ERROR])
    t.set_tensor(ff, x.numpy())
    ff.forward()
    return torch.as_tensor(np.asarray(outs[0].get_tensor(ff)))


def test_importer_maps_silu_and_fuses_on_request():
    LIN, MUL, SILU, GLU = (OperatorType.OP_LINEAR, OperatorType.OP_EW_MUL, OperatorType.OP_SILU, OperatorType.OP_GLU)
    m = _Ffn()
    with torch.no_grad():
        want = m(torch.randn(4, 16, generator=torch.Generator().manual_seed(6)))
    ff, t, outs, x = _import(m, False)
    assert sorted(o.name for o in _ops(ff)) == sorted(o.name for o in [LIN, LIN, SILU, MUL, LIN])
    assert torch.allclose(_run_imported(ff, t, outs, x), want, rtol=1e-5, atol=1e-6)
    ff, t, outs, x = _import(m, True)
    assert sorted(o.name for o in _ops(ff)) == sorted(o.name for o in [LIN, LIN, GLU, LIN])
    L = next(L for L in ff.layers if L.op_type == GLU)
    assert L.attrs["activation"] == "silu" and not L.attrs.get("packed") and len(L.inputs) == 2
    assert torch.allclose(_run_imported(ff, t, outs, x), want, rtol=1e-5, atol=1e-6)
    from flexflow_amd.torch.model import PyTorchModel
    assert PyTorchModel(m).fuse_glu is False and PyTorchModel(m, fuse_glu=True).fuse_glu is True


@pytest.mark.parametrize("act,swap", [("gelu", False), ("gelu_tanh", True), ("relu", False), ("sigmoid", True)])
def test_importer_reads_the_activation(act, swap):
    """gelu's `approximate` picks gelu or gelu_tanh; the product is matched in either operand order."""
    m = _Ffn(act, swap=swap)
    ff, t, outs, x = _import(m, True)
    L = [L for L in ff.layers if L.op_type == OperatorType.OP_GLU]
    assert len(L) == 1 and L[0].attrs["activation"] == act
    assert L[0].inputs[0].owner_layer.name != L[0].inputs[1].owner_layer.name
    with torch.no_grad():
        want = m(x)
    assert torch.allclose(_run_imported(ff, t, outs, x), want, rtol=1e-5, atol=1e-6)


def test_importer_keeps_an_activation_with_a_second_user():
    m = _Ffn(twice=True)
    ff, t, outs, x = _import(m, True)
    kinds = _ops(ff)
    assert OperatorType.OP_GLU not in kinds and OperatorType.OP_SILU in kinds and OperatorType.OP_EW_MUL in kinds
    with torch.no_grad():
        want = m(x)
    assert torch.allclose(_run_imported(ff, t, outs, x), want, rtol=1e-5, atol=1e-6)


def test_fx_front_end_maps_silu():
    from flexflow_amd.torch.model import PyTorchModel

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.act, self.b = torch.nn.Linear(8, 8), torch.nn.SiLU(), torch.nn.Linear(8, 4)

        def forward(self, x):
            return self.b(F.silu(self.act(self.a(x))))

    ff = FFModel(FFConfig(["--device", "cpu"]))
    t = ff.create_tensor([2, 8], DataType.DT_FLOAT)
    PyTorchModel(M()).torch_to_ff(ff, [t])
    assert [o for o in _ops(ff)].count(OperatorType.OP_SILU) == 2


def test_keras_activation_silu_and_swish():
    from flexflow_amd.keras.layers import Activation
    ff = FFModel(FFConfig([]))
    t = ff.create_tensor([2, 8], DataType.DT_FLOAT)
    for name in ("silu", "swish"):
        out = Activation(name)._lower(ff, [t])[0]
        assert out.owner_layer.op_type == OperatorType.OP_SILU


def _mt5_ops_before_glu():
    """The op-type sequence the importer built of this mt5 (2 encoder and 2 decoder blocks) before the glu op
    existed, written out block by block in the order the lazy builder emits them (184 layers)."""
    qkv = ["LINEAR", "RESHAPE", "TRANSPOSE"]
    core = ["TRANSPOSE", "BATCHMATMUL", "INPUT", "EW_ADD", "SOFTMAX", "BATCHMATMUL", "TRANSPOSE", "RESHAPE", "LINEAR",
            "EW_ADD"]  # scores + the constant position bias, softmax, values, output projection, residual
    norm = ["RMS_NORM"]
    attn = norm + qkv * 3 + core
    # gated-gelu FFN: wi_0 and the tanh form of gelu written out, times wi_1, then wo and the residual
    ffn = norm + ["LINEAR", "SCALAR_MULTIPLY", "POW", "SCALAR_MULTIPLY", "EW_ADD", "SCALAR_MULTIPLY", "TANH", "SCALAR_ADD",
                  "EW_MUL", "LINEAR", "EW_MUL", "LINEAR", "EW_ADD"]
    seq = (["INPUT"] * 3 + ["EMBEDDING"] + attn  # decoder block 0: self-attention
           + norm + qkv  # its cross-attention's query
           + ["EMBEDDING"] + attn + ffn + attn + ffn + norm  # the encoder
           + qkv * 2 + core + ffn  # cross-attention's keys and values, decoder block 0's FFN
           + attn + attn + ffn  # decoder block 1: self-attention, cross-attention, FFN
           + norm + ["LINEAR"])  # final norm and lm_head
    return ["OP_" + n for n in seq]


def test_mt5_default_import_is_unchanged():
    """The default import of mt5 (gated-gelu FFN written out with tanh) builds, op for op and in order, the
    layer list the importer built before the glu op existed: no glu, no silu, the FFN still gelu-by-tanh and
    a multiply."""
    transformers = pytest.importorskip("transformers")
    from flexflow_amd.torch.model import PyTorchModel
    torch.manual_seed(0)
    cfg = transformers.MT5Config(vocab_size=256, d_model=64, d_kv=16, d_ff=128, num_layers=2, num_decoder_layers=2,
                                 num_heads=4, relative_attention_num_buckets=8, dropout_rate=0.0)
    m = transformers.MT5ForConditionalGeneration(cfg)
    fc = FFConfig(["--device", "cpu"])
    fc.batch_size = 2
    ff = FFModel(fc)
    ins = [ff.create_tensor([2, 12], DataType.DT_INT64), ff.create_tensor([2, 12], DataType.DT_INT64),
           ff.create_tensor([2, 10], DataType.DT_INT64)]
    PyTorchModel(m, is_hf_model=True, input_names=["input_ids", "attention_mask", "decoder_input_ids"],
                 batch_size=2, seq_length=(12, 10)).torch_to_ff(ff, ins)
    got = [L.op_type.name for L in ff.layers]
    want = _mt5_ops_before_glu()
    assert len(want) == 184 and "OP_GLU" not in got and "OP_SILU" not in got
    assert got == want, next((i, a, b) for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)


# --------------------------------------------------------------------------------------- distributed
def test_two_ranks_tensor_parallel_ffn_matches_one_process():
    """Two gloo ranks, the ffn axis split (gate and up column-parallel, the glu on its columns, down
    row-parallel) and the batch split, against one process: weights and output after the harness's SGD
    steps (tests/test_multirank_cpu.py tolerance)."""
    import glu_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("tp")
    par, strat = A.run("tp", 2)
    assert strat["ffn_gate"]["degrees"] == [1, 1, 2, 1] and strat["ffn_up"]["degrees"] == [1, 1, 2, 1], strat
    assert strat["ffn_glu"]["degrees"] == [1, 1, 2] and strat["ffn_down"]["degrees"] == [1, 1, 1, 2], strat
    _compare(par, ref, "gated ffn tp@2")
    par, strat = A.run("batch", 2)
    assert strat["ffn_glu"]["degrees"] == [2, 1, 1], strat
    _compare(par, ref, "gated ffn batch@2")
    other = A.single("gelu_tanh")
    assert np.abs(other["__output__"] - ref["__output__"]).max() > 1e-4


# ------------------------------------------------------------------------------------------- decoder
DEFAULT_DECODER_LAYERS = ["input_ids", "tok_emb"] + [f"l{l}_{n}" for l in range(2) for n in (
    "norm1", "attn", "res1", "norm2", "ffn1", "ffn2", "res2")] + ["final_norm", "lm_head", "lm_softmax"]


def test_decoder_default_graph_is_todays():
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    dc = DecoderConfig.tiny(16)
    assert dc.mlp == "gelu" and dc == DecoderConfig(hidden=64, heads=4, kv_heads=2, layers=2, ffn=128, vocab=96, seq=16)
    ff = FFModel(FFConfig([]))
    build_rope_decoder(ff, 2, dc)
    assert [L.name for L in ff.layers] == DEFAULT_DECODER_LAYERS
    assert not any(L.op_type in (OperatorType.OP_GLU, OperatorType.OP_SILU) for L in ff.layers)
    for mlp, act, fused in (("swiglu", "silu", False), ("geglu", "gelu_tanh", True)):
        ff = FFModel(FFConfig([]))
        dc = DecoderConfig.tiny(16)
        dc.mlp, dc.fused_gate_up = mlp, fused
        build_rope_decoder(ff, 2, dc)
        names = [L.name for L in ff.layers]
        assert "l0_ffn1" not in names and "l1_ffn_glu" in names and ("l0_ffn_gate_up" in names) == fused
        glu = [L for L in ff.layers if L.op_type == OperatorType.OP_GLU]
        assert len(glu) == 2 and all(L.attrs["activation"] == act and bool(L.attrs.get("packed")) == fused for L in glu)
    with pytest.raises(ValueError, match="reglu"):
        dc.mlp = "reglu"
        build_rope_decoder(FFModel(FFConfig([])), 2, dc)


def test_swiglu_decoder_trains_cpu():
    from flexflow_amd.core import AdamOptimizer, LossType, MetricsType
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder
    torch.manual_seed(0)
    B = 4
    dc = DecoderConfig.tiny(16)
    dc.mlp = "swiglu"
    cfg = FFConfig(["--device", "cpu", "--no-hip-graphs"])
    cfg.batch_size = B
    ff = FFModel(cfg)
    ids, _ = build_rope_decoder(ff, B, dc)
    glu = [L for L in ff.layers if L.op_type == OperatorType.OP_GLU]
    assert len(glu) == dc.layers and all(L.attrs["activation"] == "silu" and not L.attrs.get("packed") for L in glu)
    assert not any(L.name.endswith(("_ffn1", "_ffn2")) for L in ff.layers)
    ff.optimizer = AdamOptimizer(ff, 3e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    rng = np.random.default_rng(0)
    tok = rng.integers(1, dc.vocab, (B, dc.seq)).astype(np.int32)
    ids.set_tensor(ff, tok)
    ff.label_tensor.set_tensor(ff, ((tok + 1) % dc.vocab)[..., None].astype(np.int32))
    losses = []
    for _ in range(6):
        ff.reset_metrics()
        ff.train_step()
        losses.append(ff.get_perf_metrics().get_loss())
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.05, losses


@pytest.mark.parametrize("extra", [[], ["--fused-gate-up"]], ids=["swiglu", "swiglu_fused"])
def test_rope_decoder_example_with_a_gated_mlp(extra):
    """examples/python/native/rope_decoder.py --small --mlp swiglu [--fused-gate-up] runs end to end in its own
    process on the CPU and its loss falls over a few steps."""
    root = os.path.dirname(HERE)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", FF_TUNABLEOP="off")
    cmd = [sys.executable, os.path.join(root, "examples", "python", "native", "rope_decoder.py"), "--small", "-b", "4",
           "--iterations", "6", "--mlp", "swiglu"] + extra
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("loss first")]
    assert line and "nan" not in r.stdout.lower(), r.stdout[-500:]
    first, last = float(line[0].split()[2]), float(line[0].split()[4])
    assert last < first - 0.1, line
    # the tiny decoder has 2 blocks: one glu op each, packed exactly when gate and up are one GEMM
    assert f"mlp swiglu: 2 glu ops, {2 if extra else 0} packed" in r.stdout, r.stdout[-500:]
