"""QK-norm without a GPU: the plain-torch path of kernels.qk_norm_rope against the float64 oracle of
qk_norm_common.py, the builder, the layer's weights, checkpoints, and two gloo ranks on the heads axis."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import qk_norm_common as Q  # noqa: E402
from flexflow_amd.core import DataType, FFConfig, FFModel  # noqa: E402


@pytest.mark.parametrize("name", ["fused_layout", "ids"])
def test_reference_path(name):
    Q.check_case(name, torch.bfloat16, "cpu")


def _mha(**kw):
    ff = FFModel(FFConfig([]))
    x = ff.create_tensor([2, 6, 16], DataType.DT_FLOAT)
    return ff.multihead_attention(x, x, x, 16, 4, **kw).owner_layer


def test_builder():
    for bad in (dict(epsilon=1e-6), dict(eps=0.0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            _mha(qk_norm=bad)
    base = _mha()
    names = [(w.short_name, tuple(w.dims)) for w in base.weights]
    assert names == [("qkv_weight", (3, 4, 4, 16)), ("qkv_bias", (3, 4, 4)), ("o_weight", (16, 4, 4)), ("o_bias", (16,))]
    assert not any("norm" in k for k in base.attrs)
    for off in (False, None):
        L = _mha(qk_norm=off)
        assert L.attrs == base.attrs and [(w.short_name, tuple(w.dims)) for w in L.weights] == names
    L = _mha(qk_norm=True, rotary=True)
    assert L.attrs["qk_norm_eps"] == 1e-6 and _mha(qk_norm=dict(eps=1e-5)).attrs["qk_norm_eps"] == 1e-5
    assert [(w.short_name, tuple(w.dims)) for w in L.weights] == names + [("q_norm_weight", (4,)), ("k_norm_weight", (4,))]
    assert L.impl.weight_maps()[-2:] == [(None,), (None,)] and not L.impl.overwrites_wgrad(len(names))
    from flexflow_amd.pcg.costmodel import cost_key
    from flexflow_amd.pcg.strategy import OpConfig
    cfg = OpConfig((1,) * len(L.impl.axis_sizes()), (0,))
    assert cost_key(L, cfg, DataType.DT_FLOAT) != cost_key(_mha(rotary=True), cfg, DataType.DT_FLOAT)
    shapes = ([(2, 6, 16)] * 3, [(2, 6, 16)])
    plain = _mha(rotary=True)
    assert L.impl.flops(*shapes, [tuple(w.dims) for w in L.weights]) > plain.impl.flops(*shapes, [tuple(w.dims) for w in plain.weights])
    assert L.impl.mem_bytes(*shapes, [tuple(w.dims) for w in L.weights]) > plain.impl.mem_bytes(*shapes, [tuple(w.dims) for w in plain.weights])


def test_checkpoint_round_trip(tmp_path):
    from flexflow_amd.core import AdamOptimizer, LossType
    from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder

    def model(qk_norm):
        ff = FFModel(FFConfig(["--no-hip-graphs"]))
        ff.config.batch_size = 2
        dc = DecoderConfig.tiny(8)
        dc.qk_norm = qk_norm
        build_rope_decoder(ff, 2, dc)
        ff.optimizer = AdamOptimizer(ff, 1e-3)
        ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[])
        return ff

    a, b = model(True), model(True)
    norm = [w for L in a.layers for w in L.weights if w.short_name.endswith("norm_weight") and "attn" in L.name]
    assert len(norm) == 4
    norm[0].set_weights(a, np.full(norm[0].dims, 1.5, dtype=np.float32))
    a.save_checkpoint(str(tmp_path / "ck"))
    b.load_checkpoint(str(tmp_path / "ck"))
    for La, Lb in zip(a.layers, b.layers):
        for wa, wb in zip(La.weights, Lb.weights):
            np.testing.assert_array_equal(np.asarray(wa.get_weights(a)), np.asarray(wb.get_weights(b)))
    plain = {w.name for L in model(False).layers for w in L.weights}
    assert plain == {w.name for L in a.layers for w in L.weights} - {w.name for w in norm}


def test_two_ranks_on_the_heads_axis_match_one_process():
    import qk_norm_dist as A
    from test_multirank_cpu import _compare
    ref = A.single("qk_norm")
    norm = [v for k, v in ref.items() if "MULTIHEAD_ATTENTION" in k and v.shape == (A.A.E // A.A.H,)]  # the harness keys by position
    assert len(norm) == 2 and all(np.abs(v - 1).max() > 1e-4 for v in norm)  # the norm weights moved: their gradients are compared
    for case, degrees in (("batch", [2, 1, 1, 1]), ("heads", [1, 1, 1, 2])):
        par, strat = A.run(case, 2)
        assert strat["attn"]["degrees"] == degrees, strat["attn"]
        _compare(par, ref, f"qk_norm {case}@2")
    assert np.abs(A.single("plain")["__output__"] - ref["__output__"]).max() > 1e-4
