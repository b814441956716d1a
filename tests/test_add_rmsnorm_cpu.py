"""The add_rms_norm op (ops/norm.py AddRMSNorm), FFModel.add_rms_norm and DecoderConfig.fused_norm without a GPU."""
import numpy as np
import pytest

from add_rmsnorm_common import decoder, step, weights
from flexflow_amd.core import FFConfig, FFModel
from flexflow_amd.models.decoder import DecoderConfig
from flexflow_amd.type import DataType, OperatorType

UNFUSED = ["input_ids", "tok_emb"] + [f"l{l}_{n}" for l in range(2) for n in (
    "norm1", "attn", "res1", "norm2", "ffn1", "ffn2", "res2")] + ["final_norm", "lm_head", "lm_softmax"]


def test_op_infers_two_outputs_and_one_weight_and_refuses_unequal_shapes():
    ff = FFModel(FFConfig([]))
    a, b = (ff.create_tensor([4, 6, 24], DataType.DT_FLOAT) for _ in range(2))
    s, y = ff.add_rms_norm(a, b, eps=1e-5, name="n")
    L = s.owner_layer
    assert y.owner_layer is L and L.op_type == OperatorType.OP_ADD_RMS_NORM and int(L.op_type.value) == 106
    assert [tuple(o.dims) for o in L.outputs] == [(4, 6, 24)] * 2 and s is L.outputs[0] and y is L.outputs[1]
    assert [tuple(w.dims) for w in L.weights] == [(24,)]
    assert L.attrs["eps"] == 1e-5 and not L.impl.saves_output()
    assert [L.impl.supports_axis(i) for i in range(3)] == [True, True, False] and L.impl.axis_kinds()[-1] == "none"
    assert L.impl.input_maps() == [(0, 1, 2)] * 2 and L.impl.output_maps() == [(0, 1, 2)] * 2
    assert L.impl.weight_maps() == [(None,)]
    shp = [(4, 6, 24)]
    rms = ff.rms_norm(a).owner_layer.impl
    assert L.impl.flops(shp * 2, shp * 2, [(24,)]) == rms.flops(shp, shp, [(24,)]) + 4 * 6 * 24
    with pytest.raises(ValueError, match="one shape"):
        ff.add_rms_norm(a, ff.create_tensor([4, 6, 12], DataType.DT_FLOAT))


def test_layer_lists_weight_names_and_checkpoint(tmp_path):
    """fused_norm off builds today's layers; on, every add is gone, the norms behind them are add_rms_norm
    layers under the same names, the weights carry the same names and start from the same values, and a
    checkpoint of the unfused model loads into the fused one."""
    assert DecoderConfig().fused_norm is False
    plain = decoder(False)[0]
    assert [L.name for L in plain.layers] == UNFUSED
    assert not any(L.op_type == OperatorType.OP_ADD_RMS_NORM for L in plain.layers)
    fused = decoder(True)[0]
    assert [L.name for L in fused.layers] == [n for n in UNFUSED if "_res" not in n]
    kinds = {L.name: L.op_type for L in fused.layers}
    assert kinds["l0_norm1"] == OperatorType.OP_RMS_NORM
    assert all(kinds[n] == OperatorType.OP_ADD_RMS_NORM for n in ("l0_norm2", "l1_norm1", "l1_norm2", "final_norm"))
    wp, wf = weights(plain), weights(fused)
    assert list(wp) == list(wf) and all(np.array_equal(wp[k], wf[k]) for k in wp)
    step(plain)
    path = str(tmp_path / "unfused.ckpt")
    plain.save_checkpoint(path)
    wt, wl = weights(plain), weights(decoder(True, load=path)[0])
    assert all(np.array_equal(wt[k], wl[k]) for k in wt) and any(not np.array_equal(wt[k], wp[k]) for k in wt)


def test_fused_decoder_trains_like_the_unfused_one():
    """Three Adam steps each way. Both graphs form the same fp32 values; what may differ is the order in which
    a sum of d = hidden terms is associated (the row statistic, and dx + ds against the executor's sum of two
    gradients): at most d * 2^-24 of the sum's magnitude each, two such sums a norm, growing at most linearly
    with the steps to first order. So the losses agree to steps * d * 2^-23, relative."""
    steps, d = 3, DecoderConfig.tiny(16).hidden
    plain, fused = decoder(False)[0], decoder(True)[0]
    lp, lf = (np.asarray([step(ff)[0] for _ in range(steps)]) for ff in (plain, fused))
    print("unfused", lp, "fused", lf)
    assert np.isfinite(lf).all() and lf[-1] < lf[0]
    np.testing.assert_allclose(lf, lp, rtol=steps * d * 2.0 ** -23, atol=0)
