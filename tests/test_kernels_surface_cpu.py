"""The names that code outside flexflow_amd/kernels reaches through the package. Every hot op goes
through `from flexflow_amd import kernels as K; K.name(...)`, so a split of the package into modules
has to keep each of these an attribute of the package itself."""
from flexflow_amd import kernels as K

# used by flexflow_amd/, examples/, bench.py, scripts/ and tests/ (collected with grep)
PUBLIC = """ACT_GELU ACT_GRADMUL ACT_NONE ACT_RELU CHANNELS_LAST EPI_BIAS EPI_NONE IMPLS TUNE_LOG act_dense
act_grad_ref act_ref adam_update attn_f32_bwd attn_f32_fwd attn_f32_supported attn_padded_dim attn_supported
batchnorm_bwd batchnorm_fwd bias_grad binary_bwd binary_fwd bmm cl_dense cl_ok conv2d_bwd conv2d_fwd
conv_bias_relu_bwd conv_geometry dense dropout_bwd dropout_fwd embedding_bwd embedding_fwd ext fill
flash_attn_bwd flash_attn_fwd fold_flush gemm gemm_dact init_normal init_uniform is_nhwc layernorm_bwd
layernorm_fwd linear_bwd linear_fwd lstm_bwd_cell lstm_fwd_cell metrics_classify moe_on_device moe_route
mse_grad native pool2d_bwd pool2d_fwd pool_out_size reductions_deferred rmsnorm_bwd rmsnorm_fwd
set_fold_batching set_reduce_stream sgd_sparse_rows sgd_update softmax_bwd softmax_fwd softmax_xent topk
topk_bwd tunable_setup tune_cache_load tune_cache_save unary_bwd unary_fwd weight_t wt_forward wt_refresh_all
xent_grad""".split()

# helpers and state that tests/ and scripts/ call as K._name (the tuner's own globals left out)
PRIVATE = """_FOLDQ _WT _bwd_picks_ours _conv_gemm_bwd _conv_gemm_fwd _conv_lib_bwd _conv_lib_fwd _conv_ours_bwd
_conv_ours_fwd _lib_gemm _lib_gemm_act _lib_gemm_splitk _lt_plan _lt_run _lt_splitk _pointwise_gemm_ok _pool_ref
_rows""".split()


def test_names_used_outside_the_package():
    missing = [n for n in PUBLIC + PRIVATE if not hasattr(K, n)]
    assert not missing, missing
    assert callable(K.gemm) and callable(K.conv2d_fwd) and isinstance(K.TUNE_LOG, list)

