"""A small pre-norm causal decoder in the shape of the current open models (LLaMA, Mistral, Qwen): token
embedding only (no position table), and per block RMSNorm -> rotary grouped-query attention -> residual,
RMSNorm -> MLP -> residual; a final RMSNorm and a vocabulary projection with softmax. Positions enter
through the rotation of the query and key heads alone (ops/attention.py, `rotary`). The MLP is
`DecoderConfig.mlp`: "gelu" (two dense layers, the default), or the gated FFN of those models,
down(act(gate(x)) * up(x)) without biases (FFModel.gated_ffn): "swiglu" (silu) or "geglu" (gelu_tanh),
with `fused_gate_up` the gate and up projections as one GEMM.
"""
from __future__ import annotations

from dataclasses import dataclass

from ..type import ActiMode, AggrMode, DataType


@dataclass
class DecoderConfig:
    hidden: int = 1024
    heads: int = 16
    kv_heads: int = 4
    layers: int = 8
    ffn: int = 4096
    vocab: int = 32000
    seq: int = 512
    rope_base: float = 10000.0
    max_positions: int = 0  # 0: seq
    mlp: str = "gelu"  # "gelu" | "swiglu" | "geglu"
    fused_gate_up: bool = False  # gated MLPs: gate and up as one dense of 2 * ffn outputs
    sliding_window: int = 0  # HuggingFace's convention: every query sees that many keys, itself included; 0: all

    @staticmethod
    def tiny(seq=32):
        return DecoderConfig(hidden=64, heads=4, kv_heads=2, layers=2, ffn=128, vocab=96, seq=seq)


GATED_MLPS = {"swiglu": "silu", "geglu": "gelu_tanh"}  # DecoderConfig.mlp -> the glu activation


def build_rope_decoder(ff, batch: int, cfg: DecoderConfig, segment_ids=None, position_ids=None):
    """Returns (ids_tensor, output). Output: [batch, seq, vocab] next-token probabilities.
    segment_ids / position_ids: optional int32 [batch, seq] tensors of packed rows (utils/packing.py):
    attention stays inside a token's own sequence and its position restarts there.
    cfg.sliding_window = W (Mistral, Gemma's local layers): every layer attends to the last W keys, the
    query included, i.e. multihead_attention(window=(W - 1, 0), causal=True); with and without packing."""
    if cfg.mlp != "gelu" and cfg.mlp not in GATED_MLPS:
        raise ValueError(f"build_rope_decoder: unknown mlp {cfg.mlp!r} (one of gelu, {', '.join(GATED_MLPS)})")
    S, H = cfg.seq, cfg.hidden
    rotary = dict(base=cfg.rope_base, max_positions=cfg.max_positions or S)
    if cfg.sliding_window < 0:
        raise ValueError(f"build_rope_decoder: sliding_window must be >= 0, got {cfg.sliding_window}")
    window = (cfg.sliding_window - 1, 0) if cfg.sliding_window else None
    ids = ff.create_tensor([batch, S], DataType.DT_INT32, name="input_ids")
    x = ff.embedding(ids, cfg.vocab, H, AggrMode.AGGR_MODE_NONE, name="tok_emb")
    for l in range(cfg.layers):
        n = ff.rms_norm(x, name=f"l{l}_norm1")
        a = ff.multihead_attention(n, n, n, H, cfg.heads, bias=False, causal=True, name=f"l{l}_attn",
                                   num_kv_heads=cfg.kv_heads, segment_ids=segment_ids, rotary=rotary,
                                   rope_position_ids=position_ids, window=window)
        x = ff.add(a, x, name=f"l{l}_res1")
        n = ff.rms_norm(x, name=f"l{l}_norm2")
        if cfg.mlp == "gelu":
            h = ff.dense(n, cfg.ffn, ActiMode.AC_MODE_GELU, name=f"l{l}_ffn1")
            h = ff.dense(h, H, name=f"l{l}_ffn2")
        else:
            h = ff.gated_ffn(n, cfg.ffn, H, activation=GATED_MLPS[cfg.mlp], fused_gate_up=cfg.fused_gate_up,
                             name=f"l{l}_ffn")
        x = ff.add(h, x, name=f"l{l}_res2")
    x = ff.rms_norm(x, name="final_norm")
    t = ff.dense(x, cfg.vocab, use_bias=False, name="lm_head")
    out = ff.softmax(t, name="lm_softmax")
    return ids, out
