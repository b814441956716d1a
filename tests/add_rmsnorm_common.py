"""Shared by test_add_rmsnorm_cpu.py and test_add_rmsnorm_gpu.py: the tiny rotary decoder with and without
fused_norm, one training step of it, and a float64 torch replica of the same model with autograd."""
import dataclasses
import math

import numpy as np
import torch
import torch.nn.functional as F

import rope_common as R
from flexflow_amd.core import AdamOptimizer, FFConfig, FFModel, LossType, MetricsType
from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder

B = 4


def decoder(fused, flags=("--no-hip-graphs", "--device", "cpu", "--dtype", "fp32"), seq=16, load=None):
    """DecoderConfig.tiny(seq) from seed 0 with one batch of tokens set: (model, config, tokens, labels)."""
    torch.manual_seed(0)
    dc = dataclasses.replace(DecoderConfig.tiny(seq), fused_norm=fused)
    cfg = FFConfig(list(flags))
    cfg.batch_size = B
    ff = FFModel(cfg)
    ids, _ = build_rope_decoder(ff, B, dc)
    ff.optimizer = AdamOptimizer(ff, 3e-3)
    ff.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY])
    if load:  # strict=True compares the layer lists, which differ by design; the weights' keys do not
        ff.load_checkpoint(load, strict=False)
    tok = np.random.default_rng(0).integers(1, dc.vocab, (B, dc.seq)).astype(np.int32)
    lab = (tok + 1) % dc.vocab
    ids.set_tensor(ff, tok)
    ff.label_tensor.set_tensor(ff, lab[..., None].astype(np.int32))
    return ff, dc, tok, lab


def weights(ff):
    return {w.name: np.asarray(w.get_weights(ff)) for L in ff.layers for w in L.weights}


def step(ff):
    """One Adam step: (loss, {weight name: its gradient, read before the update})."""
    ff.reset_metrics()
    ff.forward()
    ff.zero_gradients()
    ff.backward()
    grads = {w.name: torch.tensor(w.get_gradients(ff)).double() for L in ff.layers for w in L.weights}
    ff.update()
    return ff.get_perf_metrics().get_loss(), grads


def reference64(W, dc, tok, lab):
    """models/decoder.py (mlp "gelu") in torch in float64 on the weights W (name -> array): (loss, {weight name:
    gradient}) by autograd; the loss as the model has it, summed over a sample's tokens, averaged over the batch."""
    W = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in W.items()}

    def rms(x, name):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * W[name + ".weight"]
    S, kd, G = dc.seq, dc.hidden // dc.heads, dc.heads // dc.kv_heads
    c = R.rope_cfg(kd, S, base=dc.rope_base)
    future = torch.ones(S, S, dtype=torch.bool).triu(1)
    x = W["tok_emb.weight"][torch.as_tensor(tok, dtype=torch.long)]
    for l in range(dc.layers):
        n = rms(x, f"l{l}_norm1")
        q, k, v = ((n @ W[f"l{l}_attn.{p}_weight"].flatten(0, 1).t()).view(B, S, -1, kd).transpose(1, 2) for p in "qkv")
        q, k = R.rotate(q, c), R.rotate(k, c).repeat_interleave(G, 1)
        p = torch.softmax((q @ k.transpose(-1, -2) / math.sqrt(kd)).masked_fill(future, float("-inf")), -1)
        o = (p @ v.repeat_interleave(G, 1)).transpose(1, 2).reshape(B, S, -1)
        x = x + o @ W[f"l{l}_attn.o_weight"].flatten(1).t()
        h = F.gelu(rms(x, f"l{l}_norm2") @ W[f"l{l}_ffn1.kernel"].t() + W[f"l{l}_ffn1.bias"])
        x = x + h @ W[f"l{l}_ffn2.kernel"].t() + W[f"l{l}_ffn2.bias"]
    logits = rms(x, "final_norm") @ W["lm_head.kernel"].t()
    loss = F.cross_entropy(logits.flatten(0, 1), torch.as_tensor(lab, dtype=torch.long).flatten(), reduction="sum") / B
    loss.backward()
    return loss.item(), {k: v.grad for k, v in W.items()}
