"""A small causal decoder with rotary position embeddings on synthetic data: token embedding only (no
position table), and per block RMSNorm, rotary grouped-query attention (`multihead_attention(...,
causal=True, num_kv_heads=.., rotary=..)`), then a GELU MLP (flexflow_amd/models/decoder.py). The task is
learnable (the label of a token is its next id), so the loss falls over a few steps.

`--mlp swiglu` / `--mlp geglu` replace the GELU MLP by the gated FFN of the LLaMA family (`gated_ffn`:
down(act(gate(x)) * up(x)), the gate one launch of the glu op); `--fused-gate-up` makes gate and up one GEMM.

`--packed` trains on packed rows (flexflow_amd/utils/packing.py): sentences of random lengths are put back to
back into rows of `--seq-length` tokens; the loader feeds per-token `segment_ids` (attention stays inside a
sentence) and `position_ids` that restart at every sentence, which the rotation reads on the device
(`rope_position_ids`). The tail of a row is padding (label -100, left out of the loss).

`--window W` is sliding-window attention (`DecoderConfig.sliding_window`): every query sees the last W keys,
itself included (`window=(W - 1, 0)`), with `--packed` and without.

`--optimizer adamw --weight-decay X` trains with AdamW (decoupled weight decay X on the matrices and the
embedding table, none on the RMSNorm gains), as the recipes of these models do; the default stays Adam.

    python examples/python/native/rope_decoder.py -b 8 --iterations 20
    python examples/python/native/rope_decoder.py --small --iterations 8 --optimizer adamw --weight-decay 0.1
    python examples/python/native/rope_decoder.py --small --packed --window 8 --iterations 8
    python examples/python/native/rope_decoder.py --small --iterations 8            # CPU-sized
    python examples/python/native/rope_decoder.py --small --packed --iterations 8
    python examples/python/native/rope_decoder.py --small --mlp swiglu --iterations 8
"""
import argparse
import sys

import numpy as np
import zoo

from flexflow_amd.core import *  # noqa: F401,F403
from flexflow_amd.models.decoder import DecoderConfig, build_rope_decoder


def _labels(tok, vocab):
    return (tok + 1) % vocab


def top_level_task(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--seq-length", type=int, default=0)
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--mlp", choices=("gelu", "swiglu", "geglu"), default="gelu")
    ap.add_argument("--fused-gate-up", action="store_true")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--optimizer", choices=("adam", "adamw"), default="adam")
    ap.add_argument("--weight-decay", type=float, default=0.01)
    args, rest = ap.parse_known_args(sys.argv[1:] if argv is None else argv)
    ffconfig, ffmodel, small, iterations = zoo.setup(rest)
    b = ffconfig.batch_size
    dc = DecoderConfig.tiny(args.seq_length or 32) if small else \
        DecoderConfig(hidden=512, heads=8, kv_heads=2, layers=4, ffn=2048, vocab=4096, seq=args.seq_length or 256)
    dc.mlp, dc.fused_gate_up = args.mlp, args.fused_gate_up
    dc.sliding_window = args.window
    s = dc.seq
    seg = pos = None
    if args.packed:
        seg = ffmodel.create_tensor([b, s], DataType.DT_INT32, name="segment_ids")
        pos = ffmodel.create_tensor([b, s], DataType.DT_INT32, name="rope_position_ids")
    ids, out = build_rope_decoder(ffmodel, b, dc, segment_ids=seg, position_ids=pos)
    lr = 3e-3 if small else 1e-3
    ffmodel.optimizer = AdamWOptimizer(ffmodel, lr, weight_decay=args.weight_decay) if args.optimizer == "adamw" \
        else AdamOptimizer(ffmodel, lr)
    ffmodel.compile(loss_type=zoo.SCCE, metrics=[MetricsType.METRICS_ACCURACY], ignore_index=-100, loss_reduction="valid")
    rng = np.random.default_rng(0)
    if args.packed:
        from flexflow_amd.utils.packing import fill_ratio, pack_sequences, packed_arrays
        n = 2 * b * iterations
        lens = rng.integers(max(2, s // 8), s + 1, n)
        toks = [rng.integers(1, dc.vocab, m).astype(np.int32) for m in lens]
        rows = pack_sequences(lens, s)
        fill = fill_ratio(rows, lens, s)
        steps = (len(rows) + b - 1) // b
        rows += [[] for _ in range(steps * b - len(rows))]
        p_ids, p_pos, p_seg, p_lab = packed_arrays(rows, toks, [_labels(t, dc.vocab) for t in toks], s)
        loaders = [ffmodel.create_data_loader(ids, p_ids), ffmodel.create_data_loader(seg, p_seg),
                   ffmodel.create_data_loader(pos, p_pos), ffmodel.create_data_loader(ffmodel.label_tensor, p_lab)]
    else:
        steps = iterations
        tok = rng.integers(1, dc.vocab, (b * steps, s)).astype(np.int32)
        lab = np.stack([_labels(t, dc.vocab) for t in tok])[..., None].astype(np.int32)
        loaders = [ffmodel.create_data_loader(ids, tok), ffmodel.create_data_loader(ffmodel.label_tensor, lab)]
    ffmodel.init_layers()
    losses = []
    ts = ffconfig.get_current_time()
    for _ in range(steps):
        for dl in loaders:
            dl.next_batch(ffmodel)
        ffmodel.reset_metrics()
        ffmodel.train_step()
        losses.append(ffmodel.get_perf_metrics().get_loss())
    run_time = 1e-6 * (ffconfig.get_current_time() - ts)
    print("rope decoder%s: %d steps of %d rows x %d tokens, %.4fs, THROUGHPUT = %.2f samples/s" %
          (" packed" if args.packed else "", steps, b, s, run_time, b * steps / run_time))
    if args.packed:
        print("packed: %d sentences, fill ratio %.3f" % (len(lens), fill))
    glu = [L for L in ffmodel.layers if L.op_type == OperatorType.OP_GLU]
    print("mlp %s: %d glu ops, %d packed" % (dc.mlp, len(glu), sum(bool(L.attrs.get("packed")) for L in glu)))
    print("%.1f tokens/s (rows x tokens per row, padding included)" % (b * s * steps / run_time))
    if args.window:
        win = [L for L in ffmodel.layers if "window_left" in L.attrs]
        print("sliding window %d: %d windowed attention layers" % (args.window, len(win)))
    print("loss first %.4f last %.4f" % (losses[0], losses[-1]))
    return losses


if __name__ == "__main__":
    top_level_task()
