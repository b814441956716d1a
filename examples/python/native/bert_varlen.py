"""bert-tiny on right-padded variable-length batches: every sample carries its number of real
tokens, the data loader feeds those lengths next to the token ids, and every attention layer
leaves the pad positions out as keys (`key_lengths`, read on the device: the step still captures
into a graph). Synthetic data. By default the labels of pad positions still count in the loss;
`--ignore-pad-labels` writes -100 there and compiles with `ignore_index=-100,
loss_reduction="valid"`, so the pad rows leave loss, gradients and accuracy and the loss is the
mean over the real tokens. `--clip-grad-norm C` is FFConfig's flag: it goes through to the
optimizer, which then clips the global gradient norm to C on the device. `--optimizer lamb` trains
with LAMB (decoupled weight decay, one trust ratio per weight) in place of Adam, `--optimizer adamw`
with AdamW (the same decay, no trust ratio, one pass).

`--pack` trains the same corpus packed (flexflow_amd/utils/packing.py): the sentences are put back to
back into rows of `--seq-length` tokens, first-fit-decreasing; the loader feeds per-token
`segment_ids` and positions that restart at every sentence, attention stays inside a sentence, and the
tail of a row is padding (label -100, `ignore_index=-100, loss_reduction="valid"`). A step then has
the same batch of rows but nearly every token in it is real, so the corpus takes about half the steps.
Both modes print tokens/s over the real tokens.

    python examples/python/native/bert_varlen.py -b 8 --seq-length 64 --iterations 20
    python examples/python/native/bert_varlen.py -b 8 --seq-length 64 --iterations 20 --ignore-pad-labels
    python examples/python/native/bert_varlen.py -b 8 --seq-length 64 --ignore-pad-labels --clip-grad-norm 1.0
    python examples/python/native/bert_varlen.py -b 8 --seq-length 64 --ignore-pad-labels --optimizer lamb
    python examples/python/native/bert_varlen.py -b 8 --seq-length 64 --iterations 20 --pack
"""
import argparse
import sys

import _args  # noqa: F401  (puts the repo root on sys.path)
import numpy as np

from flexflow_amd.core import *  # noqa: F401,F403
from flexflow_amd.models.bert import BertConfig, build_bert

OPTIMIZERS = {"adam": AdamOptimizer, "adamw": AdamWOptimizer, "lamb": LAMBOptimizer}  # noqa: F405

def top_level_task(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--seq-length", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--min-length", type=int, default=8)
    ap.add_argument("--ignore-pad-labels", action="store_true")
    ap.add_argument("--optimizer", choices=sorted(OPTIMIZERS), default="adam")
    ap.add_argument("--pack", action="store_true")
    args, rest = ap.parse_known_args(sys.argv[1:] if argv is None else argv)
    ffconfig = FFConfig(rest)
    ffmodel = FFModel(ffconfig)
    b, s = ffconfig.batch_size, args.seq_length
    bc = BertConfig.tiny(s)
    if args.pack:
        return run_packed(args, ffconfig, ffmodel, bc)
    lengths = ffmodel.create_tensor([b], DataType.DT_INT32, name="key_lengths")
    ids, pos, _ = build_bert(ffmodel, b, bc, key_lengths=lengths)
    ffmodel.optimizer = OPTIMIZERS[args.optimizer](ffmodel, 1e-3)
    masking = dict(ignore_index=-100, loss_reduction="valid") if args.ignore_pad_labels else {}
    ffmodel.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY],
                    **masking)
    # a synthetic corpus: n sentences of min-length .. s tokens, right-padded with token 0
    rng = np.random.default_rng(0)
    n = b * args.iterations
    lens = rng.integers(min(args.min_length, s), s + 1, n).astype(np.int32)
    tok = rng.integers(1, bc.vocab, (n, s)).astype(np.int32)
    pad = np.arange(s)[None, :] >= lens[:, None]
    tok[pad] = 0
    labels = ((tok + 1) % bc.vocab)[..., None].astype(np.int32)  # learnable: the next id of each token
    if args.ignore_pad_labels:
        labels[pad] = -100
    loaders = [ffmodel.create_data_loader(ids, tok),
               ffmodel.create_data_loader(pos, np.tile(np.arange(s, dtype=np.int32), (n, 1))),
               ffmodel.create_data_loader(lengths, lens),
               ffmodel.create_data_loader(ffmodel.label_tensor, labels)]
    ffmodel.init_layers()
    ts = ffconfig.get_current_time()
    for _ in range(args.iterations):
        for dl in loaders:
            dl.next_batch(ffmodel)
        ffmodel.train_step()
    pm = ffmodel.get_perf_metrics()
    run_time = 1e-6 * (ffconfig.get_current_time() - ts)
    print("bert-tiny varlen: %d iterations, mean length %.1f of %d, %.4fs, THROUGHPUT = %.2f samples/s, loss %.4f" %
          (args.iterations, lens.mean(), s, run_time, b * args.iterations / run_time, pm.get_loss()))
    print("padded: %d rows per step, fill ratio %.3f, %.1f tokens/s" %
          (b, lens.sum() / float(n * s), lens.sum() / run_time))
    if args.ignore_pad_labels:
        print("pad labels ignored: loss is the mean over %d real tokens, accuracy %.2f%%" %
              (pm.train_all, pm.get_accuracy()))
    if ffmodel.optimizer.clip_norm:  # --clip-grad-norm, taken from the config by the optimizer
        print("gradient norm clipped to %g: the last step's norm before clipping was %.4f" %
              (ffmodel.optimizer.clip_norm, ffmodel.get_grad_norm()))
    return pm


def run_packed(args, ffconfig, ffmodel, bc):
    """The corpus of the padded run (same seed, same sentences and labels), packed into rows."""
    from flexflow_amd.utils.packing import fill_ratio, pack_sequences, packed_arrays
    b, s = ffconfig.batch_size, args.seq_length
    seg = ffmodel.create_tensor([b, s], DataType.DT_INT32, name="segment_ids")
    ids, pos, _ = build_bert(ffmodel, b, bc, segment_ids=seg)
    ffmodel.optimizer = OPTIMIZERS[args.optimizer](ffmodel, 1e-3)
    ffmodel.compile(loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, metrics=[MetricsType.METRICS_ACCURACY],
                    ignore_index=-100, loss_reduction="valid")
    rng = np.random.default_rng(0)
    n = b * args.iterations
    lens = rng.integers(min(args.min_length, s), s + 1, n).astype(np.int32)
    tok = rng.integers(1, bc.vocab, (n, s)).astype(np.int32)
    toks = [tok[i, :lens[i]] for i in range(n)]
    labs = [(t + 1) % bc.vocab for t in toks]
    rows = pack_sequences(lens, s)
    fill = fill_ratio(rows, lens, s)
    steps = (len(rows) + b - 1) // b
    rows += [[] for _ in range(steps * b - len(rows))]  # the last step's spare rows are all padding
    p_ids, p_pos, p_seg, p_lab = packed_arrays(rows, toks, labs, s)
    loaders = [ffmodel.create_data_loader(ids, p_ids), ffmodel.create_data_loader(pos, p_pos),
               ffmodel.create_data_loader(seg, p_seg), ffmodel.create_data_loader(ffmodel.label_tensor, p_lab)]
    ffmodel.init_layers()
    ts = ffconfig.get_current_time()
    for _ in range(steps):
        for dl in loaders:
            dl.next_batch(ffmodel)
        ffmodel.train_step()
    pm = ffmodel.get_perf_metrics()
    run_time = 1e-6 * (ffconfig.get_current_time() - ts)
    print("bert-tiny packed: %d sentences in %d steps, mean length %.1f of %d, %.4fs, THROUGHPUT = %.2f samples/s, "
          "loss %.4f" % (n, steps, lens.mean(), s, run_time, n / run_time, pm.get_loss()))
    print("packed: %d rows per step, fill ratio %.3f, %.1f tokens/s" % (b, fill, lens.sum() / run_time))
    return pm


if __name__ == "__main__":
    top_level_task()
