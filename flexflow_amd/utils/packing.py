"""Sequence packing: several variable-length sequences back to back in rows of `seq` tokens, so that a
step computes (almost) no pad tokens. Attention keeps the sequences of a row apart through per-token
`segment_ids` (ops/attention.py), the positions restart at every sequence, and the unused tail of a
row is padding (segment id -1, label -100 for `ignore_index=-100, loss_reduction="valid"`).

Pure numpy and deterministic: the same lengths give the same rows.
"""
from __future__ import annotations

import numpy as np


def pack_sequences(lengths, seq: int):
    """First-fit-decreasing bin packing of sequences of the given lengths into rows of `seq` tokens.
    Returns a list of rows, each a list of (sequence index, offset) placements in the order they sit in
    the row. Sequences are taken longest first (ties: lowest index first) and put into the first row
    with room, so the result depends on the lengths alone. A length outside 1..seq is an error."""
    lengths = [int(n) for n in lengths]
    for i, n in enumerate(lengths):
        if not 1 <= n <= seq:
            raise ValueError(f"pack_sequences: sequence {i} has length {n}, rows hold 1..{seq} tokens")
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    rows, used = [], []
    for i in order:
        for r in range(len(rows)):
            if used[r] + lengths[i] <= seq:
                break
        else:
            rows.append([])
            used.append(0)
            r = len(rows) - 1
        rows[r].append((i, used[r]))
        used[r] += lengths[i]
    return rows


def fill_ratio(rows, lengths, seq: int) -> float:
    """Real tokens over the token slots of the packed rows."""
    return float(sum(int(lengths[i]) for row in rows for i, _ in row)) / max(1, len(rows) * seq)


def packed_arrays(rows, tokens, labels, seq: int, pad_token: int = 0, pad_label: int = -100):
    """The packed rows as model inputs: int32 arrays `ids` [R, seq], `position_ids` [R, seq]
    (restarting at 0 in every sequence; 0 on the tail), `segment_ids` [R, seq] (0, 1, .. in row order;
    -1 on the tail) and `labels` [R, seq, 1] (pad_label on the tail). tokens / labels: one 1-D array
    per sequence, of that sequence's length."""
    R = len(rows)
    ids = np.full((R, seq), pad_token, dtype=np.int32)
    pos = np.zeros((R, seq), dtype=np.int32)
    seg = np.full((R, seq), -1, dtype=np.int32)
    lab = np.full((R, seq, 1), pad_label, dtype=np.int32)
    for r, row in enumerate(rows):
        for j, (i, off) in enumerate(row):
            t = np.asarray(tokens[i], dtype=np.int32).reshape(-1)
            n = t.shape[0]
            if off + n > seq:
                raise ValueError(f"packed_arrays: sequence {i} does not fit row {r} at offset {off}")
            ids[r, off:off + n] = t
            pos[r, off:off + n] = np.arange(n, dtype=np.int32)
            seg[r, off:off + n] = j
            lab[r, off:off + n, 0] = np.asarray(labels[i], dtype=np.int32).reshape(-1)
    return ids, pos, seg, lab
