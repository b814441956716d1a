"""Oracles shared by test_attn_window_cpu.py and test_attn_window_gpu.py, in plain Python / numpy loops,
independent of the code under test.

The public contract (flash-attention's window_size convention): query i sees key j iff
i - left <= j <= i + right, and additionally j <= i with causal, and additionally both lie in one run of
a packed row. left / right are ints >= 0; -1 (or None) is unbounded on that side. A row is a list of
run lengths as in attn_segments_common (("p", n) is a padding run), or None for an unpacked row.
"""
import numpy as np

from attn_segments_common import mask_of


def p(n):
    return ("p", n)


def band_mask(S, left, right, causal, rows=None):
    """bool [B or 1, S, S] from the sentence above, one element at a time."""
    left = -1 if left is None else left
    right = -1 if right is None else right
    B = 1 if rows is None else len(rows)
    m = np.zeros((B, S, S), dtype=bool)
    for b in range(B):
        run = None if rows is None else mask_of(rows[b], S)
        for i in range(S):
            for j in range(S):
                ok = (left < 0 or j >= i - left) and (right < 0 or j <= i + right)
                if causal and j > i:
                    ok = False
                if run is not None and not run[i, j]:
                    ok = False
                m[b, i, j] = ok
    return m


def bounds_of(mask):
    """lo, hi, klo, khi (int32 [B, S]) by brute force from a mask WITHOUT the causal bound (the kernels
    apply that on top): first visible index and one past the last, per row (query side) and per column
    (key side); a row or column that sees nothing is anchored at its own index."""
    B, S, _ = mask.shape
    out = np.zeros((4, B, S), dtype=np.int32)
    for b in range(B):
        for i in range(S):
            row = [j for j in range(S) if mask[b, i, j]]
            col = [q for q in range(S) if mask[b, q, i]]
            out[0, b, i], out[1, b, i] = (row[0], row[-1] + 1) if row else (i, i)
            out[2, b, i], out[3, b, i] = (col[0], col[-1] + 1) if col else (i, i)
    return tuple(out)


def visible_pairs(S, left, right, causal):
    return int(band_mask(S, left, right, causal).sum())


# small packed rows for the bound cases: runs shorter and longer than the windows, padding at the front,
# inside and at the end, single-token runs, an all-padding row
CPU_ROWS = [[7, 5, p(3), 9], [24], [p(2), 10, p(4), 8], [1, 1, 21, p(1)], [p(24)]]
# (S, left, right, rows): every side bounded / unbounded, zero, wider than a run, with and without packing
BOUND_CASES = [
    (24, 3, 0, None), (24, 0, 0, None), (24, 5, 2, None), (24, -1, 4, None), (24, 4, -1, None), (24, 22, 22, None),
    (24, 3, 0, CPU_ROWS), (24, 0, 0, CPU_ROWS), (24, 5, 2, CPU_ROWS), (24, -1, 4, CPU_ROWS), (24, 4, -1, CPU_ROWS),
    (24, 30, 30, CPU_ROWS), (1, 0, 0, None), (1, 0, 0, [[1]]), (1, 0, 0, [[p(1)]]), (37, 6, 11, None),
]
