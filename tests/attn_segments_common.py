"""Oracles shared by test_attn_segments_cpu.py and test_attn_segments_gpu.py. A packed row is written
as a list of run lengths, an int for a segment and ("p", n) for a padding run; everything here is
plain Python / numpy loops over those lists, independent of the code under test."""
import numpy as np


def runs_of(row, S):
    """[(begin, end, is_pad)] of a row given as run lengths; the lengths must add up to S."""
    out, at = [], 0
    for r in row:
        pad = isinstance(r, tuple)
        n = r[1] if pad else r
        out.append((at, at + n, pad))
        at += n
    assert at == S, (row, S)
    return out


def ids_of(row, S):
    """Segment ids of the row: neighbouring segments differ (0, 1, 0, ..: ids are reused along the
    row), padding runs alternate between -1 and -2."""
    ids = np.zeros(S, dtype=np.int32)
    nseg = npad = 0
    for b, e, pad in runs_of(row, S):
        if pad:
            ids[b:e] = -1 - (npad % 2)
            npad += 1
        else:
            ids[b:e] = nseg % 2
            nseg += 1
    return ids


def live_of(row, S):
    live = np.zeros(S, dtype=bool)
    for b, e, pad in runs_of(row, S):
        live[b:e] = not pad
    return live


def mask_of(row, S, causal=False):
    """bool [S, S]: query i sees key j."""
    m = np.zeros((S, S), dtype=bool)
    for b, e, pad in runs_of(row, S):
        if not pad:
            m[b:e, b:e] = True
    if causal:
        m &= np.tril(np.ones((S, S), dtype=bool))
    return m


def bounds_loop(ids):
    """lo, hi (int32, ids' shape) of segment ids [B, S] by the definition: position i's run is the
    maximal stretch of positions around i holding ids[i] >= 0; a padding position gets lo = hi = i."""
    ids = np.asarray(ids)
    lo, hi = np.zeros_like(ids, dtype=np.int32), np.zeros_like(ids, dtype=np.int32)
    for b in range(ids.shape[0]):
        row, S = ids[b], ids.shape[1]
        i = 0
        while i < S:
            j = i
            while j + 1 < S and row[j + 1] == row[i]:
                j += 1
            for t in range(i, j + 1):
                lo[b, t], hi[b, t] = (t, t) if row[i] < 0 else (i, j + 1)
            i = j + 1
    return lo, hi
