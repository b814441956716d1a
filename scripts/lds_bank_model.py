#!/usr/bin/env python3
"""LDS bank-conflict model of attn_bwd1b_kernel (csrc/kernels/attention.hip, D = 64).

A wave64 LDS instruction is served in fixed lane groups, one LDS-array cycle per group when the
group's lanes hit distinct banks (or the same dword); each further distinct dword on a busy bank
adds a cycle. Lane groups and bank functions per instruction as measured on MI355X:

  ds_read_b128          4 x 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, (+32)   bank (a/4) % 64
  ds_read_b64_tr_b16    2 x 32 lanes                                                bank (a/4) % 64
  ds_write_b64          4 x 16 consecutive lanes                                    bank (a/4) % 32
  ds_write_b128         8 x 8 consecutive lanes                                     bank (a/4) % 32

The offset functions below mirror the kernel's (aswz / aoff, k1b_off, dst1b_off and the epilogue's
row & 7 chunk XOR); `old=True` gives the layouts before the dQ stage got images of its own (aoff for
the K block, dst_off for dS^T). Run as a script for the per-pattern table and the loop / whole
kernel conflict share; tests/test_lds_bank_model.py asserts the loop is conflict-free.
"""
from collections import defaultdict

D, QT, KB, NW = 64, 64, 256, 8

_B128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
         [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G_READ_B128 = _B128 + [[l + 32 for l in g] for g in _B128]
G_2X32 = [list(range(32)), list(range(32, 64))]
G_4X16 = [list(range(16 * i, 16 * i + 16)) for i in range(4)]
G_8X8 = [list(range(8 * i, 8 * i + 8)) for i in range(8)]

# instruction -> (dwords per lane, lane groups, banks)
INSTR = {
    "ds_read_b128": (4, G_READ_B128, 64),
    "ds_read_b64_tr_b16": (2, G_2X32, 64),
    "ds_write_b64": (2, G_4X16, 32),
    "ds_write_b128": (4, G_8X8, 32),
}


def _bit(x, i):
    return (x >> i) & 1


def aswz(row):
    return (_bit(row, 1) << 2) | _bit(row, 3) | (_bit(row, 4) << 1)


def aoff(row, col):
    return row * 128 + (((col >> 3) ^ aswz(row)) << 4) + ((col & 7) << 1)


def k1b_off(row, col):
    x = (_bit(row, 1) << 1) | (_bit(row, 3) << 2) | _bit(row, 4)
    return row * 128 + (((col >> 3) ^ x) << 4) + ((col & 7) << 1)


def dst_off(row, q):
    f = (row & 7) | ((_bit(row, 1) ^ _bit(row, 3)) << 3)
    return row * 128 + (((q >> 2) ^ f) << 3) + (q & 3) * 2


def dst1b_off(row, q):
    f = _bit(row, 0) | (_bit(row, 2) << 1) | (_bit(row, 1) << 2) | (_bit(row, 3) << 3)
    return row * 128 + (((q >> 2) ^ f) << 3) + (q & 3) * 2


def cycles(instr, addr):
    """(LDS-array cycles, ideal cycles) of one wave instruction; addr(lane) = byte address."""
    nd, groups, nb = INSTR[instr]
    total = 0
    for g in groups:
        banks = defaultdict(set)
        for lane in g:
            a = addr(lane)
            for d in range(nd):
                w = a // 4 + d
                banks[w % nb].add(w)
        total += max(len(s) for s in banks.values())
    return total, len(groups)


def loop_patterns(old=False):
    """Every LDS access of one query tile (steady-state loop body), all 8 waves:
    (stage, instruction, address function) per wave instruction. The tile-buffer base, the buffer
    parity and the lse2 / delta rows (one dword per query, contiguous quads) do not change banks
    between lanes of a group beyond what is modelled here."""
    koff = aoff if old else k1b_off
    doff = dst_off if old else dst1b_off
    out = []
    for wave in range(NW):
        for qt in range(2):
            for s in range(D // 16):  # S / dP fragments: Q and dO tiles (same image, other base)
                for _tile in ("Q", "dO"):
                    out.append(("S/dP b128", "ds_read_b128",
                                lambda l, qt=qt, s=s: aoff(32 * qt + (l & 31), 16 * s + 8 * (l >> 5))))
            for g4 in range(4):  # lse2 and delta quads
                for _row in ("lse2", "delta"):
                    out.append(("lse2/delta b128", "ds_read_b128",
                                lambda l, qt=qt, g4=g4: (32 * qt + 8 * g4 + 4 * (l >> 5)) * 4))
            for dt in range(D // 32):  # dV / dK transposed reads
                for s2 in range(2):
                    for hi in range(2):
                        for _tile in ("dO", "Q"):
                            def f(l, qt=qt, dt=dt, s2=s2, hi=hi):
                                h, G, qi, pi = l >> 5, l >> 4, (l & 15) >> 2, l & 3
                                return aoff(32 * qt + 16 * s2 + 4 * h + qi + 8 * hi, dt * 32 + 16 * (G & 1) + 4 * pi)
                            out.append(("dV/dK tr", "ds_read_b64_tr_b16", f))
            for g in range(4):  # dS^T writes
                out.append(("dS^T write b64", "ds_write_b64",
                            lambda l, wave=wave, qt=qt, g=g: doff(wave * 32 + (l & 31), 32 * qt + 8 * g + 4 * (l >> 5))))
        d0, q0 = 16 * (wave & 3), 32 * (wave >> 2)
        for ks in range(KB // 32):  # dQ stage
            for add in (0, 4):
                def fk(l, ks=ks, add=add, d0=d0):
                    G, qi, pi = l >> 4, (l & 15) >> 2, l & 3
                    return koff(32 * ks + 8 * G + qi + add, d0 + 4 * pi)
                out.append(("dQ K^T tr", "ds_read_b64_tr_b16", fk))
                for j in range(2):
                    def fd(l, ks=ks, add=add, q0=q0, j=j):
                        G, qi, pi = l >> 4, (l & 15) >> 2, l & 3
                        return doff(32 * ks + 8 * G + qi + add, q0 + 16 * j + 4 * pi)
                    out.append(("dQ dS^T tr", "ds_read_b64_tr_b16", fd))
    return out


def once_patterns(old=False):
    """Prologue and epilogue LDS accesses of one workgroup (once per launch)."""
    koff = aoff if old else k1b_off
    out = []
    for wave in range(NW):
        for i in range(KB * D // 8 // (64 * NW)):  # K and V blocks staged as 16-B chunks
            def ids(l, wave=wave, i=i):
                idx = wave * 64 + l + i * 64 * NW
                return idx // 8, idx % 8
            out.append(("prologue K store b128", "ds_write_b128", lambda l, ids=ids: koff(ids(l)[0], ids(l)[1] * 8)))
            out.append(("prologue V store b128", "ds_write_b128", lambda l, ids=ids: aoff(ids(l)[0], ids(l)[1] * 8)))
        for s in range(D // 16):  # K^T / V^T fragments
            out.append(("prologue K frag b128", "ds_read_b128",
                        lambda l, wave=wave, s=s: koff(wave * 32 + (l & 31), 16 * s + 8 * (l >> 5))))
            out.append(("prologue V frag b128", "ds_read_b128",
                        lambda l, wave=wave, s=s: aoff(wave * 32 + (l & 31), 16 * s + 8 * (l >> 5))))
        for c in range(D // 8):  # epilogue: dK, dV images, 8-B writes, then whole 16-B chunks back
            for _img in ("dK", "dV"):
                def fw(l, wave=wave, c=c):
                    row = wave * 32 + (l & 31)
                    return row * 128 + ((c ^ (row & 7)) << 4) + 8 * (l >> 5)
                out.append(("epilogue dK/dV write b64", "ds_write_b64", fw))
        for i in range(KB * D // 8 // (64 * NW)):
            for _img in ("dK", "dV"):
                def fr(l, wave=wave, i=i):
                    idx = wave * 64 + l + i * 64 * NW
                    r, c = idx // 8, idx % 8
                    return r * 128 + ((c ^ (r & 7)) << 4)
                out.append(("epilogue dK/dV read b128", "ds_read_b128", fr))
    return out


def summarize(patterns):
    """stage -> [instructions, cycles, ideal cycles]"""
    tab = defaultdict(lambda: [0, 0, 0])
    for stage, instr, addr in patterns:
        c, i = cycles(instr, addr)
        t = tab[stage]
        t[0] += 1
        t[1] += c
        t[2] += i
    return dict(tab)


def conflict_share(tiles, old=False):
    """SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE the model predicts for a workgroup that runs
    `tiles` query tiles (extra cycles over all LDS-array cycles)."""
    loop, once = summarize(loop_patterns(old)), summarize(once_patterns(old))
    cyc = tiles * sum(t[1] for t in loop.values()) + sum(t[1] for t in once.values())
    ideal = tiles * sum(t[2] for t in loop.values()) + sum(t[2] for t in once.values())
    return (cyc - ideal) / cyc


if __name__ == "__main__":
    for old in (True, False):
        print("== layouts before the dQ stage's own images" if old else "== k1b_off / dst1b_off")
        for name, pats in (("per query tile, 8 waves", loop_patterns(old)), ("once per workgroup", once_patterns(old))):
            print(f" {name}")
            for stage, (n, c, i) in summarize(pats).items():
                print(f"   {stage:28s} {n:5d} instructions  {c:6d} cycles  ideal {i:6d}  x{c / i:.2f}")
        loop = summarize(loop_patterns(old))
        c, i = sum(t[1] for t in loop.values()), sum(t[2] for t in loop.values())
        print(f" loop conflict share {100 * (c - i) / c:.1f} %; whole workgroup at 8 tiles (S = 512): "
              f"{100 * conflict_share(8, old):.1f} %")
