#!/usr/bin/env python3
"""What per-sample key lengths buy: flash attention fwd and bwd on one shape, the dense call against
three length sets (all Sk; seeded uniform in [64, Sk]; all 128), interleaved rounds in one process.
Reports the time of each and the mean share of live 64-key tiles (forward) and 256-key blocks
(backward) the lengths leave.
usage: attn_varlen_probe.py [B H S D [reps]]   (default 32 16 512 64 20)"""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from flexflow_amd import kernels as Kn  # noqa: E402

B, H, S, D = (int(v) for v in sys.argv[1:5]) if len(sys.argv) > 4 else (32, 16, 512, 64)
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 20
dev = "cuda"
torch.manual_seed(0)
qkv = torch.randn(B, S, 3, H, D, device=dev).bfloat16()
o = torch.empty(B, S, H, D, device=dev, dtype=torch.bfloat16)
do = torch.randn_like(o)
dqkv = torch.empty_like(qkv)
sq = (S * 3 * H * D, D, 3 * H * D)
so = (S * H * D, D, H * D)
base, dbase = qkv.view(-1), dqkv.view(-1)
q, k, v = base, base[H * D:], base[2 * H * D:]
dq, dk, dv = dbase, dbase[H * D:], dbase[2 * H * D:]
scale = D ** -0.5
g = torch.Generator().manual_seed(1)
sets = {
    "dense (no lengths)": None,
    f"all {S}": torch.full((B,), S, dtype=torch.int32),
    f"uniform [64, {S}]": torch.randint(64, S + 1, (B,), generator=g, dtype=torch.int32),
    "all 128": torch.full((B,), min(128, S), dtype=torch.int32),
}
KB = 256 if D == 64 else 128


def timed(fn):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


fres, bres = {n: [] for n in sets}, {n: [] for n in sets}
dev_lens = {n: (t.to(dev) if t is not None else None) for n, t in sets.items()}
for rnd in range(5):
    for name, kl in dev_lens.items():
        lse = Kn.flash_attn_fwd(q, sq, k, sq, v, sq, o, so, B, H, S, S, D, scale, False, key_lens=kl)
        fres[name].append(timed(lambda: Kn.flash_attn_fwd(q, sq, k, sq, v, sq, o, so, B, H, S, S, D, scale, False,
                                                          key_lens=kl)))
        bres[name].append(timed(lambda: Kn.flash_attn_bwd(q, sq, k, sq, v, sq, o, so, do, so, lse, dq, sq, dk, sq, dv,
                                                          sq, B, H, S, S, D, scale, False, key_lens=kl)))
print(f"B={B} H={H} S={S} D={D}, {reps} calls per timing, 5 interleaved rounds; times in ms: min (all rounds)")
f0, b0 = min(fres["dense (no lengths)"]), min(bres["dense (no lengths)"])
for name, t in sets.items():
    lens = t if t is not None else torch.full((B,), S)
    tiles = ((lens + 63) // 64).float().mean().item() / ((S + 63) // 64)
    blocks = ((lens + KB - 1) // KB).clamp(min=1).float().mean().item() / ((S + KB - 1) // KB)
    f, b = min(fres[name]), min(bres[name])
    print(f"{name:22s} fwd {f:.4f} ({f / f0:.2f}x dense, live tiles {tiles:.2f}) {[round(x, 4) for x in fres[name]]}")
    print(f"{'':22s} bwd {b:.4f} ({b / b0:.2f}x dense, live blocks {blocks:.2f}) {[round(x, 4) for x in bres[name]]}")
