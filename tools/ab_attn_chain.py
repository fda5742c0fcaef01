#!/usr/bin/env python3
"""Same-box A/B of the single-token decode attention: attn_decode_fused_kernel (dh_set_tuning(40, 0)) against
attn_decode_chain_kernel (40, 1), alternating, five repeats each: us per launch and the K/V + pair-sum bytes per second.
Rows from DH_ROWS (default 32,640,2048), 545 keys, hs 64, LoRA on, 4 pair sums.  GPU box.
tune_attn.py stays what it is, a sweep of one kernel over key counts and partial counts at 32 rows with 22 caches alive: at
2 048 rows those caches would be 53 GB, and an A/B wants both arms in one process, alternating, on a few caches larger than the
MALL."""
import os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from dualhyp_amd import ops, _lib
from tools.tune_decode_common import bench, D
lib = _lib.load()
H, G, hs, S, KV, NB = 32, 4, 64, 576, 545, 3
cos = torch.randn(S, hs, device=D).bfloat16(); sin = torch.randn(S, hs, device=D).bfloat16()
Bq = torch.randn(2560, 16, device=D).bfloat16() * 0.02
for M in [int(r) for r in os.environ.get("DH_ROWS", "32,640,2048").split(",")]:
    nb = NB if M >= 256 else 22                       # small batches: one cache per call of the graph, nothing is re-read from L2
    kc = [torch.randn(M, G, S, hs, device=D).bfloat16() for _ in range(nb)]
    vt = [torch.randn(M, G, hs, S, device=D).bfloat16() for _ in range(nb)]
    q32 = [torch.randn(4, M, 2608, device=D) * 0.1 for _ in range(nb)]
    slot = torch.arange(M, dtype=torch.int32, device=D)
    kvl = torch.full((M,), KV, dtype=torch.int32, device=D)
    mb = (M * G * (KV - 1) * hs * 2 * 2 + 4 * M * 2608 * 4) / 1e6
    t = {0: [], 1: []}
    for rep in range(5):
        for arm in (0, 1):
            assert lib.dh_set_tuning(40, arm) == 0
            t[arm].append(bench(lambda i: ops.attn_decode_fused(q32[i % nb], 2560, Bq, 1.0, (2048, 2304), cos, sin, slot, kvl, kc[i % nb], vt[i % nb], H, pairs=False)))
    for arm, nm in ((0, "parent"), (1, "chain ")):
        v = sorted(t[arm])
        print(f"rows {M:5d} {nm}: " + " ".join(f"{x:6.1f}" for x in t[arm]) + f" us   median {v[2]:6.1f} us  spread {v[-1] - v[0]:4.1f} us  {mb / v[2]:5.2f} TB/s", flush=True)
    del kc, vt, q32
assert lib.dh_set_tuning(40, 1) == 0
