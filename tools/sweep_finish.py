#!/usr/bin/env python3
"""finish_norm (sum of K-slice partials + LoRA + residual + RMSNorm) per launch, by row count (GPU box).

Arms, alternating, three repeats each: finish_norm_kernel with its independent loads behind the hand-over barrier (dh_set_tuning
41 = 0) and ahead of it (41 = 1), and finish_norm_rows_kernel (43 = 1) with 2, 3 and 4 rows per block (44).
Shapes: what the decode step's producers emit at d 2048 — 8 slices + LoRA, 4 pair sums + LoRA, 11 slices, 6 pair sums, and the
one-launch total (1 partial) with and without LoRA.  Rows: the arguments, default 32 64 128 256 640 1024 2048."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from dualhyp_amd import ops, _lib
from tools.tune_decode_common import bench, D
lib = _lib.load()
d = 2048
ARMS = (("behind", 0, 0, 0), ("ahead", 0, 1, 0), ("rows2", 1, 0, 2), ("rows3", 1, 0, 3), ("rows4", 1, 0, 4))   # name, key 43, 41, 44
wn = torch.ones(d, device=D).bfloat16(); Bp = torch.randn(d, 16, device=D).bfloat16()
for B in [int(a) for a in sys.argv[1:]] or (32, 64, 128, 256, 640, 1024, 2048):
    xr = torch.randn(B, d, device=D).bfloat16()
    for ks, lora, pairs in ((8, True, True), (4, True, False), (11, False, True), (6, False, False), (1, True, False), (1, False, False)):
        ys = [torch.randn(ks, B, d + (16 if lora else 0), device=D) for _ in range(4)]
        t = {a[0]: [] for a in ARMS}
        for rep in range(3):
            for name, rows_arm, hoist, rpb in ARMS:
                assert lib.dh_set_tuning(43, rows_arm) == 0 and lib.dh_set_tuning(41, hoist) == 0 and lib.dh_set_tuning(44, rpb) == 0
                t[name].append(bench(lambda i: ops.finish_norm(ys[i % 4], d, xr, wn, 1e-5, lora_b=Bp if lora else None, lora_scale=1.0, pairs=pairs)))
        print(f"rows {B:4d} partials {ks:2d} pairs {int(pairs)} lora {int(lora)}: " +
              "   ".join(f"{n} " + " ".join(f"{x:5.1f}" for x in v) for n, v in t.items()) + " us", flush=True)
assert lib.dh_set_tuning(41, -1) == 0 and lib.dh_set_tuning(43, -1) == 0 and lib.dh_set_tuning(44, 0) == 0
