#!/usr/bin/env python3
"""finish_norm (sum of K-slice partials + LoRA + residual + RMSNorm) at 32 .. 640 rows, its independent loads requested behind
the hand-over barrier (dh_set_tuning(41, 0)) and ahead of it (41, 1), alternating, three repeats each (GPU box)."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from dualhyp_amd import ops, _lib
from tools.tune_decode_common import bench, D
lib = _lib.load()
d = 2048
wn = torch.ones(d, device=D).bfloat16(); Bp = torch.randn(d, 16, device=D).bfloat16()
for B in (32, 64, 128, 256, 640):
    xr = torch.randn(B, d, device=D).bfloat16()
    for ks, lora in ((8, True), (4, True), (11, False)):
        ys = [torch.randn(ks, B, d + (16 if lora else 0), device=D) for _ in range(4)]
        t = {0: [], 1: []}
        for rep in range(3):
            for hoist in (0, 1):
                assert lib.dh_set_tuning(41, hoist) == 0
                t[hoist].append(bench(lambda i: ops.finish_norm(ys[i % 4], d, xr, wn, 1e-5, lora_b=Bp if lora else None, lora_scale=1.0)))
        print(f"rows {B:4d} partials {ks:2d} lora {lora!s:5s}: behind " + " ".join(f"{x:5.1f}" for x in t[0]) + "   ahead " + " ".join(f"{x:5.1f}" for x in t[1]) + " us", flush=True)
assert lib.dh_set_tuning(41, -1) == 0
