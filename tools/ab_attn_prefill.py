#!/usr/bin/env python3
"""Same-box A/B of the causal prefill attention's block size (dh_set_tuning 42: 0 = all q_per_kv heads of a KV group in one block,
4 | 2 = that many waves per block), one process, the arms alternating, five repeats each: us per launch with spread, and the
checksum of y, which has to be the same number on every arm.  Shapes: the bench's 64 x 512 (32 heads / 4 groups, hs 64), 32 x 512
of the same model, and the Llama-3 side line's 32 x 1536 (32 heads / 8 groups, hs 128); DH_SHAPES=B,T,H,G,hs;... for others.
GPU box."""
import os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from dualhyp_amd import ops, _lib
from tools.tune_decode_common import bench, D
lib = _lib.load()
ARMS = (0, 4, 2)
shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("DH_SHAPES", "64,512,32,4,64;32,512,32,4,64;32,1536,32,8,128").split(";")]
i32 = torch.int32
for B, T, H, G, hs in shapes:
    g = torch.Generator(device=D).manual_seed(0)
    rn = lambda *s: (torch.randn(*s, device=D, generator=g) * 0.5).bfloat16()
    qkv = rn(B * T, (H + 2 * G) * hs)
    cos, sin = rn(T, hs), rn(T, hs)
    slot = torch.arange(B, dtype=i32, device=D).repeat_interleave(T)
    pos = torch.arange(T, dtype=i32, device=D).repeat(B)
    kc = torch.zeros(B, G, T, hs, device=D, dtype=torch.bfloat16); vt = torch.zeros(B, G, hs, T, device=D, dtype=torch.bfloat16)
    q = ops.qkv_rope_cache(qkv, cos, sin, slot, pos, kc, vt, H, G)
    del qkv
    seq = torch.arange(B, dtype=i32, device=D); qs = seq * T; ql = torch.full((B,), T, dtype=i32, device=D); z = torch.zeros(B, dtype=i32, device=D)
    t, ck = {a: [] for a in ARMS}, {}
    for rep in range(5):
        for arm in ARMS:
            assert lib.dh_set_tuning(42, arm) == 0
            t[arm].append(bench(lambda i: ops.attn_prefill(q, kc, vt, seq, qs, ql, z, T)))
            y = ops.attn_prefill(q, kc, vt, seq, qs, ql, z, T)
            ck.setdefault(arm, set()).add((y.float().abs().sum().item(), y.view(torch.int16).to(torch.int64).sum().item()))
    print(f"{B} x {T}, {H} heads / {G} groups, hs {hs}:")
    for arm in ARMS:
        v = sorted(t[arm])
        print(f"   arm {arm} ({arm or H // G} waves per block): " + " ".join(f"{x:7.1f}" for x in t[arm]) +
              f" us   median {v[2]:7.1f} us  spread {v[-1] - v[0]:5.1f} us   checksum {sorted(ck[arm])}", flush=True)
    assert all(ck[a] == ck[0] and len(ck[a]) == 1 for a in ARMS), "the arms do not give the same y"
    del q, kc, vt
