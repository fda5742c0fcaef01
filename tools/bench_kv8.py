#!/usr/bin/env python3
"""fp8 KV cache against the bf16 one (GPU box): python tools/bench_kv8.py [--out profiles/kv8.json]
Each row count is a child process under its own time limit (--step_timeout); a step that fails ends the tool, what the steps
before it measured is in --out already.

The decode-attention launch at hs 128, H 32, G 8, 1 552 cached keys, 128 and 640 rows: dh_attn_decode_bf16, the fused launch
the <= 128-row fp8 step uses today (dh_attn_decode_fused_bf16), and the kv8 step's three kernels (dh_qkv_rope_cache_kv8 +
dh_attn_decode_kv8 with its combine).  HIP events over a hipGraph of back-to-back calls, three alternating repeats; achieved
TB/s of the KV bytes each arm has to read."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from dualhyp_amd import ops
from tools.tune_decode_common import bench, D

ROOT = Path(__file__).resolve().parent.parent
HS, H, G, KEYS, S_MAX = 128, 32, 8, 1552, 1600
i32 = torch.int32


def attention_launches(rows):
    qkv_dim = (H + 2 * G) * HS
    from dualhyp_amd.gpt import build_rope_cache
    cos, sin = build_rope_cache(S_MAX, HS, torch.bfloat16, D)
    slot = torch.arange(rows, dtype=i32, device=D)
    kv_len = torch.full((rows,), KEYS, dtype=i32, device=D)
    pos = kv_len - 1
    q = torch.randn(rows, H, HS, device=D).bfloat16()
    qkv = torch.randn(rows, qkv_dim, device=D).bfloat16()
    qkv32 = qkv.float().view(1, rows, qkv_dim)
    kc = torch.randn(rows, G, S_MAX, HS, device=D).bfloat16()
    vt = torch.randn(rows, G, HS, S_MAX, device=D).bfloat16()
    k8, v8, ke, ve = ops.kv8_alloc(rows, G, S_MAX, HS, D)
    k8.copy_(torch.randint(0, 0x78, k8.shape, device=D, dtype=torch.uint8))      # finite e4m3 bytes
    v8.copy_(torch.randint(0, 0x78, v8.shape, device=D, dtype=torch.uint8))
    ke.copy_(torch.randint(-9, -5, ke.shape, device=D, dtype=torch.int8))
    ve.copy_(torch.randint(-9, -5, ve.shape, device=D, dtype=torch.int8))
    arms = {
        "bf16_split": lambda i: ops.attn_decode(q, kc, vt, slot, kv_len),
        "bf16_fused": lambda i: ops.attn_decode_fused(qkv32, qkv_dim, None, 0.0, (qkv_dim, qkv_dim), cos, sin, slot, kv_len, kc, vt, H, pairs=False),
        "kv8": lambda i: ops.attn_decode_kv8(ops.qkv_rope_cache_kv8(qkv, cos, sin, slot, pos, k8, v8, ke, ve, H, G), k8, v8, ke, ve, slot, kv_len),
    }
    us = {k: [] for k in arms}
    for _ in range(3):
        for name, fn in arms.items():
            us[name].append(bench(fn))
    elems = rows * G * KEYS * HS * 2
    kv_bytes = {"bf16_split": elems * 2, "bf16_fused": elems * 2, "kv8": elems + rows * G * KEYS * 2}
    out = {name: dict(us=[round(x, 1) for x in t], kv_bytes=kv_bytes[name], tb_per_s=round(kv_bytes[name] / (min(t) * 1e-6) / 1e12, 3))
           for name, t in us.items()}
    print(json.dumps({"decode_attention": {str(rows): out}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default="profiles/kv8.json")
    ap.add_argument("--step_timeout", type=int, default=600, help="seconds each GPU step may take")
    ap.add_argument("--worker", type=int, default=None, help="internal: the row count of one child")
    a = ap.parse_args()
    if a.worker:
        attention_launches(a.worker)
        return
    res = {"shape": dict(hs=HS, n_head=H, n_groups=G, cached_keys=KEYS, s_max=S_MAX), "decode_attention": {}}
    for step in (128, 640):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(step)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a step that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"step {step} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                print(l, flush=True)
                res["decode_attention"].update(json.loads(l)["decode_attention"])
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
