#!/usr/bin/env python3
"""Decode partial-sum GEMMs at the driver's 640 rows (and neighbours): K-sliced streaming kernel (slices) against the tiled
split-K kernel (pair sums, 128 x 128 and 128 x 256 tiles), plus the consumers on either input (GPU box).

`--chain`: the one-launch total on the register-lean tile (gemm_dt_chain_kernel, 2 and 4 stages) against the default pair-sum
route, per linear: the producer alone, and producer + consumer (qkv': the single-token attention at 544 cached keys; proj',
mlp': finish_norm, with finish_norm_kernel (dh_set_tuning 43 = 0) and with finish_norm_rows_kernel (43 = 1)), which reads one
partial instead of 4 to 6.  Three alternating repeats each; the decision is taken on the sum."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dualhyp_amd import ops, _lib
from tune_decode_common import bench
lib = _lib.load()
dev = "cuda"
d, I, L = 2048, 5632, 8
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.05).bfloat16()
Wq, Wp, Wm = [rn(2560, d) for _ in range(L)], [rn(d, d) for _ in range(L)], [rn(d, I) for _ in range(L)]
A48, A16 = [rn(48, d) for _ in range(L)], [rn(16, d) for _ in range(L)]
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def sweep_chain(M):
    H, G, hs, S = 32, 4, 64, 576
    x, xa, xr, wn = rn(M, d), rn(M, I), rn(M, d), rn(d)
    Bq, Bp = rn(2560, 16), rn(d, 16)
    cos, sin = rn(S, hs), rn(S, hs)
    kc, vt = rn(M, G, S, hs), rn(M, G, hs, S)
    slot = torch.arange(M, dtype=torch.int32, device=dev)
    kv_len = torch.full((M,), 544, dtype=torch.int32, device=dev)

    def attn(y, i):
        ops.attn_decode_fused(y, 2560, Bq, 1.0, (H * hs, (H + G) * hs), cos, sin, slot, kv_len, kc, vt, H, pairs=False)

    def fin(lora):
        return lambda y, i: ops.finish_norm(y, d, xr, wn, 1e-5, lora_b=Bp if lora else None, lora_scale=1.0, pairs=False)
    linears = (("qkv'", x, Wq, A48, 8, attn, (("attn", -1),)), ("proj'", x, Wp, A16, 8, fin(True), (("fin", 0), ("fin_rows", 1))),
               ("mlp'", xa, Wm, None, 11, fin(False), (("fin", 0), ("fin_rows", 1))))
    for name, xin, W, A, ks, cons, cons_arms in linears:
        y1 = torch.empty(M, W[0].size(0) + (A[0].size(0) if A else 0), device=dev)
        prods = (("pairs", lambda i: ops.linear_partial_pairs(xin, W[i % L], A[i % L] if A else None, ksplit=ks), 0),
                 ("chain2", lambda i: ops.linear_chain(xin, W[i % L], A[i % L] if A else None, ksplit=ks, out=y1).unsqueeze(0), 2),
                 ("chain4", lambda i: ops.linear_chain(xin, W[i % L], A[i % L] if A else None, ksplit=ks, out=y1).unsqueeze(0), 4))
        t = {}
        for rep in range(3):
            for pname, prod, stages in prods:
                lib.dh_set_tuning(7, 1 if stages else 1 << 30)
                lib.dh_set_tuning(8, stages)
                t.setdefault((pname, "alone"), []).append(bench(prod))
                for cname, k43 in cons_arms:
                    lib.dh_set_tuning(43, k43)
                    t.setdefault((pname, "+" + cname), []).append(bench(lambda i: cons(prod(i), i)))
                lib.dh_set_tuning(43, -1)
        lib.dh_set_tuning(8, 0)
        for k, v in t.items():
            print(f"M={M:5d} {name:5s} {k[0]:6s} {k[1]:9s} " + " ".join(f"{a:6.1f}" for a in v) + " us", flush=True)


if "--chain" in sys.argv:
    try:
        for M in [int(a) for a in args] or [640, 1024, 1536, 2048]:
            sweep_chain(M)
    finally:
        lib.dh_set_tuning(7, 1 << 30); lib.dh_set_tuning(8, 0); lib.dh_set_tuning(43, -1)
    sys.exit(0)

for M in [int(a) for a in args] or [160, 256, 640, 1024, 2048]:
    x, xa = rn(M, d), rn(M, I)
    xr, wn = rn(M, d), rn(d)
    row = [f"M={M:5d}"]
    for name, xin, W, A, ks in (("qkv'", x, Wq, A48, 8), ("proj'", x, Wp, A16, 8), ("mlp'", xa, Wm, None, 11)):
        t0 = bench(lambda i: ops.linear_partial(xin, W[i % L], A[i % L] if A else None, ksplit=ks))
        ts = []
        for wnv in (2, 4):
            lib.dh_set_tuning(17, wnv)
            ts.append(bench(lambda i: ops.linear_partial_pairs(xin, W[i % L], A[i % L] if A else None, ksplit=ks)))
        lib.dh_set_tuning(17, 0)
        row.append(f"{name} slices {t0:5.1f} | pairs 128x128 {ts[0]:5.1f} 128x256 {ts[1]:5.1f}")
    y8 = ops.linear_partial(x, Wp[0], A16[0], ksplit=8)
    y4 = ops.linear_partial_pairs(x, Wp[0], A16[0], ksplit=8)
    Bp = rn(d, 16)
    f8 = bench(lambda i: ops.finish_norm(y8, d, xr, wn, 1e-5, lora_b=Bp, lora_scale=1.0, pairs=True))
    f4 = bench(lambda i: ops.finish_norm(y4, d, xr, wn, 1e-5, lora_b=Bp, lora_scale=1.0, pairs=False))
    row.append(f"finish 8 slices {f8:5.1f} | 4 pairs {f4:5.1f}")
    print("  ".join(row), flush=True)
