#!/usr/bin/env python3
"""Per-block timeline of the single-token decode attention from a -DDH_ATTN_STAMPS build
(tools/build_variants.py decode_fused.hip stamps:-DDH_ATTN_STAMPS; DUALHYP_HIP_LIB=tools/bin/lib_stamps.so): thread 0 of every
block stamps entry, x·A^T handed over (first barrier), q ready (second barrier), first tile consumed, last PV done, partials
exchanged (third barrier), combine done (stores issued) and last store acknowledged.  Both kernels (dh_set_tuning 40 = 0 | 1),
DH_M rows (default 640), 545 keys, hs 64, LoRA on, 4 pair sums.  GPU box."""
import ctypes, os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np, torch
from dualhyp_amd import ops, _lib
lib = _lib.load()
raw = ctypes.CDLL(str(_lib.LIB_PATH))
D = "cuda:0"
H, G, hs, S = 32, 4, 64, 576
M = int(os.environ.get("DH_M", "640"))
KV = int(os.environ.get("DH_KV", "545"))
NB = 3
kc = [torch.randn(M, G, S, hs, device=D).bfloat16() for _ in range(NB)]
vt = [torch.randn(M, G, hs, S, device=D).bfloat16() for _ in range(NB)]
cos = torch.randn(S, hs, device=D).bfloat16(); sin = torch.randn(S, hs, device=D).bfloat16()
Bq = torch.randn(2560, 16, device=D).bfloat16() * 0.02
slot = torch.arange(M, dtype=torch.int32, device=D)
kvl = torch.full((M,), KV, dtype=torch.int32, device=D)
q32 = [torch.randn(4, M, 2608, device=D) * 0.1 for _ in range(NB)]
names = ["entry", "xA^T handed over (barrier 1)", "q ready (barrier 2)", "first tile consumed", "last PV done",
         "partials exchanged (barrier 3)", "combine done, stores issued", "last store acknowledged"]
for arm, nm in ((0, "attn_decode_fused_kernel (parent)"), (1, "attn_decode_chain_kernel")):
    assert lib.dh_set_tuning(40, arm) == 0
    for trial in range(2):
        for i in range(NB):
            ops.attn_decode_fused(q32[i], 2560, Bq, 1.0, (2048, 2304), cos, sin, slot, kvl, kc[i], vt[i], H, pairs=False)
        torch.cuda.synchronize()
        buf = np.zeros(4096 * 8, dtype=np.uint64)
        assert raw.dh_debug_attn_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0
    st = buf.reshape(4096, 8).astype(np.int64)[:min(4096, M * G)]
    rel = (st - st[:, :1]) * 0.01                       # us since the block's entry (100 MHz counter)
    life = rel[:, 7]
    span = (st[:, 7].max() - st[:, 0].min()) * 0.01
    print(f"{nm}: {M} rows, {KV} keys, {len(st)} blocks, launch span {span:.1f} us, block life median {np.median(life):.2f} us")
    print(f"   {'point':38s} {'median':>7s} {'p10':>7s} {'p90':>7s}   phase median   share of life")
    prev = np.zeros(len(st))
    for j in range(1, 8):
        ph = rel[:, j] - prev
        print(f"   {names[j]:38s} {np.median(rel[:, j]):7.2f} {np.percentile(rel[:, j], 10):7.2f} {np.percentile(rel[:, j], 90):7.2f}"
              f"   {np.median(ph):12.2f}   {100 * np.median(ph) / np.median(life):6.1f} %")
        prev = rel[:, j]
    first = st[:, 0] - st[:, 0].min() < 100               # blocks that started within the first microsecond: an idle memory system
    print(f"   blocks of the first wave ({first.sum()}): life median {np.median(life[first]):.2f} us; later blocks: {np.median(life[~first]) if (~first).any() else float('nan'):.2f} us")
assert lib.dh_set_tuning(40, 1) == 0
