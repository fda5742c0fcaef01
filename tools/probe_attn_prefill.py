#!/usr/bin/env python3
"""Per-block timeline of the causal prefill attention from a -DDH_PREFILL_STAMPS build
(tools/build_variants.py attention.hip pfstamps:-DDH_PREFILL_STAMPS; DUALHYP_HIP_LIB=tools/bin/lib_pfstamps.so): lane 0 of wave 0 of
every block stamps entry, metadata read, Q fragments in registers, first stage landed (barrier 0), per key step S MFMAs issued /
softmax done / last PV issued / barrier passed, and last store issued (attention.hip, PF_STAMP).  Medians over blocks by query-tile
index at the bench shape (64 sequences x 512 tokens, 32 heads / 4 groups, hs 64), one table per arm of dh_set_tuning 42 that the
library knows (a library from before the key prints the one kernel it has).  GPU box."""
import ctypes, os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np, torch
from dualhyp_amd import ops, _lib
lib = _lib.load()
raw = ctypes.CDLL(str(_lib.LIB_PATH))
assert hasattr(raw, "dh_debug_prefill_stamps"), "not a -DDH_PREFILL_STAMPS build of attention.hip"
D = "cuda:0"
B, T, H, G, hs = 64, 512, 32, 4, 64
NBLK, SLOTS, STEPS = 16384, 40, 8
g = torch.Generator(device=D).manual_seed(0)
rn = lambda *s: (torch.randn(*s, device=D, generator=g) * 0.5).bfloat16()
i32 = torch.int32
qkv = rn(B * T, (H + 2 * G) * hs)
cos, sin = rn(T, hs), rn(T, hs)
slot = torch.arange(B, dtype=i32, device=D).repeat_interleave(T)
pos = torch.arange(T, dtype=i32, device=D).repeat(B)
kc = torch.zeros(B, G, T, hs, device=D, dtype=torch.bfloat16); vt = torch.zeros(B, G, hs, T, device=D, dtype=torch.bfloat16)
q = ops.qkv_rope_cache(qkv, cos, sin, slot, pos, kc, vt, H, G)
seq = torch.arange(B, dtype=i32, device=D); qs = seq * T; ql = torch.full((B,), T, dtype=i32, device=D); z = torch.zeros(B, dtype=i32, device=D)
QT = T // 32


def stamps():
    buf = np.zeros(NBLK * SLOTS, dtype=np.uint64)
    assert raw.dh_debug_prefill_stamps(buf.ctypes.data_as(ctypes.c_void_p), 1) == 0
    return buf.reshape(NBLK, SLOTS).astype(np.int64)


arms = [int(a) for a in sys.argv[1:]] or [a for a in (0, 4, 2) if lib.dh_set_tuning(42, a) == 0] or [None]    # arms on the command line, or all
for arm in arms:
    if arm is not None:
        assert lib.dh_set_tuning(42, arm) == 0
    wpb = arm or H // G
    nblk = QT * G * (H // G // wpb) * B
    for trial in range(3):                                # the last launch is the one read: caches and clocks warm
        stamps()
        ops.attn_prefill(q, kc, vt, seq, qs, ql, z, T)
        torch.cuda.synchronize()
    st = stamps()[:nblk]
    assert (st[:, 0] > 0).all() and (st[:, 36] > 0).all(), "a block left no stamps"
    if os.environ.get("DH_STAMPS_NPY"):                   # the raw stamps, [block][slot], for another look
        np.save(f"{os.environ['DH_STAMPS_NPY']}_arm{arm}.npy", st)
    qt = st[:, 39]                                        # the block's query tile index (attention.hip)
    us = lambda a: a * 0.01                               # 100 MHz counter
    life = us(st[:, 36] - st[:, 0])
    span = us(st[:, 36].max() - st[:, 0].min())
    print(f"arm {arm}: {wpb} waves per block, {nblk} blocks, launch span {span:.1f} us, block life median {np.median(life):.2f} us, "
          f"sum of block lives / 256 CUs {life.sum() / 256:.0f} us")
    print("   us, medians over blocks (per-step columns: medians over the block's steps, then over blocks)")
    print(f"   {'qt':>3s} {'steps':>5s} {'life':>7s} | {'meta':>6s} {'Q regs':>6s} {'stage0':>6s} | {'S mfma':>6s} {'softmx':>6s} {'PV':>6s} {'barrier':>7s} {'step':>6s} | {'store':>6s}")
    tot = np.zeros(8)
    for t in range(QT):
        s = st[qt == t]
        n = min(t // 2 + 1, STEPS)
        step = s[:, 4:4 + 4 * n].reshape(len(s), n, 4)
        prev = np.concatenate([s[:, 3:4], step[:, :-1, 3]], axis=1)          # the barrier that opened each step
        ph = [us(np.median(step[:, :, 0] - prev, axis=1)), us(np.median(step[:, :, 1] - step[:, :, 0], axis=1)),
              us(np.median(step[:, :, 2] - step[:, :, 1], axis=1)), us(np.median(step[:, :, 3] - step[:, :, 2], axis=1))]
        pro = [us(s[:, 1] - s[:, 0]), us(s[:, 2] - s[:, 1]), us(s[:, 3] - s[:, 2])]
        epi = us(s[:, 36] - step[:, -1, 3])
        m = np.median
        print(f"   {t:3d} {t // 2 + 1:5d} {m(us(s[:, 36] - s[:, 0])):7.2f} | {m(pro[0]):6.2f} {m(pro[1]):6.2f} {m(pro[2]):6.2f} | "
              f"{m(ph[0]):6.2f} {m(ph[1]):6.2f} {m(ph[2]):6.2f} {m(ph[3]):7.2f} {m(sum(ph)):6.2f} | {m(epi):6.2f}")
        tot += np.array([p.sum() for p in pro] + [us(step[:, :, 0] - prev).sum(), us(step[:, :, 1] - step[:, :, 0]).sum(),
                                                   us(step[:, :, 2] - step[:, :, 1]).sum(), us(step[:, :, 3] - step[:, :, 2]).sum(), epi.sum()])
    names = ["metadata", "Q in registers", "stage 0 + barrier 0", "S MFMAs issued", "softmax", "PV issued", "wait + barrier", "normalise + store"]
    print("   share of all block time: " + ", ".join(f"{n} {100 * v / tot.sum():.1f} %" for n, v in zip(names, tot)))
    # which CU a block ran on (HW_ID bits 8-15 + XCC_ID): blocks resident per CU, averaged over the launch, and the time a CU
    # spent with none of the stamped intervals open (wave 0's entry to its last store: a block's launch and drain are outside)
    cu = (st[:, 38] & 15) * 256 + ((st[:, 37] >> 8) & 255)
    res, idle = [], []
    for c in np.unique(cu):
        b = st[cu == c]
        ev = sorted([(t0, 1) for t0 in b[:, 0]] + [(t1, -1) for t1 in b[:, 36]])
        open_, t_prev, none = 0, st[:, 0].min(), 0
        for tt, d in ev:
            if open_ == 0: none += tt - t_prev
            open_ += d; t_prev = tt
        res.append(us((b[:, 36] - b[:, 0]).sum()) / span); idle.append(us(none + st[:, 36].max() - t_prev))
    print(f"   {len(res)} CUs: blocks resident per CU (time average) median {np.median(res):.2f}, p10 {np.percentile(res, 10):.2f}, p90 {np.percentile(res, 90):.2f}; "
          f"blocks per CU {nblk / len(res):.1f}; time with no block open per CU: median {np.median(idle):.1f} us of {span:.1f}")
    xcc = st[:, 38] & 15
    print("   per XCD, sum of block lives / 32 CUs [us] (last store at [us]): " +
          "  ".join(f"{k}: {life[xcc == k].sum() / 32:.0f} ({us(st[xcc == k, 36].max() - st[:, 0].min()):.0f})" for k in np.unique(xcc)))
    first = st[:, 0] - st[:, 0].min() < 100               # blocks that started within the first microsecond
    print(f"   blocks of the first wave ({first.sum()}): life median {np.median(life[first]):.2f} us; later blocks: {np.median(life[~first]):.2f} us", flush=True)
