"""attn_verify_fused_kernel (csrc/decode_fused.hip) as an op, against what its header comment promises.

a. Row j of a sequence has the BITS of the single-token kernel at kv_len = len + j, and the caches end as after n_live plain
   steps: one verify launch against S launches of ops.attn_decode_fused on the same inputs, torch.equal throughout.  The inputs
   are those of tests/test_hip_decode_attn_chain.py (caches pre-filled with random bf16, so a mask mistake reads numbers and
   not zeros; seq_slot a reversed permutation; random cos / sin) with synthetic fp32 partials, so n_part and `pairs` are free:
   every head size meets every column geometry, every partial-count class on both sides of its boundary, partials that already
   are pair sums, LoRA on and off, p_max at and below s_max, and the lengths at which the S positions touch a tile edge, wave 0
   takes its second tile (key 256 = 8 waves x 32 keys), 17 tiles are walked and rows fall behind p_max.
b. Both kernels could share a mistake: real partials, and every live row against causal attention in fp64, under the gate
   tests/test_hip_ops.py::test_fused_decode_kernels defines on torch's CPU bf16 SDPA.
c. What the entry point refuses, it refuses before it launches anything."""
import math

import pytest
import torch

from conftest import ulp_diff, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_MAX = 576
HEAD_SIZES = (64, 96, 128)
# (n_head, n_groups, S): 32 columns (the benchmark model at D = 3); 32 with q_per_kv at the single-token kernel's 16; S at its
# maximum; 20 columns (ends inside the upper half); 15 (q_per_kv = 3: the single-token kernel takes any q_per_kv <= 16); the smallest
GEOMS = ((8, 1, 4), (16, 1, 2), (4, 4, 8), (8, 2, 5), (6, 2, 5), (8, 2, 2))
# (n_part, pairs): the <., 2, .>, <., 8, .> and <., 16, .> instantiations (n_part <= 2, <= 8, else), both sides of each boundary
PARTS = ((1, True), (2, True), (8, True), (11, True), (4, False), (6, False))
P_MAXES = (S_MAX, S_MAX - 64)
# each head size meets each geometry and each partial count once, in a pairing of its own; hs 64 pairs the benchmark geometry
# with the 8 K-slices a d = 2048 model emits
CASES = [(hs, GEOMS[i], PARTS[(i + 2 + 2 * k) % len(PARTS)]) for k, hs in enumerate(HEAD_SIZES) for i in range(len(GEOMS))]


@pytest.fixture(autouse=True)
def _default_kernel_afterwards():
    yield
    from dualhyp_amd import _lib
    _lib.check(_lib.load().dh_set_tuning(40, 1))


def _lens(S, p_max):
    """kv_len values (row 0's token included; row j sits at position len - 1 + j), each <= p_max as the op's caller keeps them"""
    touch = lambda edge: range(edge - S + 1, edge + 2)       # [pos, pos + S) ends at, straddles or starts at the tile edge
    lens = {1, 2, 63, 64, 65, 511, 512, 513, 545, *touch(32), *touch(256)}
    # all rows live with the last one on the last position; S - 1 rows live; one row live (len == p_max)
    lens |= {p_max - S + 1, p_max - S + 2, p_max}
    return sorted(n for n in lens if 1 <= n <= p_max)


def _inputs(hs, n_head, n_groups, S, n_part, lens, n_seq, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    qkv_dim = (n_head + 2 * n_groups) * hs
    kv_len = torch.tensor([lens[i % len(lens)] for i in range(n_seq)], dtype=torch.int32, device=DEV)
    return dict(hs=hs, n_head=n_head, n_groups=n_groups, S=S, qkv_dim=qkv_dim, n_seq=n_seq, kv_len=kv_len,
                q32=torch.randn(n_part, n_seq * S, qkv_dim + 48, device=DEV, generator=g) * 0.3,
                bq=(torch.randn(qkv_dim, 16, device=DEV, generator=g) * 0.05).bfloat16(),
                slot=torch.arange(n_seq, dtype=torch.int32, device=DEV).flip(0).contiguous(),
                cos=r(S_MAX, hs), sin=r(S_MAX, hs), kc=r(n_seq, n_groups, S_MAX, hs), vt=r(n_seq, n_groups, hs, S_MAX))


def _verify(I, q32, lora, p_max, pairs):
    from dualhyp_amd import ops
    kc, vt = I["kc"].clone(), I["vt"].clone()
    att = ops.attn_verify_fused(q32, I["qkv_dim"], lora, 2.0, (I["n_head"] * I["hs"], (I["n_head"] + I["n_groups"]) * I["hs"]), I["cos"], I["sin"],
                                I["slot"], I["kv_len"], kc, vt, I["n_head"], I["S"], p_max=p_max, pairs=pairs)
    return att, kc, vt


def _plain_steps(I, q32, lora, p_max, pairs):
    """S launches of the single-token op: launch j takes rows seq * S + j at kv_len + j, without the sequences whose position
    pos + j does not exist (>= p_max).  -> att (rows without a position stay 0), caches, live [n_seq, S]"""
    from dualhyp_amd import ops
    S, hs, n_head = I["S"], I["hs"], I["n_head"]
    kc, vt = I["kc"].clone(), I["vt"].clone()
    att = torch.zeros((I["n_seq"] * S, n_head * hs), dtype=torch.bfloat16, device=DEV)
    live = torch.zeros((I["n_seq"], S), dtype=torch.bool, device=DEV)
    for j in range(S):
        idx = (I["kv_len"] - 1 + j < p_max).nonzero().flatten()
        if idx.numel() == 0:
            break
        rows = idx * S + j
        att[rows] = ops.attn_decode_fused(q32[:, rows].contiguous(), I["qkv_dim"], lora, 2.0, (n_head * hs, (n_head + I["n_groups"]) * hs),
                                          I["cos"], I["sin"], I["slot"][idx].contiguous(), (I["kv_len"][idx] + j).to(torch.int32), kc, vt,
                                          n_head, pairs=pairs)
        live[idx, j] = True
    return att, kc, vt, live


def _check(tag, I, p_max, ver, ver2, plain):
    from dualhyp_amd import ops
    S, hs, n_seq = I["S"], I["hs"], I["n_seq"]
    att, kc, vt = ver
    att_p, kc_p, vt_p, live = plain
    lens = I["kv_len"].tolist()
    n_live = [min(S, p_max - (n - 1)) for n in lens]
    assert live.sum(1).tolist() == n_live and min(n_live) >= 1
    assert torch.isfinite(att_p.float()).all(), f"{tag}: the plain steps' rows are not finite"
    # ---- live rows: the bits of the plain step at kv_len + j
    bad = ((att != att_p).any(1) & live.flatten()).nonzero().flatten().tolist()
    if bad:
        r = bad[0]
        c = int((att[r] != att_p[r]).nonzero()[0])
        where = [(q // S, q % S, lens[q // S] + q % S) for q in bad[:8]]
        pytest.fail(f"{tag}: {len(bad)} of {int(live.sum())} live rows differ from the plain steps.  First: seq {r // S} j {r % S} "
                    f"kv_len {lens[r // S]} + {r % S} head {c // hs} channel {c % hs}: {att[r, c].item()} for {att_p[r, c].item()}.  "
                    f"(seq, j, kv_len of the step) of the first rows: {where}")
    # ---- rows without a position: finite
    bad = (~torch.isfinite(att.float()).all(1) & ~live.flatten()).nonzero().flatten().tolist()
    assert not bad, f"{tag}: rows behind p_max = {p_max} are not finite: (seq, j, kv_len) {[(q // S, q % S, lens[q // S]) for q in bad[:8]]}"
    # ---- the caches: those of the plain steps, and nothing but [pos, pos + n_live) of a sequence's slot has changed
    kp, vp = ops.kcache_to_plain(kc), ops.vcache_to_plain(vt).transpose(2, 3)           # [slot, group, key, channel]
    for name, a, b in (("K", kp, ops.kcache_to_plain(kc_p)), ("V^T", vp, ops.vcache_to_plain(vt_p).transpose(2, 3))):
        ne = (a != b).nonzero()
        if ne.numel():
            s, g, key, ch = ne[0].tolist()
            seq = n_seq - 1 - s
            pytest.fail(f"{tag}: the {name} cache differs from the plain steps' in {ne.size(0)} elements.  First: seq {seq} (slot {s}) "
                        f"kv_len {lens[seq]} group {g} position {key} (j {key - lens[seq] + 1}) channel {ch}")
    assert torch.equal(kc, kc_p) and torch.equal(vt, vt_p)
    pos_s = (I["kv_len"] - 1).flip(0).long()[:, None]                                    # by slot: slot = n_seq - 1 - seq
    end_s = pos_s + torch.tensor(n_live, device=DEV).flip(0)[:, None]
    keys = torch.arange(S_MAX, device=DEV)[None, :]
    outside = (keys < pos_s) | (keys >= end_s)
    k0, v0 = ops.kcache_to_plain(I["kc"]), ops.vcache_to_plain(I["vt"]).transpose(2, 3)
    changed = (kp != k0).any(3).any(1) | (vp != v0).any(3).any(1)                        # [slot, key]
    behind = (changed[:, p_max:]).nonzero()
    assert not behind.numel(), (f"{tag}: cache positions >= p_max = {p_max} were written: (seq, kv_len, position) "
                                f"{[(n_seq - 1 - s, lens[n_seq - 1 - s], p_max + k) for s, k in behind[:8].tolist()]}")
    stray = (changed & outside).nonzero()
    assert not stray.numel(), (f"{tag}: the append wrote outside [pos, pos + n_live): (seq, kv_len, position) "
                               f"{[(n_seq - 1 - s, lens[n_seq - 1 - s], k) for s, k in stray[:8].tolist()]}")
    assert (changed | outside).all(), f"{tag}: a live row's position kept its initial K and V"
    # ---- a second launch: the same bits (the in-launch append is read back behind a fence; a race would show here)
    att2, kc2, vt2 = ver2
    bad = (att != att2).any(1).nonzero().flatten().tolist()
    assert not bad, f"{tag}: two verify launches differ in (seq, j, kv_len) {[(q // S, q % S, lens[q // S]) for q in bad[:8]]}"
    assert torch.equal(kc, kc2) and torch.equal(vt, vt2), f"{tag}: two verify launches leave different caches"


def _run(hs, geom, part, p_max, lens=None, n_seq=None, seed=5):
    n_head, n_groups, S = geom
    n_part, pairs = part
    lens = _lens(S, p_max) if lens is None else lens
    # the (4, 4, 8) geometry also fills the chip: 72 sequences x 4 groups = 288 blocks, more than one per CU
    n_seq = n_seq or max(len(lens), 72 if n_groups == 4 else 0)
    I = _inputs(hs, n_head, n_groups, S, n_part, lens, n_seq, seed + hs + 7 * n_part + S)
    for lora in (True, False):
        # without LoRA the partials carry no x·A^T columns (n_ext = 0)
        q32, bq = (I["q32"], I["bq"]) if lora else (I["q32"][..., :I["qkv_dim"]].contiguous(), None)
        ver, ver2 = _verify(I, q32, bq, p_max, pairs), _verify(I, q32, bq, p_max, pairs)
        plain = _plain_steps(I, q32, bq, p_max, pairs)
        torch.cuda.synchronize()
        tag = f"hs {hs} (n_head, n_groups, S) {geom} n_part {n_part} pairs {pairs} lora {lora} p_max {p_max}"
        _check(tag, I, p_max, ver, ver2, plain)


@pytest.mark.parametrize("p_max", P_MAXES, ids=lambda p: f"pmax{p}")
@pytest.mark.parametrize("hs,geom,part", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"hs{v}")
def test_verify_rows_are_the_bits_of_plain_steps(hs, geom, part, p_max):
    _run(hs, geom, part, p_max)


@pytest.mark.parametrize("p_max", P_MAXES, ids=lambda p: f"pmax{p}")
def test_verify_rows_against_the_parent_single_token_kernel(p_max):
    """At hs 64 the plain steps above are attn_decode_chain_kernel's; here they are attn_decode_fused_kernel's (dh_set_tuning 40)."""
    from dualhyp_amd import _lib
    _lib.check(_lib.load().dh_set_tuning(40, 0))
    _run(64, GEOMS[0], (8, True), p_max)
    _run(64, GEOMS[2], (11, True), p_max)


@pytest.mark.parametrize("hs", HEAD_SIZES)
def test_single_sequence(hs):
    """A launch of one sequence (n_groups blocks): at a tile edge, where wave 0 takes its second tile, at 17 tiles, behind p_max."""
    for n in (1, 31, 257, 545, S_MAX - 1):
        _run(hs, (8, 2, 4), (8, True), S_MAX, lens=[n], n_seq=1)
        _run(hs, (8, 2, 4), (4, False), S_MAX - 64, lens=[min(n, S_MAX - 64 - 1)], n_seq=1)


def test_case_table_covers_every_value_at_every_head_size():
    for hs in HEAD_SIZES:
        mine = [(g, p) for h, g, p in CASES if h == hs]
        assert {g for g, _ in mine} == set(GEOMS) and {p for _, p in mine} == set(PARTS)
    for S in (2, 4, 5, 8):
        for p_max in P_MAXES:
            lens = _lens(S, p_max)
            pos = [n - 1 for n in lens]
            assert {p_max - S, p_max - S + 1, p_max - 1} <= set(pos) and max(lens) == p_max       # n_live = S, S - 1 and 1
            for edge in (32, 256):                                                               # every way of touching the edge
                assert set(range(edge - S, edge + 1)) <= set(pos)
            assert {1, 2, 63, 64, 65, 511, 512} <= set(lens) and (p_max < S_MAX or {513, 545} <= set(lens))


# ---- b. against fp64 attention -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,n_head,n_groups", ((64, 8, 1), (96, 8, 2), (128, 8, 1)))
def test_verify_rows_against_fp64_attention(hs, n_head, n_groups):
    """Real partials (ops.linear_partial of x, W and the 48 LoRA-A rows), past context through ops.qkv_rope_cache; every row j against
    causal attention over keys [0, pos + j] in fp64 from the oracle's bf16 q / k / v.  The gate is test_fused_decode_kernels':
    err <= max(2 err_ref, 2e-2) with err_ref the distance of torch's CPU bf16 SDPA from the same truth; at most 3 ulp (mean 0.5)
    from that SDPA; appended K / V^T rows within 1 ulp on at most 1 % of the elements; past cache rows bit for bit."""
    from dualhyp_amd import ops
    from dualhyp_amd.gpt import _pad_rank
    from oracle import ger_oracle as O
    from test_hip_ops import U, check_ulp
    F = torch.nn.functional
    S, r, s = 4, 16, 2.0
    lens = [31, 33, 97, 545]                        # kv_len per sequence, row 0's token included
    B = len(lens)
    d, qpk, kv = n_head * hs, n_head // n_groups, n_groups * hs
    N = d + 2 * kv
    xn = U((B * S, d), 1.0, "vx")
    W, A, Bm = U((N, d), 0.05, "vw"), U((3 * r, d), 1 / math.sqrt(d), "va"), U((N, r), 0.05, "vb")
    A48 = torch.zeros(48, d, dtype=torch.bfloat16)
    for seg in range(3):
        A48[16 * seg:16 * seg + r] = A[seg * r:(seg + 1) * r]
    y32 = ops.linear_partial(xn.to(DEV), W.to(DEV), A48.to(DEV), ksplit=2)
    cos, sin = O.build_rope_cache(S_MAX, hs)
    kc = torch.zeros((B, n_groups, S_MAX, hs), dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros((B, n_groups, hs, S_MAX), dtype=torch.bfloat16, device=DEV)
    past = [U((n - 1, N), 1.0, f"vpast{i}") for i, n in enumerate(lens)]
    i32 = torch.int32
    for i, p in enumerate(past):
        ops.qkv_rope_cache(p.to(DEV), cos.to(DEV), sin.to(DEV), torch.full((p.size(0),), i, dtype=i32, device=DEV),
                           torch.arange(p.size(0), dtype=i32, device=DEV), kc, vt, n_head, n_groups)
    y = ops.attn_verify_fused(y32, N, _pad_rank(Bm, r, 1).to(DEV), s, (d, d + kv), cos.to(DEV), sin.to(DEV), torch.arange(B, dtype=i32, device=DEV),
                              torch.tensor(lens, dtype=i32, device=DEV), kc, vt, n_head, S)
    qkv_new = O.lora_qkv_linear(xn.view(B * S, 1, d), W, A, Bm, s, (d, kv, kv))[:, 0]     # (B * S, N) bf16, reference rounding
    kcp, vtp = ops.kcache_to_plain(kc).cpu(), ops.vcache_to_plain(vt).cpu()
    y = y.float().cpu()
    scale = 1 / math.sqrt(hs)
    for i, n in enumerate(lens):
        T = n - 1 + S
        full = torch.cat([past[i], qkv_new[i * S:(i + 1) * S]]).view(1, T, n_groups, qpk + 2, hs).permute(0, 2, 3, 1, 4)
        qq, kk, vv = full.split((qpk, 1, 1), dim=2)
        qq, kk, vv = qq.reshape(1, -1, T, hs), kk.reshape(1, -1, T, hs), vv.reshape(1, -1, T, hs)
        qq, kk = O.apply_rope(qq, cos[:T], sin[:T]), O.apply_rope(kk, cos[:T], sin[:T])
        assert torch.equal(kcp[i, :, :n - 1], kk[0][:, :n - 1]), f"keys {n}: k cache, past rows"
        assert torch.equal(vtp[i, :, :, :n - 1].transpose(1, 2), vv[0][:, :n - 1]), f"keys {n}: v^T cache, past rows"
        kb, vb = kk.repeat_interleave(qpk, dim=1), vv.repeat_interleave(qpk, dim=1)
        fig = dict(max_ulp=0.0, mean_ulp=0.0, max_abs_hip_vs_fp64=0.0, max_abs_oracle_vs_fp64=0.0)
        for j in range(S):
            at = n - 1 + j                          # the row's position; it attends keys [0, at]
            check_ulp(kcp[i, :, at], kk[0][:, at], 1, 0.01, f"keys {n} row {j}: k cache, appended row")
            check_ulp(vtp[i, :, :, at], vv[0][:, at], 1, 0.01, f"keys {n} row {j}: v^T cache, appended row")
            q1, k1, v1 = qq[:, :, at:at + 1], kb[:, :, :at + 1], vb[:, :, :at + 1]
            truth = F.scaled_dot_product_attention(q1.double(), k1.double(), v1.double(), scale=scale).transpose(1, 2).reshape(-1)
            want = F.scaled_dot_product_attention(q1, k1, v1, scale=scale).transpose(1, 2).reshape(-1).float()
            got = y[i * S + j]
            err, err_ref = (got.double() - truth).abs().max().item(), (want.double() - truth).abs().max().item()
            u = ulp_diff(got, want, 1.0)
            print(f"hs {hs} keys {n} row {j}: err {err:.3e} err_ref {err_ref:.3e} max {u.max().item():.2f} ulp mean {u.mean().item():.3f} ulp")
            fig = dict(max_ulp=max(fig["max_ulp"], u.max().item()), mean_ulp=max(fig["mean_ulp"], u.mean().item()),
                       max_abs_hip_vs_fp64=max(fig["max_abs_hip_vs_fp64"], err), max_abs_oracle_vs_fp64=max(fig["max_abs_oracle_vs_fp64"], err_ref))
            assert err <= max(2 * err_ref, 2e-2), f"keys {n} row {j}: err {err} vs reference-kernel err {err_ref}"
            assert u.max().item() <= 3.0 and u.mean().item() <= 0.5, \
                f"keys {n} row {j}: max {u.max().item()} / mean {u.mean().item():.2f} ulp vs the oracle's bf16 SDPA"
        record_parity(f"attention.verify_vs_oracle_bf16.hs{hs}.keys{n}", **fig)


# ---- c. refusals -------------------------------------------------------------------------------------------------------------------
def _raw(buf, *, n_part=2, n_seq=3, S=2, n_head=8, n_groups=2, hs=64, n_ext=48, lora=True, p_max=S_MAX, qkv_dim=None):
    """dh_attn_verify_fused_bf16 itself on buffers large enough for every argument set below -> (rc, message)"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    qkv_dim = (n_head + 2 * n_groups) * hs if qkv_dim is None else qkv_dim
    rc = lib.dh_attn_verify_fused_bf16(buf["q32"].data_ptr(), n_part, 1, n_seq, S, qkv_dim, n_ext, buf["bq"].data_ptr() if lora else None, 2.0,
                                       n_head * hs, (n_head + n_groups) * hs, buf["cos"].data_ptr(), buf["sin"].data_ptr(), buf["slot"].data_ptr(),
                                       buf["kv_len"].data_ptr(), buf["kc"].data_ptr(), buf["vt"].data_ptr(), buf["y"].data_ptr(), n_head, n_groups,
                                       hs, S_MAX, p_max, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lib.dh_last_error().decode(errors="replace")


REFUSED = (
    (dict(S=1), "S = 1"),
    (dict(S=9), "S = 9"),
    (dict(S=6, n_head=12), "query columns"),                    # 6 positions x 6 heads per group = 36
    (dict(hs=80), "head_size 80"),
    (dict(p_max=S_MAX + 64), "p_max"),
    (dict(p_max=0), "p_max"),
    (dict(n_part=17), "n_part"),
    (dict(n_ext=16), "48"),
    (dict(qkv_dim=(8 + 2 * 2) * 64 + 64), "qkv_dim"),
)


def test_refusals_launch_nothing():
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    rows, width = 3 * 9, (12 + 4) * 128 + 64 + 48               # the most rows and the widest row any argument set names
    buf = dict(q32=torch.randn(17, rows, width, device=DEV, generator=g) * 0.3, bq=r(width, 16), cos=r(S_MAX + 64, 128), sin=r(S_MAX + 64, 128),
               slot=torch.arange(3, dtype=torch.int32, device=DEV).flip(0).contiguous(), kv_len=torch.tensor([5, 33, 64], dtype=torch.int32, device=DEV),
               kc=r(3, 2, S_MAX + 64, 128), vt=r(3, 2, 128, S_MAX + 64), y=r(rows, 12 * 128))
    before = {k: buf[k].clone() for k in ("y", "kc", "vt")}
    untouched = lambda: all(torch.equal(buf[k], before[k]) for k in before)
    for kw, word in REFUSED:
        rc, msg = _raw(buf, **kw)
        assert rc != 0, f"{kw}: accepted"
        assert "attn_verify_fused" in msg and word in msg, f"{kw}: refused with {msg!r}"
        assert untouched(), f"{kw}: refused, and the output or the caches changed"
    rc, msg = _raw(buf, n_seq=0)
    assert rc == 0 and untouched()
    # the same arguments unchanged are served
    rc, msg = _raw(buf)
    assert rc == 0, msg
    n_out = 3 * 2 * 8 * 64                                      # y [n_seq * S, n_head * hs] at the head of the buffer
    assert (buf["y"].flatten()[:n_out] != before["y"].flatten()[:n_out]).float().mean().item() > 0.9
    assert torch.isfinite(buf["y"].float()).all() and torch.equal(buf["y"].flatten()[n_out:], before["y"].flatten()[n_out:])


def test_op_wrapper_defaults():
    """ops.attn_verify_fused: p_max defaults to s_max, p_max = 0 is handed on (and refused), rows must be S per sequence."""
    from dualhyp_amd import ops, _lib
    I = _inputs(64, 8, 2, 2, 2, [575, S_MAX], 2, seed=3)
    splits = (8 * 64, 10 * 64)
    args = lambda kc, vt: (I["q32"], I["qkv_dim"], I["bq"], 2.0, splits, I["cos"], I["sin"], I["slot"], I["kv_len"], kc, vt, 8, 2)
    a = ops.attn_verify_fused(*args(I["kc"].clone(), I["vt"].clone()))
    b = ops.attn_verify_fused(*args(I["kc"].clone(), I["vt"].clone()), p_max=S_MAX)
    assert a.shape == (4, 8 * 64) and a.dtype == torch.bfloat16 and torch.equal(a, b)
    with pytest.raises(_lib.DualHypHipError, match="p_max"):
        ops.attn_verify_fused(*args(I["kc"].clone(), I["vt"].clone()), p_max=0)
    with pytest.raises(ValueError):
        ops.attn_verify_fused(I["q32"][:, :3].contiguous(), *args(I["kc"].clone(), I["vt"].clone())[1:])
