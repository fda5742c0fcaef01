"""The forward attention kernels pinned to exact key selection and key counts (inputs and fp64 reference: attn_exact_reference.py).

On those inputs the softmax is one-hot (or exactly uniform), every sum is exact in fp32 in any order, and the expected bits follow
from arithmetic: y must be the winner's V row (or sum / n) under torch.equal, whatever the tile size, the split count, the
tile -> wave deal or the exp accuracy.  What each part runs:

  a  ops.attn_prefill           attn_prefill_kernel<HS, PS, WPB> (csrc/attention.hip), y and lse: a packed call of lengths 1 .. 200 and a
                                call of continuations behind kv_pos0 in {1 .. 100}; dh_set_tuning 42 at its default and at 0
  b  ops.attn_decode            attn_decode_kernel + attn_decode_combine_kernel (split-KV: 32-key tiles dealt over 16 waves)
  c  ops.attn_decode_fused      attn_decode_chain_kernel (hs 64, dh_set_tuning 40 = 1, up to 13 heads per group) and
                                attn_decode_fused_kernel (key 40 = 0, 16 heads per group, hs 96 / 128): 32-key tiles of the kv_len - 1
                                cached keys dealt over 8 waves, the new token appended and merged at the combine
  d  the three ops              bit-for-bit invariance on random data: chunked against whole prefill, batch composition, slot, order
  e  attn_prefill, attn_decode  peaked and moving-max softmaxes against fp64, gated like the long case of test_hip_ops.py

Lengths where the tile -> wave deal changes: 32 keys (one tile), 64 (one prefill stage), 256 (one tile for each of the fused
kernels' 8 waves), 512 (one for each of the split-KV kernel's 16); the cases sit on and around each.

ops.attn_decode_kv8 and ops.attn_verify_fused are pinned bit for bit to the kernels tested here (test_hip_kv8.py,
test_hip_verify_attn.py).  The kernels' contract for cache contents behind kv_len (stale rows, free slots) is that they are FINITE, so
a masked key's 0 * v stays 0; NaN or Inf there is outside the contract and is not tested."""
import functools
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import attn_exact_reference as R  # noqa: E402
from conftest import record_parity, ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32


def _tuning(key, value):
    from dualhyp_amd import _lib
    _lib.check(_lib.load().dh_set_tuning(key, value))


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    _tuning(40, 1)
    _tuning(42, 4)


def _d(t):
    return t.to(DEV)


def _world_caches(c):
    """The case's world (real cached keys, decoys, stale rows) written through the cache-append op."""
    from dualhyp_amd import ops
    kc = torch.zeros(c.n_slots, c.n_groups, c.s_max, c.hs, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(c.n_slots, c.n_groups, c.hs, c.s_max, dtype=torch.bfloat16, device=DEV)
    cos, sin = (_d(t) for t in c.cos_sin())
    qkv, slot, pos = c.fill_rows()
    ops.qkv_rope_cache(_d(qkv), cos, sin, _d(slot), _d(pos), kc, vt, c.n_head, c.n_groups)
    return kc, vt, cos, sin


def _check_caches(c, kc, vt, before=None):
    """The caches hold the world with the call's rows appended, and nothing else changed."""
    from dualhyp_amd import ops
    K, V = c.final_cache()
    kp, vp = ops.kcache_to_plain(kc).cpu().double(), ops.vcache_to_plain(vt).cpu().double().transpose(2, 3)
    for name, got, want in (("K", kp, K), ("V", vp, V)):
        if not torch.equal(got, want):
            s, g, j = (got != want).any(dim=3).nonzero()[0].tolist()
            raise AssertionError(f"{c.name}: {name} cache differs at slot {s} group {g} key {j} (first of {(got != want).any(dim=3).sum().item()} rows)")
    if before is not None:
        keep = torch.ones(c.n_slots, c.s_max, dtype=torch.bool)
        for slot, cached, new, _ in c.seqs:
            keep[slot, cached:cached + new] = False
        k0, v0 = ops.kcache_to_plain(before[0]).cpu(), ops.vcache_to_plain(before[1]).cpu().transpose(2, 3)
        kb, vb = ops.kcache_to_plain(kc).cpu(), ops.vcache_to_plain(vt).cpu().transpose(2, 3)
        m = keep[:, None, :, None]
        assert torch.equal(kb * m, k0 * m) and torch.equal(vb * m, v0 * m), f"{c.name}: the append wrote outside the new rows"


def _assert_passes(c, y, lse=None):
    msgs = c.compare(y, lse)
    assert not msgs, "\n".join(msgs)


@functools.lru_cache(maxsize=None)
def _case(kind, hs, n_head, n_groups):
    c = getattr(R, kind)(hs, n_head, n_groups)
    record_parity(f"attention.exact.tie_share.{kind}.hs{hs}.h{n_head}g{n_groups}", tie_share=c.expected()["tie_share"], n_queries=c.n_q)
    return c


# ------------------------------------------------------------------------------------------------ a. prefill
PREFILL_ARMS = [(l, 4) for l in R.PREFILL_LAYOUTS] + [(R.PREFILL_LAYOUTS[0], 0)]
_lid = lambda l: f"hs{l[0]}-{l[1]}h{l[2]}g"


@pytest.mark.parametrize("kind", ("prefill_packed_case", "prefill_continuation_case"), ids=("packed", "continuation"))
@pytest.mark.parametrize("layout,wpb", PREFILL_ARMS, ids=[f"{_lid(l)}-key42={w}" for l, w in PREFILL_ARMS])
def test_prefill_selects_and_counts_exactly(layout, wpb, kind):
    from dualhyp_amd import ops
    c = _case(kind, *layout)
    kc, vt, cos, sin = _world_caches(c)
    before = (kc.clone(), vt.clone())
    qkv, tslot, tpos, sslot, qs, ql, p0 = c.token_rows()
    q = ops.qkv_rope_cache(_d(qkv), cos, sin, _d(tslot), _d(tpos), kc, vt, c.n_head, c.n_groups)
    assert torch.equal(q.cpu(), c.queries()), "identity rope changed q"
    _check_caches(c, kc, vt, before)
    _tuning(42, wpb)
    lse = torch.full((c.n_q, c.n_head), float("nan"), device=DEV)
    y = ops.attn_prefill(q, kc, vt, _d(sslot), _d(qs), _d(ql), _d(p0), int(ql.max()), lse=lse)
    torch.cuda.synchronize()
    _assert_passes(c, y, lse)


# ------------------------------------------------------------------------------------------------ b. decode
@pytest.mark.parametrize("layout", R.DECODE_LAYOUTS, ids=_lid)
def test_decode_selects_and_counts_exactly(layout):
    from dualhyp_amd import ops
    c = _case("decode_case", *layout)
    kc, vt, _, _ = _world_caches(c)
    y = ops.attn_decode(_d(c.queries()), kc, vt, _d(c.seq_slot()), _d(c.kv_len()))
    torch.cuda.synchronize()
    _assert_passes(c, y)


# ------------------------------------------------------------------------------------------------ c. the fused single-token step
FUSED_ARMS = [(l, a) for l in R.DECODE_LAYOUTS for a in ((0, 1) if l[0] == 64 else (1,))]


@pytest.mark.parametrize("layout,chain", FUSED_ARMS, ids=[f"{_lid(l)}-key40={a}" for l, a in FUSED_ARMS])
def test_fused_step_selects_counts_and_appends_exactly(layout, chain):
    from dualhyp_amd import ops
    c = _case("fused_case", *layout)
    hs, n_head, n_groups = layout
    kc, vt, cos, sin = _world_caches(c)
    before = (kc.clone(), vt.clone())
    qkv32 = _d(c.token_rows()[0].float()).unsqueeze(0).contiguous()          # n_part = 1: the new token's exact integer q, k, v
    _tuning(40, chain)
    y = ops.attn_decode_fused(qkv32, c.width, None, 1.0, (n_head * hs, (n_head + n_groups) * hs), cos, sin, _d(c.seq_slot()), _d(c.kv_len()),
                              kc, vt, n_head)
    torch.cuda.synchronize()
    _assert_passes(c, y)
    _check_caches(c, kc, vt, before)


# ------------------------------------------------------------------------------------------------ d. invariance on random data
def _random_setup(hs, n_head, n_groups, n_slots, s_max, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=gen).bfloat16()
    return dict(kc=rn(n_slots, n_groups, s_max, hs), vt=rn(n_slots, n_groups, hs, s_max), cos=rn(s_max, hs), sin=rn(s_max, hs), rn=rn)


def _i32(v):
    return torch.tensor(v, dtype=I32, device=DEV)


def _first_diff(a, b):
    rows = (a != b).reshape(a.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
    return f"{len(rows)} rows differ, first {rows[:8]}"


INV_LAYOUTS = ((64, 8, 2), (128, 8, 2), (96, 4, 4))


@pytest.mark.parametrize("hs,n_head,n_groups", INV_LAYOUTS)
def test_chunked_prefill_equals_whole_prefill_bit_for_bit(hs, n_head, n_groups):
    """Statistics are per lane (per query), tiles are walked from key 0 either way, and a tile that is fully masked for a lane adds
    p = 0 with alpha = 1: y and lse of a chunk must not depend on where the chunk starts."""
    from dualhyp_amd import ops
    n, s_max, cuts = 200, 256, (0, 1, 32, 33, 64, 97, 130, 200)
    S = _random_setup(hs, n_head, n_groups, 1, s_max, seed=21)
    qkv = S["rn"](n, (n_head + 2 * n_groups) * hs)
    kc, vt = S["kc"].clone(), S["vt"].clone()
    q = ops.qkv_rope_cache(qkv, S["cos"], S["sin"], _i32([0] * n), _i32(list(range(n))), kc, vt, n_head, n_groups)
    lse = torch.full((n, n_head), float("nan"), device=DEV)
    y = ops.attn_prefill(q, kc, vt, _i32([0]), _i32([0]), _i32([n]), _i32([0]), n, lse=lse)
    kc2, vt2 = S["kc"].clone(), S["vt"].clone()
    for a, b in zip(cuts[:-1], cuts[1:]):
        qc = ops.qkv_rope_cache(qkv[a:b].contiguous(), S["cos"], S["sin"], _i32([0] * (b - a)), _i32(list(range(a, b))), kc2, vt2, n_head, n_groups)
        assert torch.equal(qc, q[a:b])
        lc = torch.full((b - a, n_head), float("nan"), device=DEV)
        yc = ops.attn_prefill(qc, kc2, vt2, _i32([0]), _i32([0]), _i32([b - a]), _i32([a]), b - a, lse=lc)
        assert torch.isfinite(yc.float()).all() and torch.isfinite(lc).all()
        assert torch.equal(yc, y[a:b]), f"chunk [{a}, {b}): y differs from the whole prefill: {_first_diff(yc, y[a:b])} (rows count from {a})"
        assert torch.equal(lc, lse[a:b]), f"chunk [{a}, {b}): lse differs from the whole prefill: {_first_diff(lc, lse[a:b])}"
    assert torch.equal(kc, kc2) and torch.equal(vt, vt2)


@pytest.mark.parametrize("hs,n_head,n_groups", INV_LAYOUTS)
def test_prefill_rows_do_not_depend_on_the_batch(hs, n_head, n_groups):
    """A sequence's rows equal those of a call holding it alone, on another slot, and of a call with another order of q_start."""
    from dualhyp_amd import ops
    lens, pos0, slots, s_max = (70, 200, 33), (0, 17, 64), (2, 0, 1), 320
    S = _random_setup(hs, n_head, n_groups, 4, s_max, seed=22)
    kc, vt = S["kc"].clone(), S["vt"].clone()
    qs, ys, ls = [], [], []
    tok_slot = [s for s, n in zip(slots, lens) for _ in range(n)]
    tok_pos = [p for p0, n in zip(pos0, lens) for p in range(p0, p0 + n)]
    q = ops.qkv_rope_cache(S["rn"](sum(lens), (n_head + 2 * n_groups) * hs), S["cos"], S["sin"], _i32(tok_slot), _i32(tok_pos), kc, vt, n_head, n_groups)
    starts = [0, lens[0], lens[0] + lens[1]]
    lse = torch.full((sum(lens), n_head), float("nan"), device=DEV)
    y = ops.attn_prefill(q, kc, vt, _i32(slots), _i32(starts), _i32(lens), _i32(pos0), max(lens), lse=lse)
    assert torch.isfinite(y.float()).all() and torch.isfinite(lse).all()
    for i, n in enumerate(lens):
        kc1, vt1 = S["kc"].clone(), S["vt"].clone()
        kc1[3], vt1[3] = kc[slots[i]], vt[slots[i]]                         # a (slot, group) block is self-contained in fragment order
        qi = q[starts[i]:starts[i] + n].contiguous()
        l1 = torch.full((n, n_head), float("nan"), device=DEV)
        y1 = ops.attn_prefill(qi, kc1, vt1, _i32([3]), _i32([0]), _i32([n]), _i32([pos0[i]]), n, lse=l1)
        assert torch.equal(y1, y[starts[i]:starts[i] + n]), f"seq {i} alone on slot 3: y differs: {_first_diff(y1, y[starts[i]:starts[i] + n])}"
        assert torch.equal(l1, lse[starts[i]:starts[i] + n]), f"seq {i} alone on slot 3: lse differs"
    # the same three sequences packed in another order
    order = (2, 0, 1)
    q2 = torch.cat([q[starts[i]:starts[i] + lens[i]] for i in order])
    st2 = [0, lens[order[0]], lens[order[0]] + lens[order[1]]]
    l2 = torch.full((sum(lens), n_head), float("nan"), device=DEV)
    y2 = ops.attn_prefill(q2, kc, vt, _i32([slots[i] for i in order]), _i32(st2), _i32([lens[i] for i in order]), _i32([pos0[i] for i in order]),
                          max(lens), lse=l2)
    for j, i in enumerate(order):
        assert torch.equal(y2[st2[j]:st2[j] + lens[i]], y[starts[i]:starts[i] + lens[i]]), f"seq {i} at place {j} of the reordered call: y differs"
        assert torch.equal(l2[st2[j]:st2[j] + lens[i]], lse[starts[i]:starts[i] + lens[i]]), f"seq {i} at place {j} of the reordered call: lse differs"


@pytest.mark.parametrize("hs,n_head,n_groups", INV_LAYOUTS)
def test_decode_rows_do_not_depend_on_the_batch(hs, n_head, n_groups):
    """A row's bits depend neither on n_seq, nor on its slot, nor on its neighbours' kv_len: split-KV op and fused step."""
    from dualhyp_amd import ops
    kv, slots, s_max = (545, 33, 64, 1, 200), (4, 3, 2, 1, 0), 576
    S = _random_setup(hs, n_head, n_groups, 6, s_max, seed=23)
    width = (n_head + 2 * n_groups) * hs
    q = S["rn"](len(kv), n_head, hs)
    y = ops.attn_decode(q, S["kc"], S["vt"], _i32(slots), _i32(kv))
    qkv32 = torch.randn(2, len(kv), width, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 0.5
    splits = (n_head * hs, (n_head + n_groups) * hs)
    kcf, vtf = S["kc"].clone(), S["vt"].clone()
    yf = ops.attn_decode_fused(qkv32, width, None, 1.0, splits, S["cos"], S["sin"], _i32(slots), _i32(kv), kcf, vtf, n_head)
    assert torch.isfinite(y.float()).all() and torch.isfinite(yf.float()).all()
    for i in range(len(kv)):
        kc1, vt1 = S["kc"].clone(), S["vt"].clone()
        kc1[5], vt1[5] = S["kc"][slots[i]], S["vt"][slots[i]]
        y1 = ops.attn_decode(q[i:i + 1].contiguous(), kc1, vt1, _i32([5]), _i32([kv[i]]))
        assert torch.equal(y1[0], y[i]), f"attn_decode: row {i} (kv_len {kv[i]}) alone on slot 5 differs from the row in the batch of {len(kv)}"
        yf1 = ops.attn_decode_fused(qkv32[:, i:i + 1].contiguous(), width, None, 1.0, splits, S["cos"], S["sin"], _i32([5]), _i32([kv[i]]), kc1, vt1, n_head)
        assert torch.equal(yf1[0], yf[i]), f"attn_decode_fused: row {i} (kv_len {kv[i]}) alone on slot 5 differs from the row in the batch of {len(kv)}"
        assert torch.equal(kc1[5], kcf[slots[i]]) and torch.equal(vt1[5], vtf[slots[i]]), f"attn_decode_fused: row {i}: the appended cache rows differ"
    # other neighbours: the same rows in reverse order with two of them replaced
    rev = list(range(len(kv)))[::-1]
    y2 = ops.attn_decode(q[rev].contiguous(), S["kc"], S["vt"], _i32([slots[i] for i in rev]), _i32([kv[i] for i in rev]))
    assert torch.equal(y2, y[rev]), f"attn_decode: rows differ in the reversed batch: {_first_diff(y2, y[rev])}"


# ------------------------------------------------------------------------------------------------ e. peaked and moving-max regimes
REGIMES = ("q0.05", "q1", "q8", "ramp_up", "ramp_down")


def _regime_rows(regime, hs, n_head, n_groups, L, gen):
    """Interleaved qkv rows [L, width] bf16 (CPU).  q<s>: randn q, k, v with q scaled by s.  ramp_up / ramp_down: the recency digits
    (k[0] = j // 16, k[1] = j % 16 against q = +-(16 g, g), g * scale ~ 0.05: neighbouring keys 0.05 apart in score) over small random
    q elsewhere: rising, the running max moves at every tile (alpha < 1, the rescale always runs); falling, it never moves after the
    first tile (alpha == 1, the ballot skips the rescale)."""
    qpk = n_head // n_groups
    r = torch.randn(L, n_groups, qpk + 2, hs, generator=gen)
    if regime.startswith("q"):
        r[:, :, :qpk] *= float(regime[1:])
    else:
        g = 0.05 * math.sqrt(hs) * (1 if regime == "ramp_up" else -1)
        r[:, :, :qpk] *= 0.02
        r[:, :, :qpk, 0], r[:, :, :qpk, 1] = 16 * g, g
        j = torch.arange(L, dtype=torch.float32)[:, None]
        r[:, :, qpk, 0], r[:, :, qpk, 1] = (j // 16).expand(L, n_groups), (j % 16).expand(L, n_groups)
    return r.reshape(L, -1).bfloat16()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("L", (130, 545))
@pytest.mark.parametrize("hs,n_head,n_groups", ((64, 8, 2), (128, 8, 2)))
@pytest.mark.parametrize("kernel", ("prefill", "decode"))
def test_peaked_and_moving_max_regimes_against_fp64(kernel, hs, n_head, n_groups, L, regime):
    """Truth: fp64 attention on the bf16 operands.  Yardstick: torch's CPU bf16 SDPA on the same operands.  Gate: the project's own
    (long case of test_qkv_rope_cache_and_prefill_attention): ulps against the truth, max <= 1.25 yardstick + 0.5, mean <= 1.25
    yardstick + 0.02."""
    from dualhyp_amd import ops
    qpk, s_max = n_head // n_groups, 576
    gen = torch.Generator().manual_seed(1000 * hs + L + REGIMES.index(regime))
    rows = _regime_rows(regime, hs, n_head, n_groups, L, gen)
    kc = torch.zeros(1, n_groups, s_max, hs, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(1, n_groups, hs, s_max, dtype=torch.bfloat16, device=DEV)
    cos, sin = torch.ones(s_max, hs, dtype=torch.bfloat16, device=DEV), torch.zeros(s_max, hs, dtype=torch.bfloat16, device=DEV)
    q = ops.qkv_rope_cache(_d(rows), cos, sin, _i32([0] * L), _i32(list(range(L))), kc, vt, n_head, n_groups)
    x = rows.view(L, n_groups, qpk + 2, hs)
    qc, kk, vv = x[:, :, :qpk].reshape(L, n_head, hs), x[:, :, qpk].transpose(0, 1), x[:, :, qpk + 1].transpose(0, 1)     # [L,H,hs], [G,L,hs]
    assert torch.equal(q.cpu(), qc)
    if kernel == "prefill":
        got = ops.attn_prefill(q, kc, vt, _i32([0]), _i32([0]), _i32([L]), _i32([0]), L).float().cpu()
        sel = slice(0, L)
    else:
        got = ops.attn_decode(q[L - 1:].contiguous(), kc, vt, _i32([0]), _i32([L])).float().cpu()
        sel = slice(L - 1, L)
    count = (torch.arange(L)[None, :] <= torch.arange(L)[:, None]).double()[sel]
    truth = R.attention_fp64(qc[sel], kk, vv, count, 1.0 / math.sqrt(hs))[0].reshape(got.shape).float()
    qb, kb, vb = qc.transpose(0, 1)[None], kk.repeat_interleave(qpk, dim=0)[None], vv.repeat_interleave(qpk, dim=0)[None]
    if kernel == "prefill":
        yard = torch.nn.functional.scaled_dot_product_attention(qb, kb, vb, is_causal=True, scale=1 / math.sqrt(hs))
    else:
        yard = torch.nn.functional.scaled_dot_product_attention(qb[:, :, -1:], kb, vb, scale=1 / math.sqrt(hs))
    yard = yard[0].transpose(0, 1).reshape(got.shape).float()
    u_h, u_y = ulp_diff(got, truth, 1.0), ulp_diff(yard, truth, 1.0)
    record_parity(f"attention.exact.{kernel}.hs{hs}.L{L}.{regime}", max_ulp_hip_vs_fp64=u_h.max().item(), mean_ulp_hip_vs_fp64=u_h.mean().item(),
                  max_ulp_sdpa_vs_fp64=u_y.max().item(), mean_ulp_sdpa_vs_fp64=u_y.mean().item())
    assert torch.isfinite(got).all()
    assert u_h.max().item() <= 1.25 * u_y.max().item() + 0.5 and u_h.mean().item() <= 1.25 * u_y.mean().item() + 0.02, \
        f"{kernel} hs {hs} L {L} {regime}: HIP {u_h.max().item():.2f} / {u_h.mean().item():.3f} ulp (max / mean) from fp64, " \
        f"torch's bf16 SDPA {u_y.max().item():.2f} / {u_y.mean().item():.3f}"
