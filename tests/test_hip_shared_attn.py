"""attn_shared_fused_kernel (csrc/decode_fused.hip) as an op, against its definition (include/dualhyp_hip.h, "Shared-prompt
attention"): ops.attn_decode_shared over the rows of utterances that share prompts gives the BITS of ops.attn_decode_fused over the
same rows, in y and in both caches.

The inputs are those of tests/test_hip_verify_attn.py (caches pre-filled with random bf16, so a mask mistake reads numbers and not
zeros; seq_slot a reversed permutation; random cos / sin; synthetic fp32 partials, so n_part and `pairs` are free), forked: every
row's slot holds its utterance's whole prompt tiles.  One launch holds every prompt length of PROMPTS, with generated counts drawn
from GENS and ragged inside an utterance, so rows own different numbers of private tiles.

The poison: before the shared call every child's copy of its tiles < n_sh is overwritten with NaN.  The definition says those bytes
are never loaded, so the result must not change; they are put back before the caches are compared."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_MAX = 640
# (hs, n_head, n_groups): q_per_kv 8 (Gs = 4 rows per block: the benchmark model), 2 (Gs = 16), 1 (Gs = 32), 4 (Gs = 8)
GEOMS = ((64, 8, 1), (64, 4, 2), (96, 4, 4), (128, 8, 2))
# rows per utterance; 8 where 8 * q_per_kv > 32, i.e. two column groups per (utterance, group)
CASES = [(g, n) for g in GEOMS for n in (2, 3, 4)] + [(g, 8) for g in GEOMS if 8 * (g[1] // g[2]) > 32]
PROMPTS = (1, 31, 32, 33, 64, 100, 545)         # n_sh = 0, 0, 1, 1, 2, 3, 17 (more tiles than waves)
GENS = (0, 1, 30, 31, 32, 40)                   # keys generated so far, per row
# (n_part, pairs, lora): one partial and the 8 K-slices a d = 2048 model emits, summed in pairs; LoRA B on and off with each
PARTS = ((1, True, True), (8, True, False), (8, True, True), (1, True, False))


def _gens(n_utt, N):
    """row u * N + j has generated GENS[5 r % 6] keys, r its row number: neighbours differ and 6 rows in a row take every value"""
    return [[GENS[(u * N + j) * 5 % 6] for j in range(N)] for u in range(n_utt)]


def _inputs(hs, n_head, n_groups, N, n_part, seed, prompts=PROMPTS):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    n_utt, qkv_dim = len(prompts), (n_head + 2 * n_groups) * hs
    rows = n_utt * N
    gens = _gens(n_utt, N)
    # the new token of a row sits at position prompt + generated: kv_len counts it
    kv_len = torch.tensor([prompts[u] + gens[u][j] + 1 for u in range(n_utt) for j in range(N)], dtype=torch.int32, device=DEV)
    slot = torch.arange(rows, dtype=torch.int32, device=DEV).flip(0).contiguous()
    kc, vt = r(rows, n_groups, S_MAX, hs), r(rows, n_groups, hs, S_MAX)
    # the fork: 32-key tiles lie back to back from the start of a (slot, group) block in either cache, hs * 32 elements each
    kf, vf = kc.view(rows, n_groups, -1), vt.view(rows, n_groups, -1)
    shared = torch.zeros((rows, S_MAX * hs), dtype=torch.bool, device=DEV)      # by slot: a child's copy of a whole prompt tile
    for u, p in enumerate(prompts):
        n = (p // 32) * 32 * hs
        parent = int(slot[u * N])
        for j in range(1, N):
            child = int(slot[u * N + j])
            kf[child, :, :n] = kf[parent, :, :n]
            vf[child, :, :n] = vf[parent, :, :n]
            shared[child, :n] = True
    return dict(hs=hs, n_head=n_head, n_groups=n_groups, N=N, qkv_dim=qkv_dim, rows=rows, kv_len=kv_len, slot=slot, kc=kc, vt=vt,
                shared=shared, plen=torch.tensor(prompts, dtype=torch.int32, device=DEV), cos=r(S_MAX, hs), sin=r(S_MAX, hs),
                q32=torch.randn(n_part, rows, qkv_dim + 48, device=DEV, generator=g) * 0.3,
                bq=(torch.randn(qkv_dim, 16, device=DEV, generator=g) * 0.05).bfloat16())


def _call(I, shared, lora, pairs, poison=False):
    from dualhyp_amd import ops
    q32, bq = (I["q32"], I["bq"]) if lora else (I["q32"][..., :I["qkv_dim"]].contiguous(), None)
    kc, vt = I["kc"].clone(), I["vt"].clone()
    splits = (I["n_head"] * I["hs"], (I["n_head"] + I["n_groups"]) * I["hs"])
    args = (q32, I["qkv_dim"], bq, 2.0, splits, I["cos"], I["sin"], I["slot"], I["kv_len"], kc, vt, I["n_head"])
    if not shared:
        return ops.attn_decode_fused(*args, pairs=pairs), kc, vt
    where = I["shared"][:, None, :].expand(-1, I["n_groups"], -1)
    if poison:
        kc.view(I["rows"], I["n_groups"], -1)[where] = float("nan")
        vt.view(I["rows"], I["n_groups"], -1)[where] = float("nan")
    y = ops.attn_decode_shared(*args, I["N"], I["plen"], pairs=pairs)
    if poison:      # the definition never writes there either: what comes back is what was there
        assert torch.isnan(kc.view(I["rows"], I["n_groups"], -1)[where].float()).all()
        assert torch.isnan(vt.view(I["rows"], I["n_groups"], -1)[where].float()).all()
        kc.view(I["rows"], I["n_groups"], -1)[where] = I["kc"].view(I["rows"], I["n_groups"], -1)[where]
        vt.view(I["rows"], I["n_groups"], -1)[where] = I["vt"].view(I["rows"], I["n_groups"], -1)[where]
    return y, kc, vt


def _same(tag, I, got, want):
    y, kc, vt = got
    y0, kc0, vt0 = want
    assert torch.isfinite(y0.float()).all(), f"{tag}: the unshared rows are not finite"
    bad = (y != y0).any(1).nonzero().flatten().tolist()
    if bad:
        r = bad[0]
        c = int((y[r] != y0[r]).nonzero()[0])
        N, hs = I["N"], I["hs"]
        pytest.fail(f"{tag}: {len(bad)} of {I['rows']} rows differ from the unshared call.  First: utterance {r // N} row {r % N} prompt "
                    f"{int(I['plen'][r // N])} kv_len {int(I['kv_len'][r])} head {c // hs} channel {c % hs}: {y[r, c].item()} for "
                    f"{y0[r, c].item()}.  (utterance, row, kv_len): {[(q // N, q % N, int(I['kv_len'][q])) for q in bad[:8]]}")
    for name, a, b in (("K", kc, kc0), ("V^T", vt, vt0)):
        ne = (a != b).flatten(1).any(1).nonzero().flatten().tolist()
        assert not ne, f"{tag}: the {name} cache differs from the unshared call's in slots {ne[:8]}"
    assert torch.equal(kc, kc0) and torch.equal(vt, vt0)


@pytest.mark.parametrize("geom,N", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"N{v}")
def test_shared_rows_are_the_bits_of_the_unshared_call(geom, N):
    hs, n_head, n_groups = geom
    for n_part, pairs, lora in PARTS:
        I = _inputs(hs, n_head, n_groups, N, n_part, seed=11 + hs + 7 * n_part + N)
        want = _call(I, False, lora, pairs)
        got, again = _call(I, True, lora, pairs, poison=True), _call(I, True, lora, pairs)
        torch.cuda.synchronize()
        tag = f"hs {hs} n_head {n_head} n_groups {n_groups} N {N} n_part {n_part} pairs {pairs} lora {lora}"
        _same(tag + " (children's prompt tiles poisoned)", I, got, want)
        _same(tag, I, again, want)


def test_shared_rows_against_the_parent_single_token_kernel():
    """At hs 64 the unshared call above is attn_decode_chain_kernel's; here it is attn_decode_fused_kernel's (dh_set_tuning 40)."""
    from dualhyp_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dh_set_tuning(40, 0))
    try:
        I = _inputs(64, 8, 1, 4, 8, seed=3)
        want, got = _call(I, False, True, True), _call(I, True, True, True, poison=True)
        torch.cuda.synchronize()
        _same("hs 64, key 40 = 0", I, got, want)
    finally:
        _lib.check(lib.dh_set_tuning(40, 1))


def test_many_partials_and_pair_sums():
    """The <., 16, .> instantiation (more than 8 partials) and partials that already are pair sums."""
    for n_part, pairs in ((11, True), (6, False)):
        I = _inputs(128, 8, 2, 3, n_part, seed=5 + n_part)
        want, got = _call(I, False, True, pairs), _call(I, True, True, pairs, poison=True)
        torch.cuda.synchronize()
        _same(f"n_part {n_part} pairs {pairs}", I, got, want)


def test_one_utterance_fills_no_more_than_its_blocks():
    """A launch of one utterance: n_groups x column-group blocks, at 17 shared tiles and at none."""
    for p in (545, 7):
        I = _inputs(64, 8, 1, 8, 2, seed=9 + p, prompts=(p,))
        want, got = _call(I, False, True, True), _call(I, True, True, True, poison=True)
        torch.cuda.synchronize()
        _same(f"one utterance, prompt {p}", I, got, want)


def test_case_table():
    assert len(CASES) == 13 and [c for c in CASES if c[1] == 8] == [((64, 8, 1), 8)]
    assert [p // 32 for p in PROMPTS] == [0, 0, 1, 1, 2, 3, 17]
    for N in (2, 3, 4, 8):
        gens = _gens(len(PROMPTS), N)
        assert {x for row in gens for x in row} == set(GENS)
        assert all(len(set(row)) > 1 for row in gens), "ragged inside every utterance"
        # rows of one utterance own different numbers of private tiles somewhere
        tiles = [{(p + x + 31) // 32 - p // 32 for x in row} for p, row in zip(PROMPTS, gens)]
        assert any(len(t) > 1 for t in tiles)
    assert max(PROMPTS) + max(GENS) + 1 <= S_MAX


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _raw(buf, *, n_part=2, n_seq=6, N=3, n_head=8, n_groups=2, hs=64, n_ext=48, plen=True, qkv_dim=None):
    from dualhyp_amd import _lib
    lib = _lib.load()
    qkv_dim = (n_head + 2 * n_groups) * hs if qkv_dim is None else qkv_dim
    rc = lib.dh_attn_decode_shared_bf16(buf["q32"].data_ptr(), n_part, 1, n_seq, qkv_dim, n_ext, buf["bq"].data_ptr(), 2.0, n_head * hs,
                                        (n_head + n_groups) * hs, buf["cos"].data_ptr(), buf["sin"].data_ptr(), buf["slot"].data_ptr(),
                                        buf["kv_len"].data_ptr(), buf["kc"].data_ptr(), buf["vt"].data_ptr(), buf["y"].data_ptr(), n_head,
                                        n_groups, hs, S_MAX, N, buf["plen"].data_ptr() if plen else None,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lib.dh_last_error().decode(errors="replace")


REFUSED = (
    (dict(N=1), "group_rows = 1"),
    (dict(N=9, n_seq=9), "group_rows = 9"),
    (dict(N=4), "n_seq = 6"),
    (dict(plen=False), "prompt_len"),
    (dict(hs=80), "head_size 80"),
    (dict(n_part=17), "n_part"),
    (dict(n_ext=16), "48"),
    (dict(qkv_dim=(8 + 2 * 2) * 64 + 64), "qkv_dim"),
)


def test_refusals_launch_nothing():
    from dualhyp_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    rows, width = 9, (8 + 4) * 128 + 64 + 48
    buf = dict(q32=torch.randn(17, rows, width, device=DEV, generator=g) * 0.3, bq=r(width, 16), cos=r(S_MAX, 128), sin=r(S_MAX, 128),
               slot=torch.arange(rows, dtype=torch.int32, device=DEV), kv_len=torch.tensor([5, 33, 64] * 3, dtype=torch.int32, device=DEV),
               plen=torch.tensor([4, 4, 4], dtype=torch.int32, device=DEV), kc=r(rows, 2, S_MAX, 128), vt=r(rows, 2, 128, S_MAX),
               y=r(rows, 8 * 128))
    before = {k: buf[k].clone() for k in ("y", "kc", "vt")}
    untouched = lambda: all(torch.equal(buf[k], before[k]) for k in before)
    count = _lib.load().dh_attn_shared_launch_count
    c0 = count()
    for kw, word in REFUSED:
        rc, msg = _raw(buf, **kw)
        assert rc != 0, f"{kw}: accepted"
        assert "dh_attn_decode_shared_bf16" in msg and word in msg, f"{kw}: refused with {msg!r}"
        assert untouched() and count() == c0, f"{kw}: refused, and something was launched"
    rc, msg = _raw(buf, n_seq=0)
    assert rc == 0 and untouched() and count() == c0
    rc, msg = _raw(buf)
    assert rc == 0, msg
    assert count() == c0 + 1 and not torch.equal(buf["y"], before["y"]) and torch.isfinite(buf["y"].float()).all()


def test_op_wrapper_checks_its_arguments():
    from dualhyp_amd import ops
    I = _inputs(64, 8, 2, 2, 2, seed=3, prompts=(33, 70))
    splits = (8 * 64, 10 * 64)
    args = (I["q32"], I["qkv_dim"], I["bq"], 2.0, splits, I["cos"], I["sin"], I["slot"], I["kv_len"], I["kc"].clone(), I["vt"].clone(), 8)
    y = ops.attn_decode_shared(*args, 2, I["plen"])
    assert y.shape == (4, 8 * 64) and y.dtype == torch.bfloat16
    for N, plen in ((1, I["plen"]), (3, I["plen"]), (True, I["plen"]), (2, I["plen"][:1]), (2, I["plen"].long()), (2, None)):
        with pytest.raises(ValueError):
            ops.attn_decode_shared(*args, N, plen)
