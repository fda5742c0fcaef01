"""The table variant of attn_shared_fused_kernel (csrc/decode_fused.hip) as an op, against its definition (include/dualhyp_hip.h,
"Beam KV tile table"): ops.attn_decode_shared(..., tile_tab=) over caches in which a hypothesis' closed tiles lie SCATTERED over its
siblings' slots gives the BITS of ops.attn_decode_fused over a reference cache that has every row's lineage in its own slot.

Both caches are random bf16 per (slot, tile).  In the scattered one every (slot, tile) that no table entry references and every whole
prompt tile outside slot u * W is NaN: the definition says they are never loaded.  The rows of an utterance are in lockstep at step t
(new key at position P + t - 1); the closed tiles get random owners, the open tile the row itself."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_MAX, NT = 192, 4
GEOMS = ((64, 8, 1), (64, 4, 2), (96, 4, 4), (128, 8, 2))       # tests/test_hip_shared_attn.py's head layouts
PROMPTS = (31, 32, 70)                                           # n_sh = 0, 1, 2; tile0 partial, aligned, partial
STEPS = (1, 2, 33, 34, 66)                                       # generated counts: one, two and three private tiles
PARTS = ((8, True, True), (1, True, False))                      # (n_part, pairs, lora)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(hs, n_head, n_groups, W, n_part, t, seed, identity=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cg = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    n_utt, qkv_dim = len(PROMPTS), (n_head + 2 * n_groups) * hs
    rows = n_utt * W
    pos = [PROMPTS[u] + t - 1 for u in range(n_utt) for _ in range(W)]
    kv_len = torch.tensor([p + 1 for p in pos], dtype=torch.int32, device=DEV)
    slot = torch.arange(rows, dtype=torch.int32, device=DEV).flip(0).contiguous()
    sl = slot.tolist()
    kc, vt = r(rows, n_groups, S_MAX, hs), r(rows, n_groups, hs, S_MAX)          # scattered: random per (slot, tile)
    ref_k, ref_v = r(rows, n_groups, S_MAX, hs), r(rows, n_groups, hs, S_MAX)    # reference: filled in below
    tiles = lambda c: c.view(rows, n_groups, S_MAX // 32, hs * 32)               # 32-key tiles back to back in either cache
    tab = torch.arange(W, dtype=torch.int32).view(1, W, 1).expand(n_utt, W, NT).contiguous()
    used = torch.zeros((rows, S_MAX // 32), dtype=torch.bool)                    # by slot: a tile some row reads or writes
    sibling_reads = 0
    for u, P in enumerate(PROMPTS):
        tile0, cur = P >> 5, ((P + t - 1) >> 5) - (P >> 5)
        for w in range(W):
            row = u * W + w
            for tl in range(tile0):                                              # whole prompt tiles: read from slot u * W
                for src, dst in ((kc, ref_k), (vt, ref_v)):
                    tiles(dst)[sl[row], :, tl] = tiles(src)[sl[u * W], :, tl]
                used[sl[u * W], tl] = True
            for j in range(cur + 1):
                own = j == cur or identity
                b = w if own else int(torch.randint(W, (1,), generator=cg))
                tab[u, w, j] = b
                sibling_reads += b != w
                used[sl[u * W + b], tile0 + j] = True
                for src, dst in ((kc, ref_k), (vt, ref_v)):
                    tiles(dst)[sl[row], :, tile0 + j] = tiles(src)[sl[u * W + b], :, tile0 + j]
    dead = (~used).to(DEV)[:, None, :, None].expand(rows, n_groups, S_MAX // 32, hs * 32)
    tiles(kc)[dead] = float("nan")
    tiles(vt)[dead] = float("nan")
    planes = torch.stack([tab.view(rows, NT), tab.view(rows, NT)]).contiguous().to(DEV)
    return dict(hs=hs, n_head=n_head, n_groups=n_groups, W=W, qkv_dim=qkv_dim, rows=rows, pos=pos, kv_len=kv_len, slot=slot, kc=kc, vt=vt,
                ref_k=ref_k, ref_v=ref_v, planes=planes, sibling_reads=int(sibling_reads), dead=int((~used).sum()),
                plen=torch.tensor(PROMPTS, dtype=torch.int32, device=DEV), cos=r(S_MAX, hs), sin=r(S_MAX, hs),
                q32=torch.randn(n_part, rows, qkv_dim + 48, device=DEV, generator=g) * 0.3,
                bq=(torch.randn(qkv_dim, 16, device=DEV, generator=g) * 0.05).bfloat16())


def _args(I, lora, kc, vt):
    q32, bq = (I["q32"], I["bq"]) if lora else (I["q32"][..., :I["qkv_dim"]].contiguous(), None)
    splits = (I["n_head"] * I["hs"], (I["n_head"] + I["n_groups"]) * I["hs"])
    return (q32, I["qkv_dim"], bq, 2.0, splits, I["cos"], I["sin"], I["slot"], I["kv_len"], kc, vt, I["n_head"])


def _check(tag, I, lora, pairs, planes=None, step_dev=None):
    from dualhyp_amd import ops
    kc, vt, rk, rv = I["kc"].clone(), I["vt"].clone(), I["ref_k"].clone(), I["ref_v"].clone()
    want = ops.attn_decode_fused(*_args(I, lora, rk, rv), pairs=pairs)
    got = ops.attn_decode_shared(*_args(I, lora, kc, vt), I["W"], I["plen"], pairs=pairs,
                                 tile_tab=I["planes"] if planes is None else planes, step_dev=step_dev)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all(), f"{tag}: the reference rows are not finite"
    bad = (got != want).any(1).nonzero().flatten().tolist()
    assert not bad, (f"{tag}: rows {bad[:8]} of {I['rows']} differ from the reference cache's; first {got[bad[0]][:4].tolist()} for "
                     f"{want[bad[0]][:4].tolist()}")
    assert torch.equal(got, want)
    # the append: the row's own position of its own slot holds the reference call's key and value, every other byte is unchanged
    sl = I["slot"].tolist()
    for name, to_plain, after, before, ref, key_dim in (("K", ops.kcache_to_plain, kc, I["kc"], rk, 2), ("V^T", ops.vcache_to_plain, vt, I["vt"], rv, 3)):
        a, b, f = _bits(to_plain(after)), _bits(to_plain(before)), _bits(to_plain(ref))
        own = torch.zeros_like(a, dtype=torch.bool)
        for row, p in enumerate(I["pos"]):
            idx = (sl[row], slice(None), p) if key_dim == 2 else (sl[row], slice(None), slice(None), p)
            assert torch.equal(a[idx], f[idx]), f"{tag}: the appended {name} of row {row} at position {p} is not the reference call's"
            own[idx] = True
        assert torch.equal(a[~own], b[~own]), f"{tag}: the {name} cache changed outside the rows' own positions"


@pytest.mark.parametrize("geom,W", [(g, w) for g in GEOMS for w in (2, 3, 4)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"W{v}")
def test_scattered_tiles_give_the_bits_of_the_materialised_cache(geom, W):
    hs, n_head, n_groups = geom
    reads = dead = 0
    for t in STEPS:
        for n_part, pairs, lora in PARTS:
            I = _inputs(hs, n_head, n_groups, W, n_part, t, seed=17 + hs + 5 * n_part + 3 * W + t)
            _check(f"hs {hs} heads {n_head} groups {n_groups} W {W} step {t} n_part {n_part} lora {lora}", I, lora, pairs)
            reads += I["sibling_reads"]
            dead += I["dead"]
    assert reads > 0, "no closed tile was read from a sibling's slot"
    assert dead > 0, "no (slot, tile) was poisoned"


def test_the_plane_is_chosen_by_the_device_step_counter():
    """plane (t - 1) & 1 of the device counter t; the other plane names rows whose tiles are NaN where it differs, or is out of range
    and must be clamped without being read"""
    I = _inputs(64, 8, 1, 3, 8, 34, seed=5)
    junk = torch.full_like(I["planes"][0], 7)
    for t_dev in (2, 3, 34, 35):
        planes = torch.stack([junk, junk]).contiguous()
        planes[(t_dev - 1) & 1] = I["planes"][0]
        _check(f"device step {t_dev}", I, True, True, planes=planes, step_dev=torch.tensor([t_dev], dtype=torch.int32, device=DEV))
    # no counter: plane 0
    _check("no step counter", I, True, True, planes=torch.stack([I["planes"][0], junk]).contiguous())


def test_out_of_range_entries_are_clamped():
    """entries below 0 and above W - 1 read beams 0 and W - 1: nothing is trusted to index"""
    I = _inputs(64, 4, 2, 3, 8, 66, seed=9, identity=True)
    lo, hi = I["planes"].clone(), I["planes"].clone()
    lo[:, 0::3, :2] = -5                   # beam 0's closed tiles: clamped to 0, itself
    hi[:, 2::3, :2] = 1 << 20              # beam W - 1's: clamped to W - 1, itself
    for planes in (lo, hi):
        _check("clamped", I, True, True, planes=planes)


@pytest.mark.parametrize("hs,n_head,n_groups", GEOMS)
def test_identity_table_gives_the_bits_of_the_call_without_a_table(hs, n_head, n_groups):
    from dualhyp_amd import ops
    for W in (2, 4):
        for t in (2, 66):
            I = _inputs(hs, n_head, n_groups, W, 8, t, seed=3 + hs + W + t, identity=True)
            k0, v0, k1, v1 = I["ref_k"].clone(), I["ref_v"].clone(), I["ref_k"].clone(), I["ref_v"].clone()
            y0 = ops.attn_decode_shared(*_args(I, True, k0, v0), W, I["plen"])
            y1 = ops.attn_decode_shared(*_args(I, True, k1, v1), W, I["plen"], tile_tab=I["planes"])
            torch.cuda.synchronize()
            assert torch.isfinite(y0.float()).all() and torch.equal(y0, y1) and torch.equal(k0, k1) and torch.equal(v0, v1)


def test_case_table():
    assert [p >> 5 for p in PROMPTS] == [0, 1, 2] and [p & 31 for p in PROMPTS] == [31, 0, 6]
    priv = {((P + t - 1) >> 5) - (P >> 5) + 1 for P in PROMPTS for t in STEPS}
    assert priv >= {1, 2, 3}, "one, two and three private tiles"
    assert {P + t - 1 for P in PROMPTS for t in STEPS} >= {32, 64}, "positions at which the open tile holds no visible key"
    assert max(PROMPTS) + max(STEPS) <= S_MAX and all(((P + t - 1) >> 5) - (P >> 5) < NT for P in PROMPTS for t in STEPS)


def test_refusals_and_wrapper_checks():
    from dualhyp_amd import _lib, ops
    I = _inputs(64, 8, 2, 2, 2, 2, seed=3)
    args = _args(I, True, I["ref_k"].clone(), I["ref_v"].clone())
    for bad in (I["planes"][0], I["planes"].long(), I["planes"][:, :-1].contiguous(), I["planes"].cpu(), I["planes"].transpose(1, 2)):
        with pytest.raises(ValueError, match="tile_tab"):
            ops.attn_decode_shared(*args, 2, I["plen"], tile_tab=bad)
    with pytest.raises(ValueError, match="step_dev"):
        ops.attn_decode_shared(*args, 2, I["plen"], step_dev=torch.zeros(1, dtype=torch.int32, device=DEV))
    wide = torch.zeros((2, I["rows"], 65), dtype=torch.int32, device=DEV)
    count = _lib.load().dh_attn_shared_launch_count
    c0 = count()
    with pytest.raises(_lib.DualHypHipError, match="dh_attn_decode_shared_tab_bf16.*65"):
        ops.attn_decode_shared(*args, 2, I["plen"], tile_tab=wide)
    assert count() == c0
