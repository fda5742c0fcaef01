"""beam_retile_kernel (csrc/beam.hip) alone, through dh_beam_retile, against the host model (tests/beam_tiles_reference.py): the table
update behind a selection and the copy of the one open tile ("Beam KV tile table" of the header).

One layer, one group, hs 64, s_max 128.  Every one of the W ** W parent maps is an utterance of a single launch, with one more
utterance that did not take the step.  Every cache tile holds the 16-bit code of its (cache, slot, tile), so a tile that moved says
where it came from and a tile that should not have moved says so too."""
import itertools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_tiles_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HS, S_MAX, NT, MAX_NEW = 64, 128, 4, 64
# (P, t): the tile stays open; it just closed ((P + t) % 32 == 0); t = 1, open and closed; P % 32 == 0; a third private tile
CASES = ((33, 5), (20, 12), (31, 1), (32, 1), (1, 1), (64, 3), (64, 32), (30, 40), (5, 27), (47, 50))


def _launch(W, P, t, seed):
    from dualhyp_amd import ops
    maps = list(itertools.product(range(W), repeat=W))
    n_utt = len(maps) + 1                                     # the last utterance did not take the step
    rows = n_utt * W
    rng = torch.Generator().manual_seed(seed)
    tile0, cur = P >> 5, ((P + t - 1) >> 5) - (P >> 5)
    # the old plane: random owners of the closed tiles, the row itself from the open tile on (the invariant)
    old = torch.arange(W, dtype=torch.int32).view(1, W, 1).expand(n_utt, W, NT).clone()
    old[:, :, :cur] = torch.randint(W, (n_utt, W, cur), generator=rng, dtype=torch.int32)
    planes = torch.full((2, rows, NT), -77, dtype=torch.int32)
    planes[(t - 1) & 1] = old.view(rows, NT)
    parent = torch.full((n_utt, MAX_NEW, W), -1, dtype=torch.int32)
    parent[:-1, t] = torch.tensor(maps, dtype=torch.int32)
    parent[-1, t] = torch.tensor([(w + 1) % W for w in range(W)], dtype=torch.int32)      # would move everything, had it taken the step
    n_steps = torch.full((n_utt,), t + 1, dtype=torch.int32)
    n_steps[-1] = max(t - 1, 1)
    plen = torch.full((n_utt,), P, dtype=torch.int32)
    code = torch.arange(rows * (S_MAX // 32), dtype=torch.int16).view(rows, 1, S_MAX // 32, 1)
    kc = code.expand(rows, 1, S_MAX // 32, 32 * HS).contiguous().view(torch.bfloat16).view(rows, 1, S_MAX, HS).to(DEV)
    vt = (code + 16384).expand(rows, 1, S_MAX // 32, 32 * HS).contiguous().view(torch.bfloat16).view(rows, 1, HS, S_MAX).to(DEV)
    k0, v0 = kc.clone(), vt.clone()
    tab = planes.to(DEV)
    ops.beam_retile(kc, vt, tab, parent.to(DEV), n_steps.to(DEV), plen.to(DEV), t)
    torch.cuda.synchronize()
    # the host model
    want = [planes[0].tolist(), planes[1].tolist()]
    copies = []
    for u in range(n_utt):
        copies += R.update(want, t, u, W, P, maps[u] if u < len(maps) else None)
    return dict(tab=tab.cpu(), want=want, copies=copies, kc=kc, vt=vt, k0=k0, v0=v0, rows=rows, maps=maps, tile0=tile0, cur=cur,
                old=planes[(t - 1) & 1])


@pytest.mark.parametrize("W", (2, 3, 4))
def test_every_parent_map_in_one_launch(W):
    moved = closed = 0
    for i, (P, t) in enumerate(CASES):
        L = _launch(W, P, t, seed=31 * W + i)
        tag = f"W {W} P {P} step {t}"
        new = L["tab"][t & 1].tolist()
        assert new == L["want"][t & 1], f"{tag}: the new plane is not the host model's"
        assert torch.equal(L["tab"][(t - 1) & 1], L["old"]), f"{tag}: the old plane changed"
        is_open = (P + t) >> 5 == (P + t - 1) >> 5
        assert all(new[r][L["cur"] + (0 if is_open else 1)] == r % W for r in range(L["rows"]) if L["cur"] + (0 if is_open else 1) < NT), \
            f"{tag}: a row's open tile is not its own"
        assert new[-W:] == L["old"][-W:].tolist(), f"{tag}: the utterance that did not take the step did not keep its rows"
        assert bool(L["copies"]) == is_open and all(tl == L["tile0"] + L["cur"] for _, _, tl in L["copies"])
        assert all(d // W == s // W == u for u, m in enumerate(L["maps"]) for d, s, _ in L["copies"] if d // W == u)
        tiles = lambda c: c.view(L["rows"], S_MAX // 32, 32 * HS).view(torch.int16)
        for name, after, before in (("K", L["kc"], L["k0"]), ("V^T", L["vt"], L["v0"])):
            exp = tiles(before).clone()
            for d, s, tl in L["copies"]:
                exp[d, tl] = tiles(before)[s, tl]
            got = tiles(after)
            ne = (got != exp).any(-1).nonzero().tolist()
            assert not ne, (f"{tag}: {name} tiles (slot, tile) {ne[:6]} hold the codes {[int(got[a, b, 0]) for a, b in ne[:6]]}, "
                            f"expected {[int(exp[a, b, 0]) for a, b in ne[:6]]}")
        moved += len(L["copies"])
        closed += not is_open
    assert moved > 0 and closed > 0


def test_case_table():
    kinds = set()
    for P, t in CASES:
        assert 1 <= t < MAX_NEW and P + t < S_MAX and ((P + t) >> 5) - (P >> 5) < NT
        kinds.add(("closed" if (P + t) % 32 == 0 else "open", "t1" if t == 1 else "", "aligned" if P % 32 == 0 else ""))
    assert {k[0] for k in kinds} == {"open", "closed"}
    assert ("closed", "t1", "") in kinds and ("open", "t1", "aligned") in kinds and ("closed", "", "aligned") in kinds
    assert R.n_tiles(MAX_NEW, S_MAX) <= NT == S_MAX // 32


def test_refusals():
    from dualhyp_amd import _lib, ops
    rows, W = 4, 2
    kc = torch.zeros((rows, 1, S_MAX, HS), dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros((rows, 1, HS, S_MAX), dtype=torch.bfloat16, device=DEV)
    tab = torch.zeros((2, rows, NT), dtype=torch.int32, device=DEV)
    parent = torch.zeros((2, MAX_NEW, W), dtype=torch.int32, device=DEV)
    n_steps, plen = torch.full((2,), 3, dtype=torch.int32, device=DEV), torch.full((2,), 9, dtype=torch.int32, device=DEV)
    for step, word in ((0, "step 0"), (MAX_NEW, f"step {MAX_NEW}")):
        with pytest.raises(_lib.DualHypHipError, match="dh_beam_retile: " + word):
            ops.beam_retile(kc, vt, tab, parent, n_steps, plen, step)
    with pytest.raises(_lib.DualHypHipError, match="dh_beam_retile: W=1"):
        ops.beam_retile(kc, vt, tab, torch.zeros((4, MAX_NEW, 1), dtype=torch.int32, device=DEV), torch.ones(4, dtype=torch.int32, device=DEV),
                        torch.ones(4, dtype=torch.int32, device=DEV), 1)
    with pytest.raises(_lib.DualHypHipError, match="n_tiles=65"):
        ops.beam_retile(kc, vt, torch.zeros((2, rows, 65), dtype=torch.int32, device=DEV), parent, n_steps, plen, 2)
    for bad in (dict(tile_tab=tab[0]), dict(tile_tab=tab.long()), dict(n_steps=n_steps[:1]), dict(k_cache=kc[:3]),
                dict(scratch=torch.zeros(8, dtype=torch.bfloat16, device=DEV))):
        kw = dict(k_cache=kc, vT_cache=vt, tile_tab=tab, beam_parent=parent, n_steps=n_steps, prompt_len=plen, step=2)
        kw.update(bad)
        with pytest.raises(ValueError, match="beam_retile"):
            ops.beam_retile(**kw)
    assert not kc.any() and not tab.any()
