"""tests/nucleus_reference.py checked on the CPU: every case of the GPU test is decided under the derived band, the crafted rows are
what their names say, every mutant's kept set or picks differ from the right ones on a named case, and on the chunky rows the right
sampler's picks cover the kept set, so a wrong kept set cannot hide behind unlucky draws."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nucleus_reference as NR  # noqa: E402
import sampling_reference as SR  # noqa: E402

BF = torch.bfloat16
CASES = {c.name: c for c in NR.cases()}


def sc_of(c):
    return SR.scaled(NR.rows()[c.row], c.temperature)


def kept(c, mutant=None, allowed=None):
    return NR.nucleus_keep(sc_of(c), c.top_k, c.top_p, c.min_p, allowed, mutant, raw=NR.rows()[c.row])


def test_the_band_is_derived_and_capped():
    assert NR.BAND == 2.0 ** -18 + 2.0 ** -22 + 2.0 ** -39
    assert NR.BAND <= NR.BAND_CAP == 2.0 ** -16


def test_every_case_is_decided():
    names = [c.name for c in NR.cases()]
    assert len(set(names)) == len(names)
    # the grid crossed with the three top_p and the three min_p, the V = 515 rows, the crafted rows at both sizes
    assert len([n for n in names if not n.startswith(("crafted", "V515"))]) == len(SR.grid_cases()) * 9
    assert any(n.startswith("V515") for n in names) and any(n.startswith("crafted.V256") for n in names)
    undecided = []
    for c in NR.cases():
        ok, margin = NR.decided(sc_of(c), c.top_k, c.top_p)
        if not ok:
            undecided.append((c.name, margin))
    assert not undecided, undecided


def test_the_kept_set_on_hand_cases():
    row = torch.tensor([2.0, 1.0, 1.0, 0.0, -math.inf], dtype=BF)       # masses e^0, e^-1, e^-1, e^-2, 0: T = 1.871
    keep = lambda *a, **k: NR.nucleus_keep(row, *a, **k).tolist()         # noqa: E731
    assert keep(None, None, None) == [True] * 5
    assert keep(None, 0.5, None) == [True, False, False, False, False]    # A(1.0) / T = 0.534 >= 0.5
    assert keep(None, 0.6, None) == [True, True, True, False, False]      # the crossing value whole: both ties
    assert keep(None, 0.93, None) == [True, True, True, True, False]      # A(0.0) / T = 0.928
    assert keep(2, 0.6, None) == [True, True, True, False, False]         # K0 = the three (the tie at the 2nd value stays)
    assert keep(1, 0.01, 1.0) == [True, False, False, False, False]
    assert keep(None, None, 1.0) == [True, False, False, False, False]
    assert keep(None, None, math.exp(-1.0) * 0.999) == [True, True, True, False, False]
    assert keep(None, None, 0.1) == [True, True, True, True, False]       # e^-2 = 0.135 >= 0.1
    assert keep(None, 0.93, 0.2) == [True, True, True, False, False]      # the intersection
    allowed = np.array([False, True, True, True, True])
    assert keep(None, 0.5, None, allowed) == [False, True, True, False, False]    # the best allowed value is always kept
    assert keep(None, None, 1.0, allowed) == [False, True, True, False, False]
    assert NR.decided(row, None, 0.5)[0] and NR.decided(row, None, None) == (True, math.inf)
    ok, margin = NR.decided(row, None, float(np.float32(math.e ** 0 / (1 + 2 / math.e + math.e ** -2))))
    assert not ok and margin < NR.BAND                                    # top_p on A(1.0) / T itself: undecided


def test_the_crafted_rows_are_what_they_claim():
    for c in NR.cases():
        if not c.chunky:
            continue
        sc = sc_of(c)
        x = sc.double().numpy()
        w = np.exp(x - x.max())
        share = w / w.sum()
        massy = share > 1e-9
        assert massy.sum() <= 12 and share[massy].min() >= 0.02, c.name
        assert share[~massy].sum() < 1e-30, c.name
    z = CASES["crafted.V1000.spans_zero"]
    bits = sc_of(z).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    k = kept(z)
    assert k[bits == 0x0000].all() and k[bits == 0x8000].all() and (bits == 0x8000).sum() == 2 and (bits == 0x0000).sum() == 1
    assert not kept(CASES["crafted.V1000.zero_dropped"])[(bits & 0x7FFF) == 0].any()
    t = CASES["crafted.V1000.ties_at_crossing"]
    at = np.flatnonzero(sc_of(t).float().numpy() == 1.0)
    assert len(at) == 6 and kept(t)[at].all() and {63, 64, 65} <= set(at.tolist()) and kept(t).sum() == 9
    for name, hi_w, lo_w in (("pair_low_byte", 0x3F82, 0x3F81), ("pair_high_byte", 0x3F00, 0x3EFF), ("pair_low_byte_neg", 0xBF81, 0xBF82),
                             ("pair_high_byte_neg", 0xBEFF, 0xBF00)):
        for v in (256, 1000):
            for suffix in ("", "_swapped"):
                c = CASES[f"crafted.V{v}.{name}{suffix}"]
                b = sc_of(c).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
                k = kept(c)
                assert k[b == hi_w].all() and not k[b == lo_w].any() and k.sum() == 3, c.name
    assert kept(CASES["crafted.V256.three_maxima_min_p_1"]).sum() == 3
    assert kept(CASES["crafted.V256.only_the_best"]).sum() == 1
    c = CASES["crafted.V1000.top_k_then_nucleus"]
    assert SR.keep_mask(sc_of(c), c.top_k).sum() == 5 and kept(c).sum() == 4
    c = CASES["crafted.V256.neg_inf_entries"]
    assert torch.isinf(sc_of(c)).sum() >= 50 and (sc_of(c) == -90.0).sum() > 100 and kept(c).sum() == 5
    assert kept(CASES["crafted.V1000.min_p_between"]).sum() == 4


# mutant -> the named cases on which its kept set (or, for the mutant of the draw, its picks) must differ
KILLS = {
    "nucleus_drops_crossing": ["crafted.V1000.ties_at_crossing", "crafted.V256.pair_low_byte", "crafted.V1000.spans_zero"],
    "ties_split_by_index": ["crafted.V1000.ties_at_crossing", "crafted.V256.spans_zero"],
    "nucleus_before_top_k": ["crafted.V1000.top_k_then_nucleus", "crafted.V256.top_k_then_nucleus"],
    "nucleus_unscaled": ["crafted.V1000.scaled_T0.5", "V32000.k200.T0.2.g4.p0.9.m0.0"],
    "min_p_of_total": ["crafted.V1000.min_p_between", "crafted.V256.all_negative_min_p"],
    "min_p_strict": ["crafted.V256.three_maxima_min_p_1", "V1000.k5.T0.8.u3.p0.5.m1.0"],
}


@pytest.mark.parametrize("mutant", sorted(KILLS))
def test_every_kept_set_mutant_differs_on_a_named_case(mutant):
    for name in KILLS[mutant]:
        c = CASES[name]
        assert not np.array_equal(kept(c), kept(c, mutant)), (mutant, name)


def test_the_mask_mutant_differs_under_a_mask():
    """the allowed set takes the best two values away: the masses of the nucleus are those of what is left"""
    for name in ("crafted.V1000.ties_at_crossing", "crafted.V256.top_k_then_nucleus"):
        c = CASES[name]
        sc = sc_of(c)
        order = torch.argsort(sc.float(), descending=True)
        allowed = np.ones(sc.numel(), dtype=bool)
        allowed[order[:2].numpy()] = False
        right, wrong = kept(c, allowed=allowed), kept(c, "nucleus_ignores_mask", allowed=allowed)
        assert right.any() and not right[~allowed].any() and not np.array_equal(right, wrong), name


def test_the_draw_mutant_differs_in_its_picks():
    for name in ("crafted.V1000.spans_zero", "crafted.V256.ties_at_crossing"):
        c = CASES[name]
        args = (NR.rows()[c.row], c.temperature, c.top_k, c.top_p, c.min_p, NR.SEEDS[0], NR.STEPS, c.n_seq)
        assert not np.array_equal(NR.picks(None, *args), NR.picks("cdf_not_renormalised", *args)), name
    assert set(NR.MUTANTS) == set(KILLS) | {"nucleus_ignores_mask", "cdf_not_renormalised"}


def test_the_picks_cover_the_kept_set_on_every_chunky_row():
    """the union of the right sampler's picks over the GPU test's seeds and draws is the kept set: one wrongly kept or dropped value
    changes the union"""
    for c in NR.cases():
        if not c.chunky:
            continue
        seen = set()
        for seed in NR.SEEDS:
            seen |= set(NR.picks(None, NR.rows()[c.row], c.temperature, c.top_k, c.top_p, c.min_p, seed, NR.STEPS, c.n_seq).reshape(-1).tolist())
        assert seen == set(np.flatnonzero(kept(c)).tolist()), c.name
