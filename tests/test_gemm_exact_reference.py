"""The exact-integer GEMM reference on its own (tests/gemm_exact_reference.py; CPU only): every case of the GPU test's table
meets the exactness condition, every route of the library's route record has a case, and the guard and SwiGLU checks
catch what they are there for."""
import re
from pathlib import Path

import pytest
import torch

import gemm_exact_reference as R
import qgemm_exact_reference as Q

REPO = Path(__file__).resolve().parent.parent
GROUPS = sorted({(c.family, c.group) for c in R.CASES})


def _distinct(family, group):
    seen, out = set(), []
    for c in R.cases_of(family, group):
        if c.data_key not in seen:
            seen.add(c.data_key)
            out.append(c)
    return out


@pytest.mark.parametrize("family,group", GROUPS, ids=[f"{f}/{g}" for f, g in GROUPS])
def test_every_case_is_exact(family, group):
    """reference() raises InexactCase where a rounding point of a case would round (it never clips)"""
    for c in _distinct(family, group):
        ref = R.reference(c, R.operands(c))
        for k, v in ref.items():
            assert v.dtype == torch.float64 and torch.equal(v, v.round()), f"{c.id}: {k} is not an integer tensor"
        if "g" in ref:
            assert ref["g"].abs().max() <= R.SILU_G_MAX


def test_reference_raises_instead_of_clipping():
    c = R.Case("t128", "x", "linear", 64, 64, 2048)
    o = R.operands(c)
    o["x"] = o["x"] * 8 + 1                            # |acc| far beyond 256 with odd values: not representable
    with pytest.raises(R.InexactCase):
        R.reference(c, o)
    p = R.Case("rows", "x", "partial", 4, 16, 2048)
    o = R.operands(p)
    o["x"] = o["x"] * 2.0 ** 22
    with pytest.raises(R.InexactCase):
        R.reference(p, o)


def test_route_table_matches_the_library_and_every_route_has_a_case():
    src = (REPO / "dualhyp_amd" / "csrc" / "gemm.h").read_text()
    body = re.search(r"enum DhGemmRoute : int \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r"^\s*DH_ROUTE_(\w+)", body, re.M)
    assert names[-1] == "COUNT"
    assert tuple(n.lower() for n in names[:-1]) == R.ROUTES
    used = set()
    for c in R.CASES:
        assert set(c.routes) <= set(R.ROUTES) and set(c.tail_routes) <= set(R.ROUTES) and c.routes, c.id
        used |= set(c.routes) | set(c.tail_routes)
    quantised = {r for r in R.ROUTES if r.startswith(("fp8_", "mx4_"))}       # these have their cases in tests/qgemm_exact_reference.py
    assert not used & quantised
    for c in Q.CASES:
        assert set(c.routes) <= quantised and c.routes, c.id
        used |= set(c.routes)
    assert used == set(R.ROUTES), f"routes without a case: {sorted(set(R.ROUTES) - used)}"
    assert R.route_names(0b101) == {"t128_s2", "w8_pipe0"}
    for c in R.CASES:
        for k, _ in c.tune:
            assert k in R.TUNING_DEFAULTS, f"{c.id}: key {k} has no default to restore"


def test_row_split_of_the_table_shapes():
    assert R.row_split(4097, 4104, 256) == (3840, 257)          # 289 tiles: one round of 256 CUs + 33
    assert R.row_split(2049, 3592, 256) is None                 # 135 tiles: under one round
    assert R.row_split(4097, 4104, 304) is None                 # another chip: no full round
    c = next(c for c in R.CASES if c.tail_routes and c.M == 4097 and c.K == 128 and c.epi == "plain" and not c.resid)
    assert R.expected_routes(c, 256) == {"w4_persist", "t128_s4"} and R.expected_routes(c, 304) == {"w4_persist"}


def test_partial_slices_add_up_to_the_product():
    for K, ks in ((512, 2), (2048, 4), (384, 2), (96, 1), (320, 3)):
        c = R.Case("rows", "x", "partial", 5, 16, K, n_ext=16, ksplit=ks)
        steps = R.slice_ksteps(c)
        assert sorted(s for sl in steps for s in sl) == list(range(K // 32))
        o = R.operands(c)
        wf = torch.cat([o["w"], o["w_ext"]])
        parts = R.reference(c, o)["parts"]
        assert parts.shape == (ks, 5, 32) and torch.equal(parts.sum(0), o["x"] @ wf.T)
        pairs = R.reference(R.Case("pairs", "x", "pairs", 5, 16, K, n_ext=16, ksplit=ks), o)["parts"]
        assert pairs.shape == ((ks + 1) // 2, 5, 32) and torch.equal(pairs.sum(0), parts.sum(0))
    assert R.slice_ksteps(R.Case("rows", "x", "partial", 1, 16, 320, ksplit=3)) == [list(range(8)), [8, 9], []]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guard_catches_a_planted_element_on_either_side_and_a_sentinel_left_inside(dtype):
    shape = (5, 24)

    def fresh():
        g = R.Guarded(shape, dtype, "cpu", R.guard_rows(shape))
        g.t.copy_(torch.arange(120, dtype=torch.float32).view(shape))
        return g

    g = fresh()
    assert g.pre >= 256 * 24 and g.pre * g.raw.element_size() % 16 == 0 and g.t.data_ptr() % 16 == 0
    assert (g.raw.data_ptr() + g.post0 * g.raw.element_size()) % 16 == 0 and g.raw.numel() - g.post0 >= 256 * 24
    g.check("clean")
    g = fresh()
    g.raw[g.pre - 1] = 0
    with pytest.raises(AssertionError, match="BEFORE"):
        g.check("before")
    g = fresh()
    g.raw[g.pre + g.n] = 0
    with pytest.raises(AssertionError, match="BEHIND"):
        g.check("behind")
    g = fresh()
    g.raw[-1] = 0                                     # the far end of the margin as well
    with pytest.raises(AssertionError, match="BEHIND"):
        g.check("behind")
    g = fresh()
    g.raw[g.pre + 37] = g.sentinel
    with pytest.raises(AssertionError, match="never written"):
        g.check("inside")
    g.check("inside, not required", written=False)
    assert torch.isnan(R.Guarded(shape, dtype, "cpu", 8).t).all()      # the sentinel is a NaN: it fails every value comparison


def test_silu_candidates_are_the_nearest_bf16_and_its_neighbours():
    tab = R.silu_candidates()
    assert tab.shape == (2 * R.SILU_G_MAX + 1, 3) and torch.equal(tab.bfloat16().float(), tab)
    g = torch.arange(-R.SILU_G_MAX, R.SILU_G_MAX + 1, dtype=torch.float64)
    v = g / (1 + torch.exp(-g))
    err = (tab.double() - v[:, None]).abs()
    assert (err[:, 0] <= err[:, 1]).all() and (err[:, 0] <= err[:, 2]).all()
    assert (tab[:, 1] < tab[:, 0]).all() and (tab[:, 0] < tab[:, 2]).all()
    big = g.abs() <= 80                               # away from the underflow range: one neighbour is one bf16 ulp (2^-8 relative at most)
    nz = big & (g != 0)
    assert ((tab[nz, 2] - tab[nz, 1]).double() <= v[nz].abs() * 2.0 ** -6).all()
    assert tab[R.SILU_G_MAX].tolist()[0] == 0.0 and tab[R.SILU_G_MAX + 3, 0] == torch.tensor(3 / (1 + 2.718281828459045 ** -3)).bfloat16().float()


def test_swiglu_acceptance_rejects_swapped_operands_and_a_row_shift():
    gen = torch.Generator().manual_seed(3)
    g = torch.randint(-40, 41, (33, 64), generator=gen).double()
    u = torch.randint(-40, 41, (33, 64), generator=gen).double()
    tab = R.silu_candidates()

    def swiglu(g, u, col=0):
        return (tab[(g.long() + R.SILU_G_MAX)][..., col] * u.float()).bfloat16()

    ok, n, _ = R.swiglu_accept(swiglu(g, u), g, u)
    assert ok.all() and n == 0
    ok, n, _ = R.swiglu_accept(swiglu(g, u, 2), g, u)                     # one bf16 ulp of silu off: accepted, and counted
    assert ok.all() and 0 < n <= g.numel()
    two_off = (tab[:, 2] + (tab[:, 2] - tab[:, 0]))[(g.long() + R.SILU_G_MAX)]
    ok, _, _ = R.swiglu_accept((two_off * u.float()).bfloat16(), g, u)    # two ulps off: rejected wherever it changes the result
    assert not ok.all()
    ok, _, _ = R.swiglu_accept(swiglu(u, g), g, u)
    assert not ok.all(), "a swapped (g, u) pair passes"
    ok, _, _ = R.swiglu_accept(swiglu(g, u).roll(1, 0), g, u)
    assert not ok.all(), "a result shifted by one row passes"
    bad = swiglu(g, u).clone()
    bad[4, 5] = float("nan")
    ok, _, _ = R.swiglu_accept(bad, g, u)
    assert int((~ok).sum()) == 1 and "g values" in R.swiglu_failures(bad, g, u, ok)


def test_swiglu_acceptance_names_the_fp32_underflow_range():
    """a zero is accepted only where the fp32 sigmoid is below the smallest normal number, and is counted apart"""
    assert R.SILU_FLUSH_G == -88
    g = torch.tensor([[-86.0, -87.0, -88.0, -89.0, -96.0, -97.0, -120.0, 3.0]])
    u = torch.full_like(g, 7.0)
    zero = torch.zeros_like(g).bfloat16()
    ok, n, flushed = R.swiglu_accept(zero, g, u)
    assert ok.tolist() == [[False, False, True, True, True, True, True, False]]
    assert n == 1 and flushed == 3                      # -88, -89, -96 through the clause alone; at -97 zero is a neighbour, at -120 the nearest
    ok, _, flushed = R.swiglu_accept(-zero, g, u)
    assert ok.tolist() == [[False, False, True, True, True, True, True, False]] and flushed == 3
    tab = R.silu_candidates()
    exact = (tab[(g.long() + R.SILU_G_MAX)][..., 0] * u.float()).bfloat16()
    ok, n, flushed = R.swiglu_accept(exact, g, u)
    assert ok.all() and n == 0 and flushed == 0
    wrong = exact.clone()
    wrong[0, 3] = 1.0                                   # inside the range nothing but the zero is added
    ok, _, _ = R.swiglu_accept(wrong, g, u)
    assert not ok[0, 3]
