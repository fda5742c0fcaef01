"""The exact attention inputs and their fp64 reference (tests/attn_exact_reference.py) against themselves, without a GPU: one-hot
heads return the winner's V row, uniform heads the exact rational, and every distortion of the reference that a wrong kernel could
amount to is rejected by `Case.compare`, the checks tests/test_hip_attn_exact.py runs on the kernels' outputs."""
import functools
import sys
from fractions import Fraction
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attn_exact_reference as R  # noqa: E402

# one case of each kind; the GPU file runs every layout
CASES = {
    "packed": lambda: R.prefill_packed_case(64, 8, 1),
    "packed128": lambda: R.prefill_packed_case(128, 8, 2),
    "continuation": lambda: R.prefill_continuation_case(64, 6, 1),
    "continuation96": lambda: R.prefill_continuation_case(96, 4, 4),
    "decode": lambda: R.decode_case(64, 16, 1),
    "fused": lambda: R.fused_case(128, 8, 2),
}


@functools.lru_cache(maxsize=None)
def case(kind):
    return CASES[kind]()


def as_outputs(y64, lse64):
    """What a kernel would hand back: y rounded to bf16 once, lse in fp32."""
    return y64.bfloat16().reshape(y64.shape[0], -1), lse64.float()


@pytest.mark.parametrize("kind", CASES)
def test_reference_passes_its_own_checks(kind):
    c = case(kind)
    y, lse = as_outputs(*c.reference())
    assert c.compare(y, lse) == []
    E = c.expected()
    assert E["tie_share"] <= R.TIE_SHARE_MAX and torch.equal(R.tie_mask(E["y64"]), E["tie"])


@pytest.mark.parametrize("kind", CASES)
def test_one_hot_heads_return_the_winners_row_and_uniform_heads_the_exact_rational(kind):
    c = case(kind)
    E = c.expected()
    K, V = c.final_cache()
    fam = c.family.reshape(-1).tolist()
    row = 0
    for i, (slot, cached, new, _) in enumerate(c.seqs):
        for p in c.q_pos[i].tolist():
            for h in range(c.n_head):
                g = h // c.qpk
                if fam[h] < 3:
                    j = c._winner(i, g, fam[h], p)
                    assert torch.equal(E["y"][row, h].double(), V[slot, g, j]), (kind, i, p, h)
                    w = (p, 0, -abs(j - int(c.t[i, g])))[fam[h]] * (-1 if fam[h] == 1 else 1)
                    assert abs(E["lse"][row, h].item() - R.G_Q * c.scale * w) <= 1e-9 * max(1.0, abs(R.G_Q * c.scale * w))
                elif p % 7 == 0 or p < 3:              # exact rationals on a sample of the queries (Fractions are slow)
                    S = V[slot, g, :p + 1].sum(0)
                    for d in range(0, c.hs, 5):
                        exact = Fraction(int(S[d]), p + 1)
                        assert abs(Fraction(E["y64"][row, h, d].item()) - exact) <= Fraction(1, 10 ** 12)
                    assert abs(E["lse"][row, h].item() - torch.log(torch.tensor(p + 1.0, dtype=torch.float64)).item()) <= 1e-12
            row += 1
    assert row == c.n_q


def test_ties_are_the_only_place_where_fp32_quotients_may_differ():
    """Off the ties both S * (1 / n) and S / n in fp32 round to the reference's bf16; the closest non-tie is far from a boundary
    compared with the fp32 evaluation error."""
    c = case("packed")
    E = c.expected()
    uni = (c.family.reshape(-1) == 3).nonzero().flatten()
    n = torch.cat([p + 1 for p in c.q_pos]).double()[:, None, None]
    S = (E["y64"][:, uni] * n).round()
    for got in ((S.float() * (1.0 / n.float())), S.float() / n.float()):
        ok = (got.bfloat16() == E["y"][:, uni]) | E["tie"][:, uni]
        assert ok.all()
    rel = R.bf16_neighbours(E["y64"][:, uni])[2]
    assert rel[~E["tie"][:, uni]].min().item() >= 2.0 ** -19


# ---------------------------------------------------------------------------------------------- mutants
def _m_mask_high(c):
    def f(i, q, k, v, cnt):
        cnt = cnt.clone()
        for r, p in enumerate(c.q_pos[i].tolist()):
            if p + 1 < c.s_max:
                cnt[r, p + 1] = 1
        return q, k, v, cnt
    return f


def _m_mask_low(c):
    def f(i, q, k, v, cnt):
        cnt = cnt.clone()
        for r, p in enumerate(c.q_pos[i].tolist()):
            if p >= 1:
                cnt[r, p] = 0
        return q, k, v, cnt
    return f


def _m_kv_len_long(c):
    """Only the sequence's last query sees one key more: the first decoy behind the sequence."""
    def f(i, q, k, v, cnt):
        cnt = cnt.clone()
        if c.total[i] < c.s_max:
            cnt[-1, c.total[i]] = 1
        return q, k, v, cnt
    return f


def _m_first_tile_dropped(c):
    def f(i, q, k, v, cnt):
        cnt = cnt.clone()
        far = c.q_pos[i] >= 32
        cnt[far, :32] = 0
        return q, k, v, cnt
    return f


def _m_tile_swapped(c):
    """Tile 1 read where tile 0 belongs and the other way round; the mask still follows the position."""
    def f(i, q, k, v, cnt):
        idx = torch.arange(c.s_max)
        idx[:32], idx[32:64] = torch.arange(32, 64), torch.arange(32)
        return q, k[:, idx], v[:, idx], cnt
    return f


def _m_counted_twice(c):
    def f(i, q, k, v, cnt):
        cnt = cnt.clone()
        for r, p in enumerate(c.q_pos[i].tolist()):
            cnt[r, p // 2] = 2
        return q, k, v, cnt
    return f


def _m_skipped_in_uniform(c):
    """The uniform heads alone miss one key in the middle of their range."""
    def f(i, q, k, v, cnt):
        ch = cnt[:, None, :].repeat(1, c.n_head, 1)
        uni = (c.family.reshape(-1) == 3).nonzero().flatten()
        for r, p in enumerate(c.q_pos[i].tolist()):
            if p >= 1:
                ch[r, uni, p // 2] = 0
        return q, k, v, ch
    return f


def _m_heads_permuted(c):
    def f(i, q, k, v, cnt):
        qg = q.view(q.shape[0], c.n_groups, c.qpk, c.hs)
        return torch.roll(qg, 1, dims=2).reshape(q.shape), k, v, cnt
    return f


def _m_stale_row(c):
    """The rows the call appends are not seen: the cache still holds what was under them."""
    def f(i, q, k, v, cnt):
        slot = c.seqs[i][0]
        return q, c.world_k[slot], c.world_v[slot], cnt
    return f


MUTANTS = {
    "mask one key high": (_m_mask_high, ("packed", "continuation", "continuation96", "decode", "fused")),
    "mask one key low": (_m_mask_low, ("packed", "packed128", "continuation", "decode", "fused")),
    "kv_len one long": (_m_kv_len_long, ("packed", "continuation96", "decode", "fused")),
    "first tile dropped": (_m_first_tile_dropped, ("packed", "continuation", "decode", "fused")),
    "a 32-key tile swapped with its neighbour": (_m_tile_swapped, ("packed", "continuation", "decode", "fused")),
    "one key counted twice": (_m_counted_twice, ("packed", "packed128", "continuation", "decode", "fused")),
    "one key skipped in the uniform head": (_m_skipped_in_uniform, ("packed", "continuation", "decode", "fused")),
    "heads of a group permuted": (_m_heads_permuted, ("packed", "packed128", "continuation", "decode", "fused")),
    "the stale row read in place of the appended one": (_m_stale_row, ("packed", "continuation", "fused")),
}


@pytest.mark.parametrize("name,kind", [(n, k) for n, (_, kinds) in MUTANTS.items() for k in kinds])
def test_mutant_is_rejected(name, kind):
    c = case(kind)
    y, lse = as_outputs(*c.reference(MUTANTS[name][0](c)))
    msgs = c.compare(y)                                  # y alone has to show it: the decode kernels have no lse
    assert msgs, f"{name} passes the checks on the {kind} case"
    assert all(c.name in m for m in msgs)
    if name == "one key counted twice":
        # ... and the prefill kernel's lse shows it on its own, at every head: a winner counted twice is log 2 off
        E = c.expected()
        clean = E["y"].reshape(c.n_q, -1)
        assert c.compare(clean, lse), "lse does not notice a key counted twice"


def test_messages_name_the_key_the_output_equals():
    c = case("fused")
    y, _ = as_outputs(*c.reference(_m_stale_row(c)))
    msgs = c.compare(y, limit=1000)
    assert any("the stale row under key" in m and "recency" in m for m in msgs)
    c = case("decode")
    y, _ = as_outputs(*c.reference(_m_kv_len_long(c)))
    msgs = c.compare(y, limit=1000)
    assert any("(a decoy)" in m and "should equal key" in m for m in msgs) and any("uniform" in m and "sum over about" in m for m in msgs)


def test_builder_refuses_inputs_that_are_not_exact():
    with pytest.raises(AssertionError):
        R.Case("too long for two digits", 64, 4, 1, [(0, 0, 64, False)], 4096, 1, 0)
