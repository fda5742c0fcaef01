"""The checker of tests/test_hip_sampling.py has teeth (CPU only): the host model of tests/sampling_reference.py follows the
oracle's crop and softmax, and on the very inputs the GPU tests use check_pick rejects the picks of deliberately wrong host
samplers — each one a bug the top-k kernel could plausibly have — while at most a tenth of any case's draws lie so close
to an interval end that fp32 could not be told from fp64."""
import functools
import math

import numpy as np
import pytest
import torch

import sampling_reference as R

BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _us(n_seq: int, steps: tuple, swap: bool = False) -> np.ndarray:
    return np.concatenate([R.u01_grid(s, steps, n_seq, swap).reshape(-1) for s in R.SEEDS])


def _inputs():
    """(name, row, top_k, temperature, n_seq, steps) of every exact-draw input of the GPU tests."""
    out = [(c.name, R.case_row(c), c.top_k, c.temperature, c.n_seq, R.STEPS) for c in R.grid_cases()]
    out += [(n, row, k, T, R.CRAFTED_N_SEQ, R.CRAFTED_STEPS) for n, row, k, T in R.crafted_rows()]
    return out


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def rejected(inputs):
    """{mutant: set of input names on which at least one of the mutant's picks fails check_pick}; the right host sampler
    (mutant None) is run through the same code and must pass everywhere with no excess."""
    table = {m: set() for m in R.MUTANTS}
    for name, row, k, T, n_seq, steps in inputs:
        model = R.RowModel(R.scaled(row, T), k)
        us = _us(n_seq, steps)
        for mutant in [None] + R.MUTANTS:
            try:
                picks = np.concatenate([R.mutant_picks(mutant, row, T, k, s, steps, n_seq).reshape(-1) for s in R.SEEDS])
            except ValueError:
                continue                       # slab_drop_last on a vocabulary of one token per slab
            ok, excess = model.check(picks, us)
            if mutant is None:
                assert ok.all() and excess.max() == 0.0, name
            elif not ok.all():
                table[mutant].add(name)
    return table


# ---------------------------------------------------------------------------------------------------- the uniform
def test_mix64_known_answer():
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.mix64(R.M64) < 1 << 64 and R.mix64(R.M64) != R.mix64(0)


def test_u01_range_and_arguments():
    us = _us(256, (0, 1, 7))
    assert us.min() >= 0.0 and us.max() < 1.0
    assert np.all(us * 2 ** 24 == np.floor(us * 2 ** 24))            # 24 bits: exact as fp32
    base = R.u01(5, 3, 9)
    assert base != R.u01(6, 3, 9) and base != R.u01(5, 4, 9) and base != R.u01(5, 3, 10)
    assert R.u01(5, 3, 9) != R.u01(5, 9, 3)
    assert R.u01(5 + (1 << 64), 3, 9) == base and R.u01(5, 3, 9 + (1 << 32)) == base     # uint64 seed, uint32 seq
    assert R.u01(1 << 63, 0, 0) != R.u01(0, 0, 0)


def test_inverse_cdf_frequencies():
    """2^16 draws of the model on a 6-token row.  The count of token i is Binomial(N, p_i), standard deviation
    sqrt(N p_i (1 - p_i)); a fair sampler leaves 5 of them with probability 6e-7 per token, a hash that ignores an argument or
    a CDF off by one bin misses by hundreds."""
    row = torch.tensor([1.5, -0.25, 0.75, 2.0, -1.0, 0.0], dtype=BF)
    m = R.RowModel(R.scaled(row, 1.0), None)
    N = 1 << 16
    us = R.u01_grid(77, range(256), 256).reshape(-1)
    assert us.size == N
    counts = np.bincount(m.pick(us), minlength=6)
    p = torch.softmax(row.double(), 0).numpy()
    assert np.all(np.abs(counts - N * p) <= 5 * np.sqrt(N * p * (1 - p))), (counts, N * p)


# ---------------------------------------------------------------------------------------------------- the crop
def _oracle_crop(monkeypatch, row, temperature, top_k):
    """The logits that oracle.ger_oracle.pick_token hands to softmax (cropped entries are -inf there)."""
    from oracle import ger_oracle as O
    seen = []

    def capture(logits, dim=-1):
        seen.append(logits.clone())
        return torch.full_like(logits, 1.0 / logits.numel())
    monkeypatch.setattr(O.F, "softmax", capture)
    O.pick_token(row, temperature, top_k, "multinomial")
    monkeypatch.undo()
    return seen[0]


def test_keep_mask_is_the_oracles_crop(monkeypatch, inputs):
    g = torch.Generator().manual_seed(3)
    rows = [(torch.randn(V, generator=g).to(BF) * 3, k, T) for V in (17, 256, 1000) for k in (1, 2, 5, 50, 2000, None)
            for T in (0.2, 0.8, 1.0, 1.7)]
    rows += [(row, k, T) for _, row, k, T, _, _ in inputs if row.numel() <= 32064]
    n_tied = 0
    for row, k, T in rows:
        sc = R.scaled(row, T)
        keep = R.keep_mask(sc, k)
        got = _oracle_crop(monkeypatch, row, T, k)
        assert got.dtype == BF
        # kept entries reach softmax bit for bit as scaled() has them, so scaled() is the oracle's `logits / temperature`
        assert torch.equal(got[keep].view(torch.int16), sc[keep].view(torch.int16))
        assert bool(torch.isneginf(got[~keep]).all())
        n_tied += int(k is not None and int(keep.sum()) > k)
    assert n_tied >= 10
    assert R.keep_mask(torch.randn(9).to(BF), 0).all()


def test_signed_zeros_are_one_value():
    for z in ([0.0, -0.0, -1.0, 2.0], [-0.0, 0.0, -1.0, 2.0]):
        assert R.keep_mask(torch.tensor(z, dtype=BF), 2).tolist() == [True, True, False, True]


def test_tie_rows_are_among_the_inputs(inputs):
    kept = {name: int(R.keep_mask(R.scaled(row, T), k).sum()) for name, row, k, T, _, _ in inputs}
    assert kept["V32000.k200.T1.0.u3"] > 200 and kept["V32000.k5.T0.8.u3"] > 5 and kept["V128256.k5.T0.8.u3"] > 5
    assert kept["ties_at_kth"] == 15 and kept["all_equal_k5"] == 1000


# ---------------------------------------------------------------------------------------------------- the checker
def test_eps_is_the_derived_formula():
    for V in (4, 256, 1000, 32000, 32064, 128256):
        assert R.eps(V) == (3 * math.ceil(V / 1024) + 43) * 2.0 ** -24 + 2.0 ** -18


def test_check_pick_at_the_interval_ends():
    sc = torch.tensor([0.0, 1.0, -30.0, 0.5, 0.0], dtype=BF)
    m = R.RowModel(sc, 3)                                     # keeps 1.0, 0.5 and both 0.0
    assert m.keep.tolist() == [True, True, False, True, True]
    e, hi0 = m.eps, m.hi[0]
    assert R.check_pick(0, sc, 3, hi0 - 1e-9) == (None, 0.0)
    reason, excess = R.check_pick(1, sc, 3, hi0 - 0.5 * e)            # the neighbour, within the fp32 allowance
    assert reason is None and excess == pytest.approx(0.5 * e)
    reason, excess = R.check_pick(1, sc, 3, hi0 - 2 * e)
    assert reason is not None and excess == pytest.approx(2 * e)
    assert R.check_pick(0, sc, 3, hi0 + 2 * e)[0] is not None
    assert "kept set" in R.check_pick(2, sc, 3, m.lo[2])[0]           # inside its (empty) interval, but cropped
    assert R.check_pick(5, sc, 3, 0.5)[0] is not None and R.check_pick(-1, sc, 3, 0.5)[0] is not None


def test_ambiguity_cap(inputs):
    """Input sensitivity: a draw whose u lies within eps of an end of the reference pick's interval accepts two tokens, so it
    tests nothing.  At most 10 % of the draws of any GPU case may be such, from the fp64 reference alone."""
    shares = {}
    for name, row, k, T, n_seq, steps in inputs:
        shares[name] = R.RowModel(R.scaled(row, T), k).ambiguous(_us(n_seq, steps)).mean()
    worst = max(shares, key=shares.get)
    print(f"ambiguous share: worst {shares[worst]:.4f} ({worst}), mean {np.mean(list(shares.values())):.4f}")
    assert shares[worst] <= 0.10, (worst, shares[worst])
    # and flat rows of a real vocabulary are indeed beyond it: the reason the uncropped cases are peaked
    flat = R.Case("flat", 128256, None, 1.0, "u3", 256)
    assert R.RowModel(R.scaled(R.case_row(flat), 1.0), None).ambiguous(_us(256, R.STEPS)).mean() > 0.5


# ---------------------------------------------------------------------------------------------------- mutation controls
def test_every_mutant_is_rejected(rejected, inputs):
    for m in R.MUTANTS:
        print(f"{m}: rejected on {len(rejected[m])} of {len(inputs)} inputs")
        assert rejected[m], f"no GPU input tells {m} from the right sampler"


def test_hash_and_order_mutants_are_rejected_everywhere(rejected, inputs):
    names = {i[0] for i in inputs}
    assert rejected["swap_step_seq"] == names
    assert rejected["cdf_descending"] == names


def test_crop_mutants_are_rejected_where_they_bite(rejected, inputs):
    names = [i[0] for i in inputs]
    pairs = {n for n in names if n.startswith("pair_")}
    assert len(pairs) == 10 and pairs <= rejected["thr_one_key_low"]
    assert {n for n in names if ".k5." in n and n.endswith("u3")} <= rejected["thr_one_key_low"]
    ties = {"ties_at_kth", "all_equal_k5", "V32000.k200.T1.0.u3", "V32000.k5.T0.8.u3", "V128256.k5.T0.8.u3", "V128256.k200.T1.0.u3"}
    assert ties <= rejected["drop_kth_ties"]
    assert rejected["drop_neg_zero"] == set(R.ZERO_ROWS)              # and nothing else: only signed zeros tell it apart
    uncropped = {c.name for c in R.grid_cases() if c.vocab > 1024 and (c.top_k is None or c.top_k >= c.vocab - 1)}
    assert len(rejected["slab_drop_last"] & uncropped) >= len(uncropped) // 2
    assert len(rejected["temperature_unrounded"]) >= len([c for c in R.grid_cases() if c.temperature != 1.0]) // 2


# ---------------------------------------------------------------------------------------------------- side effects
def test_expected_state_rules():
    tok = torch.full((6, 4), -7, dtype=torch.int64)
    length = torch.tensor([1, 2, 3, 4, 0, 3])
    done = torch.tensor([0, 1, 0, 0, 2, 0])
    picks = [10, 11, 12, 13, 14, 9]
    t, n, d = R.expected_state(tok, length, done, picks, eos_id=9)
    assert t[0].tolist() == [-7, 10, -7, -7] and (n[0], d[0]) == (2, 0)
    assert t[1].tolist() == [-7] * 4 and (n[1], d[1]) == (2, 1)                      # finished: frozen
    assert t[2].tolist() == [-7, -7, -7, 12] and (n[2], d[2]) == (4, 2)              # length + 1 == tok_ld
    assert t[3].tolist() == [-7] * 4 and (n[3], d[3]) == (4, 2)                      # length == tok_ld: nothing written
    assert t[4].tolist() == [-7] * 4 and (n[4], d[4]) == (0, 2)
    assert t[5, 3] == 9 and (n[5], d[5]) == (4, 1)                                   # EOS wins over the full buffer
    assert R.expected_state(tok, length, done, picks, eos_id=None)[2].tolist() == [0, 1, 2, 2, 2, 2]
    # row list: row r -> sequence row_seq[r], budget min(limit, tok_ld); -1 and n_seq name nothing; 1 is finished padding
    t, n, d = R.expected_state(tok, length, done, [20, 21, 22, 23, 24, 25], eos_id=None,
                               limit=torch.tensor([2, 9, 9, 9, 9, 9]), row_seq=torch.tensor([5, 1, 1, -1, 6, 0]))
    assert t[5].tolist() == [-7, -7, -7, 20] and (n[5], d[5]) == (4, 2)
    assert t[0].tolist() == [-7, 25, -7, -7] and (n[0], d[0]) == (2, 2)              # its own limit of 2 reached
    assert np.array_equal(t[1:5], tok[1:5].numpy()) and n[1:5].tolist() == [2, 3, 4, 0] and d[1:5].tolist() == [1, 0, 0, 2]
