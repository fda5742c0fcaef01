"""tests/logprob_reference.py against closed forms: the fp64 reference that tests/test_hip_logprobs.py holds the kernel to has to be
right by something other than itself.  CPU only."""
import math

import numpy as np
import pytest
import torch

import logprob_reference as R

BF = torch.bfloat16


@pytest.mark.parametrize("V", (1, 8, 1000, 128256))
def test_all_equal_row(V):
    for value in (0.0, 1.5, -7.0):
        row = np.full(V, value)
        for t in {0, V // 2, V - 1}:
            assert R.logprob64(row, t) == pytest.approx(-math.log(V), rel=1e-15, abs=1e-15)


@pytest.mark.parametrize("V", (8, 32000))
def test_one_entry_60_over_the_rest(V):
    """rest at c, one entry at c + 60: log Z = c + 60 + log1p((V - 1) e^-60); the tail is below fp64's resolution next to 1, so the
    reference is held to an absolute 1e-15"""
    c = -2.0
    row = np.full(V, c)
    row[3] = c + 60.0
    tail = math.log1p((V - 1) * math.exp(-60.0))
    assert R.logprob64(row, 3) == pytest.approx(-tail, abs=1e-15)
    assert R.logprob64(row, 4) == pytest.approx(-60.0 - tail, rel=1e-15)


def test_minus_inf_entries_add_nothing():
    row = np.array([0.5, -np.inf, 0.5, -np.inf, 0.5, 0.5, -np.inf, -np.inf])
    for t in (0, 2, 4, 5):
        assert R.logprob64(row, t) == pytest.approx(-math.log(4), rel=1e-15)
    # the same four finite entries alone
    assert R.logprob64(row, 0) == R.logprob64(np.full(4, 0.5), 0)


def test_minus_inf_token():
    row = np.array([0.5, -np.inf, 2.0])
    assert R.logprob64(row, 1) == -np.inf
    assert np.isfinite(R.logprob64(row, 0))


def test_row_of_3e4_everywhere_is_stable():
    V = 32000
    assert R.logprob64(np.full(V, 3e4), 17) == pytest.approx(-math.log(V), rel=1e-15)
    row = np.full(V, 3e4)
    row[5] = 3e4 + 128.0            # the next bf16 value at this magnitude
    assert R.logprob64(row, 5) == pytest.approx(-math.log1p((V - 1) * math.exp(-128.0)), abs=1e-15)
    assert R.logprob64(-row, 5) == pytest.approx(-128.0 - math.log(V - 1), rel=1e-15)


def test_probabilities_sum_to_one():
    row, _ = R.make_row("normal0", 1000, seed=0)
    r = row.to(torch.float64).numpy()
    assert sum(math.exp(R.logprob64(r, t)) for t in range(1000)) == pytest.approx(1.0, rel=1e-12)


def test_case_list():
    """every kind is what its name says, for every vocabulary size of the GPU test; the values are exact bf16"""
    for V in R.VOCABS:
        rows, ids, kinds = R.case(V, 37)
        assert rows.dtype == BF and tuple(rows.shape) == (37, V) and set(kinds) == set(R.KINDS)
        assert int(ids.min()) >= 0 and int(ids.max()) < V
        ref = R.logprobs64(rows, ids)
        for i, k in enumerate(kinds):
            r = rows[i].float()
            t = int(ids[i])
            if k == "all_equal":
                assert ref[i] == pytest.approx(-math.log(V), rel=1e-15)
            elif k == "dominant":
                assert float(r.max()) == 60.0 and (V == 1 or r[t] < 60.0)
            elif k == "tenth_minus_inf":
                assert int(torch.isinf(r).sum()) >= max(1, V // 10) - 1 and torch.isfinite(r[t])
            elif k == "magnitude_3e4":
                assert float(r.abs().max()) > 3e4
            elif k == "token_argmax":
                assert r[t] == r.max()
            elif k == "token_min":
                assert r[t] == r.min()
            elif k == "token_minus_inf":
                assert ref[i] == -np.inf
            if k != "token_minus_inf":
                assert np.isfinite(ref[i]) and ref[i] <= 0.0
    for n in R.ROW_COUNTS:
        assert len(R.case(320, n)[2]) == n
    assert R.case(320, 1)[2] != R.case(320, 37)[2][:1] and R.case(320, 3)[2] != R.case(320, 37)[2][:3]


def test_gate():
    ref = np.array([-1.0, -5e4, -np.inf, -2.0, -3.0])
    got = np.array([-1.0 + 1.9e-5, -5e4 + 0.011, -np.inf, -2.0 + 3e-5, np.nan])
    assert R.within_gate(got, ref).tolist() == [True, True, True, False, False]
    assert not R.within_gate(np.array([-1e30]), np.array([-np.inf]))[0]
