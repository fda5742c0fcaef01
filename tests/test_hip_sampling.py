"""dh_sample_bf16 / dh_sample_rows_bf16 (dualhyp_amd/csrc/sampling.hip) against the fp64 host model of
tests/sampling_reference.py.  The draw is a pure function of (seed, step, seq), so the model says which token must come out:
every pick has to be a kept token whose fp64 CDF interval holds u, up to the eps(V) that the kernel's fp32 sums are allowed
(derived in sampling_reference.eps; tests/test_sampling_reference.py shows on these inputs that wrong samplers are rejected).
Per case the worst distance of u from the picked interval, in units of eps, and the share of draws too close to an interval end
to tell fp32 from fp64 go to the parity record as sampling.<case>.

Not reached by any input here: the kernel's fall-back for a u that no thread claims (a rounding gap between two slabs' ends,
or past the last bin), which takes the row's arg-max; such a pick would be rejected (MEASUREMENTS.md)."""
import numpy as np
import pytest
import torch

import sampling_reference as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _state(dev, n_seq, tok_ld, length=0, done=0, fill=-1):
    i32 = dict(dtype=torch.int32, device=dev)
    tokens = torch.full((n_seq, tok_ld), fill, dtype=torch.int64, device=dev)
    length = torch.full((n_seq,), length, **i32) if isinstance(length, int) else torch.tensor(length, **i32)
    done = torch.full((n_seq,), done, **i32) if isinstance(done, int) else torch.tensor(done, **i32)
    return tokens, length, done


def _exact_draws(dev, name, row, top_k, temperature, n_seq, steps):
    """One launch per (seed, step) on n_seq copies of `row`: every pick must pass check_pick at u01(seed, step, seq)."""
    from dualhyp_amd import ops
    model = R.RowModel(R.scaled(row, temperature), top_k)
    lg = row.to(dev).view(1, -1).expand(n_seq, -1).contiguous()
    picks, us = [], []
    for seed in R.SEEDS:
        for step in steps:
            tokens, length, done = _state(dev, n_seq, 1)
            ops.sample(lg, tokens, length, done, temperature=temperature, top_k=top_k, seed=seed, step=step)
            assert length.tolist() == [1] * n_seq
            picks.append(tokens.view(-1).cpu().numpy())
            us.append(R.u01_grid(seed, [step], n_seq).reshape(-1))
    picks, us = np.concatenate(picks), np.concatenate(us)
    ok, excess = model.check(picks, us)
    record_parity(f"sampling.{name}", vocab=row.numel(), kept=int(model.keep.sum()), draws=picks.size, rejected=int((~ok).sum()),
                  worst_excess=excess.max(), worst_excess_over_eps=excess.max() / model.eps,
                  ambiguous_share=model.ambiguous(us).mean(), differ_from_fp64_pick=int((picks != model.pick(us)).sum()))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {picks.size} picks rejected, first: " + "; ".join(
        R.check_pick(int(picks[i]), R.scaled(row, temperature), top_k, float(us[i]), model)[0] for i in bad[:3])
    return picks, model


@pytest.mark.parametrize("case", R.grid_cases(), ids=lambda c: c.name)
def test_exact_draws(dev, case):
    _exact_draws(dev, case.name, R.case_row(case), case.top_k, case.temperature, case.n_seq, R.STEPS)


@pytest.mark.parametrize("name,row,top_k,temperature", R.crafted_rows(), ids=[c[0] for c in R.crafted_rows()])
def test_crafted_rows(dev, name, row, top_k, temperature):
    """The edges of the crop: ties at the k-th value, negative thresholds, keys one apart in either radix pass, equal logits,
    -inf, signed zeros.  Every pick is a kept token at its exact place in the CDF, and every kept token with a fair share
    of the mass comes out."""
    picks, model = _exact_draws(dev, name, row, top_k, temperature, R.CRAFTED_N_SEQ, R.CRAFTED_STEPS)
    assert bool(torch.isfinite(R.scaled(row, temperature)[torch.from_numpy(picks)].float()).all())
    # a kept token of probability p is missed by all N draws with probability (1 - p)^N < e^-20 for p >= 20 / N
    likely = np.nonzero(model.hi - model.lo >= 20.0 / picks.size)[0]
    assert set(likely.tolist()) <= set(picks.tolist())


# ---------------------------------------------------------------------------------------------------- arg-max
def _argmax_rows(V):
    g = torch.Generator().manual_seed(V)
    rows = ((torch.rand((12, V), generator=g, dtype=torch.float64) * 2 - 1) * 3).to(BF)
    last8 = (V - 1) // 8 * 8                      # first token of the last group of 8 (partial unless V % 8 == 0)
    rows[0, [min(777, V - 2), V - 1]] = 9.0       # exact tie: the lower index
    rows[1, V - 1] = 9.0
    rows[2, last8] = 9.0
    rows[3, [min(last8 + 1, V - 1), V - 1]] = 8.5
    rows[4] = 0                                   # distinct bf16 logits that the bf16 divide by 0.2 makes equal (8.8125):
    rows[4, 10], rows[4, 20] = 1.7578125, 1.765625        # the lower index there; at 1.7 they stay apart and 20 wins
    rows[5] = -float("inf")                       # nothing is greater than -inf: token 0
    rows[6, [0, V - 1]] = 9.0
    rows[7, 3072 * 8 if V > 3072 * 8 else 512] = 9.0      # the fourth 16-byte load of a thread's first pass
    rows[8, [85, 82]] = 9.0                       # a tie within one group of 8
    rows[9] = -1.5                                # all equal: token 0
    rows[10] = -float("inf")
    rows[10, V - 2] = -7.0
    rows[11, [V - 1, V - 9]] = 9.0
    return rows


@pytest.mark.parametrize("V,offset", [(1000, 0), (1000, 4), (1001, 0), (1004, 0), (32064, 0), (32064, 4), (128256, 0)])
def test_argmax(dev, V, offset):
    """top_k == 1 picks nonzero(l == l.max())[0] of l = bf16(logit / temperature).  V a multiple of 8 on 16-byte aligned rows
    takes the vector loads (V = 1000 too: its rows are 2000 bytes apart); V = 1001 and 1004, and rows that start 8 bytes into
    the allocation, take the scalar loop."""
    from dualhyp_amd import ops
    rows = _argmax_rows(V)
    n = rows.size(0)
    buf = torch.zeros(n * V + offset, dtype=BF, device=dev)
    lg = buf[offset:].view(n, V)
    lg.copy_(rows)
    assert lg.data_ptr() % 16 == (2 * offset) % 16
    for temperature in (0.2, 1.7):
        want = [R.argmax_ref(R.scaled(r, temperature)) for r in rows]
        # row 4: a tie only after the rounding of logit / temperature; an arg-max of the unrounded quotients would pick 20
        a, b = R.scaled(rows[4, [10, 20]], temperature).float().tolist()
        assert rows[4, 10].view(torch.int16).item() != rows[4, 20].view(torch.int16).item() and rows[4, 10] < rows[4, 20]
        assert (a == b == 8.8125 and want[4] == 10) if temperature == 0.2 else (a < b and want[4] == 20)
        tokens, length, done = _state(dev, n, 1)
        ops.sample(lg, tokens, length, done, temperature=temperature, top_k=1, seed=3, step=2)
        assert tokens.view(-1).tolist() == want, temperature
    assert want[0] == min(777, V - 2) and want[1] == V - 1 and want[5] == 0 and want[9] == 0 and want[10] == V - 2


# ---------------------------------------------------------------------------------------------------- side effects
def _planted(V, winners):
    rows = torch.full((len(winners), V), -2.0, dtype=BF)
    rows[torch.arange(len(winners)), torch.tensor(winners)] = 4.0
    return rows


@pytest.mark.parametrize("eos_id", [5, None])
def test_sample_state(dev, eos_id):
    """dh_sample_bf16's writes: finished rows keep tokens / length / done bit for bit; the EOS token is written and done = 1;
    length + 1 == tok_ld gives done = 2; length == tok_ld writes nothing; eos_id None never sets done = 1."""
    from dualhyp_amd import ops
    tok_ld, picks = 8, [100, 101, 5, 100, 42, 5, 42, 5]
    length0 = [3, 8, 2, 7, 8, 7, 0, 8]
    done0 = [1, 2, 0, 0, 0, 0, 0, 0]
    tokens, length, done = _state(dev, 8, tok_ld, length0, done0)
    tokens.copy_(-(torch.arange(8 * tok_ld).view(8, tok_ld) + 1000))
    t0 = tokens.cpu()
    ops.sample(_planted(256, picks).to(dev), tokens, length, done, temperature=0.8, top_k=1, eos_id=eos_id)
    t, n, d = R.expected_state(t0, length0, done0, picks, eos_id=eos_id)
    assert np.array_equal(tokens.cpu().numpy(), t) and length.tolist() == n.tolist() and done.tolist() == d.tolist()
    # the model's figures, spelled out
    assert length.tolist() == [3, 8, 3, 8, 8, 8, 1, 8]
    assert done.tolist() == ([1, 2, 1, 2, 2, 1, 0, 1] if eos_id == 5 else [1, 2, 0, 2, 2, 2, 0, 2])
    assert torch.equal(tokens.cpu()[[0, 1, 4, 7]], t0[[0, 1, 4, 7]])
    assert tokens[2, 2].item() == 5 and tokens[3, 7].item() == 100 and tokens[5, 7].item() == 5 and tokens[6, 0].item() == 42


def test_sample_refuses_bad_arguments(dev):
    from dualhyp_amd import ops
    from dualhyp_amd._lib import DualHypHipError
    lg = _planted(256, [1, 2]).to(dev)
    tokens, length, done = _state(dev, 2, 4)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1)):
        with pytest.raises(DualHypHipError):
            ops.sample(lg, tokens, length, done, **kw)
    assert length.tolist() == [0, 0] and done.tolist() == [0, 0] and bool((tokens == -1).all())


# ---------------------------------------------------------------------------------------------------- the row list
V_ROWS, TOP_K_ROWS, T_ROWS, MAX_NEW, TOK_LD = 1000, 50, 0.8, 5, 16
N_SEQ = 12
PLEN = [3, 4, 2, 5, 6, 1, 7, 12, 2, 3, 4, 5]     # prompt lengths of the 12 sequences of the call
GEN = [0, 2, 4, 1, 3, 2, 0, 3, 1, 0, 4, 2]       # tokens generated so far: the step of each sequence's draw
ROW_SEQ = [5, 2, 7, 3, 0, 3, -1, 3, 12]          # 9 rows. live: 5, 2, 7, 0 (permuted); three padding rows on finished 3; -1, n_seq
DONE0 = [0, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0, 0]


def _rows_setup(dev):
    g = torch.Generator().manual_seed(41)
    logits = (torch.randn((len(ROW_SEQ), V_ROWS), generator=g, dtype=torch.float64) * 4).to(BF)
    limit = [p + MAX_NEW for p in PLEN]          # sequence 7: 17 > TOK_LD, its budget is the buffer
    length0 = [p + n for p, n in zip(PLEN, GEN)]
    tokens, length, done = _state(dev, N_SEQ, TOK_LD, length0, DONE0)
    tokens.copy_(-(torch.arange(N_SEQ * TOK_LD).view(N_SEQ, TOK_LD) + 1000))
    return logits, torch.tensor(limit, dtype=torch.int32, device=dev), torch.tensor(ROW_SEQ, dtype=torch.int32, device=dev), \
        length0, tokens, length, done


def _live_rows():
    return [(r, u) for r, u in enumerate(ROW_SEQ) if 0 <= u < N_SEQ and not DONE0[u]]


def test_sample_rows(dev):
    """dh_sample_rows_bf16 directly: a permuted list of 9 rows over the 12 sequences of the call, sequences at different
    generated counts in one launch.  Each live row's pick is the model's at (seed, length - (limit - max_new), sequence) and what dh_sample_bf16
    gives for the same logits at that step and row; padding rows on a finished sequence, -1 and n_seq change nothing; sequences
    that no row names are untouched; done = 2 exactly when length reaches min(limit, tok_ld)."""
    from dualhyp_amd import ops
    seed = R.SEEDS[1]
    logits, limit, row_seq, length0, tokens, length, done = _rows_setup(dev)
    t0 = tokens.cpu()
    ops.sample_rows(logits.to(dev), tokens, length, done, limit, row_seq, MAX_NEW, temperature=T_ROWS, top_k=TOP_K_ROWS, seed=seed)
    got = tokens.cpu()
    picks = [0] * len(ROW_SEQ)
    for r, u in _live_rows():
        picks[r] = int(got[u, length0[u]])
        sc = R.scaled(logits[r], T_ROWS)
        model = R.RowModel(sc, TOP_K_ROWS)
        uu = R.u01(seed, GEN[u], u)
        reason, _ = R.check_pick(picks[r], sc, TOP_K_ROWS, uu, model)
        assert reason is None, f"row {r} -> sequence {u} at step {GEN[u]}: {reason}"
        if not model.ambiguous([uu])[0]:
            assert picks[r] == int(model.pick([uu])[0])
    t, n, d = R.expected_state(t0, length0, DONE0, picks, eos_id=None, limit=limit.cpu(), row_seq=ROW_SEQ)
    assert np.array_equal(got.numpy(), t) and length.tolist() == n.tolist() and done.tolist() == d.tolist()
    # the model's figures, spelled out: 2 reaches its limit of 7, 7 the end of the buffer; 1, 4, 6, 8-11 are named by no row
    assert length.tolist() == [4, 6, 7, 6, 9, 4, 7, 16, 3, 3, 8, 7] and done.tolist() == [0, 0, 2, 1, 0, 0, 0, 2, 0, 2, 0, 0]
    untouched = [1, 3, 4, 6, 8, 9, 10, 11]
    assert torch.equal(got[untouched], t0[untouched])
    # the same draws through dh_sample_bf16: logits row of sequence u at row u, step = its generated count
    by_seq = torch.zeros((N_SEQ, V_ROWS), dtype=BF)
    for r, u in _live_rows():
        by_seq[u] = logits[r]
    for step in sorted({GEN[u] for _, u in _live_rows()}):
        tok2, len2, done2 = _state(dev, N_SEQ, 1)
        ops.sample(by_seq.to(dev), tok2, len2, done2, temperature=T_ROWS, top_k=TOP_K_ROWS, seed=seed, step=step)
        for r, u in _live_rows():
            if GEN[u] == step:
                assert tok2[u, 0].item() == picks[r], (r, u, step)


def test_sample_rows_eos_and_argmax(dev):
    from dualhyp_amd import ops
    logits, limit, row_seq, length0, tokens, length, done = _rows_setup(dev)
    t0 = tokens.cpu()
    want = [R.argmax_ref(R.scaled(row, T_ROWS)) for row in logits]
    eos = want[0]                                 # row 0 -> sequence 5 ends on EOS; sequence 2 still spends its budget
    ops.sample_rows(logits.to(dev), tokens, length, done, limit, row_seq, MAX_NEW, temperature=T_ROWS, top_k=1, eos_id=eos)
    t, n, d = R.expected_state(t0, length0, DONE0, want, eos_id=eos, limit=limit.cpu(), row_seq=ROW_SEQ)
    assert np.array_equal(tokens.cpu().numpy(), t) and length.tolist() == n.tolist() and done.tolist() == d.tolist()
    assert done.tolist() == [0, 0, 2, 1, 0, 1, 0, 2, 0, 2, 0, 0] and tokens[5, length0[5]].item() == eos


def test_sample_rows_refuses_bad_arguments(dev):
    from dualhyp_amd import ops, _lib
    logits, limit, row_seq, length0, tokens, length, done = _rows_setup(dev)
    lg, t0 = logits.to(dev), tokens.clone()
    for max_new, kw in ((0, {}), (MAX_NEW, dict(temperature=0.0)), (MAX_NEW, dict(top_k=-1))):
        with pytest.raises(_lib.DualHypHipError):
            ops.sample_rows(lg, tokens, length, done, limit, row_seq, max_new, **kw)
    rc = _lib.load().dh_sample_rows_bf16(lg.data_ptr(), V_ROWS, tokens.data_ptr(), TOK_LD, length.data_ptr(), done.data_ptr(),
                                         None, row_seq.data_ptr(), len(ROW_SEQ), N_SEQ, MAX_NEW, 1.0, 0, -1, 0,
                                         torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.DualHypHipError):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(tokens, t0) and length.tolist() == length0 and done.tolist() == DONE0
