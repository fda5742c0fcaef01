"""The exported sampling ladder on the GPU: dh_sample_bf16 and dh_sample_rows_bf16, each with its _ex, _top, _mask, _ngram, _stop,
_nucleus, _penalty and _bias entries, called directly with the full signature.  Every entry takes the options of the one before it and
adds its own behind them; called with what it adds switched off (null, top_p = 1, min_p = 0) it has to be the entry before it.  What
each call must leave in tokens / length / done comes from the host model of tests/sampling_reference.py, not from another entry, and
the comparison is exact.  The two entries that cannot be off: _mask refuses a null mask and gets an all-ones one; _ngram refuses
ngram = 0 and gets ngram = 8, which bans nothing while fewer than 8 tokens lie behind a prompt (the buffer holds 5).

The shapes are the smallest at which a wrapper can go wrong: 3 sequences of which one has finished, a vocabulary of 65 (no multiple of
32: a mask row is 3 words), logprobs and 2 alternatives on, and for the row list a permutation whose last row names the finished
sequence.  Nothing here provokes a refusal."""
import functools

import numpy as np
import pytest
import torch

import logprob_reference as L
import sampling_reference as R
import top_logprob_reference as T
from dualhyp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")

V, N_SEQ, TOK_LD, MAX_NEW, TOP_N = 65, 3, 6, 4, 2
MASK_LD = (V + 31) // 32
LENGTH = [2, 3, 1]
START = [1, 1, 1]                                # the prompt lengths; limit = start + MAX_NEW, so start is also limit - max_new
DONE = [0, 1, 0]                                 # sequence 1 has finished
ROW_SEQ = [2, 0, 1]                              # the row list: logits row r belongs to sequence ROW_SEQ[r]; row 2 names the finished one
SEED, STEP, TEMPERATURE = 5, 2, 0.7
TOP_KS = (1, 4)                                  # the arg-max, and a sampled draw
HEADS = tuple(_lib.SAMPLE_HEADS)
SUFFIXES = ("",) + tuple(s for s, _ in _lib.SAMPLE_TAIL)


@functools.lru_cache(maxsize=None)
def inputs():
    """(logits [3, 65] bf16, tokens [3, 6] int64 of valid ids), on the host; never written.  The generator's seed is one at which the
    sampled draw is not the arg-max (the test asserts it)."""
    g = torch.Generator().manual_seed(71)
    logits = (torch.randn((N_SEQ, V), generator=g, dtype=torch.float64) * 3).to(BF)
    tokens = torch.randint(0, V, (N_SEQ, TOK_LD), generator=g, dtype=torch.int64)
    return logits, tokens


@functools.lru_cache(maxsize=None)
def expected(rows: bool, top_k: int):
    """(tokens, length, done, {sequence: (logits row, place in the buffer, pick)} of the sequences that pick) by the host model.
    dh_sample_bf16 draws sequence u at (seed, step, u); the row list draws it at (seed, tokens generated so far, u)."""
    logits, tokens = inputs()
    seq_of = ROW_SEQ if rows else list(range(N_SEQ))
    picks, wrote = [], {}
    for r, u in enumerate(seq_of):
        sc = R.scaled(logits[r], TEMPERATURE)
        if top_k == 1:
            pick = R.argmax_ref(sc)
        else:
            uu = R.u01(SEED, LENGTH[u] - START[u] if rows else STEP, u)
            model = R.RowModel(sc, top_k)
            assert not model.ambiguous([uu])[0], "the inputs put a draw on an interval end: choose another generator seed"
            pick = int(model.pick([uu])[0])
        picks.append(pick)
        if not DONE[u]:
            wrote[u] = (r, LENGTH[u], pick)
    limit = [s + MAX_NEW for s in START] if rows else None
    t, n, d = R.expected_state(tokens, LENGTH, DONE, picks, eos_id=None, limit=limit, row_seq=ROW_SEQ if rows else None)
    return t, n, d, wrote


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("top_k", TOP_KS)
@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("head", HEADS)
def test_entry_with_its_options_off_is_the_host_model(head, suffix, top_k):
    rows = head == "dh_sample_rows_bf16"
    logits_h, tokens_h = inputs()
    logits, tokens = logits_h.to(DEV), tokens_h.to(DEV)
    length, done, start, limit, row_seq = _i32(LENGTH), _i32(DONE), _i32(START), _i32([s + MAX_NEW for s in START]), _i32(ROW_SEQ)
    lp = torch.full((N_SEQ, TOK_LD), NAN, dtype=torch.float32, device=DEV)
    top_ids = torch.full((N_SEQ, TOK_LD, TOP_N), -1, dtype=torch.int32, device=DEV)
    top_lp = torch.full((N_SEQ, TOK_LD, TOP_N), NAN, dtype=torch.float32, device=DEV)
    ones = torch.full((N_SEQ, MASK_LD), -1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    if rows:
        args = [logits.data_ptr(), V, tokens.data_ptr(), TOK_LD, length.data_ptr(), done.data_ptr(), limit.data_ptr(), row_seq.data_ptr(),
                len(ROW_SEQ), N_SEQ, MAX_NEW, TEMPERATURE, top_k, -1, SEED, stream]
    else:
        args = [logits.data_ptr(), V, tokens.data_ptr(), TOK_LD, length.data_ptr(), done.data_ptr(), N_SEQ, TEMPERATURE, top_k, -1, SEED, STEP,
                stream]
    # what each entry adds, off; a null mask keeps a mask_ld that nothing may read
    off = {"_ex": [lp.data_ptr()], "_top": [TOP_N, top_ids.data_ptr(), top_lp.data_ptr()], "_mask": [None, MASK_LD], "_ngram": [0, None],
           "_stop": [None], "_nucleus": [1.0, 0.0], "_penalty": [None], "_bias": [None]}
    if suffix == "_mask":
        off["_mask"] = [ones.data_ptr(), MASK_LD]
    if suffix == "_ngram":
        off["_ngram"] = [8, start.data_ptr()]
    for s in SUFFIXES[1:SUFFIXES.index(suffix) + 1]:
        args += off[s]
    assert len(args) == len(_lib.SIGNATURES[head + suffix][1])
    _lib.check(getattr(_lib.load(), head + suffix)(*args))

    want_t, want_n, want_d, wrote = expected(rows, top_k)
    assert np.array_equal(tokens.cpu().numpy(), want_t) and length.tolist() == want_n.tolist() and done.tolist() == want_d.tolist()
    assert sorted(wrote) == [0, 2] and bool((logits == logits_h.to(DEV)).all())
    if top_k != 1:
        assert wrote != expected(rows, 1)[3], "the sampled draw's picks are the arg-max's: it would pin nothing of its own"
    # the log-probabilities: tests/test_hip_logprobs.py's reference and gate, |got - ref64| <= 2e-5 + 2.4e-7 |ref64|; the alternatives:
    # tests/test_hip_top_logprobs.py's reference ids, exactly, and that gate on each one's value; nothing else is written
    written = torch.zeros((N_SEQ, TOK_LD), dtype=torch.bool, device=DEV)
    for u, (r, n, pick) in wrote.items():
        written[u, n] = True
        if suffix:
            ref = L.logprobs64(logits_h[r:r + 1], [pick])
            assert L.within_gate(lp[u, n:n + 1].cpu().numpy(), ref).all(), (u, lp[u, n].item(), ref)
        if suffix not in ("", "_ex"):
            ids = T.top_ids(logits_h[r:r + 1], TOP_N)[0]
            assert top_ids[u, n].cpu().tolist() == ids.tolist(), u
            ref = L.logprobs64(logits_h[r:r + 1].expand(TOP_N, V), ids.tolist())
            assert L.within_gate(top_lp[u, n].cpu().numpy(), ref).all(), (u, top_lp[u, n].tolist(), ref)
    if not suffix:
        written[:] = False
    assert bool(torch.isnan(lp[~written]).all())
    if suffix in ("", "_ex"):
        written[:] = False
    assert bool((top_ids[~written] == -1).all()) and bool(torch.isnan(top_lp[~written]).all())
