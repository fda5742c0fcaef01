"""Penalties in the sampling kernels on the GPU (include/dualhyp_hip.h, "Penalties").  Every check is exact.

ops.sample and ops.sample_rows with penalties must equal the same call WITHOUT penalties on the copy of the logits that
tests/penalty_reference.py builds on the host: the same tokens, length and done arrays.  The log-probabilities and alternatives are
those of the raw rows, and the logits tensor is bit-identical before and after the call.  tests/test_penalty_host.py shows, by the
reference alone, that the fixture rows marked "flips" change their arg-max, so a kernel that ignored the penalties would fail here."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import ops  # noqa: E402
from dualhyp_amd import stop as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
K = 3
VOCABS = (250, 256, 32000, 128256)
SAMPLERS = {
    "argmax": dict(temperature=0.7, top_k=1),
    "top5": dict(temperature=1.3, top_k=5, seed=99),
    "nucleus": dict(temperature=1.1, top_k=40, top_p=0.9, min_p=0.05, seed=7),
}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class State:
    """tokens / length / done and the report buffers of one call, on the device"""

    def __init__(self, tokens, length):
        self.tokens = tokens.to(DEV).contiguous()
        self.length = torch.tensor(length, dtype=torch.int32, device=DEV)
        self.done = torch.zeros(len(length), dtype=torch.int32, device=DEV)
        shape = tuple(self.tokens.shape)
        self.lp = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
        self.top = (torch.full(shape + (K,), -1, dtype=torch.int32, device=DEV), torch.full(shape + (K,), NAN, dtype=torch.float32, device=DEV))

    def same_picks(self, o):
        return torch.equal(self.tokens, o.tokens) and torch.equal(self.length, o.length) and torch.equal(self.done, o.done)


@pytest.fixture(scope="module")
def data():
    """vocab -> (raw logits on the device, tokens, length, start, histories); built once per vocab"""
    out = {}

    def get(vocab):
        if vocab not in out:
            bits, tokens, length = PR.fixture(vocab)
            lg = PR.tensor_of(bits, DEV).contiguous()
            out[vocab] = (lg, tokens, length, torch.tensor(PR.START, dtype=torch.int32, device=DEV), PR.histories(tokens, PR.START, length))
        return out[vocab]

    return get


def run_pair(lg, tokens, length, start, hist, sampler, pen, step=3, **more):
    """the penalised call on the raw logits, and the plain call on the adjusted copy -> (got, want, the raw logits' bits before)"""
    before = lg.clone()
    got, want = State(tokens, length), State(tokens, length)
    ops.sample(lg, got.tokens, got.length, got.done, step=step, logprobs=got.lp, top_logprobs=got.top, start=start, **sampler, **pen, **more)
    adj = PR.adjusted_rows(lg, hist, pen)
    # `start` goes with a control that reads the history; the plain call may have none
    wstart = start if more.get("no_repeat_ngram") or (more.get("stop") is not None and more["stop"].sequences) else None
    ops.sample(adj, want.tokens, want.length, want.done, step=step, logprobs=want.lp, top_logprobs=want.top, start=wstart, **sampler, **more)
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int16), before.view(torch.int16)), "the logits were written"
    return got, want


def check_reports(lg, got, length):
    """log-probabilities and alternatives are the raw rows'"""
    rows = torch.arange(len(length), device=DEV)
    at = torch.tensor(length, device=DEV)
    picked = got.tokens[rows, at]
    assert same_bits(got.lp[rows, at], ops.token_logprobs(lg, picked))
    ids, lp = ops.token_top_logprobs(lg, K)
    assert torch.equal(got.top[0][rows, at], ids) and same_bits(got.top[1][rows, at], lp)


@pytest.mark.parametrize("name", sorted(PR.PENALTIES))
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("vocab", VOCABS)
def test_sample_equals_the_plain_call_on_the_adjusted_rows(data, vocab, sampler, name):
    lg, tokens, length, start, hist = data(vocab)
    pen = PR.PENALTIES[name]
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], pen)
    assert got.same_picks(want)
    assert got.length.tolist() == [n + 1 for n in length]
    assert int(got.done[PR.ROW_FULL]) == 2 and got.done[:PR.ROW_FULL].tolist() == [0] * PR.ROW_FULL      # the full row spent its buffer
    check_reports(lg, got, length)
    if sampler == "argmax":                     # the rows the host test shows to flip, flipped; the empty history is the plain pick
        plain = State(tokens, length)
        ops.sample(lg, plain.tokens, plain.length, plain.done, step=3, **SAMPLERS[sampler])
        picks = lambda s: [int(s.tokens[r, length[r]]) for r in range(PR.N_ROWS)]      # noqa: E731
        for r in PR.FLIPS[name]:
            assert picks(plain)[r] == PR.TOP and picks(got)[r] == PR.RUNNER
        assert picks(plain)[PR.ROW_EMPTY] == picks(got)[PR.ROW_EMPTY]


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("vocab", VOCABS)
def test_sample_rows_equals_the_plain_call_on_the_adjusted_rows(data, vocab, sampler):
    """the row-list sampler: logits row r belongs to sequence row_seq[r], in an order that is not the sequences'"""
    lg, tokens, length, start, hist = data(vocab)
    kw = {k: v for k, v in SAMPLERS[sampler].items()}
    pen = PR.PENALTIES["all"]
    max_new = 64
    limit = torch.tensor([s + max_new for s in PR.START], dtype=torch.int32, device=DEV)
    order = [4, 2, 0, 5, 3, 1]
    row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
    rows = lg[order].contiguous()
    before = rows.clone()
    got, want = State(tokens, length), State(tokens, length)
    ops.sample_rows(rows, got.tokens, got.length, got.done, limit, row_seq, max_new, logprobs=got.lp, top_logprobs=got.top, start=start, **kw, **pen)
    adj = PR.adjusted_rows(rows, [hist[u] for u in order], pen)
    ops.sample_rows(adj, want.tokens, want.length, want.done, limit, row_seq, max_new, logprobs=want.lp, top_logprobs=want.top, **kw)
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int16), before.view(torch.int16))
    assert got.same_picks(want) and got.length.tolist() == [n + 1 for n in length]
    check_reports(lg, got, length)


@pytest.mark.parametrize("sampler", ("argmax", "nucleus"))
def test_a_history_longer_than_the_block(sampler):
    """1290 generated tokens over 300 distinct ids: a quarter of the 1024 threads take a second token, and the counts differ"""
    vocab, tok_ld, B = 32000, 1300, 2
    g = torch.Generator().manual_seed(17)
    lg = (torch.randn((B, vocab), generator=g) * 2.0).clamp_(max=6.0).to(torch.bfloat16)
    ids = torch.randperm(vocab, generator=g)[:300]
    lg[:, ids] += 3.0                                            # the repeated ids are the likely ones: the penalties decide the pick
    lg = lg.to(DEV).contiguous()
    start = [5, 9]
    length = [tok_ld - 5, tok_ld - 1]
    tokens = torch.randint(0, vocab, (B, tok_ld), generator=g, dtype=torch.int64)
    for u in range(B):
        n = length[u] - start[u]
        tokens[u, start[u]:length[u]] = ids[torch.randint(0, 300, (n,), generator=g) % (100 + 200 * u)]
    hist = PR.histories(tokens, start, length)
    assert len(hist[0]) > 1024 and max(PR.counts(hist[0]).values()) > min(PR.counts(hist[0]).values())
    start_d = torch.tensor(start, dtype=torch.int32, device=DEV)
    for name in ("frequency", "all"):
        got, want = run_pair(lg, tokens, length, start_d, hist, SAMPLERS[sampler], PR.PENALTIES[name])
        assert got.same_picks(want)
        check_reports(lg, got, length)
        if sampler == "argmax":
            raw = [PR.argmax_bits(PR.bits_of(lg[u])) for u in range(B)]
            assert [int(got.tokens[u, length[u]]) for u in range(B)] != raw


def test_with_a_mask(data):
    lg, tokens, length, start, hist = data(32000)
    g = np.random.default_rng(3)
    allowed = g.random((PR.N_ROWS, 32000)) < 0.5
    allowed[:, PR.RUNNER] = True
    allowed[PR.ROW_COUNT, PR.RUNNER] = False                    # the flip has to go further down
    mask = CR.pack_bits(allowed).to(DEV)
    for sampler in ("argmax", "nucleus"):
        got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], PR.PENALTIES["all"], mask=mask)
        assert got.same_picks(want)
        assert all(allowed[r, int(got.tokens[r, length[r]])] for r in range(PR.N_ROWS))
        check_reports(lg, got, length)


def test_with_no_repeat_ngram(data):
    lg, tokens, length, start, hist = data(32000)
    # ROW_COUNT ends on FILLER[3], which FILLER[3] and TOP have followed: both are banned, the penalised columns among them
    assert hist[PR.ROW_COUNT][-1] == PR.FILLER[3]
    for sampler in ("argmax", "top5"):
        got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], PR.PENALTIES["all"], no_repeat_ngram=2)
        assert got.same_picks(want)
        assert int(got.tokens[PR.ROW_COUNT, length[PR.ROW_COUNT]]) not in (PR.TOP, PR.FILLER[3])
        check_reports(lg, got, length)


def test_with_a_stop_set(data):
    lg, tokens, length, start, hist = data(32000)
    # the id the penalised arg-max flips to stops: the stop test sees the penalised pick
    spec = S.as_spec([PR.RUNNER, [PR.FILLER[2], PR.RUNNER]], 32000, torch.device(DEV))
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS["argmax"], PR.PENALTIES["all"], stop=spec)
    assert got.same_picks(want)
    assert int(got.done[PR.ROW_ARGMAX]) == 3 and int(got.done[PR.ROW_COUNT]) == 3 and int(got.done[PR.ROW_EMPTY]) == 0


@pytest.mark.parametrize("vocab", (250, 32000))
def test_off_values_are_the_call_without_the_keywords(data, vocab):
    lg, tokens, length, start, hist = data(vocab)
    for sampler in sorted(SAMPLERS):
        plain = State(tokens, length)
        ops.sample(lg, plain.tokens, plain.length, plain.done, step=3, logprobs=plain.lp, top_logprobs=plain.top, **SAMPLERS[sampler])
        for off in (dict(repetition_penalty=1.0), dict(frequency_penalty=0.0), dict(presence_penalty=0.0),
                    dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0),
                    dict(repetition_penalty=None, frequency_penalty=None, presence_penalty=None)):
            got = State(tokens, length)
            ops.sample(lg, got.tokens, got.length, got.done, step=3, logprobs=got.lp, top_logprobs=got.top, **SAMPLERS[sampler], **off)
            assert got.same_picks(plain) and same_bits(got.lp, plain.lp) and torch.equal(got.top[0], plain.top[0]) and \
                same_bits(got.top[1], plain.top[1])


def test_refusals_leave_the_buffers_untouched(data):
    lg, tokens, length, start, hist = data(256)
    st = State(tokens, length)
    keep = st.tokens.clone()
    with pytest.raises(ValueError, match="need start"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="not in"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, frequency_penalty=8.5)
    with pytest.raises(TypeError):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, presence_penalty=True)
    wide = torch.zeros((PR.N_ROWS, 2049), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="2048"):
        ops.sample(lg, wide, st.length, st.done, top_k=1, start=start, presence_penalty=0.5)
    torch.cuda.synchronize()
    assert torch.equal(st.tokens, keep) and st.length.tolist() == list(length) and not bool(wide.any())
