"""Contextual biasing in the sampling kernels on the GPU (include/dualhyp_hip.h, "Contextual biasing").  Every check is exact.

ops.sample and ops.sample_rows with a bias must equal the same call WITHOUT one (and without penalties) on the copy of the logits
that tests/bias_reference.py builds on the host: the same tokens, length and done arrays.  The log-probabilities and alternatives are
those of the raw rows, and the logits tensor is bit-identical before and after the call.  tests/test_bias_host.py shows, by the
reference alone, that every fixture row changes its arg-max, so a kernel that ignored the bias would fail here."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bias_reference as BR  # noqa: E402
import constrain_reference as CR  # noqa: E402
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import bias as Bi  # noqa: E402
from dualhyp_amd import ops  # noqa: E402
from dualhyp_amd import stop as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
K = 3
VOCABS = (250, 256, 32000, 128256)
SAMPLERS = {
    "argmax": dict(temperature=0.7, top_k=1),
    "top50": dict(temperature=1.3, top_k=50, seed=99),
    "nucleus": dict(temperature=1.1, top_k=0, top_p=0.9, min_p=0.02, seed=7),
}
ENTRIES = [(list(ids), b) for ids, b in BR.ENTRIES]
ALL = PR.PENALTIES["all"]


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

    def picks(self, length):
        return [int(self.tokens[r, n]) for r, n in enumerate(length)]


@pytest.fixture(scope="module")
def data():
    """vocab -> (raw logits on the device, tokens, length, start, histories, the compiled bias); built once per vocab"""
    out = {}

    def get(vocab):
        if vocab not in out:
            bits, tokens, length = BR.fixture(vocab)
            lg = PR.tensor_of(bits, DEV).contiguous()
            out[vocab] = (lg, tokens, length, torch.tensor(BR.START, dtype=torch.int32, device=DEV), BR.histories(tokens, BR.START, length),
                          Bi.compile_bias(ENTRIES, vocab, DEV))
        return out[vocab]

    return get


def run_pair(lg, tokens, length, start, hist, sampler, bias, entries=BR.ENTRIES, pen={}, step=3, **more):
    """the biased call on the raw logits, and the plain call on the adjusted copy -> (got, want)"""
    before = lg.clone()
    got, want = State(tokens, length), State(tokens, length)
    ops.sample(lg, got.tokens, got.length, got.done, step=step, logprobs=got.lp, top_logprobs=got.top, start=start, bias=bias, **sampler, **pen,
               **more)
    adj = BR.adjusted_rows(lg, hist, entries, pen)
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


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("vocab", VOCABS)
def test_sample_equals_the_plain_call_on_the_adjusted_rows(data, vocab, sampler):
    lg, tokens, length, start, hist, bias = data(vocab)
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], bias)
    assert got.same_picks(want)
    assert got.length.tolist() == [n + 1 for n in length] and got.done.tolist() == [0] * BR.N_ROWS
    check_reports(lg, got, length)
    if sampler == "argmax":                     # every row the host test shows to flip, flipped
        plain = State(tokens, length)
        ops.sample(lg, plain.tokens, plain.length, plain.done, step=3, **SAMPLERS[sampler])
        assert plain.picks(length) == [BR.FLIPS[r][0] for r in range(BR.N_ROWS)]
        assert got.picks(length) == [BR.FLIPS[r][1] for r in range(BR.N_ROWS)]
        # a list of pairs is compiled by the call
        again = State(tokens, length)
        ops.sample(lg, again.tokens, again.length, again.done, step=3, start=start, bias=ENTRIES, **SAMPLERS[sampler])
        assert again.same_picks(got)


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("vocab", VOCABS)
def test_sample_rows_equals_the_plain_call_on_the_adjusted_rows(data, vocab, sampler):
    """the row-list sampler: logits row r belongs to sequence row_seq[r], in an order that is not the sequences'"""
    lg, tokens, length, start, hist, bias = data(vocab)
    kw = dict(SAMPLERS[sampler])
    max_new = 64
    limit = torch.tensor([s + max_new for s in BR.START], dtype=torch.int32, device=DEV)
    order = [4, 2, 0, 5, 3, 1]
    row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
    rows = lg[order].contiguous()
    before = rows.clone()
    got, want = State(tokens, length), State(tokens, length)
    ops.sample_rows(rows, got.tokens, got.length, got.done, limit, row_seq, max_new, logprobs=got.lp, top_logprobs=got.top, start=start, bias=bias,
                    **kw)
    adj = BR.adjusted_rows(rows, [hist[u] for u in order], BR.ENTRIES)
    ops.sample_rows(adj, want.tokens, want.length, want.done, limit, row_seq, max_new, logprobs=want.lp, top_logprobs=want.top, **kw)
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int16), before.view(torch.int16))
    assert got.same_picks(want) and got.length.tolist() == [n + 1 for n in length]
    check_reports(lg, got, length)
    if sampler == "argmax":
        assert got.picks(length) == [BR.FLIPS[r][1] for r in range(BR.N_ROWS)]


@pytest.mark.parametrize("vocab", (250, 32000))
def test_with_a_mask(data, vocab):
    lg, tokens, length, start, hist, bias = data(vocab)
    g = np.random.default_rng(3)
    allowed = g.random((BR.N_ROWS, vocab)) < 0.5
    allowed[:, [BR.TOP, BR.C, BR.D, BR.S, BR.Q, BR.DEEP[7]]] = True
    allowed[BR.ROW_PHRASE, BR.C] = False                        # the boosted id is disallowed: the row keeps its raw arg-max
    mask = CR.pack_bits(allowed).to(DEV)
    for sampler in ("argmax", "nucleus"):
        got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], bias, mask=mask)
        assert got.same_picks(want)
        assert all(allowed[r, t] for r, t in enumerate(got.picks(length)))
        check_reports(lg, got, length)
        if sampler == "argmax":
            assert got.picks(length)[BR.ROW_PHRASE] == BR.TOP and got.picks(length)[BR.ROW_DONE] == BR.D


@pytest.mark.parametrize("vocab", (256, 32000))
def test_with_no_repeat_ngram(data, vocab):
    lg, tokens, length, start, hist, bias = data(vocab)
    # ROW_REPEAT ends on r, which r has followed: under no_repeat_ngram = 2 the boosted r is banned; s is not
    assert hist[BR.ROW_REPEAT][-2:] == [BR.R, BR.R]
    for sampler in ("argmax", "top50"):
        got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], bias, no_repeat_ngram=2)
        assert got.same_picks(want)
        assert got.picks(length)[BR.ROW_REPEAT] != BR.R
        check_reports(lg, got, length)
    # a boost that would win, on the banned id
    strong = [([BR.R], 30.0)]
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS["argmax"], strong, entries=strong, no_repeat_ngram=2)
    assert got.same_picks(want)
    assert got.picks(length)[BR.ROW_REPEAT] == BR.TOP and got.picks(length)[BR.ROW_DONE] == BR.R


def test_with_a_stop_set(data):
    lg, tokens, length, start, hist, bias = data(32000)
    # the ids the biased arg-max flips to stop: the stop test sees the biased pick
    spec = S.as_spec([BR.C, [BR.P, BR.Q]], 32000, torch.device(DEV))
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS["argmax"], bias, stop=spec)
    assert got.same_picks(want)
    assert [int(v) for v in got.done] == [3 if r in (BR.ROW_PHRASE, BR.ROW_SIGNS) else 0 for r in range(BR.N_ROWS)]


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("vocab", VOCABS)
def test_with_all_three_penalties(data, vocab, sampler):
    """r is generated three times and proposed: its column holds bf16(z + B); s, c, d are proposed and never generated: no penalty"""
    lg, tokens, length, start, hist, bias = data(vocab)
    got, want = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], bias, pen=ALL)
    assert got.same_picks(want)
    check_reports(lg, got, length)
    only_pen, _ = run_pair(lg, tokens, length, start, hist, SAMPLERS[sampler], None, entries=(), pen=ALL)
    if sampler == "argmax":
        assert got.picks(length) == [BR.FLIPS[r][1] for r in range(BR.N_ROWS)]
        assert only_pen.picks(length) != got.picks(length)


@pytest.mark.parametrize("pen", ({}, ALL), ids=("bias", "bias+penalties"))
def test_a_history_longer_than_1024_tokens(pen):
    """1290 generated tokens: with penalties on, a quarter of the threads hold two history places' counts in registers while the table
    takes the boost keys; the phrase at the end of the history is matched at its last 2 and 7 places"""
    vocab, tok_ld, B = 32000, 1300, 2
    g = torch.Generator().manual_seed(17)
    lg = (torch.randn((B, vocab), generator=g) * 2.0).clamp_(max=6.0).to(torch.bfloat16)
    ids = torch.randperm(vocab - 200, generator=g)[:300] + 200
    lg[:, ids] += 3.0
    start = [5, 9]
    length = [tok_ld - 5, tok_ld - 1]
    tokens = torch.randint(0, vocab, (B, tok_ld), generator=g, dtype=torch.int64)
    for u in range(B):
        n = length[u] - start[u]
        tokens[u, start[u]:length[u]] = ids[torch.randint(0, 300, (n,), generator=g) % (100 + 200 * u)]
    tokens[0, length[0] - 2:length[0]] = torch.tensor([BR.A, BR.B])
    tokens[1, length[1] - 7:length[1]] = torch.tensor(BR.DEEP[:7])
    # a generated and often repeated id is proposed as well
    often = int(ids[0])
    entries = list(BR.ENTRIES) + [((often,), 2.5), ((BR.B, often), 1.25)]
    lg[:, list(BR.FIRST_IDS) + [often]] = 1.0               # what is proposed in every row stays low
    lg[:, BR.TOP] = 9.5                                     # the raw arg-max of both rows
    lg[0, BR.C], lg[1, BR.DEEP[7]] = 7.0, 6.5               # + 3 and + 5
    lg = lg.to(DEV).contiguous()
    hist = PR.histories(tokens, start, length)
    assert len(hist[0]) > 1024 and hist[0].count(often) > 1
    start_d = torch.tensor(start, dtype=torch.int32, device=DEV)
    for sampler in ("argmax", "nucleus"):
        got, want = run_pair(lg, tokens, length, start_d, hist, SAMPLERS[sampler], [(list(i), b) for i, b in entries], entries=entries, pen=pen)
        assert got.same_picks(want)
        check_reports(lg, got, length)
        if sampler == "argmax":
            assert got.picks(length) == [BR.C, BR.DEEP[7]]
            assert [PR.argmax_bits(PR.bits_of(lg[u])) for u in range(B)] != got.picks(length)


def test_a_full_table():
    """256 entries of 8 ids: every thread takes two (entry, depth) pairs"""
    vocab = 32000
    entries = BR.full_table(vocab)
    g = torch.Generator().manual_seed(29)
    B, tok_ld = 6, 48
    lg = (torch.randn((B, vocab), generator=g) * 2.0).clamp_(max=6.0).to(torch.bfloat16)
    tokens = torch.randint(0, vocab, (B, tok_ld), generator=g, dtype=torch.int64)
    start = [3] * B
    # (entry, how many of its ids were generated): the shared prefix of entries 0 / 1, the duplicates 2 / 3, depth 7, a whole phrase
    cases = [(0, 5), (2, 4), (200, 7), (255, 1), (17, 8), (100, 0)]
    length = []
    want_ids = []
    for u, (e, k) in enumerate(cases):
        ids = entries[e][0]
        tokens[u, start[u] + 2:start[u] + 2 + k] = torch.tensor(ids[:k], dtype=torch.int64)
        length.append(start[u] + 2 + k)
        if k < 8:
            lg[u, ids[k]] = 6.0                             # + at least 1: above every unboosted value ...
            want_ids.append(ids[k])
        else:
            want_ids.append(None)
    lg[0, entries[1][0][5]] = 6.0                           # ... entry 1 proposes another id behind the shared prefix, with a larger boost
    first = [ids[0] for ids, _ in entries]
    lg[:, first] = -4.0                                     # the 256 first ids, always proposed, stay low
    lg = lg.to(DEV).contiguous()
    hist = PR.histories(tokens, start, length)
    start_d = torch.tensor(start, dtype=torch.int32, device=DEV)
    spec = Bi.compile_bias([(list(i), b) for i, b in entries], vocab, DEV)
    for sampler in sorted(SAMPLERS):
        got, want = run_pair(lg, tokens, length, start_d, hist, SAMPLERS[sampler], spec, entries=entries)
        assert got.same_picks(want)
        check_reports(lg, got, length)
    got, _ = run_pair(lg, tokens, length, start_d, hist, SAMPLERS["argmax"], spec, entries=entries)
    picks = got.picks(length)
    assert picks[0] == entries[1][0][5] and picks[1:4] == want_ids[1:4]
    st = State(tokens, length)
    with pytest.raises(ValueError, match="2048"):           # with a penalty on, 48 places and 2048 ids do not fit the shared tables
        ops.sample(lg, st.tokens, st.length, st.done, start=start_d, bias=spec, **SAMPLERS["top50"], **ALL)
    torch.cuda.synchronize()
    assert st.length.tolist() == list(length)


@pytest.mark.parametrize("vocab", (250, 32000))
def test_a_null_or_empty_bias_is_the_call_without_the_keyword(data, vocab):
    lg, tokens, length, start, hist, bias = data(vocab)
    for sampler in sorted(SAMPLERS):
        plain = State(tokens, length)
        ops.sample(lg, plain.tokens, plain.length, plain.done, step=3, logprobs=plain.lp, top_logprobs=plain.top, **SAMPLERS[sampler])
        for off in (dict(bias=None), dict(bias=[]), dict(bias=())):
            got = State(tokens, length)
            ops.sample(lg, got.tokens, got.length, got.done, step=3, logprobs=got.lp, top_logprobs=got.top, **SAMPLERS[sampler], **off)
            assert got.same_picks(plain) and same_bits(got.lp, plain.lp) and torch.equal(got.top[0], plain.top[0]) and \
                same_bits(got.top[1], plain.top[1])


def test_refusals_leave_the_buffers_untouched(data):
    lg, tokens, length, start, hist, bias = data(256)
    st = State(tokens, length)
    keep = st.tokens.clone()
    with pytest.raises(ValueError, match="needs start"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, bias=bias)
    with pytest.raises(ValueError, match="id 256, outside"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, bias=[([256], 1.0)])
    with pytest.raises(ValueError, match="holds 9 ids"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, bias=[([1] * 9, 1.0)])
    with pytest.raises(ValueError, match="not a finite"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, bias=[([1], float("inf"))])
    with pytest.raises(ValueError, match="compiled for 32000"):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, bias=Bi.compile_bias(ENTRIES, 32000, DEV))
    with pytest.raises(TypeError):
        ops.sample(lg, st.tokens, st.length, st.done, top_k=1, start=start, bias="Ada")
    wide = torch.zeros((BR.N_ROWS, 2040), dtype=torch.int64, device=DEV)       # 2040 places + 25 ids, with a penalty on
    with pytest.raises(ValueError, match="2048"):
        ops.sample(lg, wide, st.length, st.done, top_k=1, start=start, bias=bias, presence_penalty=0.5)
    limit = torch.tensor([s + 8 for s in BR.START], dtype=torch.int32, device=DEV)
    row_seq = torch.arange(BR.N_ROWS, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="needs start"):
        ops.sample_rows(lg, st.tokens, st.length, st.done, limit, row_seq, 8, top_k=1, bias=bias)
    torch.cuda.synchronize()
    assert torch.equal(st.tokens, keep) and st.length.tolist() == list(length) and not bool(wide.any())
