"""Automaton constraints in the samplers on the GPU (include/dualhyp_hip.h, "Automaton constraints").  Every check is exact.

A pick under an automaton is the existing masked pick (ops.sample(mask=...), pinned by test_hip_constrain.py) under the row the host
model builds from the sequence's state (automaton_reference.allowed_row), and the state behind it is the host model's transition.  One
hand-built set holds the states the kernel can go wrong on: out-degree 0 (a dead end: the EOS alone), 1, 3 and 1 500 (more edges than
the block has threads; all but two ids at the smallest vocabulary), edges on token 0 and on token vocab - 1, and a state whose edges the
mask removes entirely.  The log-probabilities and alternatives are those of the raw rows."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import automaton_reference as AR  # noqa: E402
import constrain_reference as CR  # noqa: E402
from dualhyp_amd import _lib, ops  # noqa: E402
from dualhyp_amd import automaton as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
VOCABS = (65, 32000, 128256)         # a ragged last word; the 16-byte path; the largest production vocabulary
EOS = 1
TOK_LD = 12
K_TOP = 3
S_DEAD, S_ONE, S_THREE, S_BIG, S_ENDS, S_MASKED, S_EOS = range(7)
MAX_NEW = 8


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def hand_built(V):
    """(edge_off, edge_tok, edge_dst) of the seven states"""
    r = np.random.default_rng(V)
    big = sorted(int(t) for t in r.choice(np.arange(2, V), min(1500, V - 2), replace=False))
    states = [{},                                                        # S_DEAD
              {5: S_THREE},                                              # S_ONE
              {3: S_ONE, 9: S_BIG, 20: S_THREE},                         # S_THREE
              {t: t % 7 for t in big},                                   # S_BIG
              {0: S_ONE, V - 1: S_THREE},                                # S_ENDS: the first and the last id
              {7: S_ONE, 11: S_BIG},                                     # S_MASKED: the masks of the masked cases remove both
              {EOS: S_EOS, 30: S_ONE}]                                   # S_EOS: may end the text
    off, tok, dst = [0], [], []
    for e in states:
        for t in sorted(e):
            tok.append(t)
            dst.append(e[t])
        off.append(len(tok))
    return off, tok, dst


# (generated text, the state entry before the call, init, done): the text only feeds the ban, the penalties and the bias
SEQS = (([4, 6], S_DEAD, S_ONE, 0),            # a dead end: the EOS, done = 1, the state stays
        ([5, 5], S_ONE, S_THREE, 0),           # one edge; under ngram = 2 the ban would empty the row: the fallback
        ([3, 9, 3], S_THREE, S_ONE, 0),        # three edges; under ngram = 2 the ban removes 9
        ([8], S_BIG, S_ONE, 0),                # more edges than threads
        ([2, 2], S_ENDS, S_ONE, 0),            # token 0 and token vocab - 1
        ([6], S_MASKED, S_ONE, 0),             # under a mask: nothing left, the EOS alone, the mask ignored
        ([], S_ONE, S_THREE, 0),               # nothing generated: init is read, not the valid but wrong state entry
        ([3, 9], S_THREE, S_ONE, 1),           # finished: neither the tokens nor the state change
        ([], S_DEAD, S_ENDS, 0),
        ([30, 5, 3], S_EOS, S_ONE, 0),
        ([9], S_BIG, S_BIG, 0))
PROMPT = [40, 41]

_RAW = {}


def raw_rows(V):
    if V not in _RAW:
        g = torch.Generator().manual_seed(V)
        rows = (torch.randn(len(SEQS), V, generator=g) * 3).to(BF)
        rows[2, 9] = 40.0                      # the id the ban removes would win
        rows[5, EOS] = -20.0                   # the dead end's EOS is nobody's favourite
        _RAW[V] = rows
    return _RAW[V]


def buffers(seqs=SEQS):
    n = len(seqs)
    tokens = torch.full((n, TOK_LD), -1, dtype=torch.int64)
    for u, (g, _, _, _) in enumerate(seqs):
        tokens[u, :len(PROMPT) + len(g)] = torch.tensor(PROMPT + list(g), dtype=torch.int64)
    length = torch.tensor([len(PROMPT) + len(s[0]) for s in seqs], dtype=torch.int32)
    done = torch.tensor([s[3] for s in seqs], dtype=torch.int32)
    start = torch.full((n,), len(PROMPT), dtype=torch.int32)
    return tokens.to(DEV), length.to(DEV), done.to(DEV), start.to(DEV)


def out_bufs():
    shape = (len(SEQS), TOK_LD)
    return (torch.full(shape, NAN, dtype=torch.float32, device=DEV), torch.full(shape + (K_TOP,), -1, dtype=torch.int32, device=DEV),
            torch.full(shape + (K_TOP,), NAN, dtype=torch.float32, device=DEV))


def user_mask(V, kind):
    """bool [n, V] or None: a random half of the ids per sequence, S_MASKED's two ids and the EOS never among them"""
    if kind == "none":
        return None
    r = np.random.default_rng(V + 1)
    a = r.random((len(SEQS), V)) < 0.5
    a[:, [7, 11, EOS]] = False
    a[2, [3, 9, 20]] = True                    # the three-edge state keeps its edges: the ban case stays what it is
    a[1, 5] = True
    a[6, 3] = a[8, 0] = True                   # the two sequences that have generated nothing keep an edge of their start states
    return a


def pack_with_garbage(allowed):
    m = CR.pack_bits(allowed)
    V = allowed.shape[1]
    if V % 32:
        m[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)    # bits at and behind vocab: never allowed ids
    return m


def fresh_set(V):
    off, tok, dst = hand_built(V)
    aset = A.AutomatonSet(off, tok, dst, [s[2] for s in SEQS], V).to(DEV)
    aset.state.copy_(torch.tensor([s[1] for s in SEQS], dtype=torch.int32))
    return aset, (off, tok, dst)


def host_rows(arr, V, base, ngram):
    """(bool [n, V] the rows the picks are taken among, R0 of every sequence, dead ends, fallbacks)"""
    off, tok, _ = arr
    rows, r0s, dead, fell = [], [], 0, 0
    for u, (g, st, init, _) in enumerate(SEQS):
        q = AR.state_at([s[2] for s in SEQS], [s[1] for s in SEQS], u, len(g))
        row, d, f = AR.allowed_row(off, tok, q, V, EOS, None if base is None else base[u], g, ngram)
        r0s.append(AR.allowed_row(off, tok, q, V, EOS, None if base is None else base[u])[0])
        rows.append(row)
        dead += d
        fell += f
    return np.stack(rows), np.stack(r0s), dead, fell


def host_states(arr, picked):
    off, tok, dst = arr
    out = []
    for u, (g, st, init, fin) in enumerate(SEQS):
        q = AR.state_at([s[2] for s in SEQS], [s[1] for s in SEQS], u, len(g))
        out.append(st if fin else AR.transition(off, tok, dst, q, int(picked[u])))
    return out


def compare(got, lp, t_ids, t_lp, want, wlp, wt_ids, wt_lp, what):
    for x, y, name in zip(got[:3], want[:3], ("tokens", "length", "done")):
        assert torch.equal(x, y), f"{what}: {name}\n{x}\n{y}"
    assert same_bits(lp, wlp) and torch.equal(t_ids, wt_ids) and same_bits(t_lp, wt_lp), what


@pytest.mark.parametrize("top_k", (1, 4))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_is_the_masked_pick_under_the_state_row(V, top_k):
    raw = raw_rows(V).to(DEV)
    n = len(SEQS)
    kw = dict(temperature=0.7, top_k=top_k, eos_id=EOS, seed=99, step=3)
    for kind in ("none", "half"):
        base = user_mask(V, kind)
        m = None if base is None else pack_with_garbage(base).to(DEV)
        for ngram in (0, 2):
            aset, arr = fresh_set(V)
            rows, r0s, dead, fell = host_rows(arr, V, base, ngram)
            what = f"V={V} top_k={top_k} mask={kind} ngram={ngram}"
            assert dead >= (1 if base is None else 2), what        # S_DEAD, and S_MASKED under a mask
            if ngram:
                assert fell >= 1 and rows[2].sum() == r0s[2].sum() - 1 and not rows[2, 9], what
            assert rows[5, EOS] == (base is not None) and (base is None or not base[5, EOS])
            want = buffers()
            wlp, wt_ids, wt_lp = out_bufs()
            ops.sample(raw, *want[:3], logprobs=wlp, top_logprobs=(wt_ids, wt_lp), mask=CR.pack_bits(rows).to(DEV), **kw)
            got = buffers()
            lp, t_ids, t_lp = out_bufs()
            ops.sample(raw, *got[:3], logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m, no_repeat_ngram=ngram, start=got[3], automaton=aset,
                       **kw)
            compare(got, lp, t_ids, t_lp, want, wlp, wt_ids, wt_lp, what)
            picked = got[0][torch.arange(n), (got[1] - 1).long()].tolist()
            for u in range(n):
                assert SEQS[u][3] or rows[u, picked[u]], f"{what}: sequence {u} picked {picked[u]}"
            assert picked[0] == EOS and got[2][0].item() == 1 and picked[8] in (0, V - 1) and picked[6] in (3, 9, 20), what
            assert got[2][7].item() == 1 and got[1][7].item() == len(PROMPT) + 2
            assert aset.state.tolist() == host_states(arr, picked), what
            if ngram:       # the existing ban on the state's own row is the same pick
                w2 = buffers()
                ops.sample(raw, *w2[:3], mask=CR.pack_bits(r0s).to(DEV), no_repeat_ngram=ngram, start=w2[3], **kw)
                assert torch.equal(w2[0], got[0]), what


@pytest.mark.parametrize("top_k", (1, 4))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_rows_in_another_row_order(V, top_k):
    raw = raw_rows(V).to(DEV)
    n = len(SEQS)
    order = [9, 3, 7, 0, 10, 5, 1, 8, 2, 6, 4, 7]                  # every sequence, not in order; the finished one twice
    row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
    logits = raw[row_seq.long()].contiguous()
    kw = dict(temperature=0.7, top_k=top_k, eos_id=EOS, seed=99)
    for kind, ngram in (("none", 0), ("half", 2)):
        base = user_mask(V, kind)
        m = None if base is None else pack_with_garbage(base).to(DEV)
        aset, arr = fresh_set(V)
        rows, _, _, _ = host_rows(arr, V, base, ngram)
        what = f"V={V} top_k={top_k} mask={kind} ngram={ngram}"
        want = buffers()
        limit = (want[3] + MAX_NEW).contiguous()
        wlp, wt_ids, wt_lp = out_bufs()
        ops.sample_rows(logits, *want[:3], limit, row_seq, MAX_NEW, logprobs=wlp, top_logprobs=(wt_ids, wt_lp),
                        mask=CR.pack_bits(rows).to(DEV), **kw)
        got = buffers()
        lp, t_ids, t_lp = out_bufs()
        ops.sample_rows(logits, *got[:3], limit, row_seq, MAX_NEW, logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m, no_repeat_ngram=ngram,
                        start=got[3], automaton=aset, **kw)
        compare(got, lp, t_ids, t_lp, want, wlp, wt_ids, wt_lp, what)
        picked = got[0][torch.arange(n), (got[1] - 1).long()].tolist()
        assert aset.state.tolist() == host_states(arr, picked), what


@pytest.mark.parametrize("V", VOCABS)
def test_penalties_and_a_bias_work_on_the_state_row(V):
    """against the existing calls under the host's R0: the ban, the penalties and the bias are what they were, on another start row"""
    raw = raw_rows(V).to(DEV)
    n = len(SEQS)
    bias = [([3], 6.0), ([9, 20], -3.0), ([5], 2.5), ([30, 5], 4.0)]
    for top_k in (1, 4):
        for kind, ngram in (("none", 0), ("half", 2)):
            base = user_mask(V, kind)
            m = None if base is None else pack_with_garbage(base).to(DEV)
            aset, arr = fresh_set(V)
            _, r0s, _, _ = host_rows(arr, V, base, 0)
            kw = dict(temperature=0.7, top_k=top_k, eos_id=EOS, seed=5, step=2, no_repeat_ngram=ngram, repetition_penalty=1.5,
                      frequency_penalty=0.25, presence_penalty=-0.5, bias=bias)
            want = buffers()
            ops.sample(raw, *want[:3], mask=CR.pack_bits(r0s).to(DEV), start=want[3], **kw)
            got = buffers()
            ops.sample(raw, *got[:3], mask=m, start=got[3], automaton=aset, **kw)
            what = f"V={V} top_k={top_k} mask={kind} ngram={ngram}"
            for x, y, name in zip(got[:3], want[:3], ("tokens", "length", "done")):
                assert torch.equal(x, y), f"{what}: {name}\n{x}\n{y}"
            picked = got[0][torch.arange(n), (got[1] - 1).long()].tolist()
            assert aset.state.tolist() == host_states(arr, picked), what


def test_refusals_before_any_launch():
    V = 65
    raw = raw_rows(V).to(DEV)
    aset, _ = fresh_set(V)
    kw = dict(temperature=1.0, top_k=1, seed=1, step=0)

    def call(**more):
        b = buffers()
        args = dict(start=b[3], automaton=aset, eos_id=EOS)
        args.update(more)
        ops.sample(raw, *b[:3], **kw, **args)
        return b

    call()                                                             # the set itself is fine
    with pytest.raises(ValueError, match="eos_id"):
        call(eos_id=None)
    with pytest.raises(ValueError, match="eos_id"):
        call(eos_id=V)
    with pytest.raises(ValueError, match="start"):
        call(start=None)
    with pytest.raises(ValueError, match="sequences"):
        b = buffers(SEQS[:4])
        ops.sample(raw[:4], *b[:3], start=b[3], automaton=aset, eos_id=EOS, **kw)
    with pytest.raises(TypeError):
        call(automaton=[1, 2, 3])
    # the C entry's own checks, on the host copies: each is broken in place behind the Python checks, then mended
    for name, t, i, bad, msg in (("edge_tok", aset.edge_tok, 1, V, "outside the vocabulary"), ("edge_tok", aset.edge_tok, 3, 1, "ascending"),
                                 ("edge_dst", aset.edge_dst, 2, 7, "outside the 7 states"), ("init", aset.init, 4, -1, "starts in state"),
                                 ("edge_off", aset.edge_off, 2, 5, "monotone"), ("edge_off", aset.edge_off, 0, 1, "from 0"),
                                 ("edge_off", aset.edge_off, 7, 5, "from 0")):
        keep = int(t[i])
        t[i] = bad
        state = aset.state.clone()
        with pytest.raises(_lib.DualHypHipError, match=msg):
            call()
        t[i] = keep
        assert torch.equal(aset.state, state), name                      # nothing ran
    # eos_id < 0 at the C entry itself
    b = buffers()
    k = ops._Keep()
    logits, suffix, tail = ops._sample_tail(k, False, raw, b[0], None, None, None, 0, b[3], None, None, None, None, None, None, None, aset, EOS)
    assert suffix == "_automaton"
    rc = _lib.load().dh_sample_bf16_automaton(logits.data_ptr(), V, b[0].data_ptr(), TOK_LD, b[1].data_ptr(), b[2].data_ptr(), len(SEQS), 1.0, 1,
                                              -1, 1, 0, None, *tail)
    assert rc != 0 and "eos_id" in _lib.load().dh_last_error().decode()
    big = torch.zeros((len(SEQS), 131073), dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="131072"):
        b = buffers()
        ops.sample(big, *b[:3], start=b[3], automaton=aset, eos_id=EOS, **kw)
    call()
