"""The host side of automaton constraints (dualhyp_amd/automaton.py; include/dualhyp_hip.h, "Automaton constraints"), on the CPU: the
two builders against statements of what they accept, the checks by name, and the --constrain chain flags."""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import automaton_reference as AR  # noqa: E402
from dualhyp_amd import automaton as A  # noqa: E402
from dualhyp_amd import inference as I  # noqa: E402

EOS = 7                     # outside the 7 ids of the texts


def arrays(aset):
    return aset.edge_off.tolist(), aset.edge_tok.tolist(), aset.edge_dst.tolist(), aset.init.tolist()


def well_formed(aset):
    off, tok, dst, init = arrays(aset)
    assert off[0] == 0 and off[-1] == len(tok) == len(dst) == aset.n_edges and len(off) == aset.n_states + 1
    for q in range(aset.n_states):
        assert off[q] <= off[q + 1]
        seg = tok[off[q]:off[q + 1]]
        assert all(a < b for a, b in zip(seg, seg[1:])), f"state {q}: {seg}"
    assert all(0 <= d < aset.n_states for d in dst) and all(0 <= q < aset.n_states for q in init)
    assert A.check_automaton(off, tok, dst, init, 8) == (aset.n_states, aset.n_edges, aset.n_seq)


def test_trie_accepts_exactly_the_listed_sequences():
    lists = [[[1, 2, 3], [1, 2], [1, 4], [5]],          # [1, 2] is a prefix of [1, 2, 3]: an EOS edge and a child
             [[0]],
             [[], [6, 6, 6]]]                            # the empty text is listed: the start state has the EOS edge
    aset = A.from_sequences(lists, EOS)
    well_formed(aset)
    assert aset.n_seq == 3
    off, tok, dst, init = arrays(aset)
    for u, seqs in enumerate(lists):
        listed = {tuple(s) for s in seqs}
        for n in range(0, 5):
            for text in itertools.product(range(7), repeat=n):
                want = text in listed
                assert A.accepts(aset, u, text, EOS) == want, (u, text)
                assert AR.accepts(off, tok, dst, init[u], text, EOS) == want, (u, text)
        # prefix acceptance: a text its budget cut short
        for s in seqs:
            for k in range(len(s) + 1):
                assert A.accepts(aset, u, s[:k], EOS, complete=False)
    q12 = A.walk(aset, 0, [1, 2])[-1]
    assert set(aset.edges(q12)) == {3, EOS}
    assert A.walk(aset, 0, [1, 2]) == AR.walk(off, tok, dst, init[0], [1, 2])
    assert A.walk(aset, 1, [3])[-1] == init[1]           # no edge: the kernels' transition stays
    with pytest.raises(ValueError, match="eos_id"):
        A.from_sequences([[[1, EOS]]], EOS)
    with pytest.raises(ValueError, match="no sequence"):
        A.from_sequences([[]], EOS)


def chain_prompts(K):
    r = np.random.default_rng(100 + K)
    lens = [1, 2, 40] + [int(v) for v in r.integers(1, 41, 3)]
    return [[int(t) for t in r.integers(0, 7, n)] for n in lens]


@pytest.mark.parametrize("K", (2, 3, 4))
def test_chain_automaton_is_the_window_rule(K):
    prompts = chain_prompts(K)
    aset = A.from_prompts(prompts, order=K, eos_id=EOS)
    well_formed(aset)
    off, tok, dst, init = arrays(aset)
    edges = [AR.edges_of(off, tok, dst, q) for q in range(aset.n_states)]
    assert all(EOS in e for e in edges)                  # every state may end the text
    accepted = rejected = 0
    for u, p in enumerate(prompts):
        occurs = lambda w: any(p[i:i + len(w)] == w for i in range(len(p) - len(w) + 1))
        # every text of up to 5 tokens over the 7 ids, a prefix before its extensions: (text, the automaton's state or None, the rule)
        level = [((), init[u], True)]
        for n in range(1, 6):
            nxt = []
            for text, q, ok in level:
                for t in range(7):
                    g = list(text) + [t]
                    rule = ok and occurs(g[max(0, len(g) - K):])
                    q2 = None if q is None else edges[q].get(t)
                    assert (q2 is not None) == rule, (K, u, p, g)
                    accepted += rule
                    rejected += not rule
                    nxt.append((tuple(g), q2, rule))
            level = nxt
        assert len(level) == 7 ** 5
        # the incremental statement above is the literal one, and the package's accepts is the model's
        r = np.random.default_rng(u)
        for text, q, ok in [level[int(i)] for i in r.integers(0, len(level), 200)] + [lv for lv in level if lv[2]][:50]:
            assert AR.window_accepts(p, text, K) == ok
            assert A.accepts(aset, u, text, EOS) == ok and A.accepts(aset, u, text, EOS, complete=False) == ok
        assert A.accepts(aset, u, p[:5], EOS)            # the prompt's own opening
    assert accepted > 0 and rejected > 0


def test_chain_automaton_takes_tensors_and_refuses_bad_orders():
    p = torch.tensor([3, 1, 3, 2], dtype=torch.int64)
    a = A.from_prompts([p], order=2, eos_id=EOS)
    b = A.from_prompts([p.tolist()], order=2, eos_id=EOS)
    assert arrays(a) == arrays(b)
    assert set(a.edges(int(a.init[0]))) == {1, 2, 3, EOS}
    after3 = A.walk(a, 0, [3])[-1]
    assert set(a.edges(after3)) == {1, 2, EOS}
    # an eos_id inside the prompt is the EOS edge, not a continuation
    c = A.from_prompts([[3, EOS, 2]], order=2, eos_id=EOS)
    assert set(c.edges(int(c.init[0]))) == {2, 3, EOS} and not A.accepts(c, 0, [3, EOS, 2], EOS)
    for bad in (1, 5, 2.0, True, None):
        with pytest.raises(ValueError, match="order"):
            A.from_prompts([[1, 2]], order=bad, eos_id=EOS)
    with pytest.raises(ValueError, match="eos_id"):
        A.from_prompts([[1, 2]], order=2, eos_id=None)
    # repeat / padded share the states and give every row a start state
    two = A.from_prompts([[1, 2], [3]], order=2, eos_id=EOS)
    assert two.repeat(3).init.tolist() == [two.init[0].item()] * 3 + [two.init[1].item()] * 3
    assert two.padded().init.tolist() == two.init.tolist() + [two.init[0].item()] and two.padded().n_seq == 3


def test_check_automaton_refuses_each_malformed_case_by_name():
    off, tok, dst, init = [0, 2, 3, 3], [1, 4, 0], [1, 2, 0], [0, 2]
    assert A.check_automaton(off, tok, dst, init, 5) == (3, 3, 2)
    cases = (("edge_off", dict(off=[1, 2, 3, 3])),                       # not from 0
             ("edge_off", dict(off=[0, 2, 3, 2])),                       # not to E
             ("edge_off", dict(off=[0, 3, 2, 3])),                       # not monotone
             ("edge_tok", dict(tok=[1, 5, 0])),                          # outside [0, vocab)
             ("edge_tok", dict(tok=[-1, 4, 0])),
             ("edge_tok", dict(tok=[4, 1, 0])),                          # not ascending
             ("edge_tok", dict(tok=[4, 4, 0])),                          # not strictly
             ("edge_dst", dict(dst=[1, 3, 0])),
             ("edge_dst", dict(dst=[-1, 2, 0])),
             ("edge_dst", dict(dst=[1, 2])),
             ("init", dict(init=[0, 3])),
             ("init", dict(init=[-1])),
             ("init", dict(init=[])),
             ("vocab", dict(vocab=131073)))
    for name, change in cases:
        kw = dict(off=off, tok=tok, dst=dst, init=init, vocab=5)
        kw.update(change)
        with pytest.raises(ValueError, match=name):
            A.check_automaton(kw["off"], kw["tok"], kw["dst"], kw["init"], kw["vocab"])
        if name != "vocab":
            with pytest.raises(ValueError, match=name):
                A.AutomatonSet(kw["off"], kw["tok"], kw["dst"], kw["init"], kw["vocab"])
    aset = A.AutomatonSet(off, tok, dst, init)
    # what depends on the call
    with pytest.raises(ValueError, match="eos_id"):
        A.as_set(aset, 2, 5, "cpu", None)
    with pytest.raises(ValueError, match="eos_id"):
        A.as_set(aset, 2, 5, "cpu", 5)
    with pytest.raises(ValueError, match="vocabulary"):
        A.as_set(aset, 2, 4, "cpu", 0)
    with pytest.raises(ValueError, match="131072"):
        A.as_set(aset, 2, 131073, "cpu", 0)
    with pytest.raises(ValueError, match="2 sequences"):
        A.as_set(aset, 3, 5, "cpu", 0)
    with pytest.raises(TypeError):
        A.as_set([off, tok, dst, init], 2, 5, "cpu", 0)
    assert A.as_set(None, 2, 5, "cpu", None) is None


def test_constrain_chain_flags(tmp_path):
    base = ["--test_path", "x.json", "--random_init"]
    a = I.parse_args(base)
    assert a.constrain == "off" and a.constrain_order == 2
    a = I.parse_args(base + ["--constrain", "chain"])
    assert a.constrain == "chain" and a.constrain_order == 2
    for K in (2, 3, 4):
        assert I.parse_args(base + ["--constrain", "chain", "--constrain_order", str(K)]).constrain_order == K
    for more in (["--schedule", "continuous"], ["--share_prefix", "auto"], ["--top_logprobs", "4"], ["--quantize", "fp8", "--kv_cache", "fp8"],
                 ["--no_repeat_ngram", "2"], ["--num_samples", "2", "--top_k", "5"]):
        assert I.parse_args(base + ["--constrain", "chain"] + more).constrain == "chain"
    extra = tmp_path / "extra.txt"
    extra.write_text("13\n")
    for more in (["--constrain_extra", str(extra)], ["--speculate", "3"], ["--num_beams", "2"], ["--constrain_order", "1"],
                 ["--constrain_order", "5"]):
        with pytest.raises(SystemExit):
            I.parse_args(base + ["--constrain", "chain"] + more)
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--constrain_order", "3"])                  # goes with --constrain chain
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--constrain", "prompt", "--constrain_order", "3"])
