"""Automaton constraints: the host side of the per-sequence DFAs the sampling kernels walk (include/dualhyp_hip.h, "Automaton
constraints").

An automaton set holds S states, numbered globally over all automata of a call, in CSR form: edge_off [S + 1], edge_tok [E] (strictly
ascending inside a state), edge_dst [E], and init [n_seq], each sequence's start state.  "This state may end the text" is an ordinary
edge on the call's eos_id.  At a pick, a sequence may produce the tokens on the edges of its state (and the EOS alone where that, under
a token mask, leaves nothing); the pick moves it along the edge.  The kernels build the allowed row and make the transition themselves
(csrc/sampling.hip); from_sequences and from_prompts build the two automata the correctors ask for, accepts and walk are the host model
the records and the tests use, and nothing else here touches the GPU.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

MAX_VOCAB = 131072          # the ids the sampler's LDS row holds
ORDERS = (2, 3, 4)          # from_prompts: the window lengths K
SPEC_REFUSAL = "a verify position's state would depend on the picks of its own step's earlier positions"
BEAM_REFUSAL = "a re-parented beam would have to take over its parent's state, which the selection does not carry"


def _ints(values, name: str) -> List[int]:
    if isinstance(values, torch.Tensor):
        values = values.reshape(-1).tolist()
    out = []
    for v in values:
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} holds ints, got {v!r}")
        out.append(v)
    return out


def check_automaton(edge_off, edge_tok, edge_dst, init, vocab: Optional[int] = None) -> Tuple[int, int, int]:
    """(S, E, n_seq) of the four arrays, checked as the C entries check them, each refusal naming its array: edge_off monotone from 0 to
    E; edge_tok in [0, vocab) (vocab None: only >= 0) and strictly ascending inside a state; edge_dst and init in [0, S); vocab at most
    131072."""
    edge_off, edge_tok, edge_dst, init = (_ints(a, n) for a, n in ((edge_off, "edge_off"), (edge_tok, "edge_tok"), (edge_dst, "edge_dst"),
                                                                  (init, "init")))
    if vocab is not None:
        if isinstance(vocab, bool) or not isinstance(vocab, int) or vocab < 1:
            raise ValueError(f"vocab is a positive int, got {vocab!r}")
        if vocab > MAX_VOCAB:
            raise ValueError(f"vocab: an automaton's allowed row is an LDS row of {MAX_VOCAB} ids; a vocab of {vocab} does not fit")
    S, E = len(edge_off) - 1, len(edge_tok)
    if S < 1:
        raise ValueError(f"edge_off: {len(edge_off)} offsets describe no state (S + 1 are needed, S >= 1)")
    if len(edge_dst) != E:
        raise ValueError(f"edge_dst: {len(edge_dst)} destinations for {E} edge tokens")
    if not init:
        raise ValueError("init: no sequence")
    if edge_off[0] != 0 or edge_off[S] != E:
        raise ValueError(f"edge_off: the offsets run from {edge_off[0]} to {edge_off[S]}, not from 0 to the {E} edges")
    for q in range(S):
        if not edge_off[q] <= edge_off[q + 1] <= E:
            raise ValueError(f"edge_off: not monotone at state {q} ({edge_off[q]}, then {edge_off[q + 1]}, of {E} edges)")
    for q in range(S):
        lo, hi = edge_off[q], edge_off[q + 1]
        for e in range(lo, hi):
            t = edge_tok[e]
            if t < 0 or (vocab is not None and t >= vocab):
                raise ValueError(f"edge_tok: state {q} has an edge on token {t}, outside [0, {vocab})")
            if e > lo and edge_tok[e - 1] >= t:
                raise ValueError(f"edge_tok: the tokens of state {q} are not strictly ascending ({edge_tok[e - 1]}, then {t})")
            if not 0 <= edge_dst[e] < S:
                raise ValueError(f"edge_dst: an edge of state {q} leads to state {edge_dst[e]}, outside the {S} states")
    for u, q in enumerate(init):
        if not 0 <= q < S:
            raise ValueError(f"init: sequence {u} starts in state {q}, outside the {S} states")
    return S, E, len(init)


class AutomatonSet:
    """The automaton set of one call: the four arrays as int32 CPU tensors (`edge_off`, `edge_tok`, `edge_dst`, `init`), which accepts
    and walk read, and, after to(device), their device copies (`d_edge_off`, ...) and `state`, the int32 [n_seq] buffer the kernels
    write and nobody initialises."""

    def __init__(self, edge_off, edge_tok, edge_dst, init, vocab: Optional[int] = None) -> None:
        self.n_states, self.n_edges, self.n_seq = check_automaton(edge_off, edge_tok, edge_dst, init, vocab)
        as_t = lambda a: a.detach().reshape(-1).to("cpu", torch.int32).contiguous() if isinstance(a, torch.Tensor) \
            else torch.tensor(list(a), dtype=torch.int32)
        self.edge_off, self.edge_tok, self.edge_dst, self.init = as_t(edge_off), as_t(edge_tok), as_t(edge_dst), as_t(init)
        self.max_tok = int(self.edge_tok.max()) if self.n_edges else -1
        self.device = None
        self.d_edge_off = self.d_edge_tok = self.d_edge_dst = self.d_init = self.state = None
        self._c = self._host = None

    def _shared(self, init) -> "AutomatonSet":
        """The same states and edges with another list of start states (the arrays are shared, not copied)."""
        other = AutomatonSet.__new__(AutomatonSet)
        other.__dict__.update(self.__dict__)
        init = torch.tensor(_ints(init, "init"), dtype=torch.int32)
        if init.numel() == 0 or int(init.min()) < 0 or int(init.max()) >= self.n_states:
            raise ValueError(f"init: start states outside the {self.n_states} states")
        other.init, other.n_seq = init, int(init.numel())
        other._c = other._host = other.state = other.d_init = None
        if self.device is not None:
            other.d_init = init.to(self.device)
            other.state = torch.empty(other.n_seq, dtype=torch.int32, device=self.device)
        return other

    def repeat(self, n: int) -> "AutomatonSet":
        """Sequence u * n + j starts where sequence u starts: the rows of sample_batch's n candidates per utterance."""
        return self._shared(self.init.repeat_interleave(int(n)))

    def padded(self) -> "AutomatonSet":
        """One sequence more, starting where sequence 0 starts: the dummy sequence of generate_stream's padding rows, which never picks."""
        return self._shared(torch.cat([self.init, self.init[:1]]))

    def to(self, device) -> "AutomatonSet":
        """This set with its arrays and a fresh state buffer on `device` (itself, when it is there already)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # "cuda" and "cuda:0" are one place: the state buffer must not fork
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device == device:
            return self
        other = AutomatonSet.__new__(AutomatonSet)
        other.__dict__.update(self.__dict__)
        other.device = device
        pad = lambda t: t if t.numel() else torch.zeros(1, dtype=torch.int32)      # never a null pointer for a set without edges
        other.d_edge_off, other.d_edge_tok = self.edge_off.to(device), pad(self.edge_tok).to(device)
        other.d_edge_dst, other.d_init = pad(self.edge_dst).to(device), self.init.to(device)
        other.state = torch.empty(self.n_seq, dtype=torch.int32, device=device)
        other._c = other._host = None
        return other

    def c_struct(self):
        """dh_automaton_spec of the device arrays and their host copies (all kept alive by this object)."""
        from . import _lib
        if self.device is None:
            raise _lib.DualHypHipError("the automaton set has no device arrays (AutomatonSet.to): the HIP path has no CPU fallback")
        if self._c is None:
            pad = lambda t: t if t.numel() else torch.zeros(1, dtype=torch.int32)
            self._host = (self.edge_off, pad(self.edge_tok), pad(self.edge_dst), self.init)
            self._c = _lib.AutomatonSpec(edge_off=self.d_edge_off.data_ptr(), edge_tok=self.d_edge_tok.data_ptr(),
                                         edge_dst=self.d_edge_dst.data_ptr(), init=self.d_init.data_ptr(), state=self.state.data_ptr(),
                                         h_edge_off=self._host[0].data_ptr(), h_edge_tok=self._host[1].data_ptr(),
                                         h_edge_dst=self._host[2].data_ptr(), h_init=self._host[3].data_ptr(), n_states=self.n_states,
                                         n_edges=self.n_edges, n_seq=self.n_seq)
        return self._c

    def edges(self, q: int) -> Dict[int, int]:
        """{token: destination} of state q."""
        lo, hi = int(self.edge_off[q]), int(self.edge_off[q + 1])
        return dict(zip(self.edge_tok[lo:hi].tolist(), self.edge_dst[lo:hi].tolist()))


def as_set(automaton, n_seq: int, vocab: int, device, eos_id) -> Optional[AutomatonSet]:
    """The `automaton=` argument of the generate functions and the sampling ops as an AutomatonSet on `device`, checked against the
    call, or None when it is off."""
    if automaton is None:
        return None
    if not isinstance(automaton, AutomatonSet):
        raise TypeError(f"automaton is a dualhyp_amd.automaton.AutomatonSet (from_sequences, from_prompts), not {automaton!r}")
    if eos_id is None or not 0 <= int(eos_id) < vocab:
        raise ValueError(f"an automaton needs an eos_id in [0, {vocab}), got {eos_id!r}: a dead end ends the sequence with it")
    if vocab > MAX_VOCAB:
        raise ValueError(f"an automaton's allowed row is an LDS row of {MAX_VOCAB} ids; a vocab of {vocab} does not fit")
    if automaton.max_tok >= vocab:
        raise ValueError(f"the automaton set has an edge on token {automaton.max_tok}, outside the vocabulary of {vocab}")
    if automaton.n_seq != n_seq:
        raise ValueError(f"the automaton set holds start states for {automaton.n_seq} sequences, the call has {n_seq}")
    return automaton.to(device)


def _pack(states: List[Dict[int, int]], init: List[int]) -> AutomatonSet:
    off, tok, dst = [0], [], []
    for edges in states:
        for t in sorted(edges):
            tok.append(t)
            dst.append(edges[t])
        off.append(len(tok))
    return AutomatonSet(off, tok, dst, init)


def _eos(eos_id) -> int:
    if isinstance(eos_id, bool) or not isinstance(eos_id, int) or eos_id < 0:
        raise ValueError(f"eos_id is a token id >= 0, got {eos_id!r}: a state that may end the text has an edge on it")
    return eos_id


def from_sequences(per_utterance_id_lists: Sequence[Sequence[Sequence[int]]], eos_id: int) -> AutomatonSet:
    """A trie per utterance over its listed id sequences, with an EOS edge wherever a listed sequence ends: the texts the automaton of
    utterance u accepts are exactly per_utterance_id_lists[u] ("select one of the n-best by generating it").  A sequence may be a prefix
    of another (its end state has the EOS edge and children), and may be empty; none holds the eos_id."""
    eos_id = _eos(eos_id)
    states: List[Dict[int, int]] = []
    init = []
    for u, seqs in enumerate(per_utterance_id_lists):
        if len(seqs) == 0:
            raise ValueError(f"utterance {u} lists no sequence: its automaton would accept nothing")
        root = len(states)
        states.append({})
        init.append(root)
        for seq in seqs:
            q = root
            for t in _ints(seq, f"utterance {u}'s sequences"):
                if t == eos_id or t < 0:
                    raise ValueError(f"utterance {u} lists a sequence holding {t}: ids are >= 0 and the eos_id ({eos_id}) ends a text")
                if t not in states[q]:
                    states[q][t] = len(states)
                    states.append({})
                q = states[q][t]
            states[q][eos_id] = q           # the destination of an EOS edge is ignored
    if not init:
        raise ValueError("from_sequences: no utterance")
    return _pack(states, init)


def from_prompts(prompts: Sequence, order: int = 2, eos_id: int = None) -> AutomatonSet:
    """The chain automaton of order K = `order` (2 .. 4) per prompt p: every run of K generated tokens is a run the prompt holds.  A state
    is the context c of the last min(m, K - 1) generated tokens; the empty context allows every distinct id of the prompt, a context of
    length j allows {p[i + j] : p[i .. i + j) == c}, and the next context is c + [t] cut to its last K - 1 tokens — a gram of the prompt
    by construction.  Every state has an EOS edge; an eos_id inside the prompt is that edge, not a continuation."""
    if isinstance(order, bool) or not isinstance(order, int) or order not in ORDERS:
        raise ValueError(f"order is the window length K, an int in {ORDERS[0]} .. {ORDERS[-1]}, got {order!r}")
    eos_id = _eos(eos_id)
    K = order
    states: List[Dict[int, int]] = []
    init = []
    for u, prompt in enumerate(prompts):
        p = _ints(prompt, f"prompt {u}")
        # follow[c] = the ids that follow the gram c in the prompt, for every gram of length 0 .. K - 1
        follow: Dict[Tuple[int, ...], set] = {(): set()}
        for j in range(K):
            for i in range(len(p) - j + 1):
                c = tuple(p[i:i + j])
                s = follow.setdefault(c, set())
                if i + j < len(p) and p[i + j] != eos_id:
                    s.add(p[i + j])
        index: Dict[Tuple[int, ...], int] = {}
        order_seen: List[Tuple[int, ...]] = []

        def state_of(c):
            if c not in index:
                index[c] = len(states) + len(order_seen)
                order_seen.append(c)
            return index[c]

        init.append(state_of(()))
        built = 0
        mine: List[Dict[int, int]] = []
        while built < len(order_seen):      # the contexts reachable from the empty one
            c = order_seen[built]
            built += 1
            edges = {t: state_of((c + (t,))[-(K - 1):]) for t in follow.get(c, ())}
            edges[eos_id] = index[c]
            mine.append(edges)
        states.extend(mine)
    if not init:
        raise ValueError("from_prompts: no prompt")
    return _pack(states, init)


def walk(aset: AutomatonSet, u: int, ids: Iterable[int]) -> List[int]:
    """The states sequence u passes through while it produces `ids`, its start state first (len(ids) + 1 of them), by the kernels'
    transition: along the state's edge on the id, and staying where the state has none."""
    q = int(aset.init[u])
    out = [q]
    for t in ids:
        q = aset.edges(q).get(int(t), q)
        out.append(q)
    return out


def accepts(aset: AutomatonSet, u: int, ids: Iterable[int], eos_id: int, complete: bool = True) -> bool:
    """True when sequence u's automaton accepts `ids` (the generated text, without its EOS): every id lies on an edge of the state it is
    produced in, and the last state has an EOS edge.  complete=False: the first condition alone — a text its budget cut short."""
    q = int(aset.init[u])
    for t in ids:
        edges = aset.edges(q)
        if int(t) == int(eos_id) or int(t) not in edges:
            return False
        q = edges[int(t)]
    return not complete or int(eos_id) in aset.edges(q)
