"""Host model of automaton constraints (include/dualhyp_hip.h, "Automaton constraints").  CPU only, plain Python and numpy; it imports
neither the library nor dualhyp_amd.automaton, so the definition under test is held against this one.

The model is the definition read literally, on the four CSR arrays as plain lists: the state at a pick, the allowed row (points 1 - 4,
the ban through ngram_reference.pick_row), the transition, acceptance, and a brute-force statement of the chain automaton's window
rule.  The reference of an automaton pick is the existing masked sampler under allowed_row.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import ngram_reference as NR


def edges_of(edge_off: Sequence[int], edge_tok: Sequence[int], edge_dst: Sequence[int], q: int) -> Dict[int, int]:
    return {int(edge_tok[e]): int(edge_dst[e]) for e in range(int(edge_off[q]), int(edge_off[q + 1]))}


def state_at(init: Sequence[int], state: Sequence[int], u: int, m: int) -> int:
    """the state sequence u is in behind m generated tokens"""
    return int(init[u]) if m == 0 else int(state[u])


def allowed_row(edge_off, edge_tok, q: int, vocab: int, eos_id: int, mask_row: Optional[np.ndarray] = None,
                generated: Sequence[int] = (), ngram: int = 0) -> Tuple[np.ndarray, bool, bool]:
    """(bool [vocab]: the ids the pick is taken among, dead end, the ban's fallback applied)"""
    r0 = np.zeros(vocab, dtype=bool)
    for e in range(int(edge_off[q]), int(edge_off[q + 1])):
        r0[int(edge_tok[e])] = True                                       # 1
    if mask_row is not None:
        r0 &= np.asarray(mask_row[:vocab], dtype=bool)                   # 2
    dead = not r0.any()
    if dead:                                                             # 3: the mask is ignored
        r0[:] = False
        r0[eos_id] = True
    if ngram:                                                            # 4
        row, fell = NR.pick_row(r0, generated, ngram, vocab)
        return row, dead, fell
    return r0, dead, False


def transition(edge_off, edge_tok, edge_dst, q: int, c: int) -> int:
    return edges_of(edge_off, edge_tok, edge_dst, q).get(int(c), int(q))


def walk(edge_off, edge_tok, edge_dst, q0: int, ids: Sequence[int]) -> List[int]:
    out = [int(q0)]
    for t in ids:
        out.append(transition(edge_off, edge_tok, edge_dst, out[-1], t))
    return out


def accepts(edge_off, edge_tok, edge_dst, q0: int, ids: Sequence[int], eos_id: int, complete: bool = True) -> bool:
    q = int(q0)
    for t in ids:
        e = edges_of(edge_off, edge_tok, edge_dst, q)
        if int(t) == eos_id or int(t) not in e:
            return False
        q = e[int(t)]
    return not complete or eos_id in edges_of(edge_off, edge_tok, edge_dst, q)


def window_accepts(prompt: Sequence[int], text: Sequence[int], K: int) -> bool:
    """the chain rule, by brute force: every run of up to K tokens that ends a prefix of `text` — all of the prefix while it is shorter
    than K — occurs in `prompt` as a contiguous run"""
    p, g = list(prompt), list(text)
    for n in range(len(g)):
        w = g[max(0, n - K + 1):n + 1]
        if not any(p[i:i + len(w)] == w for i in range(len(p) - len(w) + 1)):
            return False
    return True
