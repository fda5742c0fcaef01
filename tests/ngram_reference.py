"""Host model of no-repeat n-grams (include/dualhyp_hip.h, "No-repeat n-grams") and the histories of tests/test_hip_ngram.py.  CPU
only, plain Python; it imports neither the library nor dualhyp_amd.ngram, so the definition under test is held against this one.

The model is the definition read literally: walk every start i of an n-gram that lies whole in the generated text, compare its
first n - 1 tokens with the last n - 1 generated tokens, and ban what follows.  The reference of a banned pick is the UNMASKED
sampler (pinned by test_hip_sampling.py) on constrain_reference.substitute(rows, pick_rows(...)).
"""
from __future__ import annotations

import zlib
from typing import List, Optional, Sequence, Set, Tuple

import numpy as np


def banned(generated: Sequence[int], n: int) -> Set[int]:
    g = list(generated)
    m = len(g)
    out: Set[int] = set()
    if m < n:
        return out
    for i in range(0, m - n + 1):
        same = True
        for j in range(n - 1):
            if g[i + j] != g[m - n + 1 + j]:
                same = False
        if same:
            out.add(g[i + n - 1])
    return out


def pick_row(allowed_row: Optional[np.ndarray], generated: Sequence[int], n: int, vocab: int) -> Tuple[np.ndarray, bool]:
    """(bool [vocab]: the ids the step picks among, whether the fallback applied).  allowed_row None: no mask, every id."""
    base = np.ones(vocab, dtype=bool) if allowed_row is None else np.asarray(allowed_row[:vocab], dtype=bool).copy()
    row = base.copy()
    for t in banned(generated, n):
        if 0 <= t < vocab:
            row[t] = False
    if not row.any():
        return base, True
    return row, False


def pick_rows(allowed: Optional[np.ndarray], histories: Sequence[Sequence[int]], n: int, vocab: int) -> np.ndarray:
    """bool [len(histories), vocab]: pick_row of every sequence (allowed: bool [n_seq, vocab] or None)."""
    return np.stack([pick_row(None if allowed is None else allowed[u], h, n, vocab)[0] for u, h in enumerate(histories)])


def ban_positions(generated: Sequence[int], n: int) -> List[int]:
    g = list(generated)
    return [t for t in range(len(g)) if banned(g[:t], n)]


# ---- the histories of the op tests ------------------------------------------------------------------------------------------------
KINDS = ("short", "no_occurrence", "several_followers", "overlapping", "right_before", "adjacent", "prompt_only", "empty", "random",
         "every_id")


def history(kind: str, n: int, hot: Sequence[int], vocab: int, seed: int) -> Tuple[List[int], List[int]]:
    """(prompt, generated) of one kind for n-grams; `hot` are three ids the sampler is likely to pick (the raw row's largest), so that
    the bans move picks.  Every id is in [0, vocab), vocab >= 8.  The kinds are the hand-written cases of test_ngram_host.py at size."""
    r = np.random.default_rng(zlib.crc32(f"hist/{kind}/{n}/{vocab}/{seed}".encode()))
    a, b, c = (int(hot[i]) for i in range(3))
    others = [i for i in range(vocab) if i not in (a, b, c)]
    x, y, z = (int(others[int(v)]) for v in r.choice(len(others), 3, replace=False))
    suf = [x] * (n - 1)                                                # n = 1: the empty suffix, which every position matches
    if kind == "short":                                                # m = n - 1: no n-gram is complete
        return [a, b], [a] * (n - 1)
    if kind == "no_occurrence":                                        # m = n + 1 distinct tokens: the suffix occurs nowhere before
        if n == 1:                                                     # (n = 1 has no such text: one cold token)
            return [x, a], [y]
        pool = [a, b, c, x, y, z] + [i for i in others if i not in (x, y, z)]
        return [x, a], pool[:n + 1]
    if kind == "several_followers":                                    # the suffix before a, before b and before c, then once more
        return [z], suf + [a] + suf + [b] + [y] + suf + [c] + suf
    if kind == "overlapping":                                          # a a a a: occurrences that overlap each other and the suffix
        return [b], [a] * (n + 1)
    if kind == "right_before":                                         # m = n, the one candidate i = m - n = 0 ends on the last token
        return [c], [a] * n
    if kind == "adjacent":                                             # the occurrence and its follower end where the suffix starts
        return [c], [y] + suf + [a] + suf
    if kind == "prompt_only":                                          # the n-gram lies in the prompt, its first n - 1 tokens end the text
        if n == 1:
            return [a, b], []
        return suf + [a] + suf + [b], [y] + suf
    if kind == "empty":                                                # the first pick of a prompt
        return [a, b, c], []
    if kind == "random":                                               # a small alphabet: many occurrences
        al = [a, b, x]
        return [int(al[int(v)]) for v in r.integers(0, 3, 5)], [int(al[int(v)]) for v in r.integers(0, 3, 14)]
    if kind == "every_id":                                             # n = 1 at vocab 8: everything is banned, the fallback
        ids = list(range(min(vocab, 8)))
        return [a], ids + [int(v) for v in r.permutation(ids)]
    raise ValueError(kind)


def histories(n_seq: int, n: int, hot_of, vocab: int, offset: int = 0) -> Tuple[List[List[int]], List[List[int]]]:
    """Sequence u gets kind KINDS[(u + offset) % len(KINDS)] with the hot ids hot_of(u)."""
    ps, gs = [], []
    for u in range(n_seq):
        p, g = history(KINDS[(u + offset) % len(KINDS)], n, hot_of(u), vocab, u)
        ps.append(list(p))
        gs.append(list(g))
    return ps, gs
