"""Host model of contextual biasing (include/dualhyp_hip.h, "Contextual biasing") and the fixtures the bias tests share.  It knows
nothing of the device code: the proposals are matched on Python lists, an id's boost is the largest of its proposers' by an
order-preserving integer key of the float32, and bf16(y + B) is one numpy float32 addition rounded to bf16 with integer arithmetic on
the bits (tests/penalty_reference.py).

adjusted_row(row, history, entries, theta, alpha_f, alpha_p) is the copy of a logits row on which the existing call, with neither a
bias nor a penalty, must make the biased (and penalised) call's pick.
"""
from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import penalty_reference as PR  # noqa: E402

Entry = Tuple[Sequence[int], float]


def boost_key(b: float) -> int:
    """the order-preserving unsigned key of a float32: a < b  <=>  key(a) < key(b) (-0 below +0)"""
    u = int(np.array([b], dtype=np.float32).view(np.uint32)[0])
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def key_boost(k: int) -> np.float32:
    u = k ^ 0x80000000 if k & 0x80000000 else (~k) & 0xFFFFFFFF
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def proposed(generated: Sequence[int], entries: Sequence[Entry]) -> Dict[int, np.float32]:
    """{id: B_id} at the pick behind `generated`: entry e proposes ids[k] when k <= m and the last k generated tokens are ids[:k]"""
    g = [int(t) for t in generated]
    m = len(g)
    keys: Dict[int, int] = {}
    for ids, boost in entries:
        ids = [int(t) for t in ids]
        for k in range(len(ids)):
            if k <= m and g[m - k:m] == ids[:k]:
                keys[ids[k]] = max(keys.get(ids[k], 0), boost_key(boost))
    return {t: key_boost(k) for t, k in keys.items()}


def penalised_z(bits: int, c: int, theta: float, alpha_f: float, alpha_p: float) -> np.float32:
    """z of "Penalties": the fp32 value in front of a_t's bf16 rounding (PR.adjusted_value without its last step)"""
    th, af, ap = np.float32(theta), np.float32(alpha_f), np.float32(alpha_p)
    x = PR.f32_of_bits([bits])[0]
    with np.errstate(all="ignore"):
        y = np.float32(x * th) if x < 0 else np.float32(x / th)
        p = np.float32(af * np.float32(c))
        return np.float32(np.float32(y - p) - ap)


def boosted_value(y: np.float32, boost) -> int:
    """bf16(y + B) as bits: one fp32 add, then round to nearest even"""
    with np.errstate(all="ignore"):
        return int(PR.bf16_bits(np.float32(np.float32(y) + np.float32(boost)))[0])


def adjusted_bits(row_bits: np.ndarray, history: Sequence[int], entries: Sequence[Entry], theta: float = 1.0, alpha_f: float = 0.0,
                  alpha_p: float = 0.0) -> np.ndarray:
    """the row's bf16 bits as the pick sees them: a_t in the columns of the penalised history, bf16(y + B_t) in the proposed ones"""
    pen_on = theta != 1.0 or alpha_f != 0.0 or alpha_p != 0.0
    out = PR.adjusted_bits(row_bits, history, theta, alpha_f, alpha_p) if pen_on else np.array(row_bits, dtype=np.uint16, copy=True)
    cnt = PR.counts(history) if pen_on else {}
    for t, b in proposed(history, entries).items():
        if 0 <= t < out.size:
            raw = int(row_bits[t])
            y = penalised_z(raw, cnt[t], theta, alpha_f, alpha_p) if cnt.get(t, 0) > 0 else PR.f32_of_bits([raw])[0]
            out[t] = boosted_value(y, b)
    return out


def adjusted_row(row_bf16: torch.Tensor, history: Sequence[int], entries: Sequence[Entry], theta: float = 1.0, alpha_f: float = 0.0,
                 alpha_p: float = 0.0) -> torch.Tensor:
    assert row_bf16.dtype == torch.bfloat16 and row_bf16.dim() == 1
    return PR.tensor_of(adjusted_bits(PR.bits_of(row_bf16), history, entries, theta, alpha_f, alpha_p), row_bf16.device)


def adjusted_rows(logits: torch.Tensor, histories: Sequence[Sequence[int]], entries: Sequence[Entry], pen: Dict[str, float] = {}) -> torch.Tensor:
    """adjusted_row over the rows of a [rows, vocab] tensor; pen holds the sampling ops' penalty keywords (none: off)"""
    th, af, ap = pen.get("repetition_penalty", 1.0), pen.get("frequency_penalty", 0.0), pen.get("presence_penalty", 0.0)
    return torch.stack([adjusted_row(logits[r], h, entries, th, af, ap) for r, h in enumerate(histories)]).contiguous()


def hits(generated: Sequence[int], entries: Sequence[Entry]) -> int:
    """the generated tokens that were proposed at a depth >= 1 when they were picked"""
    g = [int(t) for t in generated]
    n = 0
    for i, t in enumerate(g):
        deep = any(1 <= k <= i and g[i - k:i] == [int(v) for v in ids[:k]] and int(ids[k]) == t
                   for ids, _ in entries for k in range(1, len(ids)))
        n += bool(deep)
    return n


# ---- the kernel-level fixture -----------------------------------------------------------------------------------------------------------
A, B, C, D = 60, 61, 62, 63                 # the overlapping phrases a b c and b c d
R, S = 70, 71                               # the phrase with a repeated id, r r s
DEEP = tuple(range(80, 88))                 # the 8-id entry
P, Q = 90, 91                               # q is proposed by a one-id entry (negative) and by p q (positive): the maximum wins
NINF, TIE, ODD = 100, 101, 102              # one-id entries on special raw values
ENTRIES: Tuple[Entry, ...] = (
    ((A, B, C), 3.0),
    ((B, C, D), 2.0),
    ((R, R, S), 3.5),
    (DEEP, 5.0),
    ((Q,), -6.0),
    ((P, Q), 3.0),
    ((NINF,), 1.0),
    ((TIE,), 2.0 ** -8),                    # 1 + 2^-8: a tie, rounds to the even 0x3F80
    ((ODD,), 3 * 2.0 ** -8),                # 1 + 3 * 2^-8: a tie, rounds to the even 0x3F82
)
FIRST_IDS = (A, B, R, DEEP[0], P)           # proposed at depth 0 in every row with a positive boost: kept low in the raw rows
ROW_EMPTY, ROW_PHRASE, ROW_DEEP, ROW_REPEAT, ROW_DONE, ROW_SIGNS = range(6)
N_ROWS = 6
START = (4, 5, 2, 4, 1, 2)                  # prompt lengths
TOP = 7                                     # 8.5 in every raw row
# row -> (the raw arg-max, the biased arg-max); every row flips
FLIPS = {ROW_EMPTY: (Q, TOP), ROW_PHRASE: (TOP, C), ROW_DEEP: (TOP, DEEP[7]), ROW_REPEAT: (TOP, S), ROW_DONE: (TOP, D), ROW_SIGNS: (TOP, Q)}
FILLER = tuple(range(40, 56))


@lru_cache(maxsize=None)
def fixture(vocab: int, tok_ld: int = 48, seed: int = 11):
    """(logits bits uint16 [N_ROWS, vocab], tokens int64 [N_ROWS, tok_ld], length [N_ROWS]) on the host.  Every raw value is at most 6
    except where a row sets its own."""
    assert vocab >= 128 and tok_ld >= 32
    g = torch.Generator().manual_seed(seed + vocab)
    lg = (torch.randn((N_ROWS, vocab), generator=g) * 2.0).clamp_(max=6.0).to(torch.bfloat16)
    bits = np.array(PR.bits_of(lg)).reshape(N_ROWS, vocab)
    b = lambda v: int(PR.bf16_bits(np.float32(v))[0])       # noqa: E731
    for t in FIRST_IDS:
        bits[:, t] = b(1.0)
    bits[:, TOP] = b(8.5)
    bits[:, Q] = b(7.0)                                     # - 6 everywhere but in ROW_SIGNS, where p q gives + 3
    bits[:, NINF], bits[:, TIE], bits[:, ODD] = PR.NEG_INF, b(1.0), b(1.0)
    bits[ROW_EMPTY, Q] = b(9.0)                             # the raw arg-max, pushed below TOP
    bits[ROW_PHRASE, C] = b(7.0)                            # + 3 (a b c at depth 2; b c d's + 2 at depth 1 loses)
    bits[ROW_DEEP, DEEP[7]] = b(5.0)                        # + 5 at depth 7
    bits[ROW_REPEAT, S] = b(6.0)                            # + 3.5 at depth 2 of r r s, behind r r r
    bits[ROW_DONE, D] = b(7.0)                              # + 2: b c d at depth 2 behind the whole a b c, which proposes nothing
    bits[ROW_DONE, C] = b(1.0)
    tokens = torch.randint(0, vocab, (N_ROWS, tok_ld), generator=g, dtype=torch.int64)
    hist: List[List[int]] = [[] for _ in range(N_ROWS)]
    hist[ROW_PHRASE] = [FILLER[0], A, B]
    hist[ROW_DEEP] = [FILLER[1]] + list(DEEP[:7])
    hist[ROW_REPEAT] = [FILLER[2], R, R, R]
    hist[ROW_DONE] = [A, B, C]
    hist[ROW_SIGNS] = [FILLER[3], FILLER[4], P]
    length = []
    for r in range(N_ROWS):
        tokens[r, START[r]:START[r] + len(hist[r])] = torch.tensor(hist[r], dtype=torch.int64)
        length.append(START[r] + len(hist[r]))
    tokens[ROW_EMPTY, :START[ROW_EMPTY]] = torch.tensor([FILLER[5], FILLER[6], A, B])      # a prompt tail that is a b: no match
    return bits, tokens, tuple(length)


def histories(tokens: torch.Tensor, start: Sequence[int], length: Sequence[int]) -> List[List[int]]:
    return PR.histories(tokens, start, length)


@lru_cache(maxsize=None)
def full_table(vocab: int = 32000, seed: int = 23) -> Tuple[Entry, ...]:
    """256 entries of 8 ids: every (entry, depth) pair of the block is taken.  Entry e's boost is 1 + (e % 8) / 8."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(200, vocab, (256, 8), generator=g)
    ids[1, :5] = ids[0, :5]                             # two entries share a prefix of 5 and differ behind it
    ids[3] = ids[2]                                     # a duplicate with another boost
    return tuple((tuple(int(t) for t in row), 1.0 + (e % 8) / 8.0) for e, row in enumerate(ids))
