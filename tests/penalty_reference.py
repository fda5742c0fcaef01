"""Host model of the penalties (include/dualhyp_hip.h, "Penalties") and the fixtures the penalty tests share.  It knows nothing of the
device code: a_t is computed in numpy float32 scalar operations, one rounding per operation, and rounded to bf16 with integer
arithmetic on the bits.

adjusted_row(row, history, theta, alpha_f, alpha_p) is the copy of a logits row on which the existing, unpenalised call must make the
penalised call's pick.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Sequence

import numpy as np
import torch

NEG_INF, POS_ZERO, NEG_ZERO = 0xFF80, 0x0000, 0x8000


def f32_of_bits(bits) -> np.ndarray:
    """bf16 bit patterns widened to float32"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even, by integer arithmetic on the bits (a NaN keeps its sign and goes quiet)"""
    u = np.atleast_1d(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def adjusted_value(bits: int, c: int, theta: float, alpha_f: float, alpha_p: float) -> int:
    """a_t of the header as bf16 bits, from the raw column's bf16 bits and the id's count c > 0"""
    th, af, ap = np.float32(theta), np.float32(alpha_f), np.float32(alpha_p)
    x = f32_of_bits([bits])[0]
    with np.errstate(all="ignore"):
        y = np.float32(x * th) if x < 0 else np.float32(x / th)        # the HF rule; NaN and the zeros take the division
        p = np.float32(af * np.float32(c))
        z = np.float32(np.float32(y - p) - ap)
    return int(bf16_bits(z)[0])


def counts(history: Sequence[int]) -> Dict[int, int]:
    c: Dict[int, int] = {}
    for t in history:
        c[int(t)] = c.get(int(t), 0) + 1
    return c


def adjusted_bits(row_bits: np.ndarray, history: Sequence[int], theta: float, alpha_f: float, alpha_p: float) -> np.ndarray:
    """the row's bf16 bits with a_t in every column t in [0, vocab) that occurs in `history`"""
    out = np.array(row_bits, dtype=np.uint16, copy=True)
    for t, c in counts(history).items():
        if 0 <= t < out.size:
            out[t] = adjusted_value(int(row_bits[t]), c, theta, alpha_f, alpha_p)
    return out


def bits_of(row: torch.Tensor) -> np.ndarray:
    return row.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def tensor_of(bits: np.ndarray, device="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(device)


def adjusted_row(row_bf16: torch.Tensor, history: Sequence[int], theta: float = 1.0, alpha_f: float = 0.0, alpha_p: float = 0.0) -> torch.Tensor:
    """The adjusted copy of a 1-D bf16 logits row, on the row's device."""
    assert row_bf16.dtype == torch.bfloat16 and row_bf16.dim() == 1
    return tensor_of(adjusted_bits(bits_of(row_bf16), history, theta, alpha_f, alpha_p), row_bf16.device)


def adjusted_rows(logits: torch.Tensor, histories: Sequence[Sequence[int]], pen: Dict[str, float]) -> torch.Tensor:
    """adjusted_row over the rows of a [rows, vocab] tensor; pen holds the sampling ops' keywords"""
    th, af, ap = pen.get("repetition_penalty", 1.0), pen.get("frequency_penalty", 0.0), pen.get("presence_penalty", 0.0)
    return torch.stack([adjusted_row(logits[r], h, th, af, ap) for r, h in enumerate(histories)]).contiguous()


def argmax_bits(bits: np.ndarray) -> int:
    """the lowest index among the largest values (-0 == +0), as the samplers' arg-max takes it"""
    return int(np.argmax(f32_of_bits(bits)))


# ---- the penalties the tests run: each alone, and all together ---------------------------------------------------------------------------
# ALL's alpha_f is not a short binary fraction, so alpha_f * 3 is rounded: FUSED below rounds differently when the product and the
# subtraction are contracted into one FMA.
PENALTIES = {
    "repetition": dict(repetition_penalty=1.3),
    "frequency": dict(frequency_penalty=0.75),
    "presence": dict(presence_penalty=0.75),
    "all": dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=0.3),
}
# x = -6.6875 three times in the history under ALL: 0xC131 by three separately rounded operations, 0xC132 with the product fused
FUSED = dict(bits=0xC0D6, count=3, want=0xC131, fused=0xC132)

# ---- the kernel-level fixture -----------------------------------------------------------------------------------------------------------
# rows and what their histories are
ROW_EMPTY, ROW_ONE, ROW_ARGMAX, ROW_COUNT, ROW_SPECIAL, ROW_FULL = range(6)
N_ROWS = 6
START = (3, 5, 2, 4, 1, 2)                  # prompt lengths
TOP, RUNNER = 7, 11                         # the raw arg-max of rows ROW_ARGMAX / ROW_COUNT and what the pick flips to
SPECIAL_IDS = (20, 21, 22, 23, 24, 25)      # ROW_SPECIAL: -inf, +0, -0, negative, positive, the FUSED value
SPECIAL_BITS = (NEG_INF, POS_ZERO, NEG_ZERO, 0xC040, 0x4020, FUSED["bits"])
FILLER = tuple(range(40, 56))               # ids the histories are padded with
# (penalty name) -> rows whose arg-max must differ between the adjusted and the raw row; ROW_COUNT's margin of 1.5 is above one
# presence penalty of 0.75 and below three frequency penalties of 0.75
FLIPS = {"repetition": (ROW_ARGMAX, ROW_COUNT), "frequency": (ROW_ARGMAX, ROW_COUNT), "presence": (ROW_ARGMAX,), "all": (ROW_ARGMAX, ROW_COUNT)}


@lru_cache(maxsize=None)
def fixture(vocab: int, tok_ld: int = 48, seed: int = 5):
    """(logits bits uint16 [N_ROWS, vocab], tokens int64 [N_ROWS, tok_ld], length [N_ROWS]) on the host.  Every raw value is at most 6
    except where a row sets its own: TOP and RUNNER in ROW_ARGMAX (8.5 / 8.0) and ROW_COUNT (9.5 / 8.0)."""
    assert vocab >= 64 and tok_ld >= 32
    g = torch.Generator().manual_seed(seed + vocab)
    lg = (torch.randn((N_ROWS, vocab), generator=g) * 2.0).clamp_(max=6.0).to(torch.bfloat16)
    bits = np.array(bits_of(lg)).reshape(N_ROWS, vocab)
    b = lambda v: int(bf16_bits(np.float32(v))[0])       # noqa: E731
    bits[ROW_ARGMAX, TOP], bits[ROW_ARGMAX, RUNNER] = b(8.5), b(8.0)
    bits[ROW_COUNT, TOP], bits[ROW_COUNT, RUNNER] = b(9.5), b(8.0)
    for t, v in zip(SPECIAL_IDS, SPECIAL_BITS):
        bits[ROW_SPECIAL, t] = v
    tokens = torch.randint(0, vocab, (N_ROWS, tok_ld), generator=g, dtype=torch.int64)
    hist: List[List[int]] = [[] for _ in range(N_ROWS)]
    hist[ROW_ONE] = [int(torch.randint(0, vocab, (1,), generator=g))]
    hist[ROW_ARGMAX] = [FILLER[0], TOP, FILLER[1], FILLER[2]]
    hist[ROW_COUNT] = [TOP, FILLER[3], FILLER[3], TOP, FILLER[4], TOP, FILLER[3]]
    hist[ROW_SPECIAL] = list(SPECIAL_IDS) + [SPECIAL_IDS[5], SPECIAL_IDS[3], SPECIAL_IDS[5], vocab - 1, 0]
    # to the last free place: one place is left for the pick; one id lies outside the vocab (no column to override)
    n_full = tok_ld - 1 - START[ROW_FULL]
    hist[ROW_FULL] = [int(t) for t in torch.randint(0, min(vocab, 200), (n_full,), generator=g)]
    hist[ROW_FULL][3] = vocab + 5
    length = []
    for r in range(N_ROWS):
        tokens[r, START[r]:START[r] + len(hist[r])] = torch.tensor(hist[r], dtype=torch.int64)
        length.append(START[r] + len(hist[r]))
    return bits, tokens, tuple(length)


def histories(tokens: torch.Tensor, start: Sequence[int], length: Sequence[int]) -> List[List[int]]:
    """H of every sequence: tokens[u, start[u]:length[u]]"""
    return [tokens[u, int(s):int(n)].tolist() for u, (s, n) in enumerate(zip(start, length))]
