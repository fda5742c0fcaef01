"""Repetition, frequency and presence penalties: the argument checks every entry point runs before anything is launched, and the
host's side of the bookkeeping.  The definition is in include/dualhyp_hip.h, "Penalties"; the adjusted values themselves are computed in
the sampling kernels (csrc/sampling.hip) — nothing here touches the GPU.
"""
from __future__ import annotations

import math
import numbers
from typing import Dict, Optional, Sequence, Tuple

MIN_REPETITION, MAX_REPETITION = 0.125, 8.0     # theta of the header; 1 = off
MAX_ALPHA = 8.0                                 # |alpha_f|, |alpha_p| of the header; 0 = off
MAX_HISTORY = 2048                              # DH_MAX_PENALTY_HISTORY: the generated tokens the sampler's static LDS tables hold
MAX_VOCAB = 131072                              # the ids the sampler's static LDS row holds


def _number(value, name: str) -> float:
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise TypeError(f"{name} is a number, not {value!r}")
    return float(value)


def check_repetition(repetition) -> float:
    """theta as the C entries take it: None is 1.0 (off); a value outside [1/8, 8], an infinity or a NaN is refused."""
    if repetition is None:
        return 1.0
    v = _number(repetition, "repetition_penalty")
    if math.isnan(v) or not MIN_REPETITION <= v <= MAX_REPETITION:
        raise ValueError(f"repetition_penalty={repetition!r} is not in [{MIN_REPETITION}, {MAX_REPETITION}] (1 or None = off)")
    return v


def _check_alpha(value, name: str) -> float:
    if value is None:
        return 0.0
    v = _number(value, name)
    if math.isnan(v) or not -MAX_ALPHA <= v <= MAX_ALPHA:
        raise ValueError(f"{name}={value!r} is not in [{-MAX_ALPHA}, {MAX_ALPHA}] (0 or None = off)")
    return v


def check_penalties(repetition, frequency, presence) -> Tuple[float, float, float]:
    """(repetition, frequency, presence) checked; (1.0, 0.0, 0.0) is off."""
    return check_repetition(repetition), _check_alpha(frequency, "frequency_penalty"), _check_alpha(presence, "presence_penalty")


def penalties_on(repetition: float, frequency: float, presence: float) -> bool:
    """True when the checked triple asks for anything."""
    return repetition != 1.0 or frequency != 0.0 or presence != 0.0


def check_history(tok_ld: int, vocab: int = 0) -> None:
    """A penalised call's token buffer and vocab, refused before anything is launched where the sampler's LDS tables could not hold
    them: a sequence's history is at most the tok_ld places of its row."""
    if tok_ld > MAX_HISTORY:
        raise ValueError(f"penalties keep a sequence's distinct ids in LDS tables of {MAX_HISTORY} entries; a token buffer of {tok_ld} "
                         f"places may not fit")
    if vocab > MAX_VOCAB:
        raise ValueError(f"penalties keep a sequence's overridden columns in an LDS row of {MAX_VOCAB} ids; a vocab of {vocab} does not fit")


def counts(history: Sequence[int]) -> Dict[int, int]:
    """c_t of the header: how often each id occurs in `history`, what a sequence has generated so far, the prompt excluded."""
    c: Dict[int, int] = {}
    for t in history:
        c[int(t)] = c.get(int(t), 0) + 1
    return c


def record(repetition: float, frequency: float, presence: float) -> Optional[Dict[str, float]]:
    """The `penalties` field of a prediction record: the three values when any is off its default, else None (no field)."""
    r, f, p = check_penalties(repetition, frequency, presence)
    if not penalties_on(r, f, p):
        return None
    return {"repetition": r, "frequency": f, "presence": p}
