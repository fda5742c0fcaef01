"""Nucleus (top-p) and min-p sampling: the argument checks every entry point runs before anything is launched.  The definition
is in include/dualhyp_hip.h, "Nucleus and min-p"; the crop itself is in the sampling kernels (csrc/sampling.hip)."""
from __future__ import annotations

import math
import numbers
from typing import Optional, Tuple


def _number(value, name: str) -> float:
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise TypeError(f"{name} is a number, not {value!r}")
    return float(value)


def check_top_p(top_p) -> float:
    """top_p as the C entries take it: None is 1.0 (off); a value outside (0, 1] or a NaN is refused."""
    if top_p is None:
        return 1.0
    p = _number(top_p, "top_p")
    if math.isnan(p) or not 0.0 < p <= 1.0:
        raise ValueError(f"top_p={top_p!r} is not in (0, 1] (1 or None = off)")
    return p


def check_min_p(min_p) -> float:
    """min_p as the C entries take it: None is 0.0 (off); a value outside [0, 1] or a NaN is refused."""
    if min_p is None:
        return 0.0
    p = _number(min_p, "min_p")
    if math.isnan(p) or not 0.0 <= p <= 1.0:
        raise ValueError(f"min_p={min_p!r} is not in [0, 1] (0 or None = off)")
    return p


def check_nucleus(top_p, min_p) -> Tuple[float, float]:
    """(top_p, min_p) checked; (1.0, 0.0) is off."""
    return check_top_p(top_p), check_min_p(min_p)


def nucleus_on(top_p: Optional[float], min_p: Optional[float]) -> bool:
    """True when the checked pair asks for a crop."""
    p, q = check_nucleus(top_p, min_p)
    return p < 1.0 or q > 0.0
