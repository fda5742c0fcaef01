"""No-repeat n-grams: the host definition of what the sampling kernels compute (include/dualhyp_hip.h, "No-repeat n-grams").

`generated` is what a sequence has produced so far, the prompt excluded; a token is banned at a step when it would complete an
n-gram that `generated` already holds.  The kernels build the same set on the device from the token buffer; these functions are what
the argument checks, the prediction records (`ngram_bans`) and the tests use — nothing here touches the GPU.
"""
from __future__ import annotations

from typing import List, Sequence, Set

MAX_NGRAM = 8               # n of the header: 1 .. 8
MAX_VOCAB = 131072          # the ids the sampler's static LDS row holds


def check_ngram(no_repeat_ngram, vocab: int = 0) -> int:
    """n of a call (0: off), refused before anything is launched: an int in 0 .. 8, and with n > 0 a vocab the LDS row holds."""
    if isinstance(no_repeat_ngram, bool) or not isinstance(no_repeat_ngram, int):
        raise TypeError(f"no_repeat_ngram is an int in 0 .. {MAX_NGRAM}, got {no_repeat_ngram!r}")
    if not 0 <= no_repeat_ngram <= MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram={no_repeat_ngram} is outside 0 .. {MAX_NGRAM} (0: off)")
    if no_repeat_ngram and vocab > MAX_VOCAB:
        raise ValueError(f"no_repeat_ngram keeps a sequence's allowed ids in an LDS row of {MAX_VOCAB} ids; a vocab of {vocab} does not fit")
    return no_repeat_ngram


def banned(generated: Sequence[int], n: int) -> Set[int]:
    """The ban set of the next pick: { g[i + n - 1] : 0 <= i <= m - n, g[i .. i + n - 1) == g[m - n + 1 .. m) }, m = len(generated).
    Empty while m < n; for n = 1 every id generated so far."""
    if not 1 <= n <= MAX_NGRAM:
        raise ValueError(f"n={n} is outside 1 .. {MAX_NGRAM}")
    g = [int(t) for t in generated]
    m = len(g)
    if m < n:
        return set()
    suffix = g[m - n + 1:]
    return {g[i + n - 1] for i in range(m - n + 1) if g[i:i + n - 1] == suffix}


def ban_positions(generated: Sequence[int], n: int) -> List[int]:
    """The positions t of `generated` whose pick had a non-empty ban set, banned(generated[:t], n), in order."""
    g = [int(t) for t in generated]
    return [t for t in range(len(g)) if banned(g[:t], n)]
