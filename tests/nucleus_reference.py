"""Host model of nucleus (top-p) and min-p sampling (include/dualhyp_hip.h, "Nucleus and min-p") in fp64, and the inputs of
tests/test_hip_nucleus.py.  CPU only, and it does not import the library: tests/test_nucleus_reference.py shows on these same inputs
that the kept sets reject the bugs they are meant to catch.

The row is the one the sampler uses (sampling_reference.scaled, with bf16 -inf where `allowed` is false):
    K0      = sampling_reference.keep_mask(row, top_k)                     ties at the k-th value kept, -0 == +0
    min_p   : i passes iff fl32(l_i - m) >= lmin, lmin = float32(log(float64(float32(min_p)))), m = max l        (numpy fp32)
    top_p   : a value v of K0 passes iff A(v) < float32(top_p) * T, A the fp64 mass of the entries of K0 strictly above v, T that of K0
    kept    = K0 & min_p & top_p                                                                                   (nucleus_keep)
The GPU test never compares picks with this model's: it packs the kept set into a token mask and asks the masked sampler, top_k off,
for the picks (the header's equivalence).  So the only device arithmetic this model has to bound is the one behind the kept set.

The band (BAND).  The kernel (dualhyp_amd/csrc/sampling.hip, pick_token) decides A_int(v) < P with
    q_i    = (uint64)(fl32(__expf(l_i - m)) * 2^40)         the product is exact (a power of two), the conversion truncates
    A_int  = the integer sum of q over the entries of K0 strictly above v, T_int that over K0: integer sums are exact in any order
    P      = clamp((uint64)(fl64(top_p) * fl64(T_int)), 1, T_int)
against the exact A(v) < top_p * T.  In units of T:
  exp       each __expf term carries a relative error delta <= (2.5 x + 2) 2^-24, x = |l - m| (sampling_reference.eps derives it).
            Perturbing every term of a normalised partial sum a = A / T by a relative delta moves it by at most 2 delta a (1 - a)
            <= delta / 2, so 2^-18 covers delta up to 2^-17: every term within x <= 50 of the maximum.  Terms beyond x = 27.8 have q = 0.
  truncate  each q_i loses less than one unit; the best entry alone has q = 2^40, so a unit is at most 2^-40 T_int.  A row has at
            most 2^17 entries (BAN_MAX_VOCAB), so A_int and T_int are each short by less than 2^-23 T, and their ratio moves by less
            than 2^-22.  (This also covers the entries whose q is 0.)
  P         T_int < 2^57 rounds to fp64 within 2^-53 relative, so does the product; the conversion drops less than one unit,
            2^-40 T; comparing the integer A_int with floor(y) instead of y differs only where A_int = floor(y), again within a unit.
            The clamp acts only where top_p * T_int < 1 or > T_int, neither of which the checks on top_p allow beyond a unit.
            Together below 2^-39.
BAND = 2^-18 + 2^-22 + 2^-39.  A case is DECIDED when no A(v) / T lies within BAND of top_p (decided); then the kernel's kept set is this
model's.  BAND may not exceed BAND_CAP = 2^-16, and every case of this file is decided (tests/test_nucleus_reference.py).
The min_p test is exact on both sides: one IEEE fp32 subtraction of two bf16 values and one comparison.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import sampling_reference as SR

BF = torch.bfloat16
BAND = 2.0 ** -18 + 2.0 ** -22 + 2.0 ** -39
BAND_CAP = 2.0 ** -16
assert BAND <= BAND_CAP

TOP_PS = (0.5, 0.9, 0.95)
MIN_PS = (0.0, 0.05, 1.0)

MUTANTS = ["nucleus_drops_crossing", "ties_split_by_index", "nucleus_before_top_k", "nucleus_unscaled", "nucleus_ignores_mask",
           "min_p_of_total", "min_p_strict", "cdf_not_renormalised"]


def _f32(x) -> float:
    return float(np.float32(x))


def lmin_of(min_p: float) -> np.float32:
    """(float)log((double)min_p) of the fp32 value the C entry receives."""
    return np.float32(math.log(_f32(min_p)))


def masked_row(sc: torch.Tensor, allowed: Optional[np.ndarray]) -> torch.Tensor:
    """The scaled bf16 row with bf16 -inf where `allowed` (bool [V], None: everything) is false."""
    assert sc.dtype == BF and sc.dim() == 1
    if allowed is None:
        return sc
    out = sc.clone()
    out[~torch.from_numpy(np.asarray(allowed, dtype=bool))] = -math.inf
    return out


def _masses(x: torch.Tensor) -> np.ndarray:
    """fp64 w_i = exp(l_i - m) of a row; -inf weighs 0."""
    v = x.double().numpy()
    return np.exp(v - v.max())


def _value_table(vals: np.ndarray, w: np.ndarray, k0: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """(distinct values of K0 descending, M(v), A(v), T): -0 and +0 are one value (numpy's == on floats)."""
    v, m = vals[k0], w[k0]
    uniq, inv = np.unique(v, return_inverse=True)               # ascending; -0.0 == 0.0
    mass = np.zeros(uniq.size, dtype=np.float64)
    np.add.at(mass, inv, m)
    uniq, mass = uniq[::-1], mass[::-1]
    above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])
    return uniq, mass, above, float(mass.sum())


def nucleus_keep(sc: torch.Tensor, top_k: Optional[int], top_p: Optional[float], min_p: Optional[float],
                 allowed: Optional[np.ndarray] = None, mutant: Optional[str] = None, raw: Optional[torch.Tensor] = None) -> np.ndarray:
    """bool [V]: the kept set of the scaled bf16 row `sc` under (top_k, top_p, min_p) and the allowed set; None / 1.0 / 0.0 are off.
    mutant: one of MUTANTS, a deliberately wrong kept set (nucleus_unscaled needs `raw`, the unscaled logits):
      nucleus_drops_crossing  the value whose mass crosses top_p is dropped (the best value stays)
      ties_split_by_index     entries, not values: sorted by value then index, an entry stays while the mass before it is below top_p T
      nucleus_before_top_k    the nucleus is taken over the whole row, then cut by top_k
      nucleus_unscaled        the masses come from the raw logits, not from logit / temperature
      nucleus_ignores_mask    the masses are those of the row without the allowed set
      min_p_of_total          an entry passes when its share of the kept mass is at least min_p
      min_p_strict            the comparison is > instead of >=
    (cdf_not_renormalised keeps the right set: it is a mutant of the draw, see picks.)"""
    assert mutant is None or mutant in MUTANTS
    x = masked_row(sc, allowed)
    vals = x.double().numpy()
    k0 = SR.keep_mask(x, top_k).numpy()
    keep = k0.copy()
    p = 1.0 if top_p is None else _f32(top_p)
    if p < 1.0:
        src, base = x, k0
        if mutant == "nucleus_unscaled":
            src = masked_row(raw, allowed)
        elif mutant == "nucleus_ignores_mask":
            src, base = sc, SR.keep_mask(sc, top_k).numpy()
        elif mutant == "nucleus_before_top_k":
            base = np.ones_like(k0)
        w = _masses(src)
        svals = src.double().numpy()
        if mutant == "ties_split_by_index":
            idx = np.flatnonzero(base)
            order = idx[np.lexsort((idx, -svals[idx]))]
            before = np.concatenate([[0.0], np.cumsum(w[order])[:-1]])
            ok = np.zeros_like(k0)
            ok[order[before < p * w[base].sum()]] = True
        else:
            uniq, mass, above, T = _value_table(svals, w, base)
            good = above < p * T
            if mutant == "nucleus_drops_crossing":
                good = above + mass <= p * T
                good[0] = True
            thr = uniq[good].min()
            ok = svals >= thr
        keep &= ok
    q = 0.0 if min_p is None else _f32(min_p)
    if q > 0.0:
        l32 = x.float().numpy()
        m32 = np.float32(l32.max())
        with np.errstate(invalid="ignore"):
            d = (l32 - m32).astype(np.float32)
        if mutant == "min_p_of_total":
            w = _masses(x)
            keep &= w / w[k0].sum() >= q
        elif mutant == "min_p_strict":
            keep &= d > lmin_of(q)
        else:
            keep &= d >= lmin_of(q)
    return keep


def decided(sc: torch.Tensor, top_k: Optional[int], top_p: Optional[float], allowed: Optional[np.ndarray] = None) -> Tuple[bool, float]:
    """(margin > BAND, margin): margin = min over the values v of K0 of |A(v) / T - top_p|; inf with top_p off.  min_p needs no
    margin: its test is exact."""
    p = 1.0 if top_p is None else _f32(top_p)
    if p >= 1.0:
        return True, math.inf
    x = masked_row(sc, allowed)
    k0 = SR.keep_mask(x, top_k).numpy()
    _, _, above, T = _value_table(x.double().numpy(), _masses(x), k0)
    margin = float(np.abs(above / T - p).min())
    return margin > BAND, margin


def picks(mutant: Optional[str], logits: torch.Tensor, temperature: float, top_k: Optional[int], top_p: Optional[float],
          min_p: Optional[float], seed: int, steps: Sequence[int], n_seq: int, allowed: Optional[np.ndarray] = None) -> np.ndarray:
    """[len(steps), n_seq] fp64 picks of the host sampler over the kept set (mutant None: the right one).  cdf_not_renormalised: the
    CDF over the kept entries is divided by the mass of K0, not by the kept mass; a draw past its end takes the last kept entry."""
    sc = SR.scaled(logits, temperature)
    keep = nucleus_keep(sc, top_k, top_p, min_p, allowed, None if mutant == "cdf_not_renormalised" else mutant, raw=logits)
    x = masked_row(sc, allowed)
    w = np.where(keep, _masses(x), 0.0)
    hi = np.cumsum(w)
    total = hi[-1]
    if mutant == "cdf_not_renormalised":
        total = _masses(x)[SR.keep_mask(x, top_k).numpy()].sum()
    hi = hi / total
    out = np.searchsorted(hi, SR.u01_grid(seed, steps, n_seq), side="right")
    return np.minimum(out, np.flatnonzero(keep).max())


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
SEEDS = SR.SEEDS
STEPS = SR.STEPS


@dataclass(frozen=True)
class Case:
    name: str
    row: str                      # key of rows(): the bf16 logits row every sequence of the case has
    top_k: Optional[int]
    temperature: float
    top_p: Optional[float]
    min_p: Optional[float]
    n_seq: int
    chunky: bool = False          # a crafted row: at most a dozen entries carry the mass, each at least 2 % of it


# a case whose A(v) / T came within BAND of its top_p gets another top_p here (never another band): none so far
TOP_P_OVERRIDE: Dict[str, float] = {}


def _bits(*words: int) -> torch.Tensor:
    return torch.tensor([w - 0x10000 if w >= 0x8000 else w for w in words], dtype=torch.int16).view(BF)


def _spread(vocab: int, n: int) -> List[int]:
    """n positions of a row of `vocab` (256 or 1000) on both sides of a 64-lane boundary and across the thread slabs"""
    fixed = [63, 64, 65, 1, vocab - 1, 130, vocab // 2, 200, 7, vocab - 2, 129, 191]
    assert n <= len(fixed)
    return fixed[:n]


def _chunky(vocab: int, at: Sequence[int], values, background: float = -math.inf) -> torch.Tensor:
    row = torch.full((vocab,), background, dtype=BF)
    row[torch.tensor(list(at))] = values if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=BF)
    return row


def _crafted(vocab: int) -> List[Tuple[str, torch.Tensor, Optional[int], float, Optional[float], Optional[float]]]:
    """(name, row, top_k, temperature, top_p, min_p) at one vocabulary size; the masses and crossings are checked by
    tests/test_nucleus_reference.py (every entry that carries mass has at least 2 % of it, every case is decided)."""
    S = lambda n: _spread(vocab, n)        # noqa: E731
    out = []
    # three values above, six entries tied at the crossing value (1.0) in different slabs and waves, two below: masses
    # 7.39 5.75 4.48 | 6 x 2.72 | 2 x 1.65 of 37.2; A(1.0) / T = 0.47, the next value's 0.91
    out.append(("ties_at_crossing", _chunky(vocab, [5, 300 % vocab, 77] + S(6) + [20, 250], [2.0, 1.75, 1.5] + [1.0] * 6 + [0.5, 0.5]),
                None, 1.0, 0.7, None))
    # the crossing value and its neighbour one key apart: the upper crosses top_p and is kept, the lower is dropped
    # (A(upper) / T = 0.56, A(lower) / T = 0.69 in all four)
    for name, hi_w, lo_w, tops, p in (("pair_low_byte", 0x3F82, 0x3F81, [2.0, 1.5], 0.62), ("pair_high_byte", 0x3F00, 0x3EFF, [1.5, 1.0], 0.62),
                                      ("pair_low_byte_neg", 0xBF81, 0xBF82, [0.0, -0.5], 0.62),
                                      ("pair_high_byte_neg", 0xBEFF, 0xBF00, [0.5, 0.0], 0.62)):
        pair = _bits(hi_w, lo_w).float().tolist()
        low = [pair[1] - 0.25, pair[1] - 0.5]
        vals = torch.cat([torch.tensor(tops, dtype=BF), _bits(hi_w, lo_w), torch.tensor(low, dtype=BF)])
        out.append((name, _chunky(vocab, S(6), vals), None, 1.0, p, None))
        out.append((name + "_swapped", _chunky(vocab, S(6)[::-1], vals), None, 1.0, p, None))
    # the kept set spans zero and ends on it: +0 and -0 are one value, kept together
    out.append(("spans_zero", _chunky(vocab, S(7), [1.0, 0.5, 0.0, -0.0, -0.5, -1.0, -0.0]), None, 1.0, 0.75, None))
    out.append(("zero_dropped", _chunky(vocab, S(7), [1.0, 0.5, 0.0, -0.0, -0.5, -1.0, -0.0]), None, 1.0, 0.4, None))
    out.append(("all_negative", _chunky(vocab, S(8), [-1.0, -1.25, -1.5, -1.5, -2.0, -2.25, -2.5, -2.5]), None, 1.0, 0.6, None))
    out.append(("all_negative_min_p", _chunky(vocab, S(8), [-1.0, -1.25, -1.5, -1.5, -2.0, -2.25, -2.5, -2.5]), None, 1.0, None, 0.3))
    # -inf entries among a background that is finite but weighs nothing (q = 0 in the kernel's fixed point)
    inf_row = _chunky(vocab, S(8), [1.0, 0.5, 0.5, 0.0, -0.25, -0.5, -0.5, -1.0], background=-90.0)
    inf_row[torch.arange(2, vocab, 3)[:60]] = -math.inf
    inf_row[torch.tensor(S(8))] = torch.tensor([1.0, 0.5, 0.5, 0.0, -0.25, -0.5, -0.5, -1.0], dtype=BF)
    out.append(("neg_inf_entries", inf_row, None, 1.0, 0.8, 0.05))
    out.append(("three_maxima_min_p_1", _chunky(vocab, S(9), [1.5, 1.0, 1.5, 0.5, 1.25, 1.5, 0.75, 1.0, 0.5]), None, 1.0, None, 1.0))
    out.append(("only_the_best", _chunky(vocab, S(10), [2.0, 1.5, 1.5, 1.25, 1.0, 1.0, 0.75, 0.75, 0.5, 0.5]), None, 1.0, 0.05, None))
    # top_k crops 5 of 12, and the nucleus is taken over the 5: 0.7 of their mass, not of the row's
    twelve = [2.0, 1.875, 1.75, 1.625, 1.5, 1.375, 1.25, 1.125, 1.0, 0.875, 0.75, 0.625]
    out.append(("top_k_then_nucleus", _chunky(vocab, S(12), twelve), 5, 1.0, 0.7, None))
    # temperature 0.5 doubles the logits exactly: the masses are those of the scaled row
    out.append(("scaled_T0.5", _chunky(vocab, S(8), [1.0, 0.875, 0.75, 0.625, 0.5, 0.375, 0.25, 0.125]), None, 0.5, 0.6, None))
    # min_p between two values: log(0.25) = -1.386 keeps -1.375 below the best and drops -1.5
    out.append(("min_p_between", _chunky(vocab, S(6), [0.5, 0.0, -0.5, -0.875, -1.0, -1.25]), None, 1.0, None, 0.25))
    out.append(("min_p_and_top_p", _chunky(vocab, S(6), [0.5, 0.0, -0.5, -0.875, -1.0, -1.25]), 4, 1.0, 0.9, 0.25))
    return out


_ROWS: Dict[str, torch.Tensor] = {}
_CASES: List[Case] = []


def _build() -> None:
    if _CASES:
        return
    for c in SR.grid_cases():
        key = f"{c.dist}/{c.vocab}"
        _ROWS.setdefault(key, SR.case_row(c))
        for p in TOP_PS:
            for q in MIN_PS:
                name = f"{c.name}.p{p}.m{q}"
                _CASES.append(Case(name, key, c.top_k, c.temperature, TOP_P_OVERRIDE.get(name, p), q, c.n_seq))
    # V = 515: the scalar path (515 % 8 != 0) and a ragged last mask word (515 = 16 * 32 + 3)
    for dist, top_k, T in (("g4", None, 1.0), ("u3", 50, 0.8), ("g6", 514, 1.7), ("u3", None, 0.2)):
        c = SR.Case(f"V515.k{top_k}.T{T}.{dist}", 515, top_k, T, dist, 1024)
        key = f"{dist}/515"
        _ROWS.setdefault(key, SR.case_row(c))
        for p, q in ((0.9, 0.0), (0.5, 0.05), (0.95, 1.0), (None, 0.05)):
            name = f"{c.name}.p{p}.m{q}"
            _CASES.append(Case(name, key, top_k, T, TOP_P_OVERRIDE.get(name, p), q, 1024))
    for vocab in (256, 1000):
        for name, row, top_k, T, p, q in _crafted(vocab):
            key = f"crafted/{vocab}/{name}"
            _ROWS[key] = row
            _CASES.append(Case(f"crafted.V{vocab}.{name}", key, top_k, T, p, q, 1024, chunky=True))


def rows() -> Dict[str, torch.Tensor]:
    _build()
    return _ROWS


def cases() -> List[Case]:
    _build()
    return list(_CASES)


def case_keep(c: Case) -> np.ndarray:
    """The kept set of a case's row."""
    return nucleus_keep(SR.scaled(rows()[c.row], c.temperature), c.top_k, c.top_p, c.min_p)
