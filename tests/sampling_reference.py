"""Host model of the decode-loop tail (dualhyp_amd/csrc/sampling.hip: dh_sample_bf16, dh_sample_rows_bf16) in Python integers
and fp64, and the inputs of tests/test_hip_sampling.py.  CPU only, and it does not import the library:
tests/test_sampling_reference.py shows on those same inputs that the checker rejects the bugs it is meant to catch.

The draw of sequence `seq` at step `step` is deterministic:
    u = (mix64(seed ^ mix64((step << 32) | uint32(seq))) >> 40) / 2**24                     (u01)
    l = bf16(float(logit) / float32(temperature))                                            (scaled)
    keep = ~(l < k-th largest l)           ties at the k-th value all kept, -0 == +0         (keep_mask)
    pick = the kept token i with lo[i] <= u < hi[i], lo / hi the cumulative softmax over the kept entries in ascending
           index order, normalised to 1                                                      (cdf64)
The kernel evaluates lo / hi in fp32, so a pick is accepted when u lies within eps(V) of the fp64 interval (check_pick).
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

BF = torch.bfloat16
M64 = (1 << 64) - 1
NT = 1024                    # threads of the sampling block: one contiguous slab of ceil(V / NT) tokens each


# ---------------------------------------------------------------------------------------------------- the uniform
def mix64(z: int) -> int:
    """The splitmix64 step, modulo 2**64.  mix64(0) == 0xE220A8397B1DCDAF."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u01(seed: int, step: int, seq: int) -> float:
    """The uniform in [0, 1) of (seed, step, seq): 24 bits, exact in fp32 and fp64."""
    h = mix64((seed & M64) ^ mix64(((step << 32) & M64) | (seq & 0xFFFFFFFF)))
    return (h >> 40) / 2.0 ** 24


def u01_grid(seed: int, steps: Sequence[int], n_seq: int, swap: bool = False) -> np.ndarray:
    """[len(steps), n_seq] fp64 of u01(seed, step, seq); swap: the two hash arguments exchanged (a mutation control)."""
    return np.array([[u01(seed, q, s) if swap else u01(seed, s, q) for q in range(n_seq)] for s in steps], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- the distribution
def scaled(logits: torch.Tensor, temperature: float) -> torch.Tensor:
    """bf16(float(logit) / float32(temperature)): `logits / temperature` of a bf16 tensor and a Python float."""
    assert logits.dtype == BF
    return (logits.float() / torch.tensor(temperature, dtype=torch.float32)).to(BF)


def keep_mask(sc: torch.Tensor, top_k: Optional[int]) -> torch.Tensor:
    """The crop of the oracle's pick_token on one row: topk(min(k, V)), keep ~(l < kth); top_k 0 or None keeps all."""
    if not top_k:
        return torch.ones(sc.numel(), dtype=torch.bool)
    v, _ = torch.topk(sc, min(int(top_k), sc.numel()))
    return ~(sc < v[-1])


def cdf64(sc: torch.Tensor, keep: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) fp64 [V]: token i owns [lo[i], hi[i]) of the cumulative fp64 softmax over the kept entries, ascending index
    order, hi[last] == 1.  Entries that are not kept (and kept -inf) own an empty interval."""
    x = sc.double()
    x = torch.where(keep, x, torch.full_like(x, -math.inf))
    w = torch.exp(x - x.max())
    hi = torch.cumsum(w, 0)
    hi = (hi / hi[-1]).numpy()
    lo = np.concatenate([[0.0], hi[:-1]])
    return lo, hi


def eps(vocab: int) -> float:
    """How far, in units of the total mass, the kernel's fp32 evaluation may move an interval end of the fp64 CDF.

    The kernel takes the token i whose fp32 running sum c_i first exceeds u_k = fl(u * total), so against the exact
    test u < C_i / T it errs by at most  err(c_i) / T + u * err(total) / T + 2^-24 (the product u * total).  Every fp32 add
    rounds by at most 2^-24 of its result, and no partial sum exceeds the total, so an operation costs at most 2^-24 in these
    units.  With per = ceil(V / 1024) tokens in a thread's slab:
      c_i    per - 1  serial adds of each earlier thread's slab sum (relative to the slab sums, which add up to < total)
             6        levels of the wave inclusive scan
             15       serial adds of the wave totals below the thread's wave
             2        excl = (base + incl) - mine
             per      the thread walks its slab again from excl, one add per token, each now at the size of the running total
      total  per - 1 + 6 + 15   slab sums, scan, the 16 wave totals
    together (3 per + 43) * 2^-24 with the product.  The slab / scan / totals chain is counted twice, once in the boundary and
    once in `total`, because the two are different sums with different roundings; the walk's adds count at the size of the
    running total, not of the slab.

    exp: each term is __expf(l - mx) = exp2((l - mx) * log2 e) on the hardware exp2.  Relative error of a term with
    x = |l - mx|: x 2^-24 from the fp32 subtraction (two bf16 values more than 16 binades apart), 1.5 x 2^-24 from the product
    with the rounded constant, 2 * 2^-24 for exp2: delta <= (2.5 x + 2) 2^-24.  Perturbing every term of a normalised partial
    sum p by a relative delta moves it by at most 2 delta p (1 - p) <= delta / 2.  2^-18 therefore covers delta up to 2^-17,
    i.e. every term within x <= 50 of the maximum; the terms beyond weigh less than V e^-50 together.
    """
    per = -(-vocab // NT)
    return (3 * per + 43) * 2.0 ** -24 + 2.0 ** -18


class RowModel:
    """The fp64 reference of one logits row: kept set, CDF, and the checks of picks against uniforms (vectorised)."""

    def __init__(self, sc: torch.Tensor, top_k: Optional[int]):
        self.vocab = sc.numel()
        self.keep = keep_mask(sc, top_k).numpy()
        self.lo, self.hi = cdf64(sc, torch.from_numpy(self.keep))
        self.eps = eps(self.vocab)

    def pick(self, u) -> np.ndarray:
        """The reference's token for each uniform: the first i with u < hi[i]."""
        return np.searchsorted(self.hi, np.asarray(u, dtype=np.float64), side="right")

    def check(self, picks, u) -> Tuple[np.ndarray, np.ndarray]:
        """-> (ok, excess) per draw.  ok: the pick is kept and lo - eps <= u < hi + eps.  excess: how far u lies outside
        [lo, hi) of the pick, 0 inside (inf for a pick outside the vocabulary)."""
        picks, u = np.asarray(picks, dtype=np.int64).reshape(-1), np.asarray(u, dtype=np.float64).reshape(-1)
        inside = (picks >= 0) & (picks < self.vocab)
        p = np.where(inside, picks, 0)
        lo, hi = self.lo[p], self.hi[p]
        excess = np.where(inside, np.maximum(0.0, np.maximum(lo - u, u - hi)), np.inf)
        ok = inside & self.keep[p] & (lo - self.eps <= u) & (u < hi + self.eps)
        return ok, excess

    def ambiguous(self, u) -> np.ndarray:
        """Draws whose u lies within eps of an end of the reference pick's interval: fp32 may legitimately pick a neighbour."""
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        p = self.pick(u)
        return np.minimum(u - self.lo[p], self.hi[p] - u) < self.eps


def check_pick(pick: int, sc: torch.Tensor, top_k: Optional[int], u: float, model: Optional[RowModel] = None):
    """-> (None or the reason the pick is rejected, excess).  Accepted only if the token is kept and
    lo[pick] - eps <= u < hi[pick] + eps; excess is the distance of u from the unwidened interval (0 inside)."""
    m = model if model is not None else RowModel(sc, top_k)
    ok, excess = m.check([pick], [u])
    if ok[0]:
        return None, float(excess[0])
    if not 0 <= pick < m.vocab:
        return f"pick {pick} outside the vocabulary of {m.vocab}", math.inf
    if not m.keep[pick]:
        return f"pick {pick} (l = {float(sc[pick])}) is not in the kept set of top_k = {top_k}", float(excess[0])
    return (f"pick {pick} owns [{m.lo[pick]:.9f}, {m.hi[pick]:.9f}), u = {u:.9f} is {excess[0]:.3g} outside "
            f"(eps = {m.eps:.3g}; the reference picks {int(m.pick([u])[0])})"), float(excess[0])


# ---------------------------------------------------------------------------------------------------- mutation controls
MUTANTS = ["thr_one_key_low", "drop_kth_ties", "drop_neg_zero", "slab_drop_last", "cdf_descending", "swap_step_seq",
           "temperature_unrounded"]


def bf16_keys(sc: torch.Tensor) -> np.ndarray:
    """The order-preserving 16-bit keys of bf16 values with the two zeros apart (-0 below +0)."""
    b = sc.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def mutant_picks(mutant: Optional[str], logits: torch.Tensor, temperature: float, top_k: Optional[int], seed: int,
                 steps: Sequence[int], n_seq: int) -> np.ndarray:
    """[len(steps), n_seq] picks of a deliberately wrong host sampler (None: the right one), all in fp64:
      thr_one_key_low        the threshold one distinct value too low (k + 1 distinct values kept)
      drop_kth_ties          exactly k entries kept: ties at the k-th value dropped
      drop_neg_zero          the crop compares keys in which -0 < +0 (a -0 equal to a +0 threshold is dropped)
      slab_drop_last         the last token of each of the 1024 slabs left out of the sums
      cdf_descending         the CDF walked from the last token down
      swap_step_seq          step and seq exchanged in the hash
      temperature_unrounded  logit / temperature not rounded to bf16"""
    assert mutant is None or mutant in MUTANTS
    V = logits.numel()
    sc = scaled(logits, temperature)
    x = sc.double()
    if mutant == "temperature_unrounded":
        x = logits.double() / float(torch.tensor(temperature, dtype=torch.float32))
    k = min(int(top_k), V) if top_k else 0
    keep = torch.ones(V, dtype=torch.bool)
    if k:
        v, idx = torch.topk(x, k)
        keep = ~(x < v[-1])
        if mutant == "thr_one_key_low" and bool((x < v[-1]).any()):
            keep = ~(x < x[x < v[-1]].max())
        elif mutant == "drop_kth_ties":
            keep = torch.zeros(V, dtype=torch.bool)
            keep[idx] = True
        elif mutant == "drop_neg_zero":
            keys = bf16_keys(sc)
            keep = torch.from_numpy(keys >= np.sort(keys)[V - k])
    w = torch.where(keep, torch.exp(x - x[keep].max()), torch.zeros((), dtype=torch.float64)).numpy()
    if mutant == "slab_drop_last":
        per = -(-V // NT)
        if per < 2:
            raise ValueError("slab_drop_last needs slabs of more than one token (V > 1024)")
        last = np.minimum(np.arange(NT) * per + per, V) - 1
        w[last[(np.arange(NT) * per < V)]] = 0.0
    if mutant == "cdf_descending":
        w = w[::-1]
    hi = np.cumsum(w)
    hi /= hi[-1]
    picks = np.searchsorted(hi, u01_grid(seed, steps, n_seq, swap=mutant == "swap_step_seq"), side="right")
    return V - 1 - picks if mutant == "cdf_descending" else picks


# ---------------------------------------------------------------------------------------------------- side effects
def expected_state(tokens, length, done, picks, *, eos_id: Optional[int], limit=None, row_seq=None):
    """(tokens, length, done) after one launch, as new int64 arrays, given the token picked for every row.
    dh_sample_bf16 (row_seq None): row i is sequence i and its budget is the buffer, lim = tok_ld.
    dh_sample_rows_bf16: row r is sequence u = row_seq[r] with lim = min(limit[u], tok_ld); rows naming no sequence
    (u < 0, u >= n_seq) are ignored.
    A sequence with done != 0 keeps everything.  Otherwise, with n = length: the pick is written at tokens[u, n] and the length
    becomes n + 1 if n < lim; done = 1 if the pick is eos_id (None: never), else 2 if n + 1 >= lim."""
    tokens, length, done = (np.array(torch.as_tensor(t).cpu().numpy(), dtype=np.int64) for t in (tokens, length, done))
    n_seq, tok_ld = tokens.shape
    rows = list(range(n_seq)) if row_seq is None else [int(u) for u in torch.as_tensor(row_seq).cpu().tolist()]
    for r, u in enumerate(rows):
        if u < 0 or u >= n_seq or done[u]:
            continue
        n = int(length[u])
        lim = tok_ld if limit is None else min(int(limit[u]), tok_ld)
        if n < lim:
            tokens[u, n] = int(picks[r])
            length[u] = n + 1
        if eos_id is not None and eos_id >= 0 and int(picks[r]) == eos_id:
            done[u] = 1
        elif n + 1 >= lim:
            done[u] = 2
    return tokens, length, done


def argmax_ref(sc: torch.Tensor) -> int:
    """top_k == 1: the lowest index among the maxima, the oracle's nonzero(l == l.max())[0]."""
    return int(torch.nonzero(sc == sc.max())[0])


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
SEEDS = (0x5EED5EED, (1 << 63) + 0x1234567)      # the second does not fit a signed 64-bit integer
STEPS = (0, 1, 7)


@dataclass(frozen=True)
class Case:
    name: str
    vocab: int
    top_k: Optional[int]
    temperature: float
    dist: str                 # 'u3': uniform in +-3 (ties heavily once rounded to bf16); 'gS': Gaussian, sigma S
    n_seq: int                # rows per launch: one draw per (seed, step, row)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def case_row(c: Case) -> torch.Tensor:
    """The bf16 logits row of a case (every sequence of the case has this row)."""
    g = _gen(f"{c.dist}/{c.vocab}")
    if c.dist == "u3":
        return ((torch.rand(c.vocab, generator=g, dtype=torch.float64) * 2 - 1) * 3).to(BF)
    return (torch.randn(c.vocab, generator=g, dtype=torch.float64) * float(c.dist[1:])).to(BF)


def _n_seq(vocab: int) -> int:
    return 1024 if vocab <= 1000 else 512 if vocab < 100000 else 256      # at most 66 MB of logits per launch


def _case(vocab, top_k, temperature, dist) -> Case:
    k = {None: "none", vocab - 1: "Vm1", vocab: "V", vocab + 7: "Vp7"}.get(top_k, top_k)
    return Case(f"V{vocab}.k{k}.T{temperature}.{dist}", vocab, top_k, temperature, dist, _n_seq(vocab))


def grid_cases() -> List[Case]:
    """V x top_k x temperature pruned to every (V, top_k) pair once, with the temperatures and the two kinds of row spread over
    them.  The uniform rows tie heavily at the top once rounded to bf16 (k = 5 keeps 40 entries at V = 32000, 171 at 128256).
    Rows that are not cropped (top_k >= V - 1, 0 or None) are peaked, a Gaussian whose sigma / temperature is at least 4: on a
    flat row of a real vocabulary an interval is narrower than eps and no pick could be told from its neighbour's
    (tests/test_sampling_reference.py holds every case to at most 10 % of such draws)."""
    out = []
    for V in (256, 1000, 32000, 32064, 128256):
        out += [_case(V, *a) for a in (
            (2, 1.0, "g4"), (5, 0.8, "u3"), (50, 1.7, "u3"), (200, 1.0, "u3"), (200, 0.2, "g4"),
            (V - 1, 0.8, "g4"), (V, 1.0, "g6"), (V + 7, 0.8, "g6"), (None, 0.2, "g4"), (None, 1.7, "g8"))]
    out += [_case(32000, 5, 1.7, "g4"), _case(32064, 50, 0.2, "u3"), _case(1000, None, 0.2, "u3"), _case(128256, 5, 1.7, "g4")]
    return out


def _bits(*words: int) -> torch.Tensor:
    return torch.tensor([w - 0x10000 if w >= 0x8000 else w for w in words], dtype=torch.int16).view(BF)


def crafted_rows() -> List[Tuple[str, torch.Tensor, Optional[int], float]]:
    """(name, bf16 row, top_k, temperature): the edges of the crop.  Every row is drawn 1024 times per seed."""
    out = []
    g = _gen("crafted")
    U = lambda n, a, b: (torch.rand(n, generator=g, dtype=torch.float64) * (b - a) + a).to(BF)

    def place(row, at, values):
        row = row.clone()
        row[torch.tensor(at)] = values if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=BF)
        return row

    # 12 entries equal to the k-th value, k = 6: three above, all twelve kept
    at = [1, 7, 64, 65, 300, 511, 512, 640, 777, 900, 998, 999]
    out.append(("ties_at_kth", place(place(U(1000, -8, -4), at, [1.5] * 12), [0, 500, 997], [3.0, 2.5, 3.0]), 6, 1.0))
    # every logit negative, so the threshold is: the negative half of the key map, in both radix passes
    out.append(("negative_kth", U(1000, -9, -1), 20, 1.0))
    out.append(("negative_kth_T0.8", U(32064, -9, -1), 200, 0.8))
    # the kept set spans zero: 600 of 1000 values uniform in +-1
    out.append(("both_signs", U(1000, -1, 1), 600, 1.0))
    # threshold pairs one key apart, the upper kept and the lower cropped, with a crowd of 12 more values of the lower one's
    # high byte below it.  low byte: the keys differ in the second radix pass only (0x3F82 / 0x3F81; 1.0 / 0x3F7F likewise);
    # high byte: 0x3F00 / 0x3EFF fall into neighbouring buckets of the first pass.  The negative pairs are the mirror
    # images, whose keys are the complements.
    for name, hi_w, lo_w in (("pair_low_byte", 0x3F82, 0x3F81), ("pair_one", 0x3F80, 0x3F7F), ("pair_high_byte", 0x3F00, 0x3EFF),
                             ("pair_low_byte_neg", 0xBF81, 0xBF82), ("pair_high_byte_neg", 0xBEFF, 0xBF00)):
        row = place(U(1000, -9, -6), [3, 250, 600, 999], [2.0, 2.5, 2.0, 2.25])
        crowd = [lo_w + 8 * j for j in range(1, 13)] if lo_w & 0x8000 else [(lo_w & 0xFF00) + 0x10 + 8 * j for j in range(12)]
        row = place(row, list(range(100, 112)), _bits(*crowd))
        row = place(row, [640, 41], _bits(hi_w, lo_w))
        out.append((name, row, 5, 1.0))
        out.append((name + "_swapped", place(row, [41, 640], _bits(hi_w, lo_w)), 5, 1.0))
    out.append(("all_equal_k5", torch.full((1000,), 0.5, dtype=BF), 5, 1.0))
    out.append(("all_equal_nocrop", torch.full((1000,), -2.0, dtype=BF), None, 0.8))
    # -inf entries: cropped away (k = 50 of 500 finite), at the threshold (k = 700: everything kept, -inf weighs 0), no crop
    inf_row = U(1000, -3, 3)
    inf_row[torch.randperm(1000, generator=g)[:500]] = -math.inf
    out += [("neg_inf_k50", inf_row, 50, 1.0), ("neg_inf_k700", inf_row, 700, 1.0), ("neg_inf_nocrop", inf_row, None, 0.8)]
    # a zero of one sign at the threshold and a zero of the other sign elsewhere: both are kept (l < kth is false for both)
    z = torch.tensor([0.0, -0.0, -1.0, 2.0], dtype=BF)
    out += [("zeros_pos_first_V4", z, 2, 1.0), ("zeros_neg_first_V4", z[[1, 0, 2, 3]], 2, 1.0)]
    wide = place(U(256, -5, -2), [200, 17, 90], [2.0, 0.0, -0.0])
    out += [("zeros_pos_first", wide, 2, 1.0), ("zeros_neg_first", place(wide, [17, 90], [-0.0, 0.0]), 2, 0.8),
            ("zeros_k3", wide, 3, 1.0)]
    return out


CRAFTED_N_SEQ = 1024
CRAFTED_STEPS = (3,)
ZERO_ROWS = ("zeros_pos_first_V4", "zeros_neg_first_V4", "zeros_pos_first", "zeros_neg_first")   # wrong before the -0 fix
