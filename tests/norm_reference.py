"""Plain CPU references, input builders, acceptance and the case table for the RMSNorm, finish-norm, fp8 row-quantisation and
embedding kernels (tests/test_hip_norm_exact.py on the GPU, tests/test_norm_reference.py on the CPU).

Everything these kernels compute is fixed by the rounding points their comments state (ger/rmsnorm.py:17-21, ger/lora.py:159-166,
DESIGN.md Q11) except ONE number per row: the fp32 order in which the row's sum of bf16-rounded squares `ss` is added.  The
references isolate it.  `ss` is summed in fp64, an interval around it that holds every fp32 summation whose chains are as long
as the kernels' (D_CHAIN) gives two candidates for ms = bf16(ss / d), and a row is DECIDED when the two are equal.  A decided
row is compared bit for bit; an undecided row must equal one of its two candidate rows bit for bit, as a whole row.  On grid
and spike inputs every partial sum of the squares is exact in fp32 in any order (the builders assert it), so ms is known and
the comparison is bit for bit throughout.  No ulp count, no allowed share of elements.

D_CHAIN.  An fp32 addition of non-negative terms has a relative error of at most u = 2^-24 (round to nearest), so a sum whose
terms each pass through at most n additions lies in [ss (1 - u)^n, ss (1 + u)^n].  Read from the kernels:
  rmsnorm_kernel (elementwise.hip)      a lane adds its 8 MAXC <= 128 squares in sequence, wave_sum has 6 butterfly stages: 134
  finish_norm_kernel, _rows_kernel      8 MAXC <= 32 per thread, 6 stages, sRed[0] + .. + sRed[3] in sequence (3):         41
  rmsnorm_quant_fp8_block_kernel        EPT <= 32 per thread, 6 stages, (a + b) + (c + d) (2):                              40
(1 + u)^134 - 1 = 134 u + 8911 u^2 < 134.001 u, and the fp64 sum of d <= 8192 squares is within 2^-39 of exact: D_CHAIN = 136
covers both with room, for all three.  Division, sqrt and reciprocal are IEEE fp32 on both sides (hipcc's default is correctly
rounded; torch's CPU fp32 ops are), fp32 division and the bf16 rounding are monotone, so the kernel's ms lies between the two
candidates, which are equal or neighbours.  With the order-free bound (d u) up to 16 % of realistic rows would be undecided;
with the chain bound about 0.2 % of the committed rows are (tests/test_norm_reference.py asserts <= 2 % per case and prints the shares).
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from dualhyp_amd.synth import stream_id, uniform
from gemm_exact_reference import InexactCase

EPS = 1e-5
U24 = 2.0 ** -24
D_CHAIN = 136
SEED = 23                           # realistic inputs: the committed seed (at most 2 % of a case's rows undecided, asserted on the CPU)
SPIKE = 32.0
GRID_Q = 0.25                       # grid values are multiples of this; their bf16-rounded squares multiples of GRID_Q^2


def rb(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 -> fp32: one rounding point"""
    return v.bfloat16().float()


def _div(a: torch.Tensor, b: float) -> torch.Tensor:
    """one correctly rounded fp32 division (tensor / tensor: a Python scalar operand may become reciprocal-then-multiply)"""
    return a / torch.full_like(a, float(b))


def bits(t: torch.Tensor) -> torch.Tensor:
    """the bit patterns of a bf16 / fp32 / uint8 tensor"""
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- references -----------------------------------------------------------------------------------------------------------
def norm_rows(x: torch.Tensor, w: torch.Tensor, eps: float, tail: Optional[torch.Tensor], ms: torch.Tensor) -> torch.Tensor:
    """bf16 [rows, d]: out = bf16(w * rb(x * r)), r = rb(1 / sqrt(t)) or, where the row's tail flag is set, rb(1 / rb(sqrt(t))),
    t = rb(ms + eps), for a given bf16-valued ms per row."""
    x, w = x.float(), w.float()
    t = rb(ms.float().view(-1, 1) + torch.tensor(eps, dtype=torch.float32))
    s = torch.sqrt(t)
    one = torch.ones_like(t)
    r = rb(one / s)
    if tail is not None:
        r = torch.where(tail.view(-1, 1).bool(), rb(one / rb(s)), r)
    return (w * rb(x * r)).bfloat16()


def squares64(x: torch.Tensor) -> torch.Tensor:
    x = x.float()
    return rb(x * x).double()


def assert_exact_sums(x: torch.Tensor, what: str) -> None:
    """Every partial sum of a row's bf16-rounded squares is exact in fp32 in ANY order: the squares are multiples of GRID_Q^2
    and a row's total stays under 2^24 of them (they are non-negative, so no partial sum exceeds the total)."""
    q = squares64(x) / (GRID_Q * GRID_Q)
    if not torch.equal(q, q.round()):
        raise InexactCase(f"{what}: {int((q != q.round()).sum())} squares are off the grid of {GRID_Q ** 2}")
    if not bool((q.sum(-1) < 2 ** 24).all()):
        raise InexactCase(f"{what}: a row's sum of squares reaches {q.sum(-1).max().item()} grid steps >= 2^24")


def ms_candidates(x: torch.Tensor, d: int, D: float = D_CHAIN) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi) fp32 [rows], bf16-valued: ms for the smallest and the largest fp32 sum within D roundings of the fp64 sum.
    D = 0: the exact sum (grid and spike rows)."""
    ss = squares64(x).sum(-1)
    return rb(_div((ss * (1 - D * U24)).float(), d)), rb(_div((ss * (1 + D * U24)).float(), d))


def candidate_rows(x: torch.Tensor, w: torch.Tensor, eps: float, tail: Optional[torch.Tensor], exact: bool):
    """(row_lo, row_hi bf16 [rows, d], undecided bool [rows]) of normalising the bf16-valued rows x"""
    lo, hi = ms_candidates(x, x.size(-1), 0 if exact else D_CHAIN)
    und = lo != hi
    a = norm_rows(x, w, eps, tail, lo)
    b = norm_rows(x, w, eps, tail, hi) if bool(und.any()) else a
    return a, b, und


def _slice_sum(h: torch.Tensor, pairs: bool) -> torch.Tensor:
    """fp32 sum over the leading dimension in the kernels' order.  pairs: acc += (h[p] + h[p + 1]) over adjacent pairs in order,
    a missing partner counts as 0; else acc += h[p] in order."""
    acc = torch.zeros_like(h[0])
    P = h.size(0)
    if pairs:
        for p in range(0, P, 2):
            acc = acc + (h[p] + (h[p + 1] if p + 1 < P else torch.zeros_like(h[p])))
    else:
        for p in range(P):
            acc = acc + h[p]
    return acc


def finish_rows(h32: torch.Tensor, n_part: int, pairs: bool, d: int, lora_b: Optional[torch.Tensor], lora_scale: float,
                x_resid: torch.Tensor) -> torch.Tensor:
    """bf16 [rows, d]: x' = bf16(x + o), o = rb(rb(acc) + rb(rb(l) * scale)) (LoRA) or rb(acc), in fp32 torch ops in the
    kernels' stated order.  h32: fp32 [n_part, rows, d (+ 16)]."""
    h = h32[:n_part].float()
    o = rb(_slice_sum(h[:, :, :d], pairs))
    if lora_b is not None:
        xa = rb(_slice_sum(h[:, :, d:d + 16], pairs))                  # [rows, 16]
        B = lora_b.float()                                             # [d, 16]
        l = torch.zeros_like(o)
        # Each product of two bf16 values has at most 16 significant bits: exact in fp32.  So the kernels' fmaf chain
        # l = fmaf(xa[k], B[c, k], l) rounds once per step, as this multiply-then-add does.
        for k in range(16):
            l = l + xa[:, k:k + 1] * B[:, k].view(1, -1)
        o = rb(o + rb(rb(l) * torch.tensor(lora_scale, dtype=torch.float32)))
    return (x_resid.float() + o).bfloat16()


def quant_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(uint8 e4m3 bytes [rows, K], fp32 scale [rows]): the oracle's row quantisation"""
    from oracle import ger_oracle as O
    q, s = O.quantize_rows_fp8(x)
    return q.view(torch.uint8), s.view(-1)


# ---- acceptance -----------------------------------------------------------------------------------------------------------
def _first_bad(ne: torch.Tensor, what: str, limit: int = 12) -> List[str]:
    """one line per failing row: (what, row, first column)"""
    rows = ne.any(-1).nonzero().flatten().tolist()
    out = [f"{what}: row {r} differs, first at column {int(ne[r].nonzero()[0])} ({int(ne[r].sum())} columns)" for r in rows[:limit]]
    if len(rows) > limit:
        out.append(f"{what}: ... and {len(rows) - limit} more rows")
    return out


def same_rows(got: torch.Tensor, want: torch.Tensor, what: str) -> List[str]:
    """bit for bit, every failing row named"""
    ne = bits(got.view(want.shape)) != bits(want)
    return _first_bad(ne.view(ne.size(0), -1), what) if bool(ne.any()) else []


@dataclass
class NormWant:
    """what a norm output may be: one of two candidate rows (the same row where the row is decided)"""
    lo: torch.Tensor
    hi: torch.Tensor
    undecided: torch.Tensor
    q: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None     # (q_lo, s_lo, q_hi, s_hi)

    def to(self, dev):
        q = None if self.q is None else tuple(t.to(dev) for t in self.q)
        return NormWant(self.lo.to(dev), self.hi.to(dev), self.undecided.to(dev), q)


def norm_want(x: torch.Tensor, w: torch.Tensor, eps: float, tail: Optional[torch.Tensor], exact: bool, quant: bool = False) -> NormWant:
    lo, hi, und = candidate_rows(x, w, eps, tail, exact)
    if exact:
        assert not bool(und.any())
    q = None
    if quant:
        ql = quant_rows(lo)
        q = ql + (ql if hi is lo else quant_rows(hi))
    return NormWant(lo, hi, und, q)


def norm_accept(want: NormWant, xn: Optional[torch.Tensor], what: str, q: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None, limit: int = 12) -> List[str]:
    """The acceptance of a norm output: every row equals, bit for bit and as a whole row, its candidate row -- one of the two
    where the row is undecided.  With q / scale: the bytes and the scale are the oracle's quantisation of THAT candidate row.
    -> one line per failing row (empty: accepted).  No row is left out."""
    R = want.lo.size(0)
    ok = [torch.ones(R, dtype=torch.bool, device=want.lo.device) for _ in range(2)]
    ne_x = ne_q = None
    if xn is not None:
        got = bits(xn.view(want.lo.shape))
        ne = [got != bits(want.lo), got != bits(want.hi)]
        ok = [o & ~n.any(-1) for o, n in zip(ok, ne)]
        ne_x = ne[0]
    if q is not None:
        q_lo, s_lo, q_hi, s_hi = want.q
        gq, gs = q.view(q_lo.shape), bits(scale.view(-1))
        ne = [(gq != q_lo) | (gs != bits(s_lo)).view(-1, 1), (gq != q_hi) | (gs != bits(s_hi)).view(-1, 1)]
        ok = [o & ~n.any(-1) for o, n in zip(ok, ne)]
        ne_q = ne[0]
    bad = (~(ok[0] | ok[1])).nonzero().flatten().tolist()
    out = []
    for r in bad[:limit]:
        und = " (undecided: neither candidate)" if bool(want.undecided[r]) else ""
        if ne_x is not None and bool(ne_x[r].any()):
            out.append(f"{what}: row {r} differs{und}, first at column {int(ne_x[r].nonzero()[0])} ({int(ne_x[r].sum())} columns)")
        elif ne_q is not None and bool(ne_q[r].any()):
            out.append(f"{what}: bytes / scale of row {r} differ{und}, first at column {int(ne_q[r].nonzero()[0])} ({int(ne_q[r].sum())} columns)")
        else:
            out.append(f"{what}: row {r}: the bf16 row and the bytes follow different candidates")
    if len(bad) > limit:
        out.append(f"{what}: ... and {len(bad) - limit} more rows")
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _grid(key, shape, kmax: int) -> torch.Tensor:
    """fp32 multiples of GRID_Q in [-kmax GRID_Q, kmax GRID_Q]"""
    return torch.randint(-kmax, kmax + 1, shape, generator=_gen(*key)).float() * GRID_Q


def grid_w(d: int) -> torch.Tensor:
    """bf16 [d] in [1, 2), multiples of 1/128, asymmetric along the row: no two 8-element chunks are equal"""
    w = 1 + torch.randint(0, 128, (d,), generator=_gen("grid_w", d)).float() / 128
    assert torch.unique(w.view(-1, 8), dim=0).size(0) == d // 8, "grid_w: two chunks are equal"
    return w.bfloat16()


def real_w(d: int) -> torch.Tensor:
    return (1 + uniform((d,), 0.25, stream_id(SEED, f"norm_w{d}")).float()).bfloat16()


def spike_positions(d: int) -> List[int]:
    """Columns p(row) of the spike sweep.  d <= 2056: every 8-element chunk in some row.  Larger d: the first and last chunk of
    every 64-chunk stride group (a lane's stride in rmsnorm_kernel and quant_rows_fp8_kernel) and of every 256-chunk group (a
    thread's stride in the block kernels), and the last two chunks of the row.  The place inside the chunk cycles 0..7."""
    n = d // 8
    if d <= 2056:
        chunks = list(range(n))
    else:
        s = set()
        for g in (64, 256):
            for c0 in range(0, n, g):
                s.update((c0, min(c0 + g, n) - 1))
        s.update((n - 2, n - 1))
        chunks = sorted(s)
    assert len(chunks) <= max(d // 8, 1)
    return [c * 8 + i % 8 for i, c in enumerate(chunks)]


def grid_rows(key, rows: int, d: int, kmax: int = 8) -> torch.Tensor:
    x = _grid(("grid", key, rows, d), (rows, d), kmax).bfloat16()
    assert_exact_sums(x, f"grid rows {key} {rows}x{d}")
    return x


def spike_rows(key, d: int) -> torch.Tensor:
    """one row per spike position: +-0.25 / +-0.5 everywhere, SPIKE at column p(row)"""
    pos = spike_positions(d)
    g = _gen("spike", key, d)
    x = (torch.randint(1, 3, (len(pos), d), generator=g).float() * (torch.randint(0, 2, (len(pos), d), generator=g).float() * 2 - 1)) * GRID_Q
    x[torch.arange(len(pos)), torch.tensor(pos)] = SPIKE
    x = x.bfloat16()
    assert_exact_sums(x, f"spike rows {key} d={d}")
    return x


def real_rows(name: str, rows: int, d: int, bound: float = 2.0) -> torch.Tensor:
    return uniform((rows, d), bound, stream_id(SEED, name))


def mixed_tail(rows: int) -> torch.Tensor:
    return (torch.arange(rows) % 3 == 1).to(torch.uint8)


def tails(rows: int) -> Dict[str, Optional[torch.Tensor]]:
    return {"none": None, "all": torch.ones(rows, dtype=torch.uint8), "mixed": mixed_tail(rows)}


# ---- RMSNorm cases -----------------------------------------------------------------------------------------------------------
NORM_D = (8, 512, 520, 2048, 2056, 3072, 4096, 4104, 8192)        # MAXC 1 | 4 | 8 | 16, full and ragged inside each class
NORM_ROWS = (1, 3, 4, 5, 259)                                     # 4 rows per block: a lone row, a ragged block, a full one, many
REAL_ROWS = 259


@dataclass(frozen=True)
class NormCase:
    d: int
    kind: str            # grid | spike | real
    rows: int
    resid: bool
    tail: str            # none | all | mixed

    @property
    def id(self) -> str:
        return f"d={self.d} {self.kind} rows={self.rows} resid={int(self.resid)} tail={self.tail}"


def norm_cases(d: int) -> List[NormCase]:
    i = NORM_D.index(d)
    T = ("none", "all", "mixed")
    out = []
    for j, rows in enumerate(NORM_ROWS):                          # every row count with and without the residual, the tails walking
        out.append(NormCase(d, "grid", rows, False, T[(i + j) % 3]))
        out.append(NormCase(d, "grid", rows, True, T[(i + j + 1) % 3]))
    n = len(spike_positions(d))
    out += [NormCase(d, "spike", n, False, T[i % 3]), NormCase(d, "spike", n, True, T[(i + 2) % 3])]
    out += [NormCase(d, "real", REAL_ROWS, r, t) for r in (False, True) for t in T]
    return out


def norm_inputs(c: NormCase) -> Dict[str, torch.Tensor]:
    """x, w (and r): bf16.  With a residual the row that is normalised is bf16(x + r) -- `sum`."""
    d = c.d
    if c.kind == "real":
        o = {"x": real_rows(f"norm_x{d}", c.rows, d), "w": real_w(d)}
        if c.resid:
            o["r"] = real_rows(f"norm_r{d}", c.rows, d, 1.0)
    else:
        o = {"w": grid_w(d)}
        if c.kind == "grid":
            o["x"] = grid_rows("x", c.rows, d, 4 if c.resid else 8)
            if c.resid:
                o["r"] = grid_rows("r", c.rows, d, 4)
        else:
            o["x"] = spike_rows("x", d)
            if c.resid:
                o["r"] = grid_rows("spike_r", c.rows, d, 2)
    o["sum"] = (o["x"].float() + o["r"].float()).bfloat16() if c.resid else o["x"]
    if c.kind != "real":
        assert_exact_sums(o["sum"], c.id)
    return o


# ---- finish-norm cases ----------------------------------------------------------------------------------------------------
FINISH_D = (64, 2048, 2056, 3072, 4096, 4104, 8192)               # MAXC 1 | 2 | 4 (256 threads x 8 columns per step)
FINISH_PARTS = ((1, 0), (2, 1), (4, 0), (5, 1), (6, 0), (11, 1), (16, 1))
FINISH_ROWS = (1, 2, 3, 5, 130)
# (key 41, key 43, key 44): plain | hoisted | the rows kernel with 2, 3, 4 rows per block and its default
FINISH_ARMS = (("plain", 0, 0, 0), ("hoisted", 1, 0, 0), ("rows2", 0, 1, 2), ("rows3", 0, 1, 3), ("rows4", 0, 1, 4), ("rows0", 0, 1, 0))
FINISH_TUNING_DEFAULTS = {41: -1, 43: -1, 44: 0}


@dataclass(frozen=True)
class FinishCase:
    d: int
    kind: str            # grid | spike | real
    rows: int
    n_part: int
    pairs: int
    lora: bool
    scale: float
    tail: str            # none | mixed
    in_place: bool = False

    @property
    def id(self) -> str:
        return (f"d={self.d} {self.kind} rows={self.rows} n_part={self.n_part} pairs={self.pairs} lora={int(self.lora)} "
                f"scale={self.scale} tail={self.tail}" + (" in-place" if self.in_place else ""))


def finish_cases(d: int) -> List[FinishCase]:
    """Grid rows carry lora_scale 2.0 (x' stays on the grid); 0.3 rides on the realistic rows, where x_out is still bit for bit."""
    i = FINISH_D.index(d)
    out = []
    for j, (n_part, pairs) in enumerate(FINISH_PARTS):
        k = i + j
        rows = FINISH_ROWS[k % 5]
        out.append(FinishCase(d, "grid", rows, n_part, pairs, k % 2 == 0, 2.0, "mixed" if k % 3 == 0 else "none"))
        out.append(FinishCase(d, "grid", 130 if rows != 130 else 5, n_part, pairs, k % 2 == 1, 2.0, "none" if k % 3 == 0 else "mixed"))
        out.append(FinishCase(d, "real", REAL_ROWS, n_part, pairs, True, 0.3 if k % 2 == 0 else 2.0, "mixed"))
    out.append(FinishCase(d, "real", REAL_ROWS, FINISH_PARTS[i][0], FINISH_PARTS[i][1], False, 2.0, "none"))
    n = len(spike_positions(d))
    out += [FinishCase(d, "spike", n, 1, 0, i % 2 == 0, 2.0, "none"), FinishCase(d, "spike", n, 2, 1, i % 2 == 1, 2.0, "mixed")]
    out.append(FinishCase(d, "grid", 130, 4, 0, True, 2.0, "none", in_place=True))         # the engine's own call
    return out


@functools.lru_cache(maxsize=1)
def _finish_real(d: int, rows: int):
    """the realistic operands of one d, drawn once: cases take leading slices and columns"""
    name = f"fin{d}"
    return (uniform((16, rows, d + 16), 2.0, stream_id(SEED, name + "h"), dtype=torch.float32), real_rows(name + "x", rows, d),
            uniform((d, 16), 0.1, stream_id(SEED, name + "b")))


def finish_inputs(c: FinishCase) -> Dict[str, torch.Tensor]:
    """h32 fp32 [n_part, rows, d (+ 16)], x bf16 [rows, d], w bf16 [d], b bf16 [d, 16] (LoRA).
    Grid and spike rows are built from factors, as a decode layer builds them: slice p of h32 is att[:, 2p:2p+2] . [W; A][:, 2p:2p+2]^T
    with att in {-1, 0, 1} / 4 and W, A, B in {-1, 0, 1}, so every partial, x.A^T, the LoRA term and x' are multiples of 1/4 --
    and the same factors go through the oracle's lora_linear on the CPU (att, W, A)."""
    d, rows, P = c.d, c.rows, c.n_part
    ld = d + (16 if c.lora else 0)
    key = (c.kind, rows, d, P, c.lora)
    if c.kind == "real":
        h, x, b = _finish_real(d, rows)
        return {"h32": h[:P, :, :ld].contiguous(), "x": x, "w": real_w(d), **({"b": b} if c.lora else {})}
    g = _gen("finish", *key)
    att = torch.randint(-1, 2, (rows, 2 * P), generator=g).float() * GRID_Q
    W = torch.randint(-1, 2, (d, 2 * P), generator=g).float()
    o = {"att": att.bfloat16(), "W": W.bfloat16(), "w": grid_w(d)}
    WA = W
    if c.lora:
        A = torch.randint(-1, 2, (16, 2 * P), generator=g).float()
        B = torch.randint(-1, 2, (d, 16), generator=g).float() * (torch.rand(d, 16, generator=g) < 0.25).float()
        WA = torch.cat([W, A])
        o.update(A=A.bfloat16(), b=B.bfloat16())
    o["h32"] = torch.stack([att[:, 2 * p:2 * p + 2] @ WA[:, 2 * p:2 * p + 2].T for p in range(P)])     # small multiples of 1/4: exact
    if c.kind == "spike":
        x = spike_rows(("fin", P), d)
    else:
        x = grid_rows(("fin", P, c.lora), rows, d, 8)
    o["x"] = x
    return o


def finish_reference(c: FinishCase, o: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, NormWant]:
    """(x_out bf16, the norm acceptance computed from it)"""
    x1 = finish_rows(o["h32"], c.n_part, bool(c.pairs), c.d, o.get("b"), c.scale, o["x"])
    exact = c.kind != "real"
    if exact:
        assert_exact_sums(x1, c.id)
    return x1, norm_want(x1, o["w"], EPS, tails(c.rows)[c.tail], exact)


# ---- RMSNorm + fp8 quantisation cases -----------------------------------------------------------------------------------------
NQ_D = (8, 2048, 2056, 3072, 4096, 4104, 8192)                    # EPT 8 | 16 | 32, full and ragged
NQ_ROWS = (1, 37, 259)


@dataclass(frozen=True)
class NormQuantCase:
    d: int
    kind: str
    rows: int
    tail: str
    xn: bool             # xn_out given (False: null)

    @property
    def id(self) -> str:
        return f"d={self.d} {self.kind} rows={self.rows} tail={self.tail} xn_out={'given' if self.xn else 'null'}"


def norm_quant_cases(d: int) -> List[NormQuantCase]:
    i = NQ_D.index(d)
    out = []
    for j, rows in enumerate((1, 37)):
        out.append(NormQuantCase(d, "grid", rows, "mixed" if (i + j) % 2 else "none", True))
        out.append(NormQuantCase(d, "grid", rows, "none" if (i + j) % 2 else "mixed", False))
    n = len(spike_positions(d))
    out += [NormQuantCase(d, "spike", n, "none", i % 2 == 0), NormQuantCase(d, "spike", n, "mixed", i % 2 == 1)]
    out += [NormQuantCase(d, "real", REAL_ROWS, t, xn) for t in ("none", "mixed") for xn in (True, False)]
    return out


def norm_quant_inputs(c: NormQuantCase) -> Dict[str, torch.Tensor]:
    return norm_inputs(NormCase(c.d, c.kind, c.rows, False, c.tail))


# ---- row quantisation cases -------------------------------------------------------------------------------------------------
QUANT_K = (8, 512, 520, 2048, 14336)
QUANT_ROWS = (1, 3, 256, 257, 259, 1030)      # <= 256: one block per row; above: one wave per row, last blocks of 1, 3 and 2 rows


def quant_inputs(K: int) -> torch.Tensor:
    """bf16 [max rows, K], cases take leading rows.  Row 1 is all zero (amax clamps to 1e-12), row 2 holds e4m3
    subnormals after scaling, every fourth row is a spike-sweep row (amax in each chunk in turn), the others are realistic."""
    n = max(QUANT_ROWS)
    x = real_rows(f"quant{K}", n, K, 3.0)
    x[1] = 0
    # |v| < 2^-13 against an amax of 3: |v| 448 / 3 < 0.0183, most of them under 2^-6 = 0.0156, the smallest normal e4m3
    x[2] = (uniform((K,), 1.0, stream_id(SEED, f"quant_sub{K}")).float() * 2.0 ** -13).bfloat16()
    x[2, K - 3] = 3.0
    sw = quant_sweep(K)
    m = min(sw.size(0), (n + 3) // 4)
    x[0:4 * m:4] = sw[:m]
    return x


def quant_sweep(K: int) -> torch.Tensor:
    """bf16 [positions, K]: small realistic values, +-SPIKE at column p(row)"""
    pos = spike_positions(K)
    x = real_rows(f"quant_sweep{K}", len(pos), K, 0.5)
    sign = torch.tensor([1.0 if i % 2 else -1.0 for i in range(len(pos))])
    x[torch.arange(len(pos)), torch.tensor(pos)] = (sign * SPIKE).bfloat16()
    return x


# ---- embedding cases --------------------------------------------------------------------------------------------------------
EMBED_D = (8, 256, 3072)
EMBED_VOCAB = 37
EMBED_IDS = (-1, EMBED_VOCAB, 3, EMBED_VOCAB + 7, 0, EMBED_VOCAB - 1)     # n_tok leading ids; -1 -> row 0, vocab and vocab + 7 -> row vocab - 1
EMBED_NTOK = (1, 5, 6)                                                      # 4 tokens per block: a lone one, a ragged second block


def embed_want(wte: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    return wte[ids.clamp(0, wte.size(0) - 1)]


# ---- CPU restatements of the kernels with a switch for deliberate defects (tests/test_norm_reference.py, sensitivity) -------------
def emulate_ss(x: torch.Tensor, defect: Optional[str] = None) -> torch.Tensor:
    """fp32 [rows]: the sum of squares in the wave-per-row order of rmsnorm_kernel (lane l adds chunks l, l + 64, .. in sequence,
    then the xor butterfly 32, 16, .. 1).  defects: drop_last_chunk | double_chunk."""
    x = x.float()
    R, d = x.shape
    n = d // 8
    sq = rb(x * x).view(R, n, 8)
    if defect == "drop_last_chunk":
        sq = sq.clone()
        sq[:, n - 1] = 0
    if defect == "double_chunk":
        sq = torch.cat([sq, sq[:, 0:1]], dim=1)
        n += 1
    per = -(-n // 64)
    pad = torch.zeros(R, per * 64, 8)
    pad[:, :n] = sq
    lanes = pad.view(R, per, 64, 8)
    acc = torch.zeros(R, 64)
    for i in range(per):
        for j in range(8):
            acc = acc + lanes[:, i, :, j]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, torch.arange(64) ^ o]
    return acc[:, 0]


def emulate_norm(x: torch.Tensor, w: torch.Tensor, eps: float, tail: Optional[torch.Tensor], defect: Optional[str] = None) -> torch.Tensor:
    """defects: drop_last_chunk | double_chunk | divisor | ignore_tail"""
    d = x.size(-1)
    ms = rb(_div(emulate_ss(x, defect), d + 8 if defect == "divisor" else d))
    return norm_rows(x, w, eps, None if defect == "ignore_tail" else tail, ms)


def emulate_finish(h32: torch.Tensor, n_part: int, pairs: bool, d: int, lora_b, lora_scale: float, x_resid: torch.Tensor,
                   defect: Optional[str] = None) -> torch.Tensor:
    """x_out with a defect: pairs_in_sequence | odd_partner_p0 | xa_previous_row"""
    h = h32[:n_part].float()
    if defect == "pairs_in_sequence":
        pairs = False
    if defect == "odd_partner_p0" and pairs and n_part % 2:
        h = torch.cat([h, h[4 * ((n_part - 1) // 4):4 * ((n_part - 1) // 4) + 1]])           # the partner of the last slice: slice p0 of its group of 4
        n_part += 1
    if defect == "xa_previous_row" and lora_b is not None:
        h = h.clone()
        h[:, :, d:] = torch.roll(h[:, :, d:], 1, dims=1)
    return finish_rows(h, n_part, pairs, d, lora_b, lora_scale, x_resid)


def emulate_quant(x: torch.Tensor, defect: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """defect: amax_without_last_chunk"""
    xf = x.float()
    K = xf.size(-1)
    amax = (xf[:, :K - 8] if defect == "amax_without_last_chunk" and K > 8 else xf).abs().amax(-1, keepdim=True).clamp_min(1e-12)
    inv = torch.full_like(amax, 448.0) / amax
    return (xf * inv).to(torch.float8_e4m3fn).view(torch.uint8), (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).view(-1)
