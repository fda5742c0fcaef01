"""Exact-integer references, guard bands and the case table for the bf16 GEMM family (tests/test_hip_gemm_exact.py on the GPU,
tests/test_gemm_exact_reference.py on the CPU).

Every operand is a small integer, so every product, partial sum and rounding point of a GEMM and its epilogue is an exactly
representable integer: the result does not depend on the summation order, and every kernel must reproduce the fp64 product —
no ulp allowance, no allowed share of differing elements.  The references below are written in fp64 (exact for these integers,
|value| < 2^53) with the library's documented rounding points (include/dualhyp_hip.h) spelled out, and at EVERY rounding point
they assert that the value survives `.bfloat16()` unchanged.  That is a condition on the inputs, not a tolerance: a case that
breaks it raises InexactCase, nothing is clipped.  Only the SwiGLU epilogue has an inexact step (silu); see swiglu_accept.

Results are compared by VALUE (-0.0 == 0.0; a NaN equals nothing).
"""
from __future__ import annotations

import math
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

# ---- route record: the bit numbers of enum DhGemmRoute (dualhyp_amd/csrc/gemm.h), read through dh_debug_gemm_routes ----------
ROUTES = ("t128_s2", "t128_s4", "w8_pipe0", "w8_pipe1", "w8_pipe2", "w8_pipe3", "w4_tile", "w4_persist", "w4_xa",
          "mid_ng1", "mid_ng2", "mid_ng4", "mid_ng1_ring", "mid_ng2_ring", "dt_fused", "skinny", "swiglu_skinny2", "skinny_n",
          "k64", "k64_mul", "rows", "partial_waves", "pairs_tiled", "chain_tiled",
          # the quantised GEMMs (csrc/fp8.hip, csrc/mxfp4.hip): their cases are tests/qgemm_exact_reference.py's
          "fp8_stream_ng1", "fp8_stream_ng2", "fp8_stream_ng4", "fp8_t128_s4", "fp8_t128_s2", "fp8_t256",
          "mx4_stream_ng1", "mx4_stream_ng2", "mx4_stream_ng4", "mx4_t128_s4", "mx4_t128_s2")


def route_names(mask: int) -> frozenset:
    assert mask >> len(ROUTES) == 0, f"route mask {mask:#x} has bits this table does not know"
    return frozenset(n for i, n in enumerate(ROUTES) if mask >> i & 1)


# every dh_set_tuning key the table touches -> the library's default (restored after each case)
TUNING_DEFAULTS = {0: 1, 1: 5, 2: 1, 4: 0, 6: 129, 7: 1 << 30, 8: 0, 9: 0, 11: 0, 13: 1, 14: 0, 15: 0, 17: 0, 21: 0, 22: 1, 28: 1, 30: 1,
                   31: 1}


class InexactCase(AssertionError):
    """A rounding point of a case's reference is not exactly representable: the case's operands are wrong for an exact test."""


def exact_bf16(v: torch.Tensor, what: str) -> torch.Tensor:
    """`v` (fp64), asserted to survive a round trip through bf16 unchanged."""
    if not torch.equal(v.bfloat16().double(), v):
        bad = v[v.bfloat16().double() != v]
        raise InexactCase(f"{what}: {bad.numel()} values are not bf16-representable (e.g. {bad.flatten()[0].item()}, max |v| {v.abs().max().item()})")
    return v


def exact_f32(v: torch.Tensor, what: str) -> torch.Tensor:
    if not bool((v.abs() < 2 ** 24).all()):
        raise InexactCase(f"{what}: |value| reaches {v.abs().max().item()} >= 2^24")
    return v


# ---- cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    family: str                       # the GPU test function that runs it
    group: str                        # the parametrize id inside the family
    op: str                           # linear | linear_lora | linear_mul | swiglu_train | partial | pairs | chain
    M: int
    N: int                            # output columns (SwiGLU: pairs; partial family: n_main)
    K: int
    epi: str = "plain"                # plain | lora | swiglu | adapter
    resid: bool = False
    splits: Optional[Tuple[int, int]] = None
    lora_scale: float = 1.0
    n_ext: int = 0
    ksplit: int = 1
    thin: bool = False                # W (and w2) with half of the entries zeroed: larger K inside the exact range
    tune: Tuple[Tuple[int, int], ...] = ()
    routes: Tuple[str, ...] = ()      # the exact set of kernels the call must launch ...
    tail_routes: Tuple[str, ...] = () # ... and, when the dispatcher's row split applies (row_split), these as well

    @property
    def data_key(self):
        """Cases with the same key share operands and reference (they differ in tuning only)."""
        return (self.op, self.M, self.N, self.K, self.epi, self.resid, self.splits, self.lora_scale, self.n_ext, self.ksplit, self.thin)

    @property
    def id(self) -> str:
        t = ",".join(f"{k}={v}" for k, v in self.tune)
        e = self.epi + ("+resid" if self.resid else "") + (f"{self.splits}" if self.splits else "")
        x = f" n_ext={self.n_ext} ksplit={self.ksplit}" if self.op in ("partial", "pairs", "chain") else ""
        return f"{self.op} {e} M={self.M} N={self.N} K={self.K}{x} tune[{t}] -> {'+'.join(self.routes)}"


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def is_big(M: int, N: int, swiglu: bool = False) -> bool:
    """The 256-tile kernels' range: at least 128 tiles of 256 rows x 256 columns (SwiGLU: 128 pairs)."""
    w = 128 if swiglu else 256
    return M >= 256 and N >= w and cdiv(M, 256) * cdiv(N, w) >= 128


def row_split(M: int, N: int, n_cu: int) -> Optional[Tuple[int, int]]:
    """(M1, M2) when a plain / LoRA GEMM in the 256-tile range is split by rows (gemm.hip, "wave quantisation"): the grid is
    R >= 1 full rounds of one tile per CU plus a remainder of at most 0.3 round; the row tiles of the full rounds go to the
    256-tile kernel, the remaining M2 <= 4096 rows to the 128-tile kernel.  None: one launch.
    (This, w4_route and mid_route restate the dispatcher's documented conditions to predict a route.  The table's 4097 x 4104
    shape is chosen for 256 CUs: on a device with another CU count the split may not apply, and the 256-tile + 128-tile pair
    is then asserted nowhere on the GPU.)"""
    nbn = cdiv(N, 256)
    tiles = cdiv(M, 256) * nbn
    rounds, rem = divmod(tiles, n_cu)
    M1 = rounds * n_cu // nbn * 256
    M2 = M - M1
    if rounds >= 1 and rem > 0 and rem * 10 <= n_cu * 3 and 0 < M2 <= 4096 and is_big(M1, N) and not is_big(M2, N):
        return M1, M2
    return None


def expected_routes(c: Case, n_cu: int) -> frozenset:
    r = set(c.routes)
    if c.tail_routes and row_split(c.M, c.N, n_cu) is not None:
        r |= set(c.tail_routes)
    return frozenset(r)


# ---- operands -------------------------------------------------------------------------------------------------------------
def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(key, shape, lo: int, hi: int) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=_gen(*key)).double()


def _x(M, K):
    x = _ints(("x", M, K), (M, K), -2, 2)
    x[:, ::7] = 1.0                 # symmetry breakers (as tests/test_hip_fp8.py): fixed values on strided k columns, different
    return x                        # strides and values for the two operands -> an operand swap or a k permutation shows


def _w(tag, N, K, thin):
    w = _ints((tag, N, K), (N, K), -1, 1)
    if thin:
        w = w * _ints((tag, "thin", N, K), (N, K), 0, 1)
    w[:, ::5] = -1.0 if tag != "w2" else 1.0
    return w


def _sparse_rows(key, rows: int, cols: int, nnz: int) -> torch.Tensor:
    """{-1, 0, 1} with exactly `nnz` non-zeros per row (bounds the LoRA branch: |x.A^T| <= 2 nnz, |xa.B^T| <= nnz max|xa|)."""
    g = _gen(*key)
    out = torch.zeros(rows, cols, dtype=torch.float64)
    pos = torch.rand(rows, cols, generator=g).argsort(dim=1)[:, :nnz]
    sign = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    out.scatter_(1, pos, sign)
    return out


def n_seg(c: Case) -> int:
    s0, s1 = c.splits if c.splits else (c.N, c.N)
    return 1 + (s0 < c.N) + (s1 < c.N)


def operands(c: Case) -> Dict[str, torch.Tensor]:
    """fp64 integer tensors of a case (CPU)."""
    M, N, K = c.M, c.N, c.K
    o = {"x": _x(M, K), "w": _w("w", N, K, c.thin)}
    if c.op in ("partial", "pairs", "chain"):
        if c.n_ext:
            o["w_ext"] = _w("w_ext", c.n_ext, K, c.thin)
        return o
    if c.epi == "swiglu" or c.op == "swiglu_train":
        o["w2"] = _w("w2", N, K, c.thin)
    if c.op == "linear_mul":
        o["mul"] = _ints(("mul", M, N), (M, N), 0, 2)
    if c.epi == "lora":
        ns = n_seg(c)
        if c.op == "linear_lora":
            o["lora_a"] = _sparse_rows(("lora_a", ns, K), 16 * ns, K, 4)          # |x.A^T| <= 8
            o["lora_b"] = _sparse_rows(("lora_b", N), N, 16, 4)                   # |xa.B^T| <= 32
        else:
            xa = _ints(("xa", M, ns), (M, 16 * ns), -2, 2)
            for s in range(ns):                                                 # the segments are told apart: independent draws and
                xa[:, 16 * s + s] = 2.0 - s                                     # a fixed column whose place and value depend on the segment
            o["xa"] = xa
            o["lora_b"] = _ints(("lora_b", N), (N, 16), -1, 1)
    if c.epi == "adapter":
        o["scale"] = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (N,), generator=_gen("scale", N))].double()
        o["bias"] = _ints(("bias", N), (N,), -4, 4)
    if c.resid:
        o["resid"] = _ints(("resid", M, N), (M, N), -64, 64)
    return o


# ---- references -----------------------------------------------------------------------------------------------------------
def _lora_term(c: Case, xa: torch.Tensor, lora_b: torch.Tensor) -> torch.Tensor:
    """bf16(bf16(xa_seg . B^T) * s) with seg(n) = (n >= split0) + (n >= split1)"""
    s0, s1 = c.splits if c.splits else (c.N, c.N)
    bounds = [0, min(s0, c.N), min(s1, c.N), c.N]
    out = torch.empty(c.M, c.N, dtype=torch.float64)
    seg = 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi > lo:
            lacc = exact_bf16(xa[:, 16 * seg:16 * seg + 16] @ lora_b[lo:hi].T, "lora_acc")
            out[:, lo:hi] = exact_bf16(lacc * c.lora_scale, "lora_acc * s")
            seg += 1
    return out


def reference(c: Case, o: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The exact outputs of a case: {"y"} | {"g", "u"} (SwiGLU: see swiglu_accept) | {"xa_work"} (linear_lora's two-launch
    form) | {"parts"} (fp32 partial family).  Raises InexactCase where a rounding point would round."""
    x, w = o["x"], o["w"]
    if c.op in ("partial", "pairs", "chain"):
        wf = torch.cat([w, o["w_ext"]]) if c.n_ext else w
        return {"parts": exact_f32(partial_slices(c, x, wf), "partial sums")}
    acc = exact_bf16(x @ w.T, "acc")
    if c.epi == "swiglu" or c.op == "swiglu_train":
        return {"g": acc, "u": exact_bf16(x @ o["w2"].T, "acc2")}
    y = acc
    out = {}
    if c.op == "linear_mul":
        y = exact_bf16(y * o["mul"], "bf16(acc) * mul")
    if c.epi == "lora":
        xa = o["xa"] if c.op == "linear" else exact_bf16(x @ o["lora_a"].T, "x.A^T")
        if c.op == "linear_lora":
            out["xa_work"] = xa
        y = exact_bf16(y + _lora_term(c, xa, o["lora_b"]), "acc + lora")
    if c.epi == "adapter":
        y = exact_bf16(o["scale"] * exact_bf16(y + o["bias"], "acc + bias"), "scale * (acc + bias)")
    if c.resid:
        y = exact_bf16(o["resid"] + y, "resid + y")
    out["y"] = y
    return out


def slice_ksteps(c: Case) -> List[List[int]]:
    """The 32-wide k-steps of each K-slice of dh_linear_partial_bf16 (include/dualhyp_hip.h).  Whole slices of 8 or 16 k-steps:
    contiguous, slice p = k-steps [p kps, (p+1) kps).  Any other (K, ksplit): runs of 8 k-steps dealt round robin, k-step ks
    in slice (ks / 8) % ksplit."""
    nks = c.K // 32
    kps = cdiv(nks, c.ksplit)
    if kps in (8, 16) and kps * c.ksplit == nks:
        return [list(range(p * kps, (p + 1) * kps)) for p in range(c.ksplit)]
    return [[ks for ks in range(nks) if ks // 8 % c.ksplit == p] for p in range(c.ksplit)]


def partial_slices(c: Case, x: torch.Tensor, wf: torch.Tensor) -> torch.Tensor:
    """fp64 [ksplit, M, N]: the slices; `pairs` cases: [(ksplit+1)//2, M, N] sums of adjacent slices; `chain`: [1, M, N] the total"""
    sl = []
    for steps in slice_ksteps(c):
        cols = torch.tensor([32 * ks + j for ks in steps for j in range(32)], dtype=torch.long)
        sl.append(x[:, cols] @ wf[:, cols].T if len(steps) else torch.zeros(c.M, wf.size(0), dtype=torch.float64))
    if c.op == "pairs":
        sl = [sl[i] + sl[i + 1] if i + 1 < len(sl) else sl[i] for i in range(0, len(sl), 2)]
    if c.op == "chain":
        sl = [sum(sl[1:], sl[0])]
    return torch.stack(sl)


# ---- SwiGLU acceptance ----------------------------------------------------------------------------------------------------
SILU_G_MAX = 512


def _bf16_value(o: int) -> float:
    """the bf16 number of ORDERED index o (sign * magnitude bits: o and o + 1 are neighbours, 0 is +-0)"""
    bits = o if o >= 0 else (0x8000 | -o)
    return struct.unpack("<f", struct.pack("<I", bits << 16))[0]


def silu_candidates() -> torch.Tensor:
    """fp32 [2 * SILU_G_MAX + 1, 3]: for integer g = row - SILU_G_MAX, the bf16 value nearest to silu(g) = g / (1 + e^-g)
    evaluated in fp64 (column 0) and that value's two bf16 neighbours (columns 1, 2)."""
    rows = []
    for g in range(-SILU_G_MAX, SILU_G_MAX + 1):
        v = g / (1.0 + math.exp(-g))
        f32 = struct.unpack("<I", struct.pack("<f", v))[0]
        o = (f32 >> 16) & 0x7FFF
        o = -o if f32 >> 31 else o
        best = min(range(o - 2, o + 3), key=lambda k: (abs(_bf16_value(k) - v), abs(k)))
        rows.append([_bf16_value(best), _bf16_value(best - 1), _bf16_value(best + 1)])
    return torch.tensor(rows, dtype=torch.float32)


_SILU = None

# The fp32 underflow range of silu, stated here and counted apart — not a silent allowance.  From this g down the sigmoid
# 1 / (1 + e^-g) is below 2^-126, the smallest normal fp32: an fp32 evaluation of silu holds a denormal factor there, and the
# hardware reciprocal silu_fast uses (csrc/common.h) returns it as zero.  The reference model's own fp32 form g / (1 + expf(-g)),
# torch's silu and the library's DH_SILU_EXACT build alike, is -0 from one integer further down (expf(89) is inf).  |silu(g)| is
# at most 5.3e-37 in the range, and from g = -97 down zero is a bf16 neighbour of the true value anyway.  Measured on an MI355X
# with the table below: every SwiGLU kernel returns -0.0 at the integers g = -96 .. -88 (all that occur), nothing else differs.
SILU_FLUSH_G = max(g for g in range(-SILU_G_MAX, 0) if 1.0 / (1.0 + math.exp(-g)) < 2.0 ** -126)       # -88


def swiglu_accept(got: torch.Tensor, g: torch.Tensor, u: torch.Tensor):
    """-> (ok [bool, shape of got], n_neighbour, n_flushed): got == bf16(s * u) for s = the bf16 nearest to the fp64 silu(g) or
    one of its two neighbours; for g <= SILU_FLUSH_G (see above) also a zero, the flushed fp32 sigmoid — nothing else.  g and u
    are the exact integer pre-activations (any float dtype, any device), so the product of the bf16 s with u is exact in fp32
    and its rounding to bf16 is the epilogue's last step.  n_neighbour counts the outputs that match through a neighbour only,
    n_flushed those that match through the flushed zero only."""
    global _SILU
    if _SILU is None:
        _SILU = silu_candidates()
    assert float(g.abs().max()) <= SILU_G_MAX
    tab = _SILU.to(g.device)
    s = tab[(g.long() + SILU_G_MAX).flatten()].view(*g.shape, 3)
    want = (s * u.float().unsqueeze(-1)).bfloat16().float()
    hit = want == got.float().unsqueeze(-1)
    near = hit.any(-1)
    flushed = (g <= SILU_FLUSH_G) & (got.float() == 0) & ~near
    return near | flushed, int((near & ~hit[..., 0]).sum()), int(flushed.sum())


def swiglu_failures(got: torch.Tensor, g: torch.Tensor, u: torch.Tensor, ok: torch.Tensor, limit: int = 12) -> str:
    """the distinct g of the rejected outputs, for the assertion message"""
    bad = ~ok
    gs = torch.unique(g[bad]).tolist()
    i = bad.nonzero()[0].tolist()
    return (f"{int(bad.sum())} outputs outside the acceptance; g values {gs[:limit]}{' ...' if len(gs) > limit else ''}; first at {i}: "
            f"g={g[tuple(i)].item()} u={u[tuple(i)].item()} got={got[tuple(i)].item()}")


# ---- guard bands ----------------------------------------------------------------------------------------------------------
SENTINEL_BF16 = 0x7FA5            # a bf16 NaN with a payload: no arithmetic produces this bit pattern
SENTINEL_F32 = 0x7FA5A5A5
SENTINEL_U8 = 0x7F                # e4m3fn bytes: the NaN, which the quantisation of a finite row never produces
GUARD_ROWS = 256                  # output margins: one full band of the largest tile, so that a whole stray tile lands in a guard


class Guarded:
    """A tensor embedded in a larger flat buffer, `margin` elements (rounded up to 16 bytes) on both sides, the whole buffer
    filled with the sentinel NaN of its dtype (bf16, fp32, or uint8 holding e4m3fn bytes).  `.t` is the embedded tensor (contiguous, 16-byte aligned as the
    ABI requires).  Inputs: `.t.copy_(values)`; a kernel that reads an out-of-range row picks up NaN.  Outputs: after the call
    `check()` wants both margins bit-identical to the sentinel and no sentinel left inside."""

    def __init__(self, shape, dtype, device, margin: int, values: Optional[torch.Tensor] = None):
        assert dtype in (torch.bfloat16, torch.float32, torch.uint8)
        self.idt, self.sentinel, size = {torch.bfloat16: (torch.int16, SENTINEL_BF16, 2), torch.float32: (torch.int32, SENTINEL_F32, 4),
                                         torch.uint8: (torch.uint8, SENTINEL_U8, 1)}[dtype]
        per16 = 16 // size
        n = 1
        for d in shape:
            n *= int(d)
        self.pre = cdiv(max(margin, 1), per16) * per16
        self.n = n
        post_pad = -n % per16                       # the margin behind starts at the next 16-byte boundary
        self.post0 = self.pre + n + post_pad
        self.raw = torch.empty(self.post0 + self.pre, dtype=self.idt, device=device)
        self.t = self.raw[self.pre:self.pre + n].view(dtype).view(*shape)
        self.refill()
        if values is not None:
            self.t.copy_(values)

    def refill(self) -> None:
        self.raw.fill_(self.sentinel)

    def check(self, what: str, written: bool = True) -> None:
        s = self.sentinel
        before, after = self.raw[:self.pre], self.raw[self.pre + self.n:]
        nb, na = int((before != s).sum()), int((after != s).sum())
        assert nb == 0, f"{what}: {nb} elements written BEFORE the tensor (first at offset {int((before != s).nonzero()[0]) - self.pre})"
        assert na == 0, f"{what}: {na} elements written BEHIND the tensor (first at offset +{int((after != s).nonzero()[0])})"
        left = self.raw[self.pre:self.pre + self.n] == s
        if written:
            nl = int(left.sum())
            assert nl == 0, f"{what}: {nl} elements never written (first flat index {int(left.nonzero()[0]) if nl else -1})"


def guard_rows(shape) -> int:
    """margin in elements for a [.., rows, cols] output: GUARD_ROWS rows"""
    return GUARD_ROWS * int(shape[-1])


# ---- the case table -------------------------------------------------------------------------------------------------------
def _t128_cases() -> List[Case]:
    Ms, Ns, Ks = (1, 127, 128, 129, 257), (8, 120, 128, 136, 264), (64, 128, 192, 256, 320)
    three = {120: (32, 64), 128: (32, 96), 136: (32, 96), 264: (96, 160)}          # segment boundaries off the 128-column tile grid
    out = []

    def add(group, M, N, K, **kw):
        for st in (2, 4):
            tune = ((1, 0), (9, st)) + (((4, 1),) if M <= 32 else ())
            out.append(Case("t128", group, "linear", M, N, K, tune=tune, routes=("t128_s2" if st == 2 else "t128_s4",), **kw))

    for K in Ks:
        for M in Ms:
            for N in Ns:
                add(f"plain-K{K}", M, N, K)
    # the other epilogues: every M, every N and every K at least once each (all M x N pairs, K walking the diagonal)
    for i, M in enumerate(Ms):
        for j, N in enumerate(Ns):
            K = Ks[(i + j) % 5]
            add("resid", M, N, K, resid=True)
            add("lora1", M, N, K, epi="lora", lora_scale=2.0)
            add("lora1+resid", M, N, K, epi="lora", resid=True)
            if N in three:                                                          # (N = 8 has no room for a second segment)
                add("lora3", M, N, Ks[(i + j + 1) % 5], epi="lora", splits=three[N], lora_scale=2.0)
                add("lora3+resid", M, N, Ks[(i + j + 2) % 5], epi="lora", splits=three[N], resid=True)
            add("adapter", M, N, K, epi="adapter")
            add("adapter+resid", M, N, K, epi="adapter", resid=True)
        for j, N in enumerate((32, 96, 160)):
            for dk in (0, 2, 3):                                                    # 5 M x 3 N x 3 K offsets: every K at every N
                add("swiglu", M, N, Ks[(i + j + dk) % 5], epi="swiglu")
    return out


def w4_route(epi: str, resid: bool, K: int, p22: int, p30: int) -> str:
    """4-wave kernel: persistent blocks by dh_set_tuning 22 (0 never, 1 where the epilogue loads nothing: plain and SwiGLU,
    2 always) and 30 (plain + residual and LoRA), and only with an even number of 64-deep stages."""
    persist = p22 == 2 or (p22 == 1 and ((epi == "plain" and not resid) or epi == "swiglu")) or (p30 and (epi == "lora" or (epi == "plain" and resid)))
    return "w4_persist" if persist and (K // 64) % 2 == 0 else "w4_tile"


def _w256_variants(epi: str, resid: bool, K: int):
    """(tune, route) of every loop variant of the 256-tile kernels for one epilogue"""
    for v, pipe in ((1, "w8_pipe2"), (2, "w8_pipe1"), (3, "w8_pipe0"), (4, "w8_pipe3" if epi in ("plain", "swiglu") else "w8_pipe2")):
        yield ((1, v),), pipe
    for p22 in (0, 1, 2):
        for p30 in (0, 1):
            # K = 64: one stage — the 4-wave kernel needs two, every variant runs on the 8-wave kernel
            yield ((1, 5), (22, p22), (30, p30)), ("w8_pipe2" if K < 128 else w4_route(epi, resid, K, p22, p30))


def _w256_cases() -> List[Case]:
    out = []
    for M, N in ((2049, 3592), (4097, 4104)):
        for K in (64, 128, 192, 256, 320):
            epis = [("plain", dict()), ("resid", dict(resid=True)), ("lora", dict(epi="lora", splits=(1056, 2336), lora_scale=2.0)),
                    ("lora+resid", dict(epi="lora", splits=(1056, 2336), resid=True)), ("swiglu", dict(epi="swiglu")), ("adapter", dict(epi="adapter"))]
            for name, kw in epis:
                epi, resid = kw.get("epi", "plain"), kw.get("resid", False)
                n = 1824 if epi == "swiglu" else N
                group = f"{name}-{M}x{n}-K{K}"
                # one launch: the row split off (key 28), and for plain K = 64 the k64 kernel off (key 31)
                fixed = ((28, 0),) + (((31, 0),) if K == 64 and name == "plain" else ())
                for tune, route in _w256_variants(epi, resid, K):
                    out.append(Case("w256", group, "linear", M, n, K, tune=tune + fixed, routes=(route,), **kw))
                if epi in ("plain", "lora"):
                    # default tuning: a grid with a small last round is split by rows, the tail on the 128-tile kernel (257 x 4104:
                    # 99 blocks -> 4 stages); 2049 x 3592 is under one round and stays one launch
                    if K == 64 and name == "plain":
                        out.append(Case("w256", group, "linear", M, n, K, routes=("k64",), **kw))
                    else:
                        route = "w8_pipe2" if K < 128 else w4_route(epi, resid, K, 1, 1)
                        out.append(Case("w256", group, "linear", M, n, K, routes=(route,), tail_routes=("t128_s4",), **kw))
    return out


def _xa_cases() -> List[Case]:
    out = []
    M, N = 2049, 3592
    for K in (128, 192, 256):
        even = (K // 64) % 2 == 0
        for p30 in (0, 1):
            w4 = "w4_persist" if p30 and even else "w4_tile"       # an odd number of stages takes the non-persistent form
            tune = ((30, p30),)
            g = f"K{K}"
            out.append(Case("xa", g, "linear_lora", M, N, K, epi="lora", splits=(2048, 2304), lora_scale=2.0, tune=tune, routes=(w4, "w4_xa")))
            out.append(Case("xa", g, "linear_lora", M, N, K, epi="lora", resid=True, tune=tune, routes=(w4, "w4_xa")))
            # a segment boundary off the 256-column grid: x.A^T by its own launch (48 columns: the skinny-N kernel), then the LoRA GEMM
            out.append(Case("xa", g, "linear_lora", M, N, K, epi="lora", splits=(2016, 2336), lora_scale=2.0, tune=tune, routes=("skinny_n", w4)))
    return out


def _mul_cases() -> List[Case]:
    M, N = 2049, 3592
    return [Case("mul", "K64-k64", "linear_mul", M, N, 64, routes=("k64_mul",)),
            Case("mul", "K64-w8", "linear_mul", M, N, 64, tune=((31, 0),), routes=("w8_pipe2",)),
            Case("mul", "K128", "linear_mul", M, N, 128, routes=("w8_pipe2",)),
            Case("mul", "K256", "linear_mul", M, N, 256, routes=("w8_pipe2",))]


def _swiglu_train_cases() -> List[Case]:
    out = []
    for K in (128, 256):
        out.append(Case("swiglu_train", f"fused-K{K}", "swiglu_train", 2049, 1824, K, epi="swiglu", routes=("w4_persist",)))
        out.append(Case("swiglu_train", f"three-launch-K{K}", "swiglu_train", 300, 1824, K, epi="swiglu", routes=("t128_s4",)))
    return out


def _k64_skinny_n_cases() -> List[Case]:
    out = []
    for M in (512, 513, 575):
        for N in (256, 264, 520):
            out.append(Case("k64_skinny_n", "k64", "linear", M, N, 64, routes=("k64",)))
    for K in (64, 128, 192, 256, 320):
        for M in (512, 513, 577):
            for N in (16, 32, 48, 64):
                out.append(Case("k64_skinny_n", f"skinny_n-K{K}", "linear", M, N, K, routes=("skinny_n",)))
    return out


def mid_route(M: int, K: int, epi: str, ring: int, dt_min_rows: int = 129) -> str:
    """decode phase (dh_set_tuning 4 = 2).  gemm_dt takes > 64 rows from dt_min_rows on (adapter: 65) when a K-part is an even
    number of k-steps (K / 32 / 2, SwiGLU K / 32 / 4); else gemm_mid with 1 / 2 / 4 groups of 32 rows, W through the LDS ring
    for up to 2 groups when key 13 is set and K is a multiple of 64 per K-part."""
    kq = 4 if epi == "swiglu" else 2
    if M > 64 and M >= (min(dt_min_rows, 65) if epi == "adapter" else dt_min_rows) and (K // 32 // kq) % 2 == 0:
        return "dt_fused"
    ng = 1 if M <= 32 else 2 if M <= 64 else 4
    return f"mid_ng{ng}" + ("_ring" if ng <= 2 and ring and K % (64 * kq) == 0 else "")


def _mid_cases() -> List[Case]:
    out = []
    for K in (128, 256, 384, 512, 640):
        for name, kw in (("plain", {}), ("resid", dict(resid=True)), ("swiglu", dict(epi="swiglu")), ("adapter", dict(epi="adapter"))):
            epi = kw.get("epi", "plain")
            for M in (1, 31, 32, 33, 63, 64, 65, 128, 257):
                route = mid_route(M, K, epi, 1)
                if M == 257 and route == "dt_fused":
                    continue                                       # 257 rows only where gemm_dt refuses (SwiGLU, odd K-part)
                for N in (16, 48, 144):
                    for ring in (0, 1):
                        out.append(Case("mid", f"{name}-K{K}", "linear", M, N, K, tune=((4, 2), (13, ring)), routes=(mid_route(M, K, epi, ring),), **kw))
    return out


def _dt_cases() -> List[Case]:
    out = []
    for name, kw, Ks in (("plain", {}, (128, 256, 384, 512)), ("resid", dict(resid=True), (128, 256, 384, 512)),
                         ("swiglu", dict(epi="swiglu"), (256, 512, 768))):
        for K in Ks:
            for M in (65, 129, 255, 257):
                for N in (16, 144, 272):
                    for st in (2, 4):
                        for wide in (-1, 0, 1):
                            out.append(Case("dt", f"{name}-K{K}", "linear", M, N, K, tune=((4, 2), (6, 65), (8, st), (15, wide)), routes=("dt_fused",), **kw))
    return out


def _skinny_cases() -> List[Case]:
    out = []
    for K in (64, 192, 320):
        for M in (1, 15, 16, 17, 31, 32):
            for N in (8, 24, 136):
                for resid in (False, True):
                    r = dict(resid=resid)
                    out.append(Case("skinny", f"plain-K{K}", "linear", M, N, K, routes=("skinny",), **r))
                    out.append(Case("skinny", f"lora-K{K}", "linear", M, N, K, epi="lora", lora_scale=2.0, routes=("skinny",), **r))
                    if N == 136:
                        out.append(Case("skinny", f"lora-K{K}", "linear", M, N, K, epi="lora", splits=(32, 96), routes=("skinny",), **r))
                    out.append(Case("skinny", f"adapter-K{K}", "linear", M, N, K, epi="adapter", routes=("skinny",), **r))
            for N in (32, 96):
                for k2 in (0, 1):
                    out.append(Case("skinny", f"swiglu-K{K}", "linear", M, N, K, epi="swiglu", tune=((2, k2),),
                                    routes=("swiglu_skinny2" if k2 else "skinny",)))
    return out


def _partial_cases() -> List[Case]:
    out = []
    whole = ((256, 1), (512, 1), (512, 2), (2048, 8), (2048, 4))
    for K, ks in whole:
        for M in (1, 32, 33, 127, 129, 640):
            # above 128 rows the rows kernel has forms by column tiles per wave (key 11) and row groups per block (key 14)
            tunes = [((11, ct), (14, ng)) for ct in (0, 1, 2, 4) for ng in (0, 8, 10)] if M > 128 else [()]
            for n_main in (16, 144):
                for n_ext in (0, 16, 48):
                    for tune in tunes:
                        out.append(Case("rows", f"K{K}-ksplit{ks}", "partial", M, n_main, K, n_ext=n_ext, ksplit=ks, tune=tune, routes=("rows",)))
    for K, ks in ((384, 2), (96, 1), (320, 3)):
        for M in (1, 33, 100):
            for n_main in (16, 144):
                for n_ext in (0, 16):
                    out.append(Case("partial_waves", f"K{K}-ksplit{ks}", "partial", M, n_main, K, n_ext=n_ext, ksplit=ks, routes=("partial_waves",)))
    for K, ks in whole:
        for M in (33, 129, 640):
            for n_main, n_ext in ((16, 0), (144, 48)):
                for wn in (0, 2, 4):
                    for wt in (0, 1):
                        out.append(Case("pairs", f"K{K}-ksplit{ks}", "pairs", M, n_main, K, n_ext=n_ext, ksplit=ks, tune=((17, wn), (21, wt)), routes=("pairs_tiled",)))
        for M in (65, 129, 640):
            for n_main, n_ext in ((16, 0), (144, 48)):
                out.append(Case("chain", f"K{K}-ksplit{ks}", "chain", M, n_main, K, n_ext=n_ext, ksplit=ks, tune=((7, 65),), routes=("chain_tiled",)))
    return out


CASES: List[Case] = (_t128_cases() + _w256_cases() + _xa_cases() + _mul_cases() + _swiglu_train_cases() + _k64_skinny_n_cases() +
                     _mid_cases() + _dt_cases() + _skinny_cases() + _partial_cases())


def groups(family: str) -> List[str]:
    seen = []
    for c in CASES:
        if c.family == family and c.group not in seen:
            seen.append(c.group)
    return seen


def cases_of(family: str, group: str) -> List[Case]:
    return [c for c in CASES if c.family == family and c.group == group]
