"""Exact references, guard bands and the case table for the quantised GEMMs: csrc/fp8.hip (e4m3 x e4m3, channel scales) and
csrc/mxfp4.hip (e4m3 x MXFP4) — tests/test_hip_qgemm_exact.py on the GPU, tests/test_qgemm_exact_reference.py on the CPU.

The epilogues of both files are single IEEE fp32 operations with documented bf16 rounding points (fp8_finish / mx4_finish, the
header's formulas); only the order of the K sum is free.  The operands here make that order irrelevant: every product is an
integer multiple of one power of two (the `unit` of its output column) and the sum of the ABSOLUTE products of every output
stays below 2^24 units, so every partial sum in every order is exact in fp32.  The accumulator is then the fp64 product, and
every output bit of the plain, residual and adapter epilogues follows for real, index-dependent fp32 scales — no ulp allowance.
The condition is asserted, never enforced by clipping: a case that breaks it raises InexactCase.

SwiGLU: g and u are determined exactly as above; the output must be bf16(s * u) with s the bf16 nearest to the fp64 silu(g) or
one of its two neighbours (gemm_exact_reference.swiglu_accept's rule, with the candidate table generalised from integer g to
any bf16 g: silu_candidates_of), plus that module's flush range g <= SILU_FLUSH_G.  The cases keep |g| < 87, below the range
where an fp32 sigmoid turns subnormal (g < -87.33), so no case depends on the flush clause.

Guarded, guard_rows, the sentinels, InexactCase, exact_f32 and route_names are gemm_exact_reference's."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

import gemm_exact_reference as R
from gemm_exact_reference import InexactCase, cdiv, exact_f32

E8M0_SENTINEL = 0xFF              # the E8M0 NaN: a scale byte read from a guard poisons the block's products
TUNING_DEFAULTS = {19: 0, 20: 0}  # every dh_set_tuning key the table touches -> the library's default (restored after each case)

FMTS = ("fp8", "mx4")
KS = (128, 256, 384, 512, 640, 1152, 2176, 4224, 5248)
K_LOOP = KS[:5]                   # every prologue / tail branch of the 4-stage loops, odd and even trips of the 2-stage loops
STREAM_M = (1, 31, 32, 33, 64, 65, 96, 97, 128)
TILED_M = (127, 128, 129, 255, 257, 577)          # 577: five row tiles, not a multiple of the band of 4
NS = {"fp8": (4, 12, 20, 60, 68, 124, 132, 252, 260, 516), "mx4": (16, 48, 80, 112, 144, 272, 528)}
EPIS = (("plain", "plain", False), ("plain+resid", "plain", True), ("adapter", "adapter", False), ("adapter+resid", "adapter", True),
        ("swiglu", "swiglu", False))
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@dataclass(frozen=True)
class Case:
    family: str
    group: str
    fmt: str                          # fp8 | mx4
    op: str                           # linear | linear_f32 (the fp32-out entry point)
    M: int
    N: int                            # output columns (SwiGLU: pairs)
    K: int
    epi: str = "plain"                # plain | adapter | swiglu
    resid: bool = False
    kernel: int = 0                   # dh_linear_*_ex's selector: 0 by row count, 1 tiled, 2 streaming
    thin: bool = False                # half of W zeroed
    data: str = "rand"                # rand | codes_x | codes_w: the "every code" operands
    tune: Tuple[Tuple[int, int], ...] = ()
    routes: Tuple[str, ...] = ()

    @property
    def data_key(self):
        return (self.fmt, self.M, self.N, self.K, self.epi, self.resid, self.thin, self.data)

    @property
    def id(self) -> str:
        t = ",".join(f"{k}={v}" for k, v in self.tune)
        e = self.epi + ("+resid" if self.resid else "")
        return (f"{self.fmt} {self.op} {e} M={self.M} N={self.N} K={self.K} kernel={self.kernel} {self.data}{' thin' if self.thin else ''} "
                f"tune[{t}] -> {'+'.join(self.routes)}")


def route_of(fmt: str, M: int, N: int, epi: str, kernel: int, tile: int = 0) -> str:
    """The launch site dh_linear_fp8_ex / dh_linear_mxfp4_ex document for a call (tile: dh_set_tuning key 19)."""
    if kernel == 2 or (kernel == 0 and M <= 128):
        return f"{fmt}_stream_ng{1 if M <= 32 else 2 if M <= 64 else 4}"
    sw = epi == "swiglu"
    if fmt == "fp8" and (tile == 256 if tile else cdiv(M, 256) * cdiv(N, 128 if sw else 256) >= 512):
        return "fp8_t256"
    return f"{fmt}_t128_s4" if cdiv(M, 128) * cdiv(N, 64 if sw else 128) < 384 else f"{fmt}_t128_s2"


# ---- operands -------------------------------------------------------------------------------------------------------------
def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(key, shape, lo: int, hi: int) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=_gen(*key)).double()


_FANCY_X = torch.tensor([3.0, -5.0, 7.0, -12.0, -1.5, 5.0, -3.0, 12.0, -7.0, 1.5], dtype=torch.float64)
_FANCY_W = torch.tensor([-3.0, 1.5, 12.0, -7.0, 5.0, -1.5, 3.0, -12.0, 7.0, -5.0], dtype=torch.float64)


def _strided(t: torch.Tensor, first: int, stride: int, values: torch.Tensor, row_step: int) -> None:
    """values with mantissa bits on the k columns first, first + stride, ..: the value depends on the row and on the column"""
    cols = torch.arange(first, t.size(1), stride)
    if cols.numel():
        idx = (torch.arange(t.size(0)).view(-1, 1) * row_step + torch.arange(cols.numel()).view(1, -1)) % values.numel()
        t[:, cols] = values[idx]


def _x(M, K):
    """e4m3 values, multiples of 0.5.  Symmetry breakers on strided k columns, with strides and values that differ from W's:
    an operand swap, a k permutation or a wrong register half shows."""
    x = _ints(("qx", M, K), (M, K), -2, 2)
    x[:, ::7] = 1.5
    _strided(x, 3, 11, _FANCY_X, 1)
    return x


def _w8(tag, N, K, thin):
    w = _ints((tag, N, K), (N, K), -1, 1)
    if thin:
        w = w * _ints((tag, "thin", N, K), (N, K), 0, 1)
    w[:, ::5] = -1.5 if tag != "w2" else 1.5
    _strided(w, 2, 13, _FANCY_W, 3)
    return w


def _codes4(tag, N, K, thin):
    """e2m1 codes: all sixteen at random (odd and even k differ: a wrong nibble order shows), code 11 (-1.5) / 3 (1.5) on every fifth k"""
    c = torch.randint(0, 16, (N, K), generator=_gen(tag, N, K))
    if thin:
        c = c * torch.randint(0, 2, (N, K), generator=_gen(tag, "thin", N, K))
    c[:, ::5] = 11 if tag != "w2" else 3
    return c.to(torch.uint8)


def _scales4(tag, N, K, narrow: bool):
    """E8M0 bytes keyed by (n, block): a per-row base of 2^-8 .. 2^5 (narrow, the SwiGLU gate: 2^-8 .. 2^-4, so that |g| stays
    small) times 2^0 .. 2^3 by block — the four blocks of a k-step differ, and the pattern moves on by one from k-step to
    k-step.  Bytes 119 .. 135: 2^-8 .. 2^8."""
    n = torch.arange(N).view(-1, 1)
    b = torch.arange(K // 32).view(1, -1)
    base = (n * 3) % 5 - 8 if narrow else (n * 5 + (3 if tag == "w2" else 0)) % 14 - 8
    return (127 + base + (b + b // 4 + n) % 4).to(torch.uint8)


def _real(idx: torch.Tensor, mul: int, add: int, mod: int, exp: int) -> torch.Tensor:
    """fp32 in (1, 2) * 2^exp: never a power of two, and different for neighbouring indices"""
    return ((1.0 + (((idx * mul + add) % mod).double() + 0.5) / mod) * 2.0 ** exp).float()


def _bf16_vec(key, shape, lo: float, hi: float) -> torch.Tensor:
    return (torch.rand(shape, generator=_gen(*key), dtype=torch.float64) * (hi - lo) + lo).bfloat16()


def dequant4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp64 [N, K] of e2m1 codes and E8M0 bytes (one per 32 k)"""
    c = codes.long()
    v = torch.tensor(E2M1, dtype=torch.float64)[c & 7] * (1.0 - 2.0 * (c >> 3).double())
    return v * torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127.0).repeat_interleave(32, dim=1)


def e4m3_bytes() -> torch.Tensor:
    """the 254 non-NaN e4m3fn bytes (subnormals, both zeros and +-448 included)"""
    return torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)


def _xs_exp(c: Case) -> int:
    """x_scale's exponent: the SwiGLU gate's standard deviation grows with sqrt(K); this keeps |g| < 87 (the reference asserts it)"""
    return -3 - (max(c.K // 128, 1).bit_length() + 1) // 2


def operands(c: Case) -> Dict[str, torch.Tensor]:
    """The operands of a case on the CPU.  x, w (fp8) fp64 [rows, K] holding e4m3 values; codes / sc (mx4) uint8 e2m1 codes
    [N, K] and E8M0 bytes [N, K / 32]; xs, ws fp32; a, b bf16 [N]; resid bf16 [M, N]; x_unit and w_unit [N]: powers of two that
    divide every value of x / of row n of the dequantised W."""
    M, N, K, fp8 = c.M, c.N, c.K, c.fmt == "fp8"
    o: Dict[str, torch.Tensor] = {}
    if c.data == "rand":
        o["x"], o["x_unit"] = _x(M, K), torch.tensor(0.5, dtype=torch.float64)
        o["xs"] = _real(torch.arange(M), 37, 11, 101, _xs_exp(c))
        if fp8:
            o["w"], o["w_unit"] = _w8("w", N, K, c.thin), torch.full((N,), 0.5, dtype=torch.float64)
            o["ws"] = _real(torch.arange(N), 53, 7, 103, -2)
            if c.epi == "swiglu":
                o["w2"], o["ws2"] = _w8("w2", N, K, c.thin), _real(torch.arange(N), 29, 3, 107, -1)
        else:
            o["codes"], o["sc"] = _codes4("w", N, K, c.thin), _scales4("w", N, K, c.epi == "swiglu")
            if c.epi == "swiglu":
                o["codes2"], o["sc2"] = _codes4("w2", N, K, c.thin), _scales4("w2", N, K, False)
    else:
        # "every code": one operand walks through every code of its format, the other is one-hot, unit scales — each output is
        # one decoded value.  M = N = K
        assert M == N == K and c.epi == "plain" and not c.resid
        eye = torch.eye(K, dtype=torch.float64)
        allb = e4m3_bytes()
        walk = allb[(torch.arange(K).view(1, -1) + 127 * torch.arange(K).view(-1, 1)) % 254].view(torch.float8_e4m3fn).double()
        o["xs"] = torch.ones(M)
        if c.data == "codes_x":
            o["x"], o["x_unit"] = walk, torch.tensor(2.0 ** -9, dtype=torch.float64)
        else:
            o["x"], o["x_unit"] = eye, torch.tensor(1.0, dtype=torch.float64)
        if fp8:
            o["w"] = eye if c.data == "codes_x" else walk
            o["w_unit"] = torch.full((N,), 1.0 if c.data == "codes_x" else 2.0 ** -9, dtype=torch.float64)
            o["ws"] = torch.ones(N)
        else:
            assert c.data == "codes_w"
            n, k = torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
            o["codes"] = ((k + n) % 16).to(torch.uint8)
            o["sc"] = (127 - 8 + (4 * n + torch.arange(K // 32).view(1, -1)) % 17).to(torch.uint8)
    if not fp8:
        for s in ("", "2"):
            if "sc" + s in o:
                o["w_unit" + s] = 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), o["sc" + s].double().amin(1) - 127.0)
    elif "w2" in o:
        o["w_unit2"] = o["w_unit"]
    if c.epi == "adapter":
        o["a"] = _bf16_vec(("a", N), (N,), 0.5, 2.0) * (1 - 2 * (torch.arange(N) % 3 == 1).to(torch.bfloat16))
        o["b"] = _bf16_vec(("b", N), (N,), -2.0, 2.0)
    if c.resid:
        o["resid"] = _bf16_vec(("resid", M, N), (M, N), -4.0, 4.0)
    return o


def weights(c: Case, o: Dict[str, torch.Tensor], second: bool = False) -> torch.Tensor:
    """the fp64 weights [N, K] the product is taken with (mx4: dequantised)"""
    s = "2" if second else ""
    return o["w" + s] if c.fmt == "fp8" else dequant4(o["codes" + s], o["sc" + s])


def encode(c: Case, o: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The byte tensors the library takes: xq, and wq (+ w2q) e4m3 bytes for fp8, or wq / wsc (+ w2q / w2sc) in
    dualhyp_amd.quant.pack_mxfp4's layout.  A value that does not survive its format raises InexactCase."""
    from dualhyp_amd.quant import pack_mxfp4

    def e4m3(v, what):
        q = v.float().to(torch.float8_e4m3fn)
        if not torch.equal(q.double(), v):
            raise InexactCase(f"{c.id}: {what} holds values that are not e4m3 numbers")
        return q.view(torch.uint8)

    out = {"xq": e4m3(o["x"], "x")}
    for s in ("", "2"):
        if c.fmt == "fp8" and "w" + s in o:
            out[f"w{s}q"] = e4m3(o["w" + s], "w" + s)
        elif "codes" + s in o:
            if int(o["sc" + s].max()) == 255:
                raise InexactCase(f"{c.id}: an E8M0 byte of 255")
            out[f"w{s}q"], out[f"w{s}sc"] = pack_mxfp4(o["codes" + s], o["sc" + s])
    return out


# ---- reference ------------------------------------------------------------------------------------------------------------
def exact_acc(x: torch.Tensor, x_unit: torch.Tensor, w: torch.Tensor, w_unit: torch.Tensor, what: str) -> torch.Tensor:
    """fp64 x . w^T, with the exactness condition asserted: every value a multiple of its unit, and per output the sum of the
    absolute products below 2^24 units — every partial sum of every summation order is then exact in fp32"""
    for v, u, nm in ((x, x_unit, "x"), (w, w_unit.view(-1, 1), "w")):
        q = v / u
        if not torch.equal(q, q.round()):
            raise InexactCase(f"{what}: {nm} holds values that are not multiples of its unit")
    exact_f32((x.abs() @ w.abs().T) / (x_unit * w_unit).view(1, -1), what + ": sum of |products| in units")
    return x @ w.T


def _rb(v: torch.Tensor) -> torch.Tensor:
    """rbf of csrc/common.h: fp32 -> bf16 (round to nearest even) -> fp32"""
    assert v.dtype == torch.float32
    return v.bfloat16().float()


def finish(c: Case, o: Dict[str, torch.Tensor], acc: torch.Tensor, second: bool = False) -> torch.Tensor:
    """fp8_finish / mx4_finish with fp32 torch ops: rbf(acc * (xs * ws)) (mx4: acc * xs), ADAPTER rbf(a * rbf(o + b)); -> fp32"""
    a32 = acc.float()
    assert torch.equal(a32.double(), acc)
    sc = o["xs"].view(-1, 1) * o["ws2" if second else "ws"].view(1, -1) if c.fmt == "fp8" else o["xs"].view(-1, 1)
    y = _rb(a32 * sc)
    if c.epi == "adapter":
        y = _rb(o["a"].float().view(1, -1) * _rb(y + o["b"].float().view(1, -1)))
    return y


def reference(c: Case, o: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """{"y": bf16 [M, N]} (linear_f32: the same values, stored as fp32) or, SwiGLU, {"g", "u": bf16, "cand": fp32 [M, N, 3]}"""
    acc = exact_acc(o["x"], o["x_unit"], weights(c, o), o["w_unit"], c.id)
    y = finish(c, o, acc)
    del acc
    if c.epi == "swiglu":
        u = finish(c, o, exact_acc(o["x"], o["x_unit"], weights(c, o, True), o["w_unit2"], c.id + " (w2)"), second=True)
        if not float(y.abs().max()) < 87.0:
            raise InexactCase(f"{c.id}: |g| reaches {float(y.abs().max())}: the gate enters the fp32 underflow range of silu")
        return {"g": y.bfloat16(), "u": u.bfloat16(), "cand": silu_candidates_of(y.double())}
    if c.resid:
        y = _rb(o["resid"].float() + y)
    return {"y": y.bfloat16()}


# ---- SwiGLU acceptance for any bf16 g --------------------------------------------------------------------------------------
def _bf16_ord(v: torch.Tensor) -> torch.Tensor:
    """ordered index of bf16 values (fp32 tensor): sign * magnitude bits, as gemm_exact_reference._bf16_value counts them"""
    bits = v.float().view(torch.int32).long()
    mag = (bits >> 16) & 0x7FFF
    return torch.where(bits < 0, -mag, mag)


def _bf16_of(o: torch.Tensor) -> torch.Tensor:
    bits = torch.where(o >= 0, o, 0x8000 | -o) << 16
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32)


def silu_candidates_of(g: torch.Tensor) -> torch.Tensor:
    """fp32 [.., 3] for bf16 values g (as fp64): the bf16 nearest to silu(g) = g / (1 + e^-g) evaluated in fp64 (a tie goes to the
    smaller magnitude), and that value's two bf16 neighbours — gemm_exact_reference.silu_candidates' rule for any g."""
    assert g.dtype == torch.float64
    v = g / (1.0 + torch.exp(-g))
    o = _bf16_ord(v.float().bfloat16().float())                    # within one step of the nearest
    ks = o.unsqueeze(-1) + torch.tensor([0, -1, 1, -2, 2])
    dist = (_bf16_of(ks).double() - v.unsqueeze(-1)).abs()
    tied = dist == dist.amin(-1, keepdim=True)
    pick = torch.where(tied, ks.abs(), torch.full_like(ks, 1 << 20)).argmin(-1, keepdim=True)
    best = ks.gather(-1, pick)
    return _bf16_of(torch.cat([best, best - 1, best + 1], dim=-1))


def swiglu_accept(got: torch.Tensor, g: torch.Tensor, u: torch.Tensor, cand: torch.Tensor):
    """gemm_exact_reference.swiglu_accept with the candidates of silu_candidates_of: -> (ok, n_neighbour, n_flushed).  s and u
    are bf16, so s * u is exact in fp32 and its rounding to bf16 is the epilogue's last step."""
    want = (cand * u.float().unsqueeze(-1)).bfloat16().float()
    hit = want == got.float().unsqueeze(-1)
    near = hit.any(-1)
    flushed = (g.float() <= R.SILU_FLUSH_G) & (got.float() == 0) & ~near
    return near | flushed, int((near & ~hit[..., 0]).sum()), int(flushed.sum())


# ---- the case table -------------------------------------------------------------------------------------------------------
def _thin(K: int) -> bool:
    return K >= 4224


def _grid_cases(fmt: str) -> List[Case]:
    """Every M class x every N class for every epilogue, K walking the diagonal (shifted by the epilogue, so that every K meets
    several shapes).  Up to 128 rows each shape runs on the streaming kernel (selector 0 and 2 alternate) AND on the tiled one
    (selector 1: the engine pins tiled for a prefill of any size); the fp32-out form takes all the streaming shapes."""
    out = []
    for e, (name, epi, resid) in enumerate(EPIS):
        for i, M in enumerate(STREAM_M):
            for j, N in enumerate(NS[fmt]):
                K = KS[(i + j + 2 * e) % len(KS)]
                kw = dict(epi=epi, resid=resid, thin=_thin(K))
                sel = 2 if (i + j) % 2 else 0
                out.append(Case("small", f"{fmt}-{name}-M{M}", fmt, "linear", M, N, K, kernel=sel, routes=(route_of(fmt, M, N, epi, sel),), **kw))
                out.append(Case("small", f"{fmt}-{name}-M{M}", fmt, "linear", M, N, K, kernel=1, routes=(route_of(fmt, M, N, epi, 1),), **kw))
                if name == "plain":
                    out.append(Case("small", f"{fmt}-{name}-M{M}", fmt, "linear_f32", M, N, K, routes=(route_of(fmt, M, N, epi, 2),), **kw))
        for i, M in enumerate(TILED_M):
            for j, N in enumerate(NS[fmt]):
                K = KS[(i + j + 2 * e + 4) % len(KS)]
                sel = 1 if M <= 128 else 0
                out.append(Case("tiled", f"{fmt}-{name}-M{M}", fmt, "linear", M, N, K, epi=epi, resid=resid, thin=_thin(K), kernel=sel,
                                routes=(route_of(fmt, M, N, epi, sel),)))
    return out


def _two_stage_cases(fmt: str) -> List[Case]:
    """16 x 24 = 384 tiles of 128: the two-stage form, last row tile one row deep, last column tile 4 (mx4: 16) wide, K one to
    five stages (odd and even trips)"""
    M, N, Np = 1921, 23 * 128 + NS[fmt][0], 23 * 64 + NS[fmt][0]
    r = (f"{fmt}_t128_s2",)
    out = [Case("two_stage", f"{fmt}-plain-K{K}", fmt, "linear", M, N, K, routes=r) for K in K_LOOP]
    out.append(Case("two_stage", f"{fmt}-plain+resid", fmt, "linear", M, N, 256, resid=True, routes=r))
    out.append(Case("two_stage", f"{fmt}-adapter", fmt, "linear", M, N, 384, epi="adapter", routes=r))
    out.append(Case("two_stage", f"{fmt}-adapter+resid", fmt, "linear", M, N, 128, epi="adapter", resid=True, routes=r))
    out += [Case("two_stage", f"{fmt}-swiglu-K{K}", fmt, "linear", M, Np, K, epi="swiglu", routes=r) for K in (128, 384)]
    return out


def _dispatch_cases(fmt: str) -> List[Case]:
    """one shape on each side of each threshold, default selector, no tuning"""
    n4 = NS[fmt][0]
    out = [Case("dispatch", f"{fmt}-rows", fmt, "linear", 128, NS[fmt][4], 384, routes=(f"{fmt}_stream_ng4",)),
           Case("dispatch", f"{fmt}-rows", fmt, "linear", 129, NS[fmt][4], 384, routes=(f"{fmt}_t128_s4",)),
           # 383 (a prime) and 384 tiles of 128 rows: one column tile
           Case("dispatch", f"{fmt}-stages-383", fmt, "linear", 383 * 128, n4, 128, routes=(f"{fmt}_t128_s4",)),
           Case("dispatch", f"{fmt}-stages-384", fmt, "linear", 383 * 128 + 1, n4, 128, routes=(f"{fmt}_t128_s2",))]
    if fmt == "fp8":
        # 16 x 31 = 496 and 16 x 32 = 512 tiles of 256 (last row band one row deep, last column tile 4 wide)
        out.append(Case("dispatch", "fp8-tile-496", fmt, "linear", 3841, 30 * 256 + 4, 128, routes=("fp8_t128_s2",)))
        out.append(Case("dispatch", "fp8-tile-512", fmt, "linear", 3841, 31 * 256 + 4, 128, routes=("fp8_t256",)))
    return out


def _tune_cases() -> List[Case]:
    """fp8 only (mxfp4.hip has one tile and a fixed band of 4).  Key 19: both tiles forced on 257 x 260 (256-tile: last row band
    one row deep, last column tile 4 wide; SwiGLU 132 pairs: a 128-pair tile and 4 pairs).  Key 20: bands of 1, 2, 4, 8 and the
    default (4; SwiGLU on the 256-tile 2) over 3 and 5 row tiles."""
    out = []
    for e, (name, epi, resid) in enumerate(EPIS):
        N = 132 if epi == "swiglu" else 260
        for K in (K_LOOP if name in ("plain", "swiglu") else (K_LOOP[e],)):
            for tile in (128, 256):
                out.append(Case("tune", f"tile-{name}", "fp8", "linear", 257, N, K, epi=epi, resid=resid, tune=((19, tile),),
                                routes=(route_of("fp8", 257, N, epi, 0, tile),)))
    for name, epi, resid in (EPIS[0], EPIS[1], EPIS[4]):
        N = 132 if epi == "swiglu" else 260
        for M, tiles in ((257, (128,)), (577, (128, 256)), (1153, (256,))):      # row tiles: 3 of 128 | 5 of 128, 3 of 256 | 5 of 256
            for tile in tiles:
                for gm in (0, 1, 2, 4, 8):
                    out.append(Case("tune", f"band-{name}-M{M}", "fp8", "linear", M, N, 256, epi=epi, resid=resid, tune=((19, tile), (20, gm)),
                                    routes=(route_of("fp8", M, N, epi, 0, tile),)))
    return out


def _code_cases() -> List[Case]:
    out = []
    for fmt, datas in (("fp8", ("codes_x", "codes_w")), ("mx4", ("codes_w",))):
        for data in datas:
            for op, sel in (("linear", 2), ("linear", 1), ("linear_f32", 0)):
                out.append(Case("codes", fmt, fmt, op, 128, 128, 128, kernel=sel, data=data, routes=(route_of(fmt, 128, 128, "plain", sel),)))
    return out


CASES: List[Case] = (_grid_cases("fp8") + _grid_cases("mx4") + _two_stage_cases("fp8") + _two_stage_cases("mx4") + _dispatch_cases("fp8") +
                     _dispatch_cases("mx4") + _tune_cases() + _code_cases())


def groups(family: str) -> List[str]:
    seen = []
    for c in CASES:
        if c.family == family and c.group not in seen:
            seen.append(c.group)
    return seen


def cases_of(family: str, group: str) -> List[Case]:
    return [c for c in CASES if c.family == family and c.group == group]
