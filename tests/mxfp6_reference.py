"""CPU reference of the MXFP6 activation format (include/dualhyp_hip.h "MXFP6 activations"), written from the header's words alone:
the quantiser in fp64 with a nearest-value search over the 32 magnitudes (the product's is fp32 with a scaled round-half-even),
the unpacker of the physical layout by index arithmetic (the product's packer is a permute), the fp64 product with the MXFP4
weights of tests/mxfp4_reference.py, and a wrapper that makes an oracle (oracle.OracleGPT, or the fp8-KV-cache oracle of
tests/kv8_reference.py) compute its block linears over MXFP6-quantised activations."""
from typing import Iterable, Tuple

import torch
from torch import Tensor

import mxfp4_reference as R4

# magnitudes of the low five bits 0..31: m / 8 for E = 0, else (1 + m / 8) * 2^(E - 1)
GRID = torch.tensor([(m / 8.0) if E == 0 else (1.0 + m / 8.0) * 2.0 ** (E - 1) for E in range(4) for m in range(8)], dtype=torch.float64)
MIDPOINTS = tuple(((GRID[i] + GRID[i + 1]) / 2).item() for i in range(31))
MIDPOINT_RESULT = tuple(GRID[i if i % 2 == 0 else i + 1].item() for i in range(31))      # the neighbour with the even code


def quantize_blocks(x: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (uint8 codes [M, K], uint8 E8M0 bytes [M, K / 32]) of the rows of x (any float dtype), all arithmetic in fp64: the nearest
    of the 32 magnitudes, the even code of two equally near ones, 7.5 for anything above it."""
    M, K = x.shape
    v = x.double().reshape(M, K // 32, 32)
    amax = v.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                  # amax = m * 2^ex with m in [0.5, 1)
    e = ((ex.long() - 1) - 2).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    a = v.abs() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double())      # exact: a power of two, no underflow in fp64
    d = (a.unsqueeze(-1) - GRID).abs()                         # distance to each magnitude; above 7.5 the nearest is 7.5
    near = d == d.amin(-1, keepdim=True)                       # one value, or two on a tie
    idx = torch.arange(32).expand_as(d)
    even = idx % 2 == 0
    code_even = torch.where(near & even, idx, torch.full_like(idx, -1)).amax(-1)
    code_any = torch.where(near, idx, torch.full_like(idx, -1)).amax(-1)
    code = torch.where((near.sum(-1) > 1) & (code_even >= 0), code_even, code_any)
    code = code | (((v < 0) & (code != 0)).long() << 5)
    return code.reshape(M, K).to(torch.uint8), (e + 127).reshape(M, K // 32).to(torch.uint8)


def dequantize_blocks(codes: Tensor, scales: Tensor) -> Tensor:
    """fp64 [M, K]: (-1)^bit5 * GRID[bits 4..0] * 2^(s - 127)."""
    M, K = codes.shape
    c = codes.long()
    v = GRID[c & 31] * (1.0 - 2.0 * (c >> 5).double())
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127.0)
    return (v.reshape(M, K // 32, 32) * s.unsqueeze(-1)).reshape(M, K)


def unpack(xq: Tensor, xs: Tensor, M: int, K: int) -> Tuple[Tensor, Tensor]:
    """The header's physical layout, read back element by element: (codes [M, K], scales [M, K / 32]) of the first M rows from the flat
    bytes.  Element i of a block is bits 6 i .. 6 i + 5 of a little-endian 192-bit number whose byte b is at plane b / 8, position b % 8."""
    xq, xs = xq.reshape(-1).cpu().long(), xs.reshape(-1).cpu()
    G = (M + 15) // 16
    assert xq.numel() == G * 16 * K * 3 // 4 and xs.numel() == G * 16 * K // 32
    m = torch.arange(M).view(-1, 1)
    k = torch.arange(K).view(1, -1)
    g, r, t, q, i = m // 16, m % 16, k // 128, (k % 128) // 32, k % 32
    l = 16 * q + r
    base = (g * (K // 128) + t) * 1536
    bit = 6 * i

    def byte(b):
        return xq[base + (b // 8) * 512 + l * 8 + b % 8]
    b0 = bit // 8
    two = byte(b0) | (byte(torch.clamp(b0 + 1, max=23)) << 8)       # a code never reaches past byte 23: bit 186 + 5 = 191
    codes = (two >> (bit % 8)) & 63
    kb = torch.arange(K // 32).view(1, -1)
    scales = xs[(g * (K // 128) + kb // 4) * 64 + 16 * (kb % 4) + r]
    return codes.to(torch.uint8), scales.to(torch.uint8)


def edge_row() -> Tensor:
    """A bf16 row of 12 blocks (384 elements) with every case the header's quantiser names."""
    blocks = []

    def block(vals, scale=1.0):
        b = torch.zeros(32, dtype=torch.float64)
        b[:len(vals)] = torch.tensor(vals, dtype=torch.float64)
        blocks.append(b * scale)
    grid = GRID.tolist()
    block(grid)                                                         # 0: amax 7.5, e = 0: every magnitude as it is -> codes 0..31
    block([-g for g in grid], 2.0 ** -9)                                # 1: their negatives at another exponent -> codes 33..63, and +0 for -0
    block([4.0] + list(MIDPOINTS))                                      # 2: amax 4, e = 0: every midpoint between neighbours
    block([-4.0] + [-t for t in MIDPOINTS], 2.0 ** 7)                   # 3: the negative midpoints, e = 7
    block([1.9375 * 4, -1.9375 * 4, 1.96875 * 4, 7.5, 7.625, -7.25])    # 4: amax mantissa 1.9375 (and above): 7.75 would round to 8 -> 7.5
    block([])                                                           # 5: all zero
    block([-0.0] * 4)                                                   # 6: all zero with negative zeros
    block([2.0 ** -133, -(2.0 ** -133), 2.0 ** -130, 3 * 2.0 ** -133])  # 7: bf16 subnormals alone: s clamps at 1
    block([2.0 ** -126, 2.0 ** -125, -(2.0 ** -124), 2.0 ** -129, 2.0 ** -130, -(2.0 ** -131)])   # 8: around the clamp, subnormals beside normals
    block([3.0e38, -1.0e38, 1.0e30, 5.0e37, 3.3e38])                    # 9: the largest binade of bf16 (amax near 2^127 * 1.99)
    block([1.0, -1e-3, 1e-6, 0.0155, 0.0157, -0.047, 0.0469])           # 10: elements far below the block's amax (e = -2: step 1/32)
    block([-7.9, 7.9, 5.01, -4.99, 3.1, 2.05, 1.99])                    # 11
    row = torch.cat(blocks).to(torch.bfloat16)
    assert row.numel() == 384
    return row


def linear(xc: Tensor, xs: Tensor, wc: Tensor, ws: Tensor) -> Tensor:
    """fp64 [M, N] = sum_k e2m3(xc) * 2^(xs - 127) * e2m1(wc) * 2^(ws - 127): the product of the definition, before the bf16 rounding."""
    return dequantize_blocks(xc, xs) @ R4.dequantize_blocks(wc, ws).T


class OracleA6:
    """An oracle whose block linears see MXFP6-quantised activations.  `oracle` computes every quantised linear through the module
    function `O.linear_fp8(x, wq, w_scale)`; while a call of this wrapper runs, that function is replaced: for the weights in
    `block_weights` (the e4m3 restatement of the MXFP4 weights, tests/mxfp4_reference.oracle_state_dict) the rows of x are quantised
    by quantize_blocks above, dequantised, multiplied in fp64 and rounded once to x's dtype; every other weight (lm_head) keeps the
    e4m3 product.  Everything else of the oracle is reached through the wrapper unchanged."""

    def __init__(self, O, oracle, block_weights: Iterable[Tensor]):
        self._O, self._oracle = O, oracle
        self._blocks = {w.data_ptr() for w in block_weights}

    def _linear(self, orig):
        def f(x, wq, w_scale):
            if wq.data_ptr() not in self._blocks:
                return orig(x, wq, w_scale)
            rows = x.reshape(-1, x.size(-1))
            xd = dequantize_blocks(*quantize_blocks(rows))
            acc = xd @ (wq.double() * w_scale.double().view(-1, 1)).T
            return acc.to(x.dtype).reshape(*x.shape[:-1], wq.size(0))
        return f

    def __call__(self, *a, **kw):
        orig = self._O.linear_fp8
        self._O.linear_fp8 = self._linear(orig)
        try:
            return self._oracle(*a, **kw)
        finally:
            self._O.linear_fp8 = orig

    def __getattr__(self, name):
        return getattr(self._oracle, name)
