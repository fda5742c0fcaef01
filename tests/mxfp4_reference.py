"""CPU reference of the MXFP4 weight format (include/dualhyp_hip.h "MXFP4 weights"), written from the header's words alone:
the quantiser in fp64 with a nearest-value search (the product's is fp32 with comparisons), the unpacker of the physical
layout by index arithmetic (the product's packer is a permute), the fp64 product, and the restatement of an MXFP4 state dict
as the e4m3 + channel-scale state dict oracle.OracleGPT already understands."""
from typing import Dict, Tuple

import torch
from torch import Tensor

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)     # magnitudes of codes 0..7
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
TIE_RESULT = (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)


def quantize_blocks(w: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (uint8 codes [N, K], uint8 E8M0 bytes [N, K / 32]) of the rows of w (any float dtype), all arithmetic in fp64."""
    N, K = w.shape
    x = w.double().reshape(N, K // 32, 32)
    amax = x.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                  # amax = m * 2^ex with m in [0.5, 1)
    e = (ex.long() - 1) - 2
    e = e.clamp(1 - 127, 254 - 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    a = x.abs() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double())      # exact: a power of two, no underflow in fp64
    d = (a.unsqueeze(-1) - GRID).abs()                         # distance to each of the eight magnitudes
    best = d.amin(-1, keepdim=True)
    near = d == best                                           # one value, or two on a tie
    even = (torch.arange(8) % 2 == 0)
    idx = torch.arange(8).expand_as(d)
    code_even = torch.where(near & even, idx, torch.full_like(idx, -1)).amax(-1)       # the tie goes to the even mantissa bit
    code_any = torch.where(near, idx, torch.full_like(idx, -1)).amax(-1)
    n_near = near.sum(-1)
    code = torch.where((n_near > 1) & (code_even >= 0), code_even, code_any)
    code = code | (((x < 0) & (code != 0)).long() << 3)
    return code.reshape(N, K).to(torch.uint8), (e + 127).reshape(N, K // 32).to(torch.uint8)


def dequantize_blocks(codes: Tensor, scales: Tensor) -> Tensor:
    """fp64 [N, K]: (-1)^bit3 * GRID[bits 2..0] * 2^(s - 127)."""
    N, K = codes.shape
    c = codes.long()
    v = GRID[c & 7] * (1.0 - 2.0 * (c >> 3).double())
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127.0)
    return (v.reshape(N, K // 32, 32) * s.unsqueeze(-1)).reshape(N, K)


def unpack(wq: Tensor, ws: Tensor, N: int, K: int) -> Tuple[Tensor, Tensor]:
    """The header's physical layout, read back element by element: (codes [N, K], scales [N, K / 32]) from the flat bytes."""
    wq, ws = wq.reshape(-1).cpu(), ws.reshape(-1).cpu()
    assert wq.numel() == N * K // 2 and ws.numel() == N * K // 32
    n = torch.arange(N).view(-1, 1)
    k = torch.arange(K).view(1, -1)
    g, r, t, q = n // 16, n % 16, k // 128, (k % 128) // 32
    l = 16 * q + r
    j = (k % 32) // 2
    byte = wq[((g * (K // 128) + t) * 1024 + l * 16 + j)]
    codes = torch.where(k % 2 == 0, byte & 15, byte >> 4)
    kb = torch.arange(K // 32).view(1, -1)
    tb, qb = kb // 4, kb % 4
    scales = ws[(g * (K // 128) + tb) * 64 + 16 * qb + r]
    return codes.to(torch.uint8), scales.to(torch.uint8)


def edge_row() -> Tensor:
    """A bf16 row of 12 blocks (384 elements) with every case the header's quantiser names."""
    blocks = []

    def block(vals, scale=1.0):
        b = torch.zeros(32, dtype=torch.float64)
        b[:len(vals)] = torch.tensor(vals, dtype=torch.float64)
        blocks.append(b * scale)
    ties = list(TIES) + [6.0, 7.0]
    block([4.0] + ties + [-t for t in ties])                            # amax 4: e = 0, the ties stand as written
    block([6.0] + ties + [-t for t in ties], 2.0 ** 5)                  # the same at another exponent, amax 6 * 2^5 exactly
    block([])                                                           # all zero
    block([-0.0] * 4)                                                   # all zero with negative zeros
    six = torch.tensor(6.0 * 2.0 ** -3, dtype=torch.bfloat16)
    block([six.item(), -1.0 * 2.0 ** -3, 0.1])
    above = (six.view(torch.int16) + 1).view(torch.bfloat16)            # one bf16 step above 6 * 2^k
    block([above.item(), 0.3, -0.05])
    below = (six.view(torch.int16) - 1).view(torch.bfloat16)
    block([-below.item(), 0.3, 0.74])
    block([2.0 ** -133, -(2.0 ** -133), 2.0 ** -130])                   # bf16 subnormals: s clamps at 1
    block([2.0 ** -126, 2.0 ** -125, -(2.0 ** -124)])                   # around the clamp
    block([3.0e38, -1.0e38, 1.0e30, 5.0e37])                            # the largest binade of bf16
    block([1.0, -1e-3, 1e-6, 0.24, 0.26, -0.124, 0.126])                # elements far below the block's amax
    block([-7.9, 7.9, 5.01, -4.99])
    row = torch.cat(blocks).to(torch.bfloat16)
    assert row.numel() == 384
    return row


def linear(xq: Tensor, xs: Tensor, codes: Tensor, scales: Tensor) -> Tensor:
    """bf16( (sum_k xq * dequant(W)) * x_scale[m] ) with the sum and the scaling in fp64 (xq: e4m3 bytes, xs fp32, both on the CPU)."""
    acc = xq.view(torch.float8_e4m3fn).double() @ dequantize_blocks(codes, scales).T
    return (acc * xs.double().view(-1, 1)).float().to(torch.bfloat16)


def block_exponent_span(scales: Tensor) -> int:
    """Largest spread (in binades) of the block exponents within a row; all-zero blocks (s = 127 with zero codes) count as they are."""
    return int((scales.int().amax(-1) - scales.int().amin(-1)).max())


def oracle_state_dict(sd: Dict[str, Tensor], cfg, O) -> Tuple[Dict[str, Tensor], Dict[str, Tuple[Tensor, Tensor]]]:
    """The state dict oracle.OracleGPT takes for an MXFP4 model: LoRA merged as the oracle merges it; every block weight row
    quantised by quantize_blocks, dequantised, divided by 2^c (c = the row's largest block exponent - 6) and stored as
    float8_e4m3fn with '<key>_scale' = 2^c; lm_head from the oracle's own fp8 quantiser.  The quotient must be exactly
    representable in e4m3: then OracleGPT computes the products of the header's formula, scaled by an exact power of two.
    -> (state dict, {key: (codes, scales)} of the block weights)."""
    fp8 = O.quantize_state_dict_fp8(sd, cfg)
    merged = O.merged_weights(sd, cfg) if any("lora_" in k for k in sd) else dict(sd)
    out, blocks = dict(merged), {}
    for k in [k for k in merged if k.endswith("linear.weight")]:
        if k.startswith("lm_head"):
            out[k], out[k + "_scale"] = fp8[k], fp8[k + "_scale"]
            continue
        codes, scales = quantize_blocks(merged[k])
        blocks[k] = (codes, scales)
        assert block_exponent_span(scales) <= 11, f"{k}: a row's block exponents span more than 11 binades"
        c = scales.int().amax(-1, keepdim=True) - 127 - 6
        quot = dequantize_blocks(codes, scales) * torch.pow(torch.tensor(2.0, dtype=torch.float64), -c.double())
        q8 = quot.float().to(torch.float8_e4m3fn)
        assert torch.equal(q8.double(), quot), f"{k}: a dequantised weight over 2^c is not an e4m3 value"
        out[k], out[k + "_scale"] = q8, torch.pow(torch.tensor(2.0), c.float()).view(-1)
    return out, blocks
