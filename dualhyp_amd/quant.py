"""fp8 (OCP e4m3fn) serving path — BASELINE config 5 / SURVEY.md §8f-4.

`quantize_model_fp8(model, kv_cache="bf16" | "fp8")` folds every LoRA update into its base weight exactly as the reference's
`merge_lora_weights` does (ger/lora.py:707-711 -> `:152-157`, `:349-365`) and then replaces each dense weight (the
seven matrices of every block and lm_head) by e4m3 rows with one fp32 scale per output channel:

    amax = max|W[n, :]| (>= 1e-12);  Wq[n, :] = fp8_rne(W[n, :] * inv), inv = 448 / amax (one IEEE division);  scale[n] = amax * fp32(1/448)

Activations are quantised the same way per token at run time by the kernels (csrc/fp8.hip), and every product runs
on the block-scaled fp8 MFMA.  The embedding table, the norm weights and the lm_head adapter vectors stay bf16.
The model is inference-only afterwards; the bf16 weights are released.

`quantize_model_mxfp4(model, kv_cache=...)` is the same path with a third weight format for the five dense matrices of every
block: OCP MX v1.0 MXFP4 (include/dualhyp_hip.h "MXFP4 weights": 32-element blocks of e2m1 with one E8M0 scale byte, 4.25 bits
per weight, packed in the order the kernels of csrc/mxfp4.hip read).  lm_head stays e4m3 with channel scales.
`activations="mxfp6"` also switches the block activations from e4m3 rows to OCP MX MXFP6 blocks (include/dualhyp_hip.h "MXFP6
activations", csrc/mxfp6.hip); `quantize_blocks_mxfp6` / `pack_mxfp6` are the host-side statement of what those kernels write.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn

FP8_MAX = 448.0


def quantize_rows_fp8(w: torch.Tensor, chunk_rows: int = 8192) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (uint8 [N, K] holding e4m3fn bit patterns, fp32 [N] scales); fp32 arithmetic, round to nearest even."""
    N = w.size(0)
    q = torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    for r0 in range(0, N, chunk_rows):
        x = w[r0:r0 + chunk_rows].float()
        amax = x.abs().amax(dim=-1, keepdim=True).clamp_min(1e-12)
        inv = torch.full_like(amax, FP8_MAX) / amax        # tensor / tensor: one correctly rounded division
        q[r0:r0 + chunk_rows] = (x * inv).to(torch.float8_e4m3fn).view(torch.uint8)
        scale[r0:r0 + chunk_rows] = (amax * torch.tensor(1.0 / FP8_MAX, dtype=torch.float32, device=w.device)).view(-1)
    return q, scale


def dequantize_rows_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).float() * scale.view(-1, 1)


def quantize_model_fp8(model, kv_cache: str = "bf16") -> None:
    """Serving-only, one way: merge LoRA, replace every dense weight by e4m3 rows + channel scales (non-persistent
    buffers).  The bf16 weights are gone afterwards, so `GPT.load_state_dict` and `save_checkpoint` refuse a quantised
    model (quantise a freshly loaded model instead).

    kv_cache: "bf16" (default) keeps the KV cache as it is; "fp8" stores every cached K (after rope) and V vector as e4m3
    bytes with one power-of-two exponent (include/dualhyp_hip.h "fp8 KV cache": 66 048 instead of 131 072 bytes per token at
    Llama-3-8B).  It sets `model.kv_cache_dtype`; calling again on a quantised model changes that setting alone (the engine
    is rebuilt, the cache contents are dropped)."""
    from .gpt import GPT, _FrozenLinear, merge_lora_weights
    assert isinstance(model, GPT)
    if kv_cache not in ("bf16", "fp8"):
        raise ValueError(f"kv_cache is 'bf16' or 'fp8', got {kv_cache!r}")
    if getattr(model, "weight_format", "") == "mxfp4":
        raise RuntimeError("quantize_model_fp8: this model was quantised to mxfp4 (quantize_model_mxfp4); its bf16 weights no longer "
                           "exist, so it cannot be requantised to fp8 (quantise a freshly loaded model instead)")
    if getattr(model, "fp8", False):
        if model.kv_cache_dtype != kv_cache:
            model.kv_cache_dtype = kv_cache
            model.refresh_engine()
        return
    model.kv_cache_dtype = kv_cache
    merge_lora_weights(model)
    for m in model.modules():
        if isinstance(m, _FrozenLinear):
            q, s = quantize_rows_fp8(m.weight.data)
            m.register_buffer("weight_fp8", q, persistent=False)
            m.register_buffer("weight_scale", s, persistent=False)
            m.weight = nn.Parameter(torch.empty(0, dtype=m.weight.dtype, device=m.weight.device), requires_grad=False)
    for p in model.parameters():
        p.requires_grad_(False)
    model.fp8 = True
    model.refresh_engine()


# ------------------------------------------------------------------------------------------ MXFP4 weights
MX_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # the magnitudes of codes 0..7; bit 3 of a code is the sign


def _pow2_f32(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for integer e in [-126, 127], from the exponent field."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_blocks_mxfp4(w: torch.Tensor, chunk_rows: int = 4096) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (uint8 [N, K] e2m1 codes, one per element, uint8 [N, K / 32] E8M0 bytes); the quantiser of include/dualhyp_hip.h
    "MXFP4 weights" in fp32: frexp for floor(log2), a power-of-two scaling and comparisons, so every step is exact."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"quantize_blocks_mxfp4: K={K} is not a multiple of {MX_BLOCK}")
    codes = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scales = torch.empty((N, K // MX_BLOCK), dtype=torch.uint8, device=w.device)
    for r0 in range(0, N, chunk_rows):
        x = w[r0:r0 + chunk_rows].float().reshape(-1, K // MX_BLOCK, MX_BLOCK)
        amax = x.abs().amax(dim=-1, keepdim=True)
        _, ex = torch.frexp(amax)                             # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
        e = (ex.to(torch.int32) - 3).clamp(-126, 127)
        e = torch.where(amax == 0, torch.zeros_like(e), e)
        a = x.abs() * _pow2_f32(-e)
        c = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
             + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
        c = c | (((x < 0) & (c != 0)).to(torch.uint8) << 3)
        codes[r0:r0 + chunk_rows] = c.reshape(-1, K)
        scales[r0:r0 + chunk_rows] = (e + 127).to(torch.uint8).reshape(-1, K // MX_BLOCK)
    return codes, scales


def dequantize_blocks_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K] = e2m1(codes) * 2^(scales - 127) (exact; scales in [1, 254])."""
    N, K = codes.shape
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    v = lut[codes.long()].reshape(N, K // MX_BLOCK, MX_BLOCK)
    return (v * _pow2_f32(scales.to(torch.int32) - 127).unsqueeze(-1)).reshape(N, K)


def pack_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (uint8 [N / 16, K / 128, 64, 16] nibble bytes, uint8 [N / 16, K / 128, 64] scale bytes): the physical layout of
    include/dualhyp_hip.h "MXFP4 weights" (index l = 16 * MX block of the k-step + row of the group; even k in the low nibble)."""
    N, K = codes.shape
    if N % 16 or K % 128:
        raise ValueError(f"pack_mxfp4: N={N} must be a multiple of 16 and K={K} of 128")
    c = codes.reshape(N // 16, 16, K // 128, 4, 16, 2)
    b = c[..., 0] | (c[..., 1] << 4)                                    # [g, r, t, q, j]
    wq = b.permute(0, 2, 3, 1, 4).reshape(N // 16, K // 128, 64, 16).contiguous()
    ws = scales.reshape(N // 16, 16, K // 128, 4).permute(0, 2, 3, 1).reshape(N // 16, K // 128, 64).contiguous()
    return wq, ws


def unpack_mxfp4(wq: torch.Tensor, ws: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """pack_mxfp4's inverse: -> (codes [N, K], scales [N, K / 32])."""
    G, T = wq.shape[:2]
    b = wq.reshape(G, T, 4, 16, 16).permute(0, 3, 1, 2, 4)              # [g, r, t, q, j]
    codes = torch.stack((b & 15, b >> 4), dim=-1).reshape(G * 16, T * 128)
    scales = ws.reshape(G, T, 4, 16).permute(0, 3, 1, 2).reshape(G * 16, T * 4)
    return codes.contiguous(), scales.contiguous()


# ------------------------------------------------------------------------------------------ MXFP6 activations
def _e2m3_values() -> Tuple[float, ...]:
    """The magnitudes of the low five bits 0..31 of an e2m3 code (bit 5 is the sign): m / 8 for E = 0, else (1 + m / 8) * 2^(E - 1)."""
    return tuple((m / 8.0) if E == 0 else (1.0 + m / 8.0) * 2.0 ** (E - 1) for E in range(4) for m in range(8))


E2M3_VALUES = _e2m3_values()


def quantize_blocks_mxfp6(x: torch.Tensor, chunk_rows: int = 4096) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (uint8 [M, K] e2m3 codes, one per element, uint8 [M, K / 32] E8M0 bytes); the quantiser of include/dualhyp_hip.h
    "MXFP6 activations" in fp32 as the kernels of csrc/mxfp6.hip run it: frexp for floor(log2), a power-of-two scaling, and a
    round-half-even in units of the grid step of the value's binade, so every step is exact."""
    M, K = x.shape
    if K % MX_BLOCK:
        raise ValueError(f"quantize_blocks_mxfp6: K={K} is not a multiple of {MX_BLOCK}")
    codes = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    scales = torch.empty((M, K // MX_BLOCK), dtype=torch.uint8, device=x.device)
    for r0 in range(0, M, chunk_rows):
        v = x[r0:r0 + chunk_rows].float().reshape(-1, K // MX_BLOCK, MX_BLOCK)
        amax = v.abs().amax(dim=-1, keepdim=True)
        _, ex = torch.frexp(amax)                             # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
        e = (ex.to(torch.int32) - 3).clamp(-126, 127)
        e = torch.where(amax == 0, torch.zeros_like(e), e)
        a = v.abs() * _pow2_f32(-e)                           # < 8
        units = torch.where(a < 2, 8.0, torch.where(a < 4, 4.0, 2.0)).to(torch.float32)
        first = torch.where(a < 2, 0, torch.where(a < 4, 8, 16))
        c = (torch.round(a * units).to(torch.int32) + first).clamp(max=31).to(torch.uint8)      # torch.round: half to even
        c = c | (((v < 0) & (c != 0)).to(torch.uint8) << 5)
        codes[r0:r0 + chunk_rows] = c.reshape(-1, K)
        scales[r0:r0 + chunk_rows] = (e + 127).to(torch.uint8).reshape(-1, K // MX_BLOCK)
    return codes, scales


def dequantize_blocks_mxfp6(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [M, K] = e2m3(codes) * 2^(scales - 127) (exact; scales in [1, 254])."""
    M, K = codes.shape
    lut = torch.tensor(E2M3_VALUES + tuple(-v for v in E2M3_VALUES), dtype=torch.float32, device=codes.device)
    v = lut[codes.long()].reshape(M, K // MX_BLOCK, MX_BLOCK)
    return (v * _pow2_f32(scales.to(torch.int32) - 127).unsqueeze(-1)).reshape(M, K)


def pack_mxfp6(codes: torch.Tensor, scales: torch.Tensor, fill: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (uint8 [ceil(M / 16), K / 128, 3, 64, 8] code bytes, uint8 [ceil(M / 16), K / 128, 64] scale bytes): the physical layout of
    include/dualhyp_hip.h "MXFP6 activations" (index l = 16 * MX block of the k-step + row of the group; a block's 32 codes as one
    little-endian 192-bit number, its 24 bytes in three planes of 8).  Every byte of the rows past M in the last group is `fill`."""
    M, K = codes.shape
    if K % 128:
        raise ValueError(f"pack_mxfp6: K={K} must be a multiple of 128")
    G, T = (M + 15) // 16, K // 128
    c = codes.reshape(M, T, 4, 8, 4).to(torch.int32)                   # [m, t, q, three-byte word, element of the word]
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    b = torch.stack((w & 255, (w >> 8) & 255, (w >> 16) & 255), dim=-1).to(torch.uint8).reshape(M, T, 4, 3, 8)   # [m, t, q, p, j]
    xq = torch.full((G * 16, T, 4, 3, 8), fill, dtype=torch.uint8, device=codes.device)
    xs = torch.full((G * 16, T, 4), fill, dtype=torch.uint8, device=codes.device)
    xq[:M] = b
    xs[:M] = scales.reshape(M, T, 4)
    xq = xq.reshape(G, 16, T, 4, 3, 8).permute(0, 2, 4, 3, 1, 5).reshape(G, T, 3, 64, 8).contiguous()
    xs = xs.reshape(G, 16, T, 4).permute(0, 2, 3, 1).reshape(G, T, 64).contiguous()
    return xq, xs


def unpack_mxfp6(xq: torch.Tensor, xs: torch.Tensor, M: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """pack_mxfp6's inverse for the first M rows: -> (codes [M, K], scales [M, K / 32])."""
    G, T = xq.shape[:2]
    b = xq.reshape(G, T, 3, 4, 16, 8).permute(0, 4, 1, 3, 2, 5).reshape(G * 16, T, 4, 8, 3).to(torch.int32)   # [m, t, q, word, byte]
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    codes = torch.stack(((w >> 0) & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63), dim=-1).to(torch.uint8).reshape(G * 16, T * 128)
    scales = xs.reshape(G, T, 4, 16).permute(0, 3, 1, 2).reshape(G * 16, T * 4)
    return codes[:M].contiguous(), scales[:M].contiguous()


def quantize_model_mxfp4(model, kv_cache: str = "bf16", activations: str = "fp8") -> None:
    """quantize_model_fp8's contract (serving only, one way, bf16 weights released, `GPT.load_state_dict` and `save_checkpoint`
    refused, idempotent apart from `kv_cache` and `activations`) with MXFP4 block weights: LoRA is merged, the five dense matrices of every block
    become packed nibbles + E8M0 bytes (buffers `weight_mx4` / `weight_mx4_scale`), lm_head becomes e4m3 rows with channel scales
    as in fp8 mode; the embedding table, norms and adapter vectors stay bf16.  The model then is an fp8 model (`model.fp8`) with
    `model.weight_format == "mxfp4"`: whatever refuses an fp8 model refuses it.  An fp8 model is refused here, as an mxfp4 model
    is by quantize_model_fp8: neither has bf16 weights left to quantise.

    activations: "fp8" (default) keeps the block activations e4m3 rows with one scale per token; "mxfp6" quantises them to OCP MX
    MXFP6 blocks instead (include/dualhyp_hip.h "MXFP6 activations": e2m3 with one E8M0 byte per 32 elements, no token scale), the
    operand pair the MFMA runs at twice the fp8 rate; the final norm, lm_head and the adapter stay e4m3.  It sets
    `model.activation_format`; a repeat call may change it, as it may change `kv_cache` (the engine is rebuilt)."""
    from .gpt import GPT, _FrozenLinear, merge_lora_weights
    assert isinstance(model, GPT)
    if kv_cache not in ("bf16", "fp8"):
        raise ValueError(f"kv_cache is 'bf16' or 'fp8', got {kv_cache!r}")
    if activations not in ("fp8", "mxfp6"):
        raise ValueError(f"activations is 'fp8' or 'mxfp6', got {activations!r}")
    if getattr(model, "fp8", False):
        if getattr(model, "weight_format", "") != "mxfp4":
            raise RuntimeError("quantize_model_mxfp4: this model was quantised to fp8 (quantize_model_fp8); its bf16 weights no longer "
                               "exist, so it cannot be requantised to mxfp4 (quantise a freshly loaded model instead)")
        if model.kv_cache_dtype != kv_cache or getattr(model, "activation_format", "fp8") != activations:
            model.kv_cache_dtype = kv_cache
            model.activation_format = activations
            model.refresh_engine()
        return
    cfg = model.config
    if cfg.n_embd % 128 or cfg.intermediate_size % 128:
        raise ValueError(f"quantize_model_mxfp4: n_embd={cfg.n_embd} and intermediate_size={cfg.intermediate_size} must be multiples of 128")
    model.kv_cache_dtype = kv_cache
    model.activation_format = activations
    merge_lora_weights(model)
    head = model.lm_head.linear
    for m in model.modules():
        if not isinstance(m, _FrozenLinear):
            continue
        if m is head:
            q, s = quantize_rows_fp8(m.weight.data)
            m.register_buffer("weight_fp8", q, persistent=False)
            m.register_buffer("weight_scale", s, persistent=False)
        else:
            q, s = pack_mxfp4(*quantize_blocks_mxfp4(m.weight.data))
            m.register_buffer("weight_mx4", q, persistent=False)
            m.register_buffer("weight_mx4_scale", s, persistent=False)
        m.weight = nn.Parameter(torch.empty(0, dtype=m.weight.dtype, device=m.weight.device), requires_grad=False)
    for p in model.parameters():
        p.requires_grad_(False)
    model.fp8 = True
    model.weight_format = "mxfp4"
    model.refresh_engine()
