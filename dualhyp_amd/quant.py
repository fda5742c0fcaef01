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


def quantize_model_mxfp4(model, kv_cache: str = "bf16") -> None:
    """quantize_model_fp8's contract (serving only, one way, bf16 weights released, `GPT.load_state_dict` and `save_checkpoint`
    refused, idempotent apart from `kv_cache`) with MXFP4 block weights: LoRA is merged, the five dense matrices of every block
    become packed nibbles + E8M0 bytes (buffers `weight_mx4` / `weight_mx4_scale`), lm_head becomes e4m3 rows with channel scales
    as in fp8 mode; the embedding table, norms and adapter vectors stay bf16.  The model then is an fp8 model (`model.fp8`) with
    `model.weight_format == "mxfp4"`: whatever refuses an fp8 model refuses it.  An fp8 model is refused here, as an mxfp4 model
    is by quantize_model_fp8: neither has bf16 weights left to quantise."""
    from .gpt import GPT, _FrozenLinear, merge_lora_weights
    assert isinstance(model, GPT)
    if kv_cache not in ("bf16", "fp8"):
        raise ValueError(f"kv_cache is 'bf16' or 'fp8', got {kv_cache!r}")
    if getattr(model, "fp8", False):
        if getattr(model, "weight_format", "") != "mxfp4":
            raise RuntimeError("quantize_model_mxfp4: this model was quantised to fp8 (quantize_model_fp8); its bf16 weights no longer "
                               "exist, so it cannot be requantised to mxfp4 (quantise a freshly loaded model instead)")
        if model.kv_cache_dtype != kv_cache:
            model.kv_cache_dtype = kv_cache
            model.refresh_engine()
        return
    cfg = model.config
    if cfg.n_embd % 128 or cfg.intermediate_size % 128:
        raise ValueError(f"quantize_model_mxfp4: n_embd={cfg.n_embd} and intermediate_size={cfg.intermediate_size} must be multiples of 128")
    model.kv_cache_dtype = kv_cache
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
