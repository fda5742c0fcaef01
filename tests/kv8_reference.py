"""CPU restatement of the fp8 KV cache scheme (include/dualhyp_hip.h "fp8 KV cache"), in torch: helpers of test_kv8_host.py and
test_hip_kv8.py.

A vector x of head_size values has amax = max |x| and the exponent e, the smallest integer with amax <= 448 * 2^e: with
amax = m * 2^ex, m in [0.5, 1) (frexp), e = ex - 9 if m <= 0.875 else ex - 8; clamped to [-100, 100]; 0 for amax == 0.
byte = e4m3fn_rne(x * 2^-e), saturated to +-448; value = e4m3 * 2^e."""
import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import ger_oracle as O

E_MIN, E_MAX = -100, 100


def _pow2(e: Tensor) -> Tensor:
    """2^e as fp32 from the exponent field (e in [-126, 127])."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def kv8_quantize(x: Tensor) -> Tuple[Tensor, Tensor]:
    """x [..., hs] (any float dtype) -> (uint8 e4m3fn bit patterns [..., hs], int8 exponents [...])."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(E_MIN, E_MAX)
    y = (xf * _pow2(-e).unsqueeze(-1)).clamp(-448.0, 448.0)      # a power of two: the scaling is exact
    return y.to(torch.float8_e4m3fn).view(torch.uint8), e.to(torch.int8)


def kv8_dequantize(q: Tensor, e: Tensor) -> Tensor:
    """-> fp32 [..., hs]: e4m3 * 2^e."""
    return q.view(torch.float8_e4m3fn).float() * _pow2(e).unsqueeze(-1)


def kv8_round_trip(x: Tensor) -> Tensor:
    return kv8_dequantize(*kv8_quantize(x)).to(x.dtype)


def edge_rows(hs: int) -> Tensor:
    """bf16 [n, hs]: all-zero; amax = 448 * 2^k exactly (k = 0, -3, 5); one bf16 step above each (the exponent must step);
    amax 1e-30; amax 3e4; a negative extreme.  The other elements are fractions of amax spread over the e4m3 range."""
    frac = torch.linspace(-1.0, 1.0, hs).mul(0.97)
    frac[1::5] *= 2.0 ** -6
    frac[2::7] *= 2.0 ** -10
    rows = [torch.zeros(hs)]

    def row(amax, sign=1.0):
        r = frac.clone() * amax
        r[hs // 3] = sign * amax
        rows.append(r)

    for k in (0, -3, 5):
        a = torch.tensor(448.0 * 2.0 ** k, dtype=torch.bfloat16)
        row(a.float().item())
        above = (a.view(torch.int16) + 1).view(torch.bfloat16)          # the next bf16 value
        row(above.float().item())
    row(1e-30)
    row(3e4)
    row(3.0e38, sign=-1.0)            # past 448 * 2^100: the exponent clamps and the bytes saturate
    row(448.0 * 2.0 ** -2, sign=-1.0)
    return torch.stack(rows).to(torch.bfloat16)


class OracleGPTKV8(O.OracleGPT):
    """OracleGPT whose attention sees k (after rope) and v through the fp8 KV cache scheme: both are rounded per KV group and
    position before the cache write and the SDPA (ger/model.py:202-268 otherwise, as OracleGPT._attention)."""

    def _attention(self, l: int, x: Tensor, cos: Tensor, sin: Tensor, mask: Optional[Tensor],
                   input_pos: Optional[Tensor]) -> Tensor:
        cfg, sd = self.cfg, self.sd
        p = f"transformer.h.{l}.attn."
        B_, T, C = x.shape
        s = (cfg.alpha / cfg.r) if self.has_lora else 0.0
        kvw = cfg.n_embd // (cfg.n_head // cfg.n_query_groups)
        qkv = O.lora_qkv_linear(x, sd[p + "attn.linear.weight"], sd.get(p + "attn.lora_A"), sd.get(p + "attn.lora_B"), s,
                                (cfg.n_embd, kvw, kvw), cfg.dropout, self.training, sd.get(p + "attn.linear.weight_scale"))
        q_per_kv = cfg.n_head // cfg.n_query_groups
        hs = cfg.head_size
        qkv = qkv.view(B_, T, cfg.n_query_groups, q_per_kv + 2, hs).permute(0, 2, 3, 1, 4)
        q, k, v = qkv.split((q_per_kv, 1, 1), dim=2)
        if cfg.n_query_groups != 1:
            k = k.expand(B_, cfg.n_query_groups, q_per_kv, T, hs)
            v = v.expand(B_, cfg.n_query_groups, q_per_kv, T, hs)
        q = q.reshape(B_, -1, T, hs)
        k = k.reshape(B_, -1, T, hs)
        v = v.reshape(B_, -1, T, hs)
        n = cfg.rope_n_elem
        q = torch.cat((O.apply_rope(q[..., :n], cos, sin), q[..., n:]), dim=-1)
        k = torch.cat((O.apply_rope(k[..., :n], cos, sin), k[..., n:]), dim=-1)
        k, v = kv8_round_trip(k), kv8_round_trip(v)          # the heads of a group hold copies: one rounding per group
        if input_pos is not None:
            ck, cv = self.kv[l]
            ck, cv = ck.to(dtype=k.dtype), cv.to(dtype=v.dtype)
            k = ck.index_copy_(2, input_pos, k)
            v = cv.index_copy_(2, input_pos, v)
            self.kv[l] = (k, v)
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, scale=1.0 / math.sqrt(hs), is_causal=mask is None)
        y = y.transpose(1, 2).reshape(B_, T, C)
        return O.lora_linear(y, sd[p + "proj.linear.weight"], sd.get(p + "proj.lora_A"), sd.get(p + "proj.lora_B"), s, cfg.dropout,
                             self.training, sd.get(p + "proj.linear.weight_scale"))
