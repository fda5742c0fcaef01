"""References, cases and gates for the four kernels of csrc/classifier.hip (tests/test_hip_classifier.py), CPU only.
tests/test_classifier_reference.py feeds the same gates mutants — each one a bug the kernels could plausibly have — to show
that they are rejected, while the truth rounded to bf16 and the bf16 yardstick pass.

Where a kernel's arithmetic is order-free or has one fixed order the reference restates it and the test compares BITS:
  im2col3        moves data, clears sign bits (relu), writes one 1.0 and zeros
  col2im3        ((0 + a0) + a1) + a2 in fp32, the gate pre > 0, the product with the mask in fp32, one rounding to bf16
  pooled means   bf16((sequential fp32 sum over t of max(h, 0)) / len), an IEEE division
Where the order is free (FMA contraction, wave reductions) there are two kinds of case:
  exact    operands chosen so that every product, partial sum and rounding point is exact (asserted here: InexactCase), value equality
  ragged   fp64 from the bit-exact bf16 pooled means; the kernel's value must be the bf16 rounding of SOME value within +-E:
             pool_head      E = (H/256 + 12) 2^-24 sum_c |m_c w_jc|
                 a thread's chain of ceil(H/256) FMAs, 6 wave-reduction additions, 3 additions of the four waves and the bias addition:
                 at most H/256 + 11 roundings, each within 2^-24 of a partial sum that sum|m w| + |bias| bounds.  The bound leaves
                 the bias out, which holds while |bias| <= sum|m w| / 16 (asserted for every logit of a case).
             pool_head_bwd  E = 8 2^-24 sum_j |dl_j w_jc| / len
                 three products, two additions, the rounded 1/len and the product with it: 7 roundings.
  The whole module is gated against fp64 autograd by its distance relative to a bf16 yardstick (module_gate below).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

import bwd_reference as BR
from gemm_exact_reference import InexactCase, exact_bf16

F64, F32, BF, I16 = torch.float64, torch.float32, torch.bfloat16, torch.int16
U24 = 2.0 ** -24
ONE_BITS = 0x3F80

# ---- the cases of tests/test_hip_classifier.py (and of the CPU tests of the gates); every one has at most 32 tokens, but for
# the single sequences of 2 pool + 3 = 43 tokens at pool 20
# im2col3 (B, T, C): the last two have more than 256 8-element chunks per row (a second pass of the kernel's loop)
IM2COL_SHAPES = [(1, 1, 8), (3, 2, 8), (2, 3, 24), (3, 5, 256), (2, 4, 1024), (2, 3, 1280)]
# pool_head / pool_head_bwd (B, T, H, pool): exact (power-of-two pool dividing T) and ragged (ceil-mode tails)
EXACT = [(2, 8, 64, 8), (3, 16, 256, 8), (2, 8, 320, 4), (3, 2, 64, 2), (2, 16, 320, 16), (5, 1, 256, 1)]
RAGGED = [(2 if T <= 16 else 1, T, H, pool) for pool in (10, 20) for T in (1, pool - 1, pool + 1, 2 * pool + 3) for H in (64, 256, 320)]
# the whole module (B, T, C, H, pool)
MODULE_CASES = [(B, T, C, H, 10) for C in (8, 1024) for H in (64, 256) for B, T in ((3, 1), (3, 2), (2, 10), (2, 11), (1, 23))]


def bits(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == BF
    return x.contiguous().view(I16)


def pack_ld(C: int) -> int:
    """The leading dimension relprompt._pack_conv gives the im2col matrix."""
    return (3 * C + 1 + 63) // 64 * 64


def rnd(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------ im2col3
def random_bf16_bits(shape, gen: torch.Generator) -> torch.Tensor:
    """Random bf16 bit patterns of both signs (int16), with -0.0, +0.0, subnormals and the largest finite values planted; no inf, no NaN."""
    b = torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32)
    is_special = (b & 0x7F80) == 0x7F80
    b = torch.where(is_special, b & ~0x4000, b)                     # exponent 0xFF -> 0xBF: finite
    flat = b.reshape(-1)
    plant = torch.tensor([-32768, 0, 0x0001, -32768 | 0x0001, 0x007F, -32768 | 0x007F, 0x7F7F, -32768 | 0x7F7F, 0x3F80, -32768 | 0x3F80], dtype=torch.int32)
    n = min(plant.numel(), flat.numel())
    pos = torch.randperm(flat.numel(), generator=gen)[:n]
    flat[pos] = plant[:n]
    return flat.reshape(shape).to(I16)


def im2col3_ref(xb: torch.Tensor, ld: int, relu: bool, mutant: Optional[str] = None) -> torch.Tensor:
    """int16 [B*T, ld] from the int16 bits xb [B, T, C]: columns dk*C + c = f(x[b, t + dk - 1, c]) (0 outside the sequence),
    column 3C = 1.0, zeros up to ld.  relu: a set sign bit gives +0.0 bits.
    mutants: 'cross_batch' (the neighbouring row of the flat [B*T, C] buffer, whichever sequence it belongs to),
             'reversed_taps' (t + 1 - dk), 'relu_keeps_neg_zero' (max(x, 0) by value: -0.0 survives)."""
    B, T, C = xb.shape
    assert ld % 8 == 0 and ld >= 3 * C + 8 and C % 8 == 0
    x = xb
    if relu:
        if mutant == "relu_keeps_neg_zero":
            x = torch.where(xb.view(BF).float() < 0, torch.zeros((), dtype=I16), xb)
        else:
            x = torch.where(xb < 0, torch.zeros((), dtype=I16), xb)
    out = torch.zeros((B, T, ld), dtype=I16)
    t = torch.arange(T)
    for dk in range(3):
        off = (1 - dk) if mutant == "reversed_taps" else (dk - 1)
        if mutant == "cross_batch":
            flat = x.reshape(B * T, C)
            r = torch.arange(B * T) + off
            ok = (r >= 0) & (r < B * T)
            tap = torch.where(ok[:, None], flat[r.clamp(0, B * T - 1)], torch.zeros((), dtype=I16)).view(B, T, C)
        else:
            ts = t + off
            ok = (ts >= 0) & (ts < T)
            tap = torch.where(ok[None, :, None], x[:, ts.clamp(0, T - 1)], torch.zeros((), dtype=I16))
        out[:, :, dk * C:(dk + 1) * C] = tap
    out[:, :, 3 * C] = ONE_BITS
    return out.view(B * T, ld)


# ------------------------------------------------------------------------------------------------------------ col2im3
def col2im3_inputs(B: int, T: int, C: int, ld: int, gen: torch.Generator, p_drop: float = 0.1) -> Dict[str, torch.Tensor]:
    """dcol [B*T, ld] with a different magnitude per tap (scales 1, 16, 256: a swapped or shifted tap changes every element) and large
    finite poison in the pad columns; pre with +0, -0 and negatives; a dropout mask of 0 and bf16(1 / (1 - p))."""
    assert ld > 3 * C
    dcol = torch.full((B * T, ld), 3.0e38, dtype=F64)
    dcol[:, 3 * C::2] = -3.0e38
    for dk, sc in enumerate((1.0, 16.0, 256.0)):
        dcol[:, dk * C:(dk + 1) * C] = (torch.rand((B * T, C), generator=gen, dtype=F64) + 0.5) * sc * torch.where(
            torch.rand((B * T, C), generator=gen) < 0.5, -1.0, 1.0)
    pre = (torch.rand((B, T, C), generator=gen, dtype=F64) * 2 - 1)
    kind = torch.randint(0, 6, (B, T, C), generator=gen)
    pre = torch.where(kind == 0, torch.zeros((), dtype=F64), pre).to(BF)
    pre = torch.where(kind == 1, torch.tensor(-0.0, dtype=BF), pre)
    assert bool((bits(pre) == -32768).any()) or pre.numel() < 12
    keep = torch.rand((B, T, C), generator=gen) >= p_drop
    mask = keep.to(BF) * (1.0 / (1.0 - p_drop))                   # as _ClassifierFn builds it: bf16(1 / (1 - p)) or 0
    return {"dcol": dcol.to(BF), "pre": pre, "mask": mask}


def col2im3_ref(dcol: torch.Tensor, B: int, T: int, C: int, pre: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [B, T, C]: dx[b, t, c] = [pre > 0] * mask * sum_dk dcol[b, t + 1 - dk, dk*C + c] in the kernel's fixed fp32 order.
    mutants: 'shift' (t - 1 + dk), 'pre_ge' (gate pre >= 0), 'no_mask'."""
    ld = dcol.size(1)
    d = dcol.to(F32).view(B, T, ld)
    s = torch.zeros((B, T, C), dtype=F32)
    t = torch.arange(T)
    for dk in range(3):
        tr = t - 1 + dk if mutant == "shift" else t + 1 - dk
        ok = (tr >= 0) & (tr < T)
        tap = torch.where(ok[None, :, None], d[:, tr.clamp(0, T - 1), dk * C:(dk + 1) * C], torch.zeros((), dtype=F32))
        s = s + tap
    if pre is not None:
        gate = pre.to(F32) >= 0 if mutant == "pre_ge" else pre.to(F32) > 0
        s = torch.where(gate, s, torch.zeros((), dtype=F32))
    if mask is not None and mutant != "no_mask":
        s = s * mask.to(F32)
    return s.to(BF)


# ------------------------------------------------------------------------------------------------------------ pooling head
def windows(T: int, pool: int):
    return [(t0, min(t0 + pool, T)) for t0 in range(0, T, pool)]


def pooled_ref(h: torch.Tensor, pool: int, mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [B*P, H]: bf16((sequential fp32 sum over the window of max(h, 0)) / len); ceil mode: the last window divides by its own
    length.  mutants: 'tail_div_pool', 'floor_mode' (a partial tail window is missing: zeros), 'relu_after_mean'."""
    B, T, H = h.shape
    x = h.to(F32)
    if mutant != "relu_after_mean":
        x = torch.clamp_min(x, 0.0)
    out = []
    for t0, t1 in windows(T, pool):
        s = torch.zeros((B, H), dtype=F32)
        for t in range(t0, t1):
            s = s + x[:, t]
        n = pool if mutant == "tail_div_pool" else t1 - t0
        m = s / torch.tensor(float(n), dtype=F32)
        if mutant == "relu_after_mean":
            m = torch.clamp_min(m, 0.0)
        if mutant == "floor_mode" and t1 - t0 < pool:
            m = torch.zeros_like(m)
        out.append(m.to(BF))
    return torch.stack(out, 1).reshape(-1, H)


def head_inputs(B: int, T: int, H: int, pool: int, gen: torch.Generator, exact: bool) -> Dict[str, torch.Tensor]:
    """exact: h in {-1, 0, 1}, w in {-1, 0, 1}, integer bias and dl — with a power-of-two pool dividing T every value the kernels form
    is a multiple of 1/pool far below 2^24/pool (exact in fp32 in any order) and the results are checked to be bf16 values.
    ragged: uniform bf16 h (+-1, a fifth of them exact zeros of either sign), w (+-0.5), bias (+-1/16), fp32 dl (+-1)."""
    if exact:
        assert pool & (pool - 1) == 0 and T % pool == 0
        h = torch.randint(-1, 2, (B, T, H), generator=gen).to(BF)
        w = torch.randint(-1, 2, (3, H), generator=gen).to(BF)
        bias = torch.randint(-3, 4, (3,), generator=gen).to(BF)
        dl = torch.randint(-4, 5, (B, (T + pool - 1) // pool, 3), generator=gen).to(F32)
    else:
        h = BR.bf16_uniform((B, T, H), 1.0, gen)
        z = torch.randint(0, 10, (B, T, H), generator=gen)
        h = torch.where(z == 0, torch.zeros((), dtype=BF), h)
        h = torch.where(z == 1, torch.tensor(-0.0, dtype=BF), h)
        w = BR.bf16_uniform((3, H), 0.5, gen)
        bias = BR.bf16_uniform((3,), 1.0 / 16, gen)
        dl = (torch.rand((B, (T + pool - 1) // pool, 3), generator=gen, dtype=F64) * 2 - 1).to(F32)
    return {"h": h, "w": w, "bias": bias, "dl": dl}


def pool_head_ref(h, w, bias, pool: int, exact: bool, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """-> {'logits': fp64 [B, P, 3], 'E': fp64 [B, P, 3]} from the bit-exact pooled means (E = 0 and a bf16-valued result for exact cases)."""
    B, T, H = h.shape
    m = pooled_ref(h, pool, mutant).to(F64)                     # [B*P, H]
    w64 = w.to(F64)
    absum = m.abs() @ w64.abs().T
    logits = m @ w64.T + bias.to(F64)
    if exact:
        if not bool((absum.max() + bias.to(F64).abs().max()) * pool < 2 ** 24):
            raise InexactCase("pool_head: partial sums leave the exact fp32 range")
        exact_bf16(m, "pooled mean")
        exact_bf16(logits, "logits")
        E = torch.zeros_like(logits)
    else:
        if mutant is None and not bool((bias.to(F64).abs()[None] <= absum / 16).all()):
            raise InexactCase("pool_head: |bias| > sum|m w| / 16: the error bound, which leaves the bias out, does not cover this case")
        E = (H / 256 + 12) * U24 * absum
    P = len(windows(T, pool))
    return {"logits": logits.view(B, P, 3), "E": E.view(B, P, 3)}


def pool_head_bwd_ref(h, w, dl, pool: int, exact: bool, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """-> {'dh': fp64 [B, T, H] (0 where h <= 0), 'E', 'pooled': bf16 [B*P, H], 'gate': bool [B, T, H]}.
    mutants: pooled_ref's, and 'dh_no_len' (dh not divided by the window length)."""
    B, T, H = h.shape
    g = torch.einsum("bpj,jc->bpc", dl.to(F64), w.to(F64))
    ga = torch.einsum("bpj,jc->bpc", dl.to(F64).abs(), w.to(F64).abs())
    dh = torch.zeros((B, T, H), dtype=F64)
    E = torch.zeros((B, T, H), dtype=F64)
    for p, (t0, t1) in enumerate(windows(T, pool)):
        n = 1 if mutant == "dh_no_len" else pool if mutant == "tail_div_pool" else t1 - t0
        if mutant == "floor_mode" and t1 - t0 < pool:
            continue
        dh[:, t0:t1] = (g[:, p] / n)[:, None]
        E[:, t0:t1] = (8 * U24 * ga[:, p] / n)[:, None]
    gate = h.to(F64) > 0
    dh = torch.where(gate, dh, torch.zeros((), dtype=F64))
    E = torch.where(gate, E, torch.zeros((), dtype=F64))
    if exact:
        exact_bf16(dh, "dh")
        E = torch.zeros_like(E)
    return {"dh": dh, "E": E, "pooled": pooled_ref(h, pool, mutant), "gate": gate}


def band_gate(got: torch.Tensor, ref: torch.Tensor, E: torch.Tensor) -> dict:
    """`got` (bf16 values) must be the bf16 rounding of some value within +-E of `ref`: rounding to nearest is monotone, so
    bf16(ref - E) <= got <= bf16(ref + E).  E = 0: value equality with bf16(ref) (-0.0 == 0.0; a NaN equals nothing)."""
    g = got.to(F64).cpu()
    lo, hi = (ref - E).to(BF).to(F64), (ref + E).to(BF).to(F64)
    bad = ~((g >= lo) & (g <= hi))
    return {"ok": not bool(bad.any()), "n_bad": int(bad.sum()), "of": bad.numel(),
            "worst": torch.where(bad, torch.maximum(lo - g, g - hi), torch.zeros_like(g)).nan_to_num(nan=math.inf).max().item()}


# ------------------------------------------------------------------------------------------------------------ whole module
PARAMS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "classifier.weight", "classifier.bias")


def module_inputs(B: int, T: int, C: int, H: int, pool: int, seed: int) -> Dict[str, torch.Tensor]:
    """bf16-valued x, parameters (fp32 tensors holding bf16 values, as the fp32 masters of a bf16 checkpoint) and dlogits."""
    g = torch.Generator().manual_seed(seed)
    P = (T + pool - 1) // pool
    u = BR.bf16_uniform
    return {"x": u((B, T, C), 1.5, g),
            "conv1.weight": u((H, C, 3), 1.0 / math.sqrt(3 * C), g).float(), "conv1.bias": u((H,), 1.0 / 16, g).float(),
            "conv2.weight": u((H, H, 3), 1.0 / math.sqrt(3 * H), g).float(), "conv2.bias": u((H,), 1.0 / 16, g).float(),
            "classifier.weight": u((3, H), 1.0 / math.sqrt(H), g).float(), "classifier.bias": u((3,), 1.0 / 16, g).float(),
            "dlogits": u((B, P, 3), 1.0, g)}


def drop_scale(p: float) -> float:
    return torch.tensor(1.0 / (1.0 - p)).to(BF).item()


def module_truth(inp: Dict[str, torch.Tensor], pool: int, keep: Optional[torch.Tensor] = None, p_drop: float = 0.0,
                 mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """fp64 autograd of the torch module (Conv1d k3 pad 1 -> ReLU -> dropout with the given keep mask [B, T, H] scaled by
    bf16(1 / (1 - p)) -> Conv1d -> ReLU -> AvgPool1d(pool, ceil_mode) -> Linear) -> {'logits', the six gradients}.
    mutants (whole-module versions of the kernels' bugs): 'conv_cross_batch' (the convolutions run over the flat B*T token axis),
    'floor_mode' (AvgPool1d without ceil_mode: logits of the tail window are 0), 'tail_div_pool' (the tail window padded with zeros)."""
    Fn = torch.nn.functional
    ps = {k: inp[k].to(F64).clone().requires_grad_() for k in PARAMS}
    x = inp["x"].to(F64)
    B, T, C = x.shape

    def conv(a, w, b):                                    # a [B, T, Cin] -> [B, T, H]
        if mutant == "conv_cross_batch":
            return Fn.conv1d(a.reshape(1, B * T, -1).transpose(1, 2), w, b, padding=1).transpose(1, 2).reshape(B, T, -1)
        return Fn.conv1d(a.transpose(1, 2), w, b, padding=1).transpose(1, 2)
    a1 = torch.relu(conv(x, ps["conv1.weight"], ps["conv1.bias"]))
    if keep is not None:
        a1 = a1 * (keep.to(F64) * drop_scale(p_drop))
    a2 = torch.relu(conv(a1, ps["conv2.weight"], ps["conv2.bias"])).transpose(1, 2)
    P = (T + pool - 1) // pool
    if mutant == "floor_mode":
        pooled = Fn.avg_pool1d(a2, pool, ceil_mode=False) if T >= pool else a2[:, :, :0]
        pooled = torch.cat([pooled, torch.zeros((B, a2.size(1), P - pooled.size(2)), dtype=F64)], 2)
    elif mutant == "tail_div_pool":
        pooled = Fn.avg_pool1d(Fn.pad(a2, (0, P * pool - T)), pool)
    else:
        pooled = Fn.avg_pool1d(a2, pool, ceil_mode=True)
    logits = pooled.transpose(1, 2) @ ps["classifier.weight"].T + ps["classifier.bias"]
    logits.backward(inp["dlogits"].to(F64))
    out = {"logits": logits.detach()}
    out.update({k: v.grad for k, v in ps.items()})
    return out


def module_yardstick(inp: Dict[str, torch.Tensor], pool: int, keep: Optional[torch.Tensor] = None, p_drop: float = 0.0,
                     acc: torch.dtype = F64, rounded: bool = True) -> Dict[str, torch.Tensor]:
    """What a correct bf16 path computes, in closed form: products accumulated in `acc` from bf16 operands; the conv outputs, the
    dropped activation, the pooled means, the logits and every activation gradient (dlogits as an operand, dh2, dcol2, dh1) rounded
    to bf16 once; parameter gradients accumulated over the tokens without rounding.  Results in fp64."""
    rnd_ = rnd if rounded else (lambda t: t)          # rounded False: the same formulas in exact arithmetic
    x = inp["x"].to(acc)
    B, T, C = x.shape
    w1, b1, w2, b2, wc, bc = (rnd_(inp[k].to(acc)) for k in PARAMS)
    H = w1.size(0)

    def col(a):                                           # [B, T, Cin] -> [B, T, 3 Cin] (tap-major, as the im2col matrix)
        z = torch.zeros_like(a[:, :1])
        return torch.cat([torch.cat([z, a[:, :-1]], 1), a, torch.cat([a[:, 1:], z], 1)], -1)

    def flat_w(w):                                        # [H, Cin, 3] -> [H, 3 Cin]
        return w.permute(0, 2, 1).reshape(w.size(0), -1)
    col1 = col(x)
    h1 = rnd_(col1 @ flat_w(w1).T + b1)
    a1 = torch.relu(h1)
    m = None
    if keep is not None:
        m = keep.to(acc) * drop_scale(p_drop)
        a1 = rnd_(a1 * m)
    col2 = col(a1)
    h2 = rnd_(col2 @ flat_w(w2).T + b2)
    r2 = torch.relu(h2)
    wins = windows(T, pool)
    pooled = torch.stack([rnd_(r2[:, t0:t1].sum(1) / (t1 - t0)) for t0, t1 in wins], 1)       # [B, P, H]
    logits = rnd_(pooled @ wc.T + bc)
    dl = inp["dlogits"].to(acc)
    gwc = torch.einsum("bpj,bpc->jc", rnd_(dl), pooled)
    gbc = dl.sum((0, 1))
    g = dl @ wc                                            # [B, P, H]
    dh2 = torch.zeros_like(h2)
    for p, (t0, t1) in enumerate(wins):
        dh2[:, t0:t1] = rnd_(g[:, p] / (t1 - t0))[:, None]
    dh2 = torch.where(h2 > 0, dh2, torch.zeros((), dtype=acc))
    gW2 = torch.einsum("bth,btk->hk", dh2, col2)
    gb2 = dh2.sum((0, 1))
    dcol2 = rnd_(dh2 @ flat_w(w2))                          # [B, T, 3H]
    z = torch.zeros_like(dcol2[:, :1, :H])
    da1 = torch.cat([dcol2[:, 1:, :H], z], 1) + dcol2[:, :, H:2 * H] + torch.cat([z, dcol2[:, :-1, 2 * H:]], 1)
    dh1 = torch.where(h1 > 0, da1, torch.zeros((), dtype=acc))
    if m is not None:
        dh1 = dh1 * m
    dh1 = rnd_(dh1)
    gW1 = torch.einsum("bth,btk->hk", dh1, col1)
    gb1 = dh1.sum((0, 1))

    def unflat(gw, cin):
        return gw.reshape(H, 3, cin).permute(0, 2, 1)
    out = {"logits": logits, "conv1.weight": unflat(gW1, C), "conv1.bias": gb1, "conv2.weight": unflat(gW2, H), "conv2.bias": gb2,
           "classifier.weight": gwc, "classifier.bias": gbc}
    return {k: v.to(F64) for k, v in out.items()}


FP32_FLOOR = 2.0 ** -16


def _rows(name: str, t: torch.Tensor) -> torch.Tensor:
    """One row per output row: [H, Cin*3] for a conv weight, [B*P, 3] logits, [3, H]; a bias is one row."""
    if t.dim() == 1:
        return t.reshape(1, 1, -1)
    return t.reshape(-1, 1, 3) if name == "logits" else t.reshape(t.size(0), 1, -1)


def module_gate(got: Dict[str, torch.Tensor], truth: Dict[str, torch.Tensor], yard: Dict[str, torch.Tensor]) -> Dict[str, dict]:
    """Logits and the six gradients, every element: per output row e = max |got - truth| / max(max |truth|_row, ROW_FLOOR x tensor max)
    (bwd_reference.row_errors), gated as bwd_reference.attn_gate gates the attention gradients: the worst row within 1.5x the
    yardstick's worst, the mean within 1.25x, and no row above 1.5x its own yardstick figure + 2^-7.
    classifier.bias has no bf16 rounding point on either path (an fp32 sum of the incoming gradient): where the yardstick's own
    error is below FP32_FLOOR = 2^-16 relative (fp32 accumulation noise of these few-hundred-term sums), that floor stands in for it."""
    res = {}
    for k in ("logits",) + PARAMS:
        tr = _rows(k, truth[k].to(F64))
        floor = BR.ROW_FLOOR * tr.abs().max().item()
        eg = BR.row_errors(_rows(k, got[k].to(F64).cpu()), tr, floor)
        ey = BR.row_errors(_rows(k, yard[k].to(F64)), tr, floor).clamp_min(FP32_FLOOR)
        r = BR.attn_gate(eg.clamp_min(FP32_FLOOR), ey)
        res[k] = r
    return res
