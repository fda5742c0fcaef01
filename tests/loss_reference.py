"""fp64 references, cases and gates for the cross-entropy kernels of csrc/loss.hip (tests/test_hip_loss.py), CPU only.
tests/test_loss_reference.py runs the same gates on mutants to show that they reject the bugs they are meant to reject,
and on an fp32 emulation of the kernel's own loop to show that a correct fp32 evaluation passes.

    forward : lse[r] = logsumexp(x[r, :]) ; loss[r] = lse[r] - x[r, t[r]]   (0 for an ignored row)
    backward: d[r, c] = g[r] * (exp(x[r, c] - lse[r]) - [c == t[r]])        (0 for an ignored row)
A row is ignored when its target lies outside [0, V): -1 is the ignore index of the fine-tune, and the kernels treat every
other out-of-range target the same way (their contract; nothing is read or written out of bounds for such a target).

The kernel walks a row with 256 threads, thread i reading columns i, i + 256, ... (one "stride" of 256 columns per
step) with an online max / sum, then combines the threads inside each wave and the four waves.

Forward gate, per row, against fp64 logsumexp of the STORED logits (R = max - min of the row's finite logits):
    |lse - ref| <= ulp32(ref) + (R + V/256 + 12) 2^-24
      ulp32(ref)   the one rounding of M + logf(S) (log S <= log V, so M + log S is ref up to what follows)
      V/256 2^-24  worst case of a thread's V/256-term fp32 sum of positive terms (relative error of S, = absolute of log S)
      R 2^-24      __expf(v - m): the fp32 difference v - m is rounded (relative 2^-24 of |v - m| <= R), which moves the
                   exponential by that much relative; terms that matter to S have |v - m| far below R
      12 2^-24     the hardware exp and log (about 1 ulp each), the 6 + 3 additions of the wave and block reductions and the rescaling
                   products s * __expf(m - wm)
    |loss - (ref - x_t)| <= the same + ulp32(max(|lse|, |x_t|))   (the rounding of the subtraction)
Backward gate, per element, given the lse the forward produced (tolerance L of its row as above), p = softmax64:
    |d - g (p - onehot)| <= |g| p (e^L - 1)                  a wrong-by-L lse scales every probability by e^(+-L)
                          + |g| (|x - lse| + 3) 2^-24 p       the rounded difference inside __expf, and the exp itself
                          + ulp32(g (p - onehot))             the subtraction and the product with g
                          + |g| 2^-126                        a probability below the smallest normal fp32 may flush to 0
  for bf16 logits the stored value must be the bf16 rounding (nearest even, monotone) of some value inside that band:
    bf16(truth - tol) <= d <= bf16(truth + tol).
  A column that holds -inf has probability 0: its gradient must be exactly 0.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
WIDTHS = (1, 3, 63, 65, 255, 256, 257, 1000, 32064, 128256)
U24 = 2.0 ** -24


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |x| (fp64 tensor in, fp64 out)."""
    a = x.to(F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def edge_columns(V: int) -> List[int]:
    """The columns at the edges of the waves (63 | 64), of the first stride (255 | 256) and of the last, partial stride."""
    tail = V - V % 256
    cols = [0, 63, 64, 255, 256, tail - 1, tail, V - 1]
    return sorted({c for c in cols if 0 <= c < V})


def _ladder(steps: int, dtype: torch.dtype) -> torch.Tensor:
    """`steps` strictly ascending values of `dtype` in [-8, 8]."""
    cand = torch.unique(torch.linspace(-8.0, 8.0, 8193, dtype=F64).to(dtype).to(F64))
    assert steps <= cand.numel()
    v = cand[torch.linspace(0, cand.numel() - 1, steps, dtype=F64).round().long()]
    assert steps == 1 or bool((v[1:] > v[:-1]).all())
    return v


def make_case(V: int, dtype: torch.dtype, seed: int = 0) -> Dict[str, object]:
    """At most 16 rows of width V (the stored logits in `dtype`, int64 targets, fp32 grad_row) and the kind of each row:
      peak      a flat row with ONE column 24 above it, on an edge column; the target on another edge column (p_t ~ 0)
      peak=t    the same with the target on the peak (p_t ~ 1)
      ascend    ascending along every thread's stride (the online max rescales at every step) ; descend: never rescales
      large     logits uniform in +-80 (bf16) / +-100 (fp32) with one column at +96 / +100 and one at -96 / -100: exp(80) still fits
                in fp32 (exp overflows above 88.7), so the bf16 row carries the +-96 pair to overflow without the max subtraction
      random    uniform in +-6
      ignored   target -1, and target V (out of range: ignored by the kernel's contract); grad_row NaN for both"""
    g = torch.Generator().manual_seed(1000 * seed + V % 9973)
    edges = edge_columns(V)
    rows, tg, kinds = [], [], []
    flat = -1.5
    for i, e in enumerate(edges):
        r = torch.full((V,), flat, dtype=F64)
        r[e] = flat + 24.0
        rows.append(r)
        tg.append(edges[(i + 1) % len(edges)])
        kinds.append("peak" if len(edges) > 1 else "peak=t")
    r = torch.full((V,), flat, dtype=F64)
    r[edges[-1]] = flat + 24.0
    rows.append(r), tg.append(edges[-1]), kinds.append("peak=t")
    steps = (V + 255) // 256
    lad = _ladder(steps, dtype)
    up = lad[torch.arange(V) // 256]
    rows.append(up), tg.append(edges[len(edges) // 2]), kinds.append("ascend")
    rows.append(lad.flip(0)[torch.arange(V) // 256]), tg.append(edges[-1]), kinds.append("descend")
    big, top = (80.0, 96.0) if dtype == BF else (100.0, 100.0)
    r = (torch.rand(V, generator=g, dtype=F64) * 2 - 1) * big
    r[int(torch.randint(0, V, (1,), generator=g))] = top
    if V > 1:
        r[(int(r.argmax()) + 1) % V] = -top
    rows.append(r), tg.append(int(torch.randint(0, V, (1,), generator=g))), kinds.append("large")
    rows.append((torch.rand(V, generator=g, dtype=F64) * 2 - 1) * 6), tg.append(int(torch.randint(0, V, (1,), generator=g))), kinds.append("random")
    rows.append((torch.rand(V, generator=g, dtype=F64) * 2 - 1) * 6), tg.append(-1), kinds.append("ignored")
    rows.append((torch.rand(V, generator=g, dtype=F64) * 2 - 1) * 6), tg.append(V), kinds.append("ignored")
    assert len(rows) <= 16
    logits = torch.stack(rows).to(dtype)
    targets = torch.tensor(tg, dtype=torch.int64)
    grow = (torch.rand(len(rows), generator=g, dtype=F64) + 0.5).to(F32)
    grow[1::2] *= -1                                   # both signs of the incoming gradient
    grow[[k == "ignored" for k in kinds]] = math.nan   # never read for an ignored row
    return {"logits": logits, "targets": targets, "grow": grow, "kinds": kinds, "V": V}


def neg_inf_case(V: int, dtype: torch.dtype, seed: int = 0) -> Dict[str, object]:
    """Rows with -inf at NON-target columns (V >= 3), as a masked vocabulary produces them:
      low      -inf at columns 0 and min(5, V - 2) and the last column below 256 (a thread's FIRST column: it meets -inf with m = -inf)
      stride   -inf on the whole first 256-column stride (V > 256), and a row with -inf on the whole second stride (V > 512)
      late     -inf only at columns >= 256 (V > 257)
      single   -inf everywhere but one column, the target
    Every row keeps at least one finite column; the target is finite."""
    assert V >= 3
    g = torch.Generator().manual_seed(77 + seed + V)
    rows, tg, kinds = [], [], []

    def base():
        return (torch.rand(V, generator=g, dtype=F64) * 2 - 1) * 6

    r = base()
    r[[0, min(5, V - 2), min(255, V - 2)]] = -math.inf
    rows.append(r), tg.append(V - 1), kinds.append("low")
    if V > 256:
        r = base()
        r[:256] = -math.inf
        rows.append(r), tg.append(256), kinds.append("stride")
    if V > 512:
        r = base()
        r[256:512] = -math.inf
        rows.append(r), tg.append(3), kinds.append("stride")
    if V > 257:
        r = base()
        r[256::3] = -math.inf
        rows.append(r), tg.append(1), kinds.append("late")
    for keep in sorted({0, V // 2, V - 1}):
        r = torch.full((V,), -math.inf, dtype=F64)
        r[keep] = float(base()[0])
        rows.append(r), tg.append(keep), kinds.append("single")
    logits = torch.stack(rows).to(dtype)
    grow = (torch.rand(len(rows), generator=g, dtype=F64) + 0.5).to(F32)
    return {"logits": logits, "targets": torch.tensor(tg, dtype=torch.int64), "grow": grow, "kinds": kinds, "V": V}


# ------------------------------------------------------------------------------------------------------------ truth
def truth(logits: torch.Tensor, targets: torch.Tensor, grow: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """fp64 from the stored logits: lse, loss (0 for ignored rows), valid, the forward tolerances, and with `grow` the gradient."""
    x = logits.to(F64)
    rows, V = x.shape
    lse = torch.logsumexp(x, -1)
    valid = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(valid, lse - xt, torch.zeros((), dtype=F64))
    fin = torch.isfinite(x)
    hi = torch.where(fin, x, torch.full_like(x, -math.inf)).amax(-1)
    lo = torch.where(fin, x, torch.full_like(x, math.inf)).amin(-1)
    tol_lse = ulp32(lse) + ((hi - lo) + V / 256 + 12) * U24
    tol_loss = tol_lse + ulp32(torch.maximum(lse.abs(), xt.abs()))
    out = {"lse": lse, "loss": loss, "valid": valid, "tol_lse": tol_lse, "tol_loss": tol_loss}
    if grow is not None:
        p = torch.exp(x - lse[:, None])
        onehot = torch.zeros_like(x).scatter_(1, targets.clamp(0, V - 1)[:, None], 1.0)
        gg = torch.where(valid, grow.to(F64), torch.zeros((), dtype=F64))[:, None]   # NaN of an ignored row never enters
        out["p"] = p
        out["grad"] = torch.where(valid[:, None], gg * (p - onehot), torch.zeros((), dtype=F64))
    return out


# ------------------------------------------------------------------------------------------------------------ gates
def fwd_gate(loss: torch.Tensor, lse: torch.Tensor, logits: torch.Tensor, targets: torch.Tensor) -> dict:
    """-> {'ok', 'lse_worst': max |err| / tolerance, 'loss_worst', 'lse_err_max', 'lse_tol_min', 'ignored_exact'}."""
    t = truth(logits, targets)
    loss, lse = loss.to(F64).cpu(), lse.to(F64).cpu()
    e_lse = (lse - t["lse"]).abs()
    e_loss = (loss - t["loss"]).abs()
    r_lse = torch.where(torch.isfinite(lse), e_lse / t["tol_lse"], torch.full_like(e_lse, math.inf))
    r_loss = torch.where(torch.isfinite(loss), e_loss / t["tol_loss"], torch.full_like(e_loss, math.inf))
    r_loss = torch.where(t["valid"], r_loss, torch.zeros_like(r_loss))
    ignored_exact = bool((loss[~t["valid"]] == 0).all())
    worst = int(r_lse.argmax())
    return {"ok": bool(r_lse.max() <= 1) and bool(r_loss.max() <= 1) and ignored_exact, "lse_worst": r_lse.max().item(),
            "loss_worst": r_loss.max().item(), "lse_err": e_lse[worst].item(), "lse_tol": t["tol_lse"][worst].item(),
            "ignored_exact": ignored_exact}


def bwd_gate(d: torch.Tensor, logits: torch.Tensor, targets: torch.Tensor, grow: torch.Tensor) -> dict:
    """Every element of the gradient `d` (the dtype of the logits) computed from a forward lse that met fwd_gate."""
    t = truth(logits, targets, grow)
    x, got = logits.to(F64), d.to(F64).cpu()
    g = torch.where(t["valid"], grow.to(F64), torch.zeros((), dtype=F64)).abs()[:, None]
    p, tr = t["p"], t["grad"]
    dist = torch.where(torch.isfinite(x), (x - t["lse"][:, None]).abs(), torch.zeros_like(x))
    tol = g * p * torch.expm1(t["tol_lse"])[:, None] + g * (dist + 3) * U24 * p + ulp32(tr) * (tr != 0) + g * 2.0 ** -126
    tol = torch.where(torch.isfinite(x), tol, torch.zeros_like(tol))          # -inf column: exactly 0
    if logits.dtype == BF:
        lo, hi = (tr - tol).to(BF).to(F64), (tr + tol).to(BF).to(F64)
    else:
        lo, hi = tr - tol, tr + tol
    bad = ~((got >= lo) & (got <= hi))                                          # a NaN is bad
    ignored_exact = bool((got[~t["valid"]] == 0).all())
    excess = torch.where(bad, torch.maximum(lo - got, got - hi), torch.zeros_like(got))
    return {"ok": not bool(bad.any()) and ignored_exact, "n_bad": int(bad.sum()), "ignored_exact": ignored_exact,
            "worst_excess": excess.nan_to_num(nan=math.inf).max().item(),
            "err_over_tol": ((got - tr).abs() / tol.clamp_min(1e-300))[tol > 0].nan_to_num(nan=math.inf).max().item() if bool((tol > 0).any()) else 0.0}


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate_fwd(logits: torch.Tensor, targets: torch.Tensor, skip_neg_inf: bool = True):
    """The kernel's loop on the CPU in fp32 (torch.exp / torch.log for __expf / logf): 256 threads with an online max / sum over
    their strides, a butterfly over the 64 lanes of each wave, then the four waves in order.  -> (loss, lse) fp32.
    skip_neg_inf False is the loop before the fix: a -inf element met while m is still -inf computes exp(-inf - -inf)."""
    x = logits.to(F32)
    rows, V = x.shape
    steps = (V + 255) // 256
    ninf = torch.tensor(-math.inf)
    pad = torch.full((rows, steps * 256), math.nan)
    pad[:, :V] = x
    pad = pad.view(rows, steps, 256)
    live = (torch.arange(steps * 256) < V).view(steps, 256)
    m = torch.full((rows, 256), -math.inf)
    s = torch.zeros((rows, 256))
    for k in range(steps):
        v, on = pad[:, k], live[k][None]
        gt = v > m
        s_gt = s * torch.exp(m - v) + 1
        if skip_neg_inf:
            s_le = torch.where(v != ninf, s + torch.exp(v - m), s)
        else:
            s_le = s + torch.exp(v - m)
        s = torch.where(on, torch.where(gt, s_gt, s_le), s)
        m = torch.where(on & gt, v, m)
    m4, s4 = m.view(rows, 4, 64), s.view(rows, 4, 64)
    wm = m4.amax(-1, keepdim=True)
    part = torch.where(m4 == ninf, torch.zeros(()), s4 * torch.exp(m4 - wm))
    o = 32
    while o:                                                   # __shfl_xor butterfly: every lane ends with the same sum
        part = part + part[..., torch.arange(64) ^ o]
        o >>= 1
    ws, wm = part[..., 0], wm[..., 0]
    M = wm.amax(-1)
    S = torch.zeros(rows)
    for w in range(4):
        S = S + torch.where(wm[:, w] == ninf, torch.zeros(()), ws[:, w] * torch.exp(wm[:, w] - M))
    lse = M + torch.log(S)
    valid = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    return torch.where(valid, lse - xt, torch.zeros(())), lse


def emulate_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, grow: torch.Tensor) -> torch.Tensor:
    """The backward kernel's arithmetic on the CPU in fp32, stored in the dtype of the logits."""
    x = logits.to(F32)
    V = x.size(1)
    valid = (targets >= 0) & (targets < V)
    onehot = torch.zeros_like(x).scatter_(1, targets.clamp(0, V - 1)[:, None], 1.0)
    g = torch.where(valid, grow.to(F32), torch.zeros(()))[:, None]
    d = g * (torch.exp(x - lse.to(F32)[:, None]) - onehot)
    return torch.where(valid[:, None], d, torch.zeros(())).to(logits.dtype)


# ------------------------------------------------------------------------------------------------------------ mutants
FWD_MUTANTS = ("drop_last_stride", "next_row_first_col", "target+1", "ignored_not_zeroed", "no_max_sub")
BWD_MUTANTS = ("lse_next_row", "target+1", "ignored_not_zeroed", "drop_last_stride")


def mutant_fwd(logits: torch.Tensor, targets: torch.Tensor, name: str):
    """(loss, lse) fp32 of a deliberately wrong forward, computed in fp64 apart from the bug itself."""
    x = logits.to(F64)
    rows, V = x.shape
    valid = (targets >= 0) & (targets < V)
    tg = targets.clamp(0, V - 1)
    if name == "drop_last_stride":                   # the partial stride of a ragged V never read
        keep = V - V % 256 if V % 256 and V > 256 else V - 1
        lse = torch.logsumexp(x[:, :keep], -1)
    elif name == "next_row_first_col":               # V + 1 columns read from the flat buffer
        flat = torch.cat([x.reshape(-1), x[0, :1]])
        nxt = flat[(torch.arange(rows) + 1) * V]
        lse = torch.logsumexp(torch.cat([x, nxt[:, None]], 1), -1)
    elif name == "no_max_sub":                       # exp(x) summed in fp32 as it stands
        lse = torch.log(torch.exp(x.to(F32)).sum(-1)).to(F64)
    else:
        lse = torch.logsumexp(x, -1)
    if name == "target+1":
        tg = (tg + 1) % V
    loss = lse - x.gather(1, tg[:, None])[:, 0]
    if name != "ignored_not_zeroed":
        loss = torch.where(valid, loss, torch.zeros((), dtype=F64))
    return loss.to(F32), lse.to(F32)


def mutant_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, grow: torch.Tensor, name: str) -> torch.Tensor:
    x = logits.to(F64)
    rows, V = x.shape
    valid = (targets >= 0) & (targets < V)
    tg = targets.clamp(0, V - 1)
    l = lse.to(F64)
    if name == "lse_next_row":
        l = torch.roll(l, -1)
    if name == "target+1":
        tg = (tg + 1) % V
    onehot = torch.zeros_like(x).scatter_(1, tg[:, None], 1.0)
    g = grow.to(F64).nan_to_num(nan=1.0)[:, None]
    d = g * (torch.exp(x - l[:, None]) - onehot)
    if name == "drop_last_stride":
        d[:, V - V % 256 if V % 256 and V > 256 else V - 1:] = 0
    if name != "ignored_not_zeroed":
        d = torch.where(valid[:, None], d, torch.zeros((), dtype=F64))
    return d.to(logits.dtype)
