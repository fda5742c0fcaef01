"""fp64 references and element-wise gates for the fine-tune backward kernels (tests/test_hip_train_bwd.py), and the
bf16 yardstick the attention gate is measured against.  CPU only: tests/test_bwd_gates.py runs the same gates on fp64
mutants of the truth to show that they catch the bugs they are meant to catch.

Attention backward, per sequence of n tokens, head h of group g = h // qpk, scale = 1/sqrt(hs):
    S = scale * q k^T (causal) ; P = exp(S - lse) ; dP = dO v^T ; D = rowsum(dO * y) ; dS = P * (dP - D)
    dq = scale * dS k ; dk_g = scale * sum_h dS^T q ; dv_g = sum_h P^T dO
truth     : fp64 from the bf16 q / k / v / dO (y and lse recomputed in fp64, nothing rounded)
yardstick : what a correct bf16 kernel computes — fp32 products from the bf16 inputs, the bf16 y and the fp32 lse, P and dS
            rounded to bf16 where they become operands of the dV / dK / dQ products, the results rounded to bf16 once
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from conftest import bf16_ulp

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def rnd_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).to(x.dtype)


def bf16_uniform(shape, bound: float, gen: torch.Generator) -> torch.Tensor:
    return ((torch.rand(shape, generator=gen, dtype=F64) * 2 - 1) * bound).to(BF)


# ---------------------------------------------------------------------------------------------------- attention
def attn_inputs(lens: Sequence[int], n_head: int, n_groups: int, hs: int, seed: int = 0, qk_bound: float = 2.0) -> Dict[str, torch.Tensor]:
    """Packed [n_tok, H | G, hs] bf16 q, k, v, dO; y = bf16 of the fp64 causal GQA attention, lse = fp32 of its fp64
    log-sum-exp (natural log of sum exp(scale * q.k)); q_start / q_len as the training step builds them."""
    g = torch.Generator().manual_seed(seed)
    n_tok = sum(lens)
    q = bf16_uniform((n_tok, n_head, hs), qk_bound, g)
    k = bf16_uniform((n_tok, n_groups, hs), qk_bound, g)
    v = bf16_uniform((n_tok, n_groups, hs), 1.0, g)
    dout = bf16_uniform((n_tok, n_head, hs), 1.0, g)
    y = torch.empty((n_tok, n_head, hs), dtype=BF)
    lse = torch.empty((n_tok, n_head), dtype=F32)
    for t0, n in _spans(lens):
        yy, ll = attn_fwd64(q[t0:t0 + n], k[t0:t0 + n], v[t0:t0 + n])
        y[t0:t0 + n], lse[t0:t0 + n] = yy.to(BF), ll.to(F32)
    i32 = torch.int32
    return {"q": q, "k": k, "v": v, "dout": dout, "y": y, "lse": lse, "lens": list(lens),
            "q_start": torch.tensor([t0 for t0, _ in _spans(lens)], dtype=i32), "q_len": torch.tensor(list(lens), dtype=i32)}


def _spans(lens):
    t0 = 0
    for n in lens:
        yield t0, n
        t0 += n


def _heads(x: torch.Tensor, qpk: int) -> torch.Tensor:
    """[n, G, hs] -> [H, n, hs] (each group's row repeated for its qpk query heads)."""
    return x.permute(1, 0, 2).repeat_interleave(qpk, dim=0)


def attn_fwd64(q, k, v):
    """-> (y [n, H, hs], lse [n, H]) in fp64 of one sequence."""
    n, H, hs = q.shape
    qpk = H // k.size(1)
    qh, kh, vh = q.permute(1, 0, 2).to(F64), _heads(k, qpk).to(F64), _heads(v, qpk).to(F64)
    s = (qh @ kh.transpose(1, 2)) / math.sqrt(hs)
    s = s.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool)), -math.inf)
    lse = torch.logsumexp(s, -1)
    y = torch.exp(s - lse[..., None]) @ vh
    return y.permute(1, 0, 2), lse.T


def attn_bwd_seq(q, k, v, dout, y=None, lse=None, *, dtype=F64, rounded: bool = False, mutant: Optional[str] = None):
    """(dq [n, H, hs], dk [n, G, hs], dv [n, G, hs]) of one sequence in closed form.
    dtype F64, rounded False, y / lse None: the truth (y, lse recomputed in fp64).
    dtype F32, rounded True, the bf16 y and fp32 lse: the bf16 yardstick (results returned in fp64, bf16-valued).
    mutant: a deliberately wrong backward (the gates must reject it; tests/test_bwd_gates.py):
      'mask+1'  the causal mask shifted by one (key <= q + 1)     'mask-1'  (key <= q - 1)
      'drop_last_key'  the last key never attended                 'dv_scaled' / 'dk_unscaled'  1/sqrt(hs) on dV / not on dK
      'lse_next_head'  the log-sum-exp of the neighbouring head
      'dk_first4'  a group's dK summed over its first 4 query heads only"""
    n, H, hs = q.shape
    G = k.size(1)
    qpk = H // G
    scale = 1.0 / math.sqrt(hs)
    if y is None or lse is None:
        y64, lse64 = attn_fwd64(q, k, v)
        y = y64 if y is None else y
        lse = lse64 if lse is None else lse
    if mutant == "lse_next_head":
        lse = torch.roll(lse, -1, dims=1)
    cast = (lambda t: t.to(dtype))
    rb = rnd_bf16 if rounded else (lambda t: t)
    qh, doh = cast(q.permute(1, 0, 2)), cast(dout.permute(1, 0, 2))
    kh, vh = cast(_heads(k, qpk)), cast(_heads(v, qpk))
    yh, lh = cast(y.permute(1, 0, 2)), cast(lse.T)
    s = (qh @ kh.transpose(1, 2)) * scale
    iq = torch.arange(n)[:, None]
    ik = torch.arange(n)[None, :]
    shift = {"mask+1": 1, "mask-1": -1}.get(mutant, 0)
    allow = ik <= iq + shift
    if mutant == "drop_last_key":
        allow = allow & (ik < n - 1)
    p = torch.where(allow, torch.exp(s - lh[..., None]), torch.zeros((), dtype=dtype))
    dp = doh @ vh.transpose(1, 2)
    dd = (doh * yh).sum(-1)
    ds = p * (dp - dd[..., None])
    pb, dsb = rb(p), rb(ds)
    dq = (dsb @ kh) * scale
    dv_h = pb.transpose(1, 2) @ doh
    dk_h = dsb.transpose(1, 2) @ qh
    dv = dv_h.view(G, qpk, n, hs).sum(1)
    if mutant == "dk_first4":
        dk = dk_h.view(G, qpk, n, hs)[:, :4].sum(1)
    else:
        dk = dk_h.view(G, qpk, n, hs).sum(1)
    dk = dk * (1.0 if mutant == "dk_unscaled" else scale)
    if mutant == "dv_scaled":
        dv = dv * scale
    out = [dq.permute(1, 0, 2), dk.permute(1, 0, 2), dv.permute(1, 0, 2)]
    return tuple(rb(o).to(F64) for o in out)


def zero_final_partial_tile(dk: torch.Tensor, dv: torch.Tensor, n: int):
    """Mutant: dK / dV of the keys of a sequence's final partial 32-key tile zeroed (nothing if n % 32 == 0)."""
    dk, dv = dk.clone(), dv.clone()
    t0 = n // 32 * 32
    if t0 < n:
        dk[t0:n] = 0
        dv[t0:n] = 0
    return dk, dv


def attn_bwd_ref(inp: Dict[str, torch.Tensor], seqs: Optional[Sequence[int]] = None, which: str = "truth", max_elems: int = 1 << 25):
    """Per-sequence (dq, dk, dv) of the packed batch `inp` (attn_inputs): which = 'truth' | 'yardstick'.
    -> list of (seq index, t0, n, (dq, dk, dv)) for the sequences `seqs` (all by default).  Groups are taken a few at a
    time so that no n x n score tensor holds more than `max_elems` values."""
    out = []
    spans = list(_spans(inp["lens"]))
    H, G = inp["q"].size(1), inp["k"].size(1)
    qpk = H // G
    for i in (range(len(spans)) if seqs is None else seqs):
        t0, n = spans[i]
        sl = slice(t0, t0 + n)
        step = max(1, min(G, max_elems // max(1, qpk * n * n)))
        parts = []
        for g0 in range(0, G, step):
            g1 = min(G, g0 + step)
            hq = slice(g0 * qpk, g1 * qpk)
            args = (inp["q"][sl, hq], inp["k"][sl, g0:g1], inp["v"][sl, g0:g1], inp["dout"][sl, hq])
            if which == "truth":
                parts.append(attn_bwd_seq(*args))
            else:
                parts.append(attn_bwd_seq(*args, inp["y"][sl, hq], inp["lse"][sl, hq], dtype=F32, rounded=True))
        out.append((i, t0, n, tuple(torch.cat([p[j] for p in parts], 1) for j in range(3))))
    return out


# ---------------------------------------------------------------------------------------------------- per-row gate
ROW_FLOOR = 2.0 ** -10     # rows whose max |truth| is below this fraction of the tensor's max are measured against it


def row_errors(got: torch.Tensor, truth: torch.Tensor, floor: float) -> torch.Tensor:
    """e_row = max |got - truth|_row / max(max |truth|_row, floor) for every row (token, head) of [n, heads, hs] tensors
    -> [n * heads].  NaN anywhere in a row of `got` gives that row an infinite error."""
    got, truth = got.to(F64).reshape(-1, got.size(-1)), truth.to(F64).reshape(-1, truth.size(-1))
    err = (got - truth).abs().amax(-1)
    err = torch.where(torch.isnan(got).any(-1), torch.full_like(err, math.inf), err)
    return err / truth.abs().amax(-1).clamp_min(floor)


MAX_RATIO, MEAN_RATIO = 1.5, 1.25
ROW_SLACK = 2.0 ** -7      # every row: e_row <= MAX_RATIO x the yardstick's e_row of the SAME row + this


def attn_gate(e_got: torch.Tensor, e_yard: torch.Tensor, max_ratio: float = MAX_RATIO, mean_ratio: float = MEAN_RATIO,
              row_slack: float = ROW_SLACK) -> dict:
    """The per-row gate of a candidate against the bf16 yardstick (e_row of the same rows): max e_row within max_ratio x the
    yardstick's, mean within mean_ratio x, and no single row above max_ratio x its own yardstick figure + row_slack (the pooled
    max alone is set by the rows whose truth nearly cancels, where the bf16 y's error dominates: a few wrong rows elsewhere would
    hide under it).  -> figures with 'ok'."""
    mg, my = e_got.max().item(), e_yard.max().item()
    ag, ay = e_got.mean().item(), e_yard.mean().item()
    worst_row = (e_got - max_ratio * e_yard).max().item()
    ok = math.isfinite(mg) and mg <= max_ratio * my and ag <= mean_ratio * ay and worst_row <= row_slack
    return {"ok": ok, "max": mg, "max_yard": my, "max_ratio": mg / my if my > 0 else math.inf,
            "mean": ag, "mean_yard": ay, "mean_ratio": ag / ay if ay > 0 else math.inf, "worst_row_excess": worst_row}


def gate_grads(got: Sequence[Sequence[torch.Tensor]], truth: Sequence[Sequence[torch.Tensor]],
               yard: Sequence[Sequence[torch.Tensor]]) -> Dict[str, dict]:
    """got / truth / yard: per sequence (dq, dk, dv).  Rows of all sequences are pooled per gradient; the floor of a row's
    denominator is ROW_FLOOR x the gradient's max |truth| over all of them."""
    res = {}
    for j, name in enumerate(("dq", "dk", "dv")):
        floor = ROW_FLOOR * max(t[j].abs().max().item() for t in truth)
        eg = torch.cat([row_errors(g[j], t[j], floor) for g, t in zip(got, truth)])
        ey = torch.cat([row_errors(y[j], t[j], floor) for y, t in zip(yard, truth)])
        res[name] = attn_gate(eg, ey)
    return res


# ---------------------------------------------------------------------------------------------------- element-wise
def ulp_rows(got: torch.Tensor, truth: torch.Tensor, floor_frac: float = 1.0 / 64) -> torch.Tensor:
    """|got - truth| in bf16 ulps at max(|got|, |truth|, floor_frac * rms of the truth's ROW) (rows = last dim)."""
    a, b = got.to(F64), truth.to(F64)
    floor = floor_frac * b.pow(2).mean(-1, keepdim=True).sqrt().clamp_min(1e-300)
    big = torch.maximum(torch.maximum(a.abs(), b.abs()), floor.expand_as(b))
    return (a - b).abs() / bf16_ulp(big).to(F64)


def rmsnorm_bwd64(dy, x, w, eps: float, dres=None, mutant: Optional[str] = None) -> torch.Tensor:
    """y = w * x * r, r = (mean(x^2) + eps)^-1/2:  dx = r * (w dy) - x * r^3 * mean(x * w dy)  (+ dres), fp64.
    mutant 'no_mean': the second term dropped."""
    x, g = x.to(F64), dy.to(F64) * w.to(F64)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    dx = r * g
    if mutant != "no_mean":
        dx = dx - x * r ** 3 * (x * g).mean(-1, keepdim=True)
    return dx + (dres.to(F64) if dres is not None else 0)


def rmsnorm_bwd32(dy, x, w, eps: float, dres=None) -> torch.Tensor:
    """The kernel's arithmetic on the CPU: fp32, the result rounded to bf16 once (the yardstick of the rmsnorm gate)."""
    x, g = x.float(), dy.float() * w.float()
    r = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.size(-1) + eps)
    k = r * r * r * (x * g).sum(-1, keepdim=True) / x.size(-1)
    return (r * g - k * x + (dres.float() if dres is not None else 0)).to(BF).to(F64)


RMSNORM_ULP = 1.0


def rmsnorm_gate(got, truth) -> dict:
    u = ulp_rows(got, truth)
    return {"ok": bool(torch.isfinite(got.to(F64)).all()) and u.max().item() <= RMSNORM_ULP, "ulp_max": u.max().item()}


def swiglu_bwd64(dact, g, u) -> torch.Tensor:
    """[dg | du] in fp64 with silu(g) rounded to bf16 where the forward rounds it (act = bf16(silu(g)) * u)."""
    gg, d, uu = g.to(F64), dact.to(F64), u.to(F64)
    sig = torch.sigmoid(gg)
    dg = d * uu * (sig * (1 + gg * (1 - sig)))
    du = d * rnd_bf16(gg * sig)
    return torch.cat([dg, du], -1)


def rope_bwd64(dq, dk, dv, cos, sin, pos, n_groups: int) -> torch.Tensor:
    """dx1 = dy1 c1 + dy2 s2 ; dx2 = dy2 c2 - dy1 s1 (fp64 on the bf16 table) in the fused [n_tok, G, qpk + 2, hs] layout."""
    n_tok, H, hs = dq.shape
    qpk, half = H // n_groups, hs // 2
    c, s = cos.to(F64)[pos.long()][:, None], sin.to(F64)[pos.long()][:, None]

    def rot(t):
        t = t.to(F64)
        y1, y2 = t[..., :half], t[..., half:]
        return torch.cat([y1 * c[..., :half] + y2 * s[..., half:], y2 * c[..., half:] - y1 * s[..., :half]], -1)
    out = torch.cat([rot(dq).view(n_tok, n_groups, qpk, hs), rot(dk)[:, :, None], dv.to(F64)[:, :, None]], 2)
    return out.reshape(n_tok, -1)


def tn_bound(a: torch.Tensor, b: torch.Tensor, scale: float) -> torch.Tensor:
    """Per-element error bound of an fp32 token contraction of T products: 8 sqrt(T) 2^-24 |scale| sum_t |a_ti b_tj|."""
    T = a.size(0)
    return 8 * math.sqrt(T) * 2.0 ** -24 * abs(scale) * (a.to(F64).abs().T @ b.to(F64).abs())
