"""Element-wise GPU tests of the fine-tune backward kernels against fp64, at the lengths and shapes the fine-tune runs.

Attention backward (ops.attn_bwd): every dq row (token, head) and every dK / dV row (key, group) against fp64 truth, gated
against the bf16 yardstick of tests/bwd_reference.py (max e_row <= 1.5x, mean <= 1.25x, every row within 1.5x its own
yardstick figure + 2^-7), on one packed batch of 14 lengths around the 32-token tiles up to 1 025, every dispatch variant
(query heads per group 1-8, hs 64 / 128, fewer than 8 (group, sequence) pairs, the A/B kernels of tunings 27 / 29), and the
bench's 32 x 560 window.  The rmsnorm / SwiGLU / rope
backward kernels against fp64 in bf16 ulps, the token contractions against an fp32 error bound.  tests/test_bwd_gates.py
shows on the CPU that the gates reject the bugs they are meant to catch."""

import pytest
import torch

import bwd_reference as R
from conftest import record_parity, ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LENS = [1, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 559, 560, 1025]
HEADS = [(64, 32, 4), (64, 4, 2), (64, 6, 2), (64, 12, 2), (64, 4, 4), (128, 32, 8), (128, 16, 2), (128, 2, 2)]
A_B = [(0, 0), (0, 1), (1, 0)]       # (tuning 27, tuning 29): the round-2/3 dq kernel, the per-wave dkdv kernel, both


def _lib():
    from dualhyp_amd import _lib
    return _lib.load()


def _attn_bwd(inp, plan=None):
    from dualhyp_amd import ops
    d = {k: inp[k].to(DEV) for k in ("q", "k", "v", "y", "dout", "lse", "q_start", "q_len")}
    lens = inp["lens"]
    return ops.attn_bwd(d["q"], d["k"], d["v"], d["y"], d["dout"], d["lse"], d["q_start"], d["q_len"], max(lens), lens=lens,
                        plan=plan)


def _attn_bwd_ab(inp):
    """-> {(t27, t29): (dq, dk, dv)} for the default and every A/B path."""
    lib = _lib()
    out = {(1, 1): _attn_bwd(inp)}
    try:
        for t27, t29 in A_B:
            lib.dh_set_tuning(27, t27)
            lib.dh_set_tuning(29, t29)
            out[(t27, t29)] = _attn_bwd(inp)
    finally:
        lib.dh_set_tuning(27, 1)
        lib.dh_set_tuning(29, 1)
    return out


def _gate_attention(key, got, inp, seqs=None):
    """got = packed (dq, dk, dv) on the GPU; the fp64 gate over the sequences `seqs` (all by default)."""
    truth = R.attn_bwd_ref(inp, seqs)
    yard = R.attn_bwd_ref(inp, seqs, which="yardstick")
    g = [tuple(x[t0:t0 + n].cpu() for x in got) for _, t0, n, _ in truth]
    for x in got:
        assert not torch.isnan(x).any().item(), f"{key}: NaN"
    res = R.gate_grads(g, [r for *_, r in truth], [r for *_, r in yard])
    figs = {}
    for name, r in res.items():
        figs.update({f"{name}_max_ratio": r["max_ratio"], f"{name}_mean_ratio": r["mean_ratio"], f"{name}_max": r["max"],
                     f"{name}_max_yard": r["max_yard"], f"{name}_worst_row_excess": r["worst_row_excess"]})
    record_parity(key, **figs)
    bad = {name: r for name, r in res.items() if not r["ok"]}
    assert not bad, f"{key}: per-row gate failed against the bf16 yardstick: {bad}"


@pytest.mark.parametrize("hs,n_head,n_groups", HEADS)
def test_attention_bwd_per_row_against_fp64(hs, n_head, n_groups):
    """One packed batch of LENS: per-row gate on every sequence; every A/B path the same bits as the default."""
    inp = R.attn_inputs(LENS, n_head, n_groups, hs, seed=hs + 7 * n_head + n_groups)
    outs = _attn_bwd_ab(inp)
    base = outs[(1, 1)]
    for ab, o in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(o, base)), f"tunings (27, 29) = {ab} changed the bits"
    _gate_attention(f"train_bwd_attn_hs{hs}_{n_head}x{n_groups}", base, inp)


@pytest.mark.parametrize("hs,n_head,n_groups,n", [(64, 32, 4, 1025), (128, 4, 4, 300)])
def test_attention_bwd_single_sequence(hs, n_head, n_groups, n):
    """Fewer than 8 (group, sequence) pairs: the dK / dV kernel's other grid (the unpacked micro-step: 4 groups x 1 sequence)."""
    inp = R.attn_inputs([n], n_head, n_groups, hs, seed=n)
    outs = _attn_bwd_ab(inp)
    for ab, o in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(o, outs[(1, 1)])), f"tunings (27, 29) = {ab} changed the bits"
    _gate_attention(f"train_bwd_attn_single_hs{hs}_{n_head}x{n_groups}_n{n}", outs[(1, 1)], inp)


def test_attention_bwd_bench_window():
    """32 x 560 packed with one shared attn_bwd_plan, as the training step calls it: every sequence's dq / dk / dv the bits
    of that sequence alone; the fp64 gate on sequences 0, 17 and 31."""
    from dualhyp_amd import ops
    B, T, hs, H, G = 32, 560, 64, 32, 4
    inp = R.attn_inputs([T] * B, H, G, hs, seed=560)
    q_start, q_len = inp["q_start"].to(DEV), inp["q_len"].to(DEV)
    plan = ops.attn_bwd_plan(q_start, q_len, B * T, [T] * B)
    got = _attn_bwd(inp, plan=plan)
    for i in range(B):
        sl = slice(i * T, (i + 1) * T)
        one = {k: inp[k][sl] for k in ("q", "k", "v", "y", "dout", "lse")}
        one.update(lens=[T], q_start=torch.zeros(1, dtype=torch.int32), q_len=torch.tensor([T], dtype=torch.int32))
        alone = _attn_bwd(one)
        assert all(torch.equal(a[sl], b) for a, b in zip(got, alone)), f"sequence {i}: packed != alone"
    _gate_attention("train_bwd_attn_bench_32x560", got, inp, seqs=[0, 17, 31])


@pytest.mark.parametrize("hs", [64, 128])
def test_rowdot_dsum_against_fp64(hs):
    """dh_rowdot_f32 (the softmax backward's D = rowsum(dO * y)) within fp32 rounding of the fp64 dot."""
    from dualhyp_amd import ops
    g = torch.Generator().manual_seed(hs)
    rows = 3 * 1025 + 7
    a, b = R.bf16_uniform((rows, hs), 1.0, g), R.bf16_uniform((rows, hs), 3.0, g)
    ad, bd = a.to(DEV), b.to(DEV)
    out = torch.empty(rows, dtype=torch.float32, device=DEV)
    ops.check(_lib().dh_rowdot_f32(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, hs, torch.cuda.current_stream().cuda_stream))
    want = (a.double() * b.double()).sum(-1)
    bound = hs * 2.0 ** -24 * (a.double() * b.double()).abs().sum(-1)
    err = (out.cpu().double() - want).abs()
    assert (err <= bound).all(), f"max err / bound {(err / bound).max().item():.3g}"


# ---------------------------------------------------------------------------------------------------- element-wise kernels
RMS_D = [8, 256, 512, 520, 2048, 2056, 4096, 4104, 8192]       # MAXC 1, 4, 8, 16 and the first width past each


@pytest.mark.parametrize("d", RMS_D)
def test_rmsnorm_bwd_against_fp64(d):
    """Row rms from 1e-3 (eps = 1e-5 matters) to 1e3, w with negative entries, with and without dres; row counts around
    the kernel's 4 rows per block."""
    from dualhyp_amd import ops
    g = torch.Generator().manual_seed(d)
    rows, eps = 4483, 1e-5
    scale = torch.logspace(-3, 3, rows, dtype=torch.float64)[torch.randperm(rows, generator=g)]
    x = (R.bf16_uniform((rows, d), 1.7, g).double() * scale[:, None]).to(R.BF)
    w, dy, dres = R.bf16_uniform((d,), 1.5, g), R.bf16_uniform((rows, d), 1.0, g), R.bf16_uniform((rows, d), 0.5, g)
    xd, wd, dyd, dresd = x.to(DEV), w.to(DEV), dy.to(DEV), dres.to(DEV)
    worst = 0.0
    for use_res in (False, True):
        truth = R.rmsnorm_bwd64(dy, x, w, eps, dres if use_res else None)
        for r in (1, 3, 4, 5, rows):
            got = ops.rmsnorm_bwd(dyd[:r], xd[:r], wd, eps, dres=dresd[:r] if use_res else None).cpu()
            res = R.rmsnorm_gate(got, truth[:r])
            worst = max(worst, res["ulp_max"])
            assert res["ok"], f"d={d} rows={r} dres={use_res}: {res}"
    record_parity(f"train_bwd_rmsnorm_d{d}", ulp_max=worst)


def test_rmsnorm_bwd_refuses_a_row_past_8192():
    from dualhyp_amd import ops, _lib as L
    x = torch.zeros((2, 8200), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.DualHypHipError):
        ops.rmsnorm_bwd(x, x, torch.ones(8200, dtype=torch.bfloat16, device=DEV), 1e-5)


@pytest.mark.parametrize("I,rows", [(384, 37), (5632, 21), (14336, 9)])
def test_swiglu_bwd_against_fp64(I, rows):
    """g across [-30, 30], and in the last row single elements at +-88, +-100 and +-1e4: finite, <= 2 ulp of fp64 (at a
    floor of 1/64 of the row's rms) with silu(g) rounded as the forward rounds it."""
    from dualhyp_amd import ops
    gen = torch.Generator().manual_seed(I)
    g = R.bf16_uniform((rows, I), 30.0, gen)
    cols = torch.randperm(I, generator=gen)[:6]
    g[-1, cols] = torch.tensor([88.0, -88.0, 100.0, -100.0, 1e4, -1e4], dtype=R.BF)
    u, dact = R.bf16_uniform((rows, I), 2.0, gen), R.bf16_uniform((rows, I), 1.0, gen)
    got = ops.swiglu_bwd(dact.to(DEV), g.to(DEV), u.to(DEV)).cpu()
    assert torch.isfinite(got.float()).all()
    want = R.swiglu_bwd64(dact, g, u)
    u_dg, u_du = R.ulp_rows(got[:, :I], want[:, :I]), R.ulp_rows(got[:, I:], want[:, I:])
    record_parity(f"train_bwd_swiglu_I{I}", dg_ulp_max=u_dg.max().item(), du_ulp_max=u_du.max().item())
    assert u_dg.max().item() <= 2 and u_du.max().item() <= 2, (u_dg.max().item(), u_du.max().item())


ROPE_HEADS = sorted({(hs, h, g) for hs, h, g in HEADS} | {(128, 8, 2)})


@pytest.mark.parametrize("hs,n_head,n_groups", ROPE_HEADS)
def test_qkv_rope_bwd_against_fp64(hs, n_head, n_groups):
    """Positions up to 2047, packed sequences restarting at 0: <= 1 ulp of fp64 on the bf16 table; v columns bit copies."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    gen = torch.Generator().manual_seed(n_head * hs + n_groups)
    lens = [2048, 700, 1, 33]
    n_tok = sum(lens)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens])
    cos, sin = O.build_rope_cache(2048, hs)
    dq = R.bf16_uniform((n_tok, n_head, hs), 1.0, gen)
    dk, dv = R.bf16_uniform((n_tok, n_groups, hs), 2.0, gen), R.bf16_uniform((n_tok, n_groups, hs), 1.0, gen)
    got = ops.qkv_rope_bwd(dq.to(DEV), dk.to(DEV), dv.to(DEV), cos.to(DEV), sin.to(DEV), pos.to(DEV)).cpu()
    want = R.rope_bwd64(dq, dk, dv, cos, sin, pos, n_groups)
    qpk = n_head // n_groups
    g5, w5 = got.view(n_tok, n_groups, qpk + 2, hs), want.view(n_tok, n_groups, qpk + 2, hs)
    assert torch.equal(g5[:, :, qpk + 1], dv)
    u = ulp_diff(g5[:, :, :qpk + 1], w5[:, :, :qpk + 1])
    record_parity(f"train_bwd_rope_hs{hs}_{n_head}x{n_groups}", ulp_max=u.max().item())
    assert u.max().item() <= 1, u.max().item()


@pytest.mark.parametrize("T", [1024, 1025, 17920, 17921])
def test_tn_accum_against_fp64(T):
    """out (+)= scale * a^T b over T tokens (one pass, and split over the grid past 1 024 tokens), the small dimension 16 or 48
    on either side, accumulate on and off, and the three-segment form: per element within 8 sqrt(T) 2^-24 sum |a b|."""
    from dualhyp_amd import ops
    gen = torch.Generator().manual_seed(T)
    L, scale = 2048, 0.375
    big, small = R.bf16_uniform((T, L), 1.0, gen), R.bf16_uniform((T, 64), 1.0, gen)
    bigd, smalld = big.to(DEV), small.to(DEV)
    ref = big.double().T @ small.double()                           # [L, 64]
    bound = R.tn_bound(big, small, scale)
    worst = 0.0
    for S, c0 in ((16, 16), (48, 0)):
        for m_large in (True, False):
            want0 = scale * ref[:, c0:c0 + S]
            bnd = bound[:, c0:c0 + S]
            if not m_large:
                want0, bnd = want0.T, bnd.T
            a, b = (bigd, smalld[:, c0:c0 + S]) if m_large else (smalld[:, c0:c0 + S], bigd)
            for acc in (False, True):
                init = R.bf16_uniform(want0.shape, 4.0, gen).float()
                out = init.to(DEV)
                ops.tn_accum(a, b, out, scale=scale, accumulate=acc)
                want = want0 + (init.double() if acc else 0)
                err = (out.cpu().double() - want).abs()
                lim = bnd + 2.0 ** -24 * want.abs()
                worst = max(worst, (err / lim).max().item())
                assert (err <= lim).all(), f"T={T} S={S} m_large={m_large} accumulate={acc}: err / bound {(err / lim).max().item():.3g}"
    # three segments of a fused QKV projection's output gradient in one launch
    s0, s1, qd = 384, 512, 640
    out = torch.zeros((qd, 16), dtype=torch.float32, device=DEV)
    ops.tn_accum(bigd[:, :qd], smalld[:, :48], out, scale=scale, accumulate=False, splits=(s0, s1))
    bounds = (0, s0, s1, qd)
    want = torch.cat([scale * ref[bounds[i]:bounds[i + 1], 16 * i:16 * i + 16] for i in range(3)])
    lim = torch.cat([bound[bounds[i]:bounds[i + 1], 16 * i:16 * i + 16] for i in range(3)])
    err = (out.cpu().double() - want).abs()
    worst = max(worst, (err / lim).max().item())
    assert (err <= lim).all(), f"T={T} segmented: err / bound {(err / lim).max().item():.3g}"
    record_parity(f"train_bwd_tn_accum_T{T}", err_over_bound_max=worst)
