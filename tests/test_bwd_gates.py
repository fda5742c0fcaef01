"""The gates of tests/test_hip_train_bwd.py have teeth (CPU only): fp64 mutants of the truth — each one a bug the fine-tune
backward kernels could plausibly have — fail the gate that the GPU tests apply, while the bf16 yardstick and the truth
rounded to bf16 pass it.  The closed-form fp64 truth is itself checked against fp64 autograd."""
import math

import pytest
import torch

import bwd_reference as R

LENS = [1, 33, 70, 560]          # a single token, partial final tiles of 1, 6 and 16 keys
HS, N_HEAD, N_GROUPS = 64, 12, 2  # 6 query heads per group


@pytest.fixture(scope="module")
def case():
    inp = R.attn_inputs(LENS, N_HEAD, N_GROUPS, HS, seed=5)
    truth = [r for *_, r in R.attn_bwd_ref(inp, which="truth")]
    yard = [r for *_, r in R.attn_bwd_ref(inp, which="yardstick")]
    return inp, truth, yard


def _per_seq(inp, **kw):
    out = []
    for i, n in enumerate(inp["lens"]):
        t0 = sum(inp["lens"][:i])
        sl = slice(t0, t0 + n)
        out.append(R.attn_bwd_seq(inp["q"][sl], inp["k"][sl], inp["v"][sl], inp["dout"][sl], **kw))
    return out


def test_closed_form_truth_is_fp64_autograd(case):
    inp, truth, _ = case
    F = torch.nn.functional
    for (i, n), (dq, dk, dv) in zip(enumerate(LENS), truth):
        t0 = sum(LENS[:i])
        q, k, v = (inp[x][t0:t0 + n].double().permute(1, 0, 2).requires_grad_() for x in ("q", "k", "v"))
        qpk = N_HEAD // N_GROUPS
        o = F.scaled_dot_product_attention(q[None], k.repeat_interleave(qpk, 0)[None], v.repeat_interleave(qpk, 0)[None],
                                           is_causal=True, scale=1 / math.sqrt(HS))[0]
        o.backward(inp["dout"][t0:t0 + n].double().permute(1, 0, 2))
        for got, want in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
            assert (got - want.permute(1, 0, 2)).abs().max().item() <= 1e-12 * want.abs().max().item() + 1e-300


def test_bf16_candidates_pass(case):
    inp, truth, yard = case
    rounded = [tuple(R.rnd_bf16(t) for t in r) for r in truth]
    for cand in (yard, rounded):
        res = R.gate_grads(cand, truth, yard)
        assert all(r["ok"] for r in res.values()), res
    # and the yardstick is a real bf16 computation, not the truth: its errors are well above fp64's
    res = R.gate_grads(yard, truth, yard)
    assert all(r["max_yard"] > 2.0 ** -10 for r in res.values()), res


MUTANTS = ["mask+1", "mask-1", "drop_last_key", "final_partial_tile", "dv_scaled", "dk_unscaled", "lse_next_head", "dk_first4",
           "dq_final_partial_tile"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_attention_mutant_is_caught(case, mutant):
    inp, truth, yard = case
    if mutant == "final_partial_tile":
        bad = []
        for n, (dq, dk, dv) in zip(LENS, truth):
            dk2, dv2 = R.zero_final_partial_tile(dk, dv, n)
            bad.append((dq, dk2, dv2))
    elif mutant == "dq_final_partial_tile":          # dq only, a few rows: under the pooled max, caught row by row
        bad = []
        for n, (dq, dk, dv) in zip(LENS, truth):
            dq2 = dq.clone()
            dq2[n // 32 * 32:] = 0
            bad.append((dq2, dk, dv))
    else:
        bad = _per_seq(inp, mutant=mutant)
    res = R.gate_grads(bad, truth, yard)
    assert not all(r["ok"] for r in res.values()), f"{mutant} passed the gate: {res}"
    print(f"[mutant caught] {mutant}: " + " ".join(f"{k} max_ratio={v['max_ratio']:.3g}" for k, v in res.items()))


def test_final_partial_tile_of_one_long_sequence_is_caught():
    """The case the global-max gate missed: n = 560, dK / dV of the last 16 keys (half the final 32-key tile) zeroed."""
    inp = R.attn_inputs([560], 8, 8, 64, seed=6, qk_bound=1.0)
    truth = [r for *_, r in R.attn_bwd_ref(inp)]
    yard = [r for *_, r in R.attn_bwd_ref(inp, which="yardstick")]
    dq, dk, dv = truth[0]
    dk2, dv2 = R.zero_final_partial_tile(dk, dv, 560)
    res = R.gate_grads([(dq, dk2, dv2)], truth, yard)
    assert not res["dk"]["ok"] and not res["dv"]["ok"], res
    assert R.gate_grads(yard, truth, yard)["dk"]["ok"]


def test_rmsnorm_gate_catches_a_missing_mean_term():
    g = torch.Generator().manual_seed(7)
    rows, d = 9, 520
    x = (R.bf16_uniform((rows, d), 1.0, g).double() * torch.logspace(-3, 3, rows, dtype=torch.float64)[:, None]).to(R.BF)
    w, dy = R.bf16_uniform((d,), 1.5, g), R.bf16_uniform((rows, d), 1.0, g)
    truth = R.rmsnorm_bwd64(dy, x, w, 1e-5)
    assert R.rmsnorm_gate(R.rmsnorm_bwd32(dy, x, w, 1e-5), truth)["ok"]
    bad = R.rmsnorm_bwd64(dy, x, w, 1e-5, mutant="no_mean").to(R.BF)
    res = R.rmsnorm_gate(bad, truth)
    assert not res["ok"], res
