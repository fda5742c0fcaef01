"""The gates of tests/test_hip_classifier.py have teeth (CPU only): mutants of the references — each one a bug the kernels of
csrc/classifier.hip could plausibly have — are rejected, while the truth rounded to bf16 and the bf16 yardstick pass.  The
references themselves are checked against torch's own unfold / avg_pool1d / autograd."""

import pytest
import torch

import classifier_reference as R
from gemm_exact_reference import InexactCase

F64, BF = torch.float64, torch.bfloat16
IM2COL_SHAPES, EXACT, RAGGED, MODULE_CASES = R.IM2COL_SHAPES, R.EXACT, R.RAGGED, R.MODULE_CASES


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ im2col3
def test_im2col_reference_is_unfold():
    for B, T, C in IM2COL_SHAPES[:4]:
        xb = R.random_bf16_bits((B, T, C), gen(1))
        ld = R.pack_ld(C)
        out = R.im2col3_ref(xb, ld, relu=False).view(B, T, ld)
        x = xb.view(BF).double()
        unf = torch.nn.functional.unfold(x.transpose(1, 2)[..., None], (3, 1), padding=(1, 0))          # [B, C*3, T], channel-major
        want = unf.view(B, C, 3, T).permute(0, 3, 2, 1).reshape(B, T, 3 * C)
        assert torch.equal(out[..., :3 * C].view(BF).double(), want)
        assert bool((out[..., 3 * C] == 0x3F80).all()) and bool((out[..., 3 * C + 1:] == 0).all())
        relu = R.im2col3_ref(xb, ld, relu=True).view(B, T, ld)[..., :3 * C]
        assert torch.equal(relu.view(BF).double(), want.clamp_min(0)) and not bool((relu < 0).any()), "relu leaves no sign bit, -0.0 included"


@pytest.mark.parametrize("mutant,relu", [("cross_batch", False), ("reversed_taps", False), ("relu_keeps_neg_zero", True)])
def test_im2col_mutant_is_caught(mutant, relu):
    caught = 0
    for B, T, C in IM2COL_SHAPES:
        xb = R.random_bf16_bits((B, T, C), gen(2))
        same = torch.equal(R.im2col3_ref(xb, R.pack_ld(C), relu), R.im2col3_ref(xb, R.pack_ld(C), relu, mutant=mutant))
        if (mutant == "cross_batch" and B == 1) or (mutant == "reversed_taps" and T == 1):
            assert same                                    # the shapes at which the bug cannot show
        else:
            assert not same, (mutant, B, T, C)
            caught += 1
    assert caught >= 4


# ------------------------------------------------------------------------------------------------------------ col2im3
def test_col2im_reference_is_the_adjoint_of_im2col():
    """<im2col(x), dcol> == <x, col2im(dcol)> on integer data (exact in fp32 and bf16)."""
    B, T, C = 3, 5, 8
    g = gen(3)
    x = torch.randint(-3, 4, (B, T, C), generator=g).to(BF)
    ld = 3 * C + 8
    dcol = torch.randint(-3, 4, (B * T, ld), generator=g).to(BF)
    col = R.im2col3_ref(R.bits(x), ld, relu=False).view(BF).double()
    dx = R.col2im3_ref(dcol, B, T, C).double()
    assert (col[:, :3 * C] * dcol.double()[:, :3 * C]).sum().item() == (x.double() * dx).sum().item()


@pytest.mark.parametrize("mutant", ["shift", "pre_ge", "no_mask"])
def test_col2im_mutant_is_caught(mutant):
    for T in (1, 2, 5):
        for C in (8, 264):
            inp = R.col2im3_inputs(3, T, C, 3 * C + 16, gen(4))
            good = R.col2im3_ref(inp["dcol"], 3, T, C, inp["pre"], inp["mask"])
            assert bool(torch.isfinite(good.float()).all()) and good.float().abs().max().item() < 1e4, "pad poison must not show"
            bad = R.col2im3_ref(inp["dcol"], 3, T, C, inp["pre"], inp["mask"], mutant=mutant)
            if mutant == "shift" and T == 1:
                assert torch.equal(R.bits(good), R.bits(bad))
            else:
                assert not torch.equal(R.bits(good), R.bits(bad)), (mutant, T, C)
    # a shifted tap changes EVERY element that has more than one tap in range (the taps' magnitudes differ by 16x)
    inp = R.col2im3_inputs(3, 5, 8, 40, gen(5))
    a, b = R.col2im3_ref(inp["dcol"], 3, 5, 8).float(), R.col2im3_ref(inp["dcol"], 3, 5, 8, mutant="shift").float()
    assert bool((a != b).all())


# ------------------------------------------------------------------------------------------------------------ pooling head
@pytest.mark.parametrize("pool", [10, 20])
def test_pooled_reference_is_avg_pool_ceil_mode(pool):
    for T in (1, pool - 1, pool, pool + 1, 2 * pool + 3):
        inp = R.head_inputs(2, T, 64, pool, gen(6), exact=False)
        want = torch.nn.functional.avg_pool1d(torch.relu(inp["h"].double()).transpose(1, 2), pool, ceil_mode=True).transpose(1, 2)
        got = R.pooled_ref(inp["h"], pool).double().view(2, -1, 64)
        assert got.shape == want.shape and (got - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item()
        ref = R.pool_head_ref(inp["h"], inp["w"], inp["bias"], pool, exact=False)
        full = want @ inp["w"].double().T + inp["bias"].double()
        assert (ref["logits"] - full).abs().max().item() <= 2.0 ** -8 * (want.abs() @ inp["w"].double().abs().T).max().item()
        # dh against autograd of the same head
        h = inp["h"].double().requires_grad_()
        lg = torch.nn.functional.avg_pool1d(torch.relu(h).transpose(1, 2), pool, ceil_mode=True).transpose(1, 2) @ inp["w"].double().T
        lg.backward(inp["dl"].double())
        b = R.pool_head_bwd_ref(inp["h"], inp["w"], inp["dl"], pool, exact=False)
        assert (b["dh"] - h.grad).abs().max().item() <= 1e-12
        assert bool((b["E"] <= 2.0 ** -19 * b["dh"].abs().max()).all())


def test_exact_cases_are_exact_and_inexact_ones_are_refused():
    for i, (B, T, H, pool) in enumerate(EXACT):
        inp = R.head_inputs(B, T, H, pool, gen(10 + i), exact=True)
        ref = R.pool_head_ref(inp["h"], inp["w"], inp["bias"], pool, exact=True)
        assert torch.equal(ref["logits"].to(BF).double(), ref["logits"]) and float(ref["E"].abs().max()) == 0
        b = R.pool_head_bwd_ref(inp["h"], inp["w"], inp["dl"], pool, exact=True)
        assert torch.equal(b["dh"].to(BF).double(), b["dh"])
        assert R.band_gate(ref["logits"].to(BF), ref["logits"], ref["E"])["ok"]
    inp = R.head_inputs(2, 10, 64, 10, gen(6), exact=False)
    with pytest.raises(InexactCase):
        R.pool_head_ref(inp["h"], inp["w"], inp["bias"], 10, exact=True)
    with pytest.raises(InexactCase):
        R.pool_head_ref(inp["h"], inp["w"], (inp["bias"].double() * 64).to(BF), 10, exact=False)


HEAD_MUTANTS = ["tail_div_pool", "floor_mode", "relu_after_mean", "dh_no_len"]


@pytest.mark.parametrize("mutant", HEAD_MUTANTS)
def test_head_mutant_is_caught(mutant):
    """Every mutant fails the bit gate on the pooled means, the band gate on the logits or the band gate on dh, at each ragged shape
    at which it differs at all; the truth rounded to bf16 and an fp32 evaluation pass."""
    caught = 0
    for i, (B, T, H, pool) in enumerate(RAGGED):
        inp = R.head_inputs(B, T, H, pool, gen(30 + i), exact=False)
        ref = R.pool_head_ref(inp["h"], inp["w"], inp["bias"], pool, exact=False)
        bw = R.pool_head_bwd_ref(inp["h"], inp["w"], inp["dl"], pool, exact=False)
        assert R.band_gate(ref["logits"].to(BF), ref["logits"], ref["E"])["ok"]
        assert R.band_gate(bw["dh"].to(BF), bw["dh"], bw["E"])["ok"]
        m32 = R.pooled_ref(inp["h"], pool).float()
        l32 = (m32 @ inp["w"].float().T + inp["bias"].float()).to(BF)
        assert R.band_gate(l32.view(ref["logits"].shape), ref["logits"], ref["E"])["ok"], "an fp32 evaluation must pass"
        differs = (mutant in ("tail_div_pool", "floor_mode") and T % pool != 0) or mutant == "relu_after_mean" or \
                  (mutant == "dh_no_len" and T > 1)
        bad_l = R.pool_head_ref(inp["h"], inp["w"], inp["bias"], pool, exact=False, mutant=mutant)
        bad_b = R.pool_head_bwd_ref(inp["h"], inp["w"], inp["dl"], pool, exact=False, mutant=mutant)
        ok_pooled = torch.equal(R.bits(bad_b["pooled"]), R.bits(bw["pooled"]))
        ok_logits = R.band_gate(bad_l["logits"].to(BF), ref["logits"], ref["E"])["ok"]
        ok_dh = R.band_gate(bad_b["dh"].to(BF), bw["dh"], bw["E"])["ok"]
        if mutant == "dh_no_len":
            assert ok_dh == (not differs), (mutant, B, T, H, pool)
        elif mutant == "relu_after_mean":
            assert not ok_pooled and not ok_logits or T == 1, (mutant, T, H, pool)
        else:
            assert (ok_pooled and ok_logits and ok_dh) == (not differs), (mutant, T, H, pool, ok_pooled, ok_logits, ok_dh)
            if differs:
                assert not ok_pooled and not ok_logits and not ok_dh, (mutant, T, H, pool, ok_pooled, ok_logits, ok_dh)
        caught += differs
    assert caught >= 6


def test_dh_gate_is_strictly_positive():
    h = torch.tensor([[[0.0], [-0.0], [-1.0], [2.0 ** -133], [1.0]]], dtype=BF).expand(1, 5, 8).contiguous()
    b = R.pool_head_bwd_ref(h, torch.ones((3, 8), dtype=BF), torch.ones((1, 1, 3)), 8, exact=False)
    assert b["gate"][0, :, 0].tolist() == [False, False, False, True, True]
    assert b["dh"][0, :, 0].tolist() == [0, 0, 0, 0.6, 0.6] and b["E"][0, :3, 0].abs().max().item() == 0


# ------------------------------------------------------------------------------------------------------------ whole module
@pytest.fixture(scope="module")
def module_refs():
    cache = {}

    def get(case):
        if case not in cache:
            B, T, C, H, pool = case
            inp = R.module_inputs(B, T, C, H, pool, seed=sum(case))
            cache[case] = (inp, R.module_truth(inp, pool), R.module_yardstick(inp, pool))
        return cache[case]
    return get


def test_yardstick_formulas_are_the_module():
    """With its roundings switched off the closed-form forward and backward of the yardstick are fp64 autograd of the torch module,
    dropout mask included."""
    for case in MODULE_CASES[:5]:
        B, T, C, H, pool = case
        inp = R.module_inputs(B, T, C, H, pool, seed=3)
        for keep in (None, torch.rand((B, T, H), generator=gen(4)) >= 0.1):
            tr, ya = R.module_truth(inp, pool, keep, 0.1), R.module_yardstick(inp, pool, keep, 0.1, rounded=False)
            for k in tr:
                assert (tr[k] - ya[k]).abs().max().item() <= 1e-12 * max(tr[k].abs().max().item(), 1.0), (case, k)
    # and the torch module itself gives the truth's logits
    from dualhyp_amd.relprompt import NoiseMaskClassifier
    B, T, C, H, pool = MODULE_CASES[3]
    inp = R.module_inputs(B, T, C, H, pool, seed=3)
    m = torch.nn.Module()
    m.conv1, m.conv2, m.classifier = torch.nn.Conv1d(C, H, 3, padding=1), torch.nn.Conv1d(H, H, 3, padding=1), torch.nn.Linear(H, 3)
    m.load_state_dict({k: inp[k] for k in R.PARAMS})
    assert set(dict(NoiseMaskClassifier(C, hidden_dim=H, pool_size=pool).named_parameters())) == set(R.PARAMS)
    m = m.double()
    y = torch.relu(m.conv2(torch.relu(m.conv1(inp["x"].double().transpose(1, 2)))))
    lg = m.classifier(torch.nn.functional.avg_pool1d(y, pool, ceil_mode=True).transpose(1, 2))
    assert (lg - R.module_truth(inp, pool)["logits"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: "B{}-T{}-C{}-H{}-pool{}".format(*c))
def test_module_gate_passes_bf16_candidates(module_refs, case):
    inp, truth, yard = module_refs(case)
    B, T, C, H, pool = case
    res = R.module_gate(yard, truth, yard)
    assert all(r["ok"] for r in res.values()), res
    # the truth, its logits rounded to bf16 as the path stores them (the path's parameter gradients are fp32 sums over the tokens:
    # at these sizes the yardstick's distance can be below one bf16 rounding of the gradient itself, so that is no candidate)
    rounded = {k: R.rnd(v) if k == "logits" else v for k, v in truth.items()}
    res = R.module_gate(rounded, truth, yard)
    assert all(r["ok"] for r in res.values()), {k: r for k, r in res.items() if not r["ok"]}
    # an independent bf16 evaluation: the same rounding points with fp32 accumulation, as the kernels
    y32 = R.module_yardstick(inp, pool, acc=torch.float32)
    res = R.module_gate(y32, truth, yard)
    assert all(r["ok"] for r in res.values()), {k: r for k, r in res.items() if not r["ok"]}
    # the yardstick is a bf16 computation, not the truth
    assert R.module_gate(yard, truth, yard)["conv1.weight"]["max_yard"] > 2.0 ** -12


@pytest.mark.parametrize("mutant", ["conv_cross_batch", "floor_mode", "tail_div_pool"])
def test_module_mutant_is_caught(module_refs, mutant):
    caught = 0
    for case in MODULE_CASES:
        B, T, C, H, pool = case
        differs = B > 1 if mutant == "conv_cross_batch" else T % pool != 0
        if not differs:
            continue
        inp, truth, yard = module_refs(case)
        bad = R.module_truth(inp, pool, mutant=mutant)
        res = R.module_gate(bad, truth, yard)
        assert not all(r["ok"] for r in res.values()), (mutant, case)
        caught += 1
    assert caught >= 4


def test_train_mode_truth_applies_the_mask():
    B, T, C, H, pool = 2, 11, 8, 64, 10
    inp = R.module_inputs(B, T, C, H, pool, seed=8)
    keep = torch.rand((B, T, H), generator=gen(9)) >= 0.1
    tr, ya = R.module_truth(inp, pool, keep, 0.1), R.module_yardstick(inp, pool, keep, 0.1)
    assert all(r["ok"] for r in R.module_gate(ya, tr, ya).values())
    assert all(r["ok"] for r in R.module_gate(R.module_yardstick(inp, pool, keep, 0.1, acc=torch.float32), tr, ya).values())
    no_mask = R.module_truth(inp, pool)                                   # the dropped mask, whole-module version
    assert not all(r["ok"] for r in R.module_gate(no_mask, tr, ya).values())
    unscaled = R.module_truth(inp, pool, keep, 0.0)                       # the mask without its 1 / (1 - p)
    assert not all(r["ok"] for r in R.module_gate(unscaled, tr, ya).values())
    assert R.drop_scale(0.1) == 1.109375
