"""Host tests of tests/dropout_reference.py: the Philox4x32-10 restatement against the published known-answer vectors, the
threshold and scale at their edges, and the SENSITIVITY of the model-level dropout tests (test_hip_dropout_grads.py) — measured on
the oracle alone, so the claim that those tests would see a wrong mask in the backward is asserted here and not just made.

Sensitivity, measured with the Philox masks (seed 1234, step 1; the worst LoRA tensor's movement in units of its own gate
max(1.3 * e_oracle_bf16, 0.02), fp32 oracle):

    mutation                                            tiny_r4 (B 2, T 64)   hs128_r16 (B 2, T 37)
    worst gate                                                0.0220                0.0200
    site 1 / 2 / 3 mask ignored on the dx path only     15.7 / 11.5 / 19.9 x   15.5 / 14.6 / 27.8 x
    no masks at all                                           55.3 x                57.0 x
    the two sites of layer 0 / layer 1 swapped            60.0 / 54.4 x         57.5 / 50.1 x
    the masks of step - 1                                     66.6 x                65.6 x
    n1 for n1d in lora_A's gradient, layer 0 / 1          34.1 / 22.1 x         35.2 / 21.0 x

Site 0's input gradient feeds only the frozen embedding: a backward that ignored site 0's mask on that path computes the same LoRA
gradients, so there is no such mutation to see (asserted below: it moves nothing)."""
import numpy as np
import pytest
import torch

import dropout_reference as R

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    """The three Random123 known-answer vectors of philox4x32-10 (kat_vectors), scalar and vectorised."""
    for ctr, key, want in KAT:
        assert R.philox4x32_10_scalar(ctr, key) == want
        assert tuple(int(v) for v in R.philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == want
    got = R.philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint64), np.array([k[1] for k in KAT], dtype=np.uint64))
    assert got.shape == (3, 4) and [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]


def test_vectorised_philox_is_the_scalar_one():
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(64, 2), dtype=np.uint64)
    ctr[0], key[0] = 0xffffffff, 0xffffffff          # every product and key bump wraps
    got = R.philox4x32_10(ctr, key)
    for i in range(64):
        assert tuple(int(v) for v in got[i]) == R.philox4x32_10_scalar(ctr[i].tolist(), key[i].tolist()), i
    one = R.philox4x32_10(ctr, key[5])               # one key for all counters
    assert tuple(int(v) for v in one[9]) == R.philox4x32_10_scalar(ctr[9].tolist(), key[5].tolist())


def test_draws_follow_the_element_layout():
    """draws() against the definition written out per element: chunk, half, lane; key mixing that wraps; a step above 2^32."""
    for seed, cid, step in ((1337, 3, 0), (2 ** 63 - 1, 0xffffffff, 2 ** 32 + 5), ((7 << 32) | 9, 43, None)):
        d = R.draws(40, seed, cid, step)
        for i in (0, 3, 4, 7, 8, 13, 39):
            want = R.philox4x32_10_scalar(R.counter_words(i, step or 0), R.key_words(seed, cid))[i % 4]
            assert int(d[i]) == want, (seed, cid, step, i)
    assert R.key_words(2 ** 63 - 1, 0xffffffff) == (0xffffffff ^ ((0xffffffff * 0x9E3779B9) & 0xffffffff), (0x7fffffff + 0xffffffff) & 0xffffffff)
    assert R.counter_words(8 * (2 ** 32 + 2) + 5, 2 ** 32 + 5) == (2, 3, 5, 1)          # hi32(c) * 2 + h


def test_threshold_and_scale():
    below_one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert R.thresh(0.0) == 0
    assert R.thresh(1e-10) == 0                                    # float(1e-10) * 2^32 = 0.43
    assert R.thresh(0.05) == 214748368                             # float(0.05) = 0.0500000007450580596923828125
    assert R.thresh(0.5) == 2 ** 31
    assert R.thresh(0.999) == int(float(np.float32(0.999)) * 2 ** 32) == 4290672384
    assert R.thresh(below_one) == 2 ** 32 - 256                    # (1 - 2^-24) * 2^32
    assert R.scale(0.05).item() == 1.0546875 and R.scale_bits(0.05) == 0x3F87
    assert R.scale(0.0).item() == 1.0 and R.scale(0.5).item() == 2.0 and R.scale(below_one).item() == 2.0 ** 24
    assert R.scale(0.999).item() == 1000.0                         # 2^24 / 16777 = 1000.013: bf16 steps by 4 there


def test_reference_dropout_values():
    x = torch.tensor([1.0, -0.0, torch.finfo(torch.bfloat16).max, float("inf"), float("nan"), 1e-40, -2.5, 0.0] * 4, dtype=torch.bfloat16)
    y, m = R.dropout(x, 0.05, 1337, 3, 0)
    keep = R.keep_mask(32, 0.05, 1337, 3, 0)
    assert keep.sum() > 24 and not keep.all()
    assert (m[keep] == 1.0546875).all() and (m[~keep].view(torch.int16) == 0).all() and (y[~keep].view(torch.int16) == 0).all()
    k = keep.view(4, 8)[:, 0]
    assert (y.view(4, 8)[k, 0] == 1.0546875).all()
    k = keep.view(4, 8)[:, 2]
    assert torch.isinf(y.view(4, 8)[k, 2]).all()                   # the largest finite bf16 overflows under the scale
    y0, m0 = R.dropout(x, 0.0, 1, 0, None)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(y0), nan) and torch.equal(y0[~nan].view(torch.int16), x[~nan].view(torch.int16)) and (m0 == 1).all()


def test_injected_dropout_hands_out_masks_in_order_and_restores_the_oracle():
    from oracle import ger_oracle as O
    real = O.F
    a, b = torch.ones(2, 3), torch.zeros(2, 3)
    with R.injected_dropout([a, b]):
        assert torch.equal(O.F.dropout(torch.full((2, 3), 5.0), 0.5, True), torch.full((2, 3), 5.0))
        assert torch.equal(O.F.dropout(torch.full((2, 3), 5.0), 0.5, True), torch.zeros(2, 3))
    assert O.F is real
    with pytest.raises(AssertionError, match="consumed"):
        with R.injected_dropout([a, b]):
            O.F.dropout(torch.ones(2, 3), 0.5, True)
    assert O.F is real
    with pytest.raises(AssertionError, match="mask"):
        with R.injected_dropout([a]):
            O.F.dropout(torch.ones(3, 2), 0.5, True)
    assert O.F is real


MUTATIONS = ["site1_dx", "site2_dx", "site3_dx", "no_masks", "swap_layer0", "swap_layer1", "step_minus_1", "a_unmasked_layer0",
             "a_unmasked_layer1"]


def _mutated(name, cfg, sd32, ids, labels, masks, seed, step):
    B, T = ids.shape
    d = cfg.n_embd
    kw = {}
    if name.endswith("_dx"):
        kw["ignore_dx"] = {int(name[4])}
    elif name == "no_masks":
        masks = [torch.ones_like(m) for m in masks]
    elif name.startswith("swap_layer"):
        l = int(name[-1])
        masks = list(masks)
        masks[2 * l], masks[2 * l + 1] = masks[2 * l + 1], masks[2 * l]
    elif name == "step_minus_1":
        masks = R.site_masks(len(masks), B * T, d, R.P_MODEL, seed, step - 1)
    elif name.startswith("a_unmasked_layer"):
        kw["a_grad_unmasked"] = {2 * int(name[-1])}
    return R.oracle_micro_step(cfg, sd32, ids, labels, masks, 4, **kw)[1]


@pytest.fixture(scope="module", params=list(R.SETTINGS))
def measured(request):
    """Per setting: the oracle's fp32 / bf16 gradients under the Philox masks and every mutation's movement in gate units."""
    key = request.param
    s = R.SETTINGS[key]
    cfg, sd = R.setting(key)
    ids, labels = R.batch(cfg, s["B"], s["T"], seed=2)
    seed, step = 1234, 1
    masks = R.site_masks(2 * cfg.n_layer, s["B"] * s["T"], cfg.n_embd, R.P_MODEL, seed, step)
    l32, g32, lbf, gbf = R.oracle_pair(cfg, sd, ids, labels, masks, 4)
    gate = R.gates(g32, gbf)
    sd32 = {k: v.float() for k, v in sd.items()}
    ratios = {}
    for name in MUTATIONS + ["site0_dx"]:
        dist = R.distances(_mutated(name, cfg, sd32, ids, labels, masks, seed, step), g32)
        ratios[name] = max(dist[k] / gate[k][1] for k in dist)
    print(f"[sensitivity] {key}: worst gate {max(g for _, g in gate.values()):.4f} " + " ".join(f"{k}={v:.1f}x" for k, v in ratios.items()))
    return key, gate, ratios


def test_gates_stay_near_two_percent(measured):
    """The yardstick is the oracle's own bf16 run: at these settings it stays close to the 2 % floor."""
    key, gate, _ = measured
    assert max(g for _, g in gate.values()) <= 0.03, (key, gate)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mask_mutation_moves_a_gradient_by_five_gates(measured, mutation):
    key, _, ratios = measured
    assert ratios[mutation] >= 5.0, f"{key}: {mutation} moves the worst LoRA gradient by only {ratios[mutation]:.2f}x its gate"


def test_site_zero_input_gradient_is_dead(measured):
    key, _, ratios = measured
    assert ratios["site0_dx"] == 0.0, (key, ratios["site0_dx"])
