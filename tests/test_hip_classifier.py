"""GPU tests of the four kernels of csrc/classifier.hip — im2col3, col2im3, pool_head, pool_head_bwd — one by one against the
references of tests/classifier_reference.py (bits where the arithmetic has one order, exact-integer cases and fp64 error bands
where it has not), and of the whole NoiseMaskClassifier, forward and backward, eval and train mode, against fp64 autograd at the
sequence lengths where the edge tokens carry most of every gradient.  tests/test_classifier_reference.py shows what the gates reject.
Every case has at most 32 tokens (one sequence of 43 at pool 20, T = 2 pool + 3)."""
import pytest
import torch

import classifier_reference as R
from conftest import record_parity
from classifier_reference import EXACT, IM2COL_SHAPES, MODULE_CASES, RAGGED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, I16 = torch.bfloat16, torch.int16
POISON = 0x7B5B                       # a large finite bf16 (~1.1e36)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("B,T,C", IM2COL_SHAPES)
def test_im2col3_bits(B, T, C):
    """Bit for bit, relu 0 and 1, at the packed ld, the minimum 3C + 8 and a larger one, written into a poisoned buffer between
    two canary rows: every pad column zero, column 3C = 1.0, nothing outside the B*T rows touched."""
    from dualhyp_amd import _lib, ops
    xb = R.random_bf16_bits((B, T, C), gen(B * 100 + T))
    x = xb.view(BF).to(DEV)
    for ld in sorted({R.pack_ld(C), 3 * C + 8, 3 * C + 200}):
        for relu in (0, 1):
            buf = torch.full((B * T + 2, ld), POISON, dtype=I16, device=DEV)
            out = buf[1:-1]
            assert out.is_contiguous() and out.data_ptr() % 16 == 0
            _lib.check(_lib.load().dh_im2col3_bf16(x.data_ptr(), out.data_ptr(), B, T, C, ld, relu, ops._stream()))
            got = buf.cpu()
            assert bool((got[0] == POISON).all()) and bool((got[-1] == POISON).all()), f"canary rows written (ld {ld}, relu {relu})"
            want = R.im2col3_ref(xb, ld, bool(relu))
            assert bool((want[:, 3 * C] == 0x3F80).all()) and bool((want[:, 3 * C + 1:] == 0).all())
            bad = (got[1:-1] != want).nonzero()
            assert bad.numel() == 0, f"ld {ld} relu {relu}: {bad.size(0)} elements differ, first at {bad[0].tolist()}"
            # the public wrapper gives the same matrix
            assert torch.equal(ops.im2col3(x, ld, relu=bool(relu)).cpu().view(I16), want)


@pytest.mark.parametrize("C", [8, 264, 1024])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_col2im3_bits(T, C):
    """The fixed fp32 order restated in torch, bit for bit: no gate, `pre` only, `pre` and mask; ld > 3C with poisoned pad columns."""
    from dualhyp_amd import ops
    B, ld = 3, 3 * C + 16
    inp = R.col2im3_inputs(B, T, C, ld, gen(T * 10 + C))
    dcol = inp["dcol"].to(DEV)
    for pre, mask in ((None, None), (inp["pre"], None), (inp["pre"], inp["mask"])):
        got = ops.col2im3(dcol, B, T, C, pre=None if pre is None else pre.to(DEV), mask=None if mask is None else mask.to(DEV)).cpu()
        want = R.col2im3_ref(inp["dcol"], B, T, C, pre, mask)
        bad = (R.bits(got) != R.bits(want)).nonzero()
        assert bad.numel() == 0, f"pre {pre is not None} mask {mask is not None}: {bad.size(0)} of {got.numel()} differ, first {bad[0].tolist()}"
        if pre is not None:
            assert bool((got[~(pre.float() > 0)] == 0).all()), "+0, -0 and negative pre-activations gate the gradient to 0"


def _head(B, T, H, pool, seed, exact):
    from dualhyp_amd import ops
    inp = R.head_inputs(B, T, H, pool, gen(seed), exact=exact)
    h, w = inp["h"].to(DEV), inp["w"].to(DEV)
    logits = ops.pool_head(h, w, inp["bias"].to(DEV), pool).cpu()
    dh, pooled = ops.pool_head_bwd(h, w, inp["dl"].to(DEV), pool)
    ref = R.pool_head_ref(inp["h"], inp["w"], inp["bias"], pool, exact=exact)
    bw = R.pool_head_bwd_ref(inp["h"], inp["w"], inp["dl"], pool, exact=exact)
    assert logits.shape == ref["logits"].shape
    bad = (R.bits(pooled.cpu()) != R.bits(bw["pooled"])).nonzero()
    assert bad.numel() == 0, f"pooled means: {bad.size(0)} of {pooled.numel()} differ in bits, first {bad[0].tolist()}"
    lg, dg = R.band_gate(logits, ref["logits"], ref["E"]), R.band_gate(dh.cpu(), bw["dh"], bw["E"])
    assert lg["ok"], ("logits", lg)
    assert dg["ok"], ("dh", dg)
    assert bool((dh.cpu()[~bw["gate"]] == 0).all()) and bool((dh.cpu()[bw["gate"] & (bw["dh"] != 0)] != 0).all()), "the dh gate is h > 0"


@pytest.mark.parametrize("B,T,H,pool", EXACT)
def test_pool_head_exact(B, T, H, pool):
    """Integer operands, power-of-two windows: every product and partial sum is exact in any order, values must be equal."""
    _head(B, T, H, pool, 10 + EXACT.index((B, T, H, pool)), exact=True)


@pytest.mark.parametrize("B,T,H,pool", RAGGED)
def test_pool_head_ragged(B, T, H, pool):
    """Ceil-mode tails (T = 1, pool - 1, pool + 1, 2 pool + 3), H = 64, 256, 320: bit-exact pooled means, logits and dh the bf16
    rounding of a value inside the fp32 error band around fp64."""
    _head(B, T, H, pool, 30 + RAGGED.index((B, T, H, pool)), exact=False)


def _run_module(case, train: bool):
    from dualhyp_amd.relprompt import NoiseMaskClassifier
    B, T, C, H, pool = case
    inp = R.module_inputs(B, T, C, H, pool, seed=sum(case))
    m = NoiseMaskClassifier(C, hidden_dim=H, dropout=0.1, pool_size=pool)
    m.load_state_dict({k: inp[k] for k in R.PARAMS})
    m = m.to(DEV).train(train)
    x = inp["x"].to(DEV)
    keep = None
    torch.manual_seed(1234)
    logits = m(x)
    if train:                                             # the draw _ClassifierFn made: same seed, same shape, same device
        torch.manual_seed(1234)
        keep = (torch.rand((B, T, H), device=DEV) >= 0.1).cpu()
        assert 0 < int((~keep).sum()) < keep.numel() // 4
    assert logits.dtype == BF and logits.shape == inp["dlogits"].shape
    logits.backward(inp["dlogits"].to(DEV))
    got = {"logits": logits.detach().float().cpu()}
    got.update({k: p.grad.float().cpu() for k, p in m.named_parameters()})
    truth = R.module_truth(inp, pool, keep, 0.1)
    yard = R.module_yardstick(inp, pool, keep, 0.1)
    res = R.module_gate(got, truth, yard)
    tag = "B{}_T{}_C{}_H{}{}".format(B, T, C, H, "_train" if train else "")
    for k, r in res.items():
        print(f"[{tag}] {k}: max {r['max']:.3e} yard {r['max_yard']:.3e} ratio {r['max_ratio']:.3f} mean ratio {r['mean_ratio']:.3f} "
              f"worst row excess {r['worst_row_excess']:.2e} ok {r['ok']}")
    record_parity(f"classifier_edges.{tag}", **{f"{k}.max_ratio": r["max_ratio"] for k, r in res.items()},
                  **{f"{k}.mean_ratio": r["mean_ratio"] for k, r in res.items()})
    bad = {k: r for k, r in res.items() if not r["ok"]}
    assert not bad, bad


@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: "B{}-T{}-C{}-H{}-pool{}".format(*c))
def test_module_edge_shapes(case):
    """NoiseMaskClassifier forward + backward (eval) against fp64 autograd: logits and all six gradients, every element, per output
    row within 1.5x the bf16 yardstick's distance."""
    _run_module(case, train=False)


def test_module_train_mode_dropout():
    """Train mode, p = 0.1: relu(h1) * mask into im2col3 and col2im3(pre=h1, mask=mask), the mask recovered by re-seeding."""
    _run_module((2, 11, 8, 64, 10), train=True)
    _run_module((2, 3, 1024, 256, 10), train=True)
