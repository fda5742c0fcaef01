"""CPU checks of tests/norm_reference.py: the references against the oracle, the input builders' own conditions, and the
sensitivity of the acceptance that tests/test_hip_norm_exact.py applies on the GPU.  No kernel enters any of this."""
import pytest
import torch

import norm_reference as R
from oracle import ger_oracle as O


def torch_tail(rows: int) -> torch.Tensor:
    """The rows on which torch's CPU bf16 rsqrt takes its scalar tail loop: the last rows % W of the call, W the
    bf16 vector width of the build in use (32 with AVX-512, 16 with 256-bit vectors)."""
    W = 32 if torch.backends.cpu.get_cpu_capability() == "AVX512" else 16
    return (torch.arange(rows) >= rows // W * W).to(torch.uint8)


# ---- cross-checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.NORM_D)
def test_oracle_rmsnorm_is_a_candidate_row(d):
    """the oracle's bf16 rmsnorm (torch's own summation order) gives, for every realistic row, one of the two candidate rows"""
    c = R.NormCase(d, "real", R.REAL_ROWS, False, "none")
    o = R.norm_inputs(c)
    want = R.norm_want(o["x"], o["w"], R.EPS, torch_tail(c.rows), exact=False)
    bad = R.norm_accept(want, O.rmsnorm(o["x"], o["w"], R.EPS), c.id)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("d", (64, 2056, 4104))
def test_finish_reference_is_the_oracle_composition(d):
    """finish_rows + norm_rows against lora_linear, the residual add and rmsnorm of the oracle, on the factors of the grid inputs"""
    n = 0
    for c in R.finish_cases(d):
        if c.kind == "real" or c.in_place:
            continue
        o = R.finish_inputs(c)
        x1 = R.finish_rows(o["h32"], c.n_part, bool(c.pairs), d, o.get("b"), c.scale, o["x"])
        x1_o = o["x"] + O.lora_linear(o["att"], o["W"], o.get("A"), o.get("b"), c.scale)
        assert not R.same_rows(x1, x1_o, c.id), c.id
        ms, hi = R.ms_candidates(x1, d, 0)
        assert torch.equal(ms, hi)
        assert not R.same_rows(R.norm_rows(x1, o["w"], R.EPS, torch_tail(c.rows), ms), O.rmsnorm(x1_o, o["w"], R.EPS), c.id), c.id
        n += 1
    assert n >= 10


@pytest.mark.parametrize("d", (256, 2048, 8192))
def test_chain_bound_holds_for_the_wave_order(d):
    """The wave-per-row order on realistic rows: its relative error is inside D_CHAIN 2^-24 (it is a few 2^-24), every row's ms
    is one of its candidates, and the order-free bound d 2^-24 would leave many times as many rows undecided."""
    rows = 1000
    x = R.real_rows(f"probe{d}", rows, d)
    ss = R.emulate_ss(x).double()
    ss64 = R.squares64(x).sum(-1)
    rel = ((ss - ss64).abs() / ss64).max().item() / R.U24
    lo, hi = R.ms_candidates(x, d)
    ms = R.rb(R._div(ss.float(), d))
    flo, fhi = R.ms_candidates(x, d, d)
    print(f"d={d}: max relative error {rel:.2f} x 2^-24; undecided {(lo != hi).float().mean().item():.3%} with D={R.D_CHAIN}, "
          f"{(flo != fhi).float().mean().item():.3%} with D=d")
    assert rel <= R.D_CHAIN
    assert bool(((ms == lo) | (ms == hi)).all())
    assert (lo != hi).float().mean().item() <= 0.02


# ---- self-checks of the inputs ------------------------------------------------------------------------------------------------
def _share(und: torch.Tensor, what: str) -> None:
    share = und.float().mean().item()
    print(f"undecided {share:.3%} ({int(und.sum())} of {und.numel()}): {what}")
    assert und.numel() >= 256 and share <= 0.02, f"{what}: {share:.3%} of the rows are undecided"


@pytest.mark.parametrize("d", R.NORM_D)
def test_rmsnorm_inputs(d):
    """the builders' exactness checks (raised inside) and the undecided share of every realistic case"""
    for c in R.norm_cases(d):
        o = R.norm_inputs(c)
        want = R.norm_want(o["sum"], o["w"], R.EPS, R.tails(c.rows)[c.tail], c.kind != "real")
        if c.kind == "real":
            _share(want.undecided, c.id)
        if c.kind == "spike":
            col = o["sum"].float().abs().argmax(-1)
            assert col.tolist() == R.spike_positions(d)
    if d <= 2056:
        assert sorted(p // 8 for p in R.spike_positions(d)) == list(range(d // 8))
    assert {p % 8 for p in R.spike_positions(d)} == set(range(min(8, d // 8)))


@pytest.mark.parametrize("d", R.FINISH_D)
def test_finish_inputs(d):
    seen = set()
    for c in R.finish_cases(d):
        o = R.finish_inputs(c)
        _, want = R.finish_reference(c, o)
        if c.kind == "real":
            _share(want.undecided, c.id)
        else:
            assert float(o["h32"].abs().max()) > 0
        seen.add((c.n_part, c.pairs))
    assert seen == set(R.FINISH_PARTS)


@pytest.mark.parametrize("d", R.NQ_D)
def test_rmsnorm_quant_inputs(d):
    for c in R.norm_quant_cases(d):
        o = R.norm_quant_inputs(c)
        want = R.norm_want(o["x"], o["w"], R.EPS, R.tails(c.rows)[c.tail], c.kind != "real", quant=True)
        assert not bool((want.q[0] == 0x7F).any()) and not bool((want.q[0] == 0xFF).any())
        if c.kind == "real":
            _share(want.undecided, c.id)


@pytest.mark.parametrize("K", R.QUANT_K)
def test_quant_inputs(K):
    x = R.quant_inputs(K)
    q, s = R.quant_rows(x)
    assert not bool(((q & 0x7F) == 0x7F).any()), "an e4m3 NaN in the reference: the uint8 sentinel would be ambiguous"
    assert float(x[1].abs().max()) == 0 and s[1].item() == pytest.approx(1e-12 / 448, rel=1e-6)
    if K > 8:
        sub = (q[2] & 0x78) == 0                                   # exponent field 0: subnormal (or zero)
        assert int(sub.sum()) >= K // 2, "the subnormal row holds few e4m3 subnormals"
    sw = R.quant_sweep(K)
    assert sw.float().abs().argmax(-1).tolist() == R.spike_positions(K)


# ---- sensitivity: deliberately wrong restatements must be rejected ------------------------------------------------------------
def _norm_failures(d: int, defect):
    out = []
    for c in R.norm_cases(d):
        if c.resid:
            continue
        o = R.norm_inputs(c)
        tail = R.tails(c.rows)[c.tail]
        want = R.norm_want(o["x"], o["w"], R.EPS, tail, c.kind != "real")
        out += R.norm_accept(want, R.emulate_norm(o["x"], o["w"], R.EPS, tail, defect), c.id)
    return out


@pytest.mark.parametrize("d", (520, 4104))
def test_acceptance_takes_the_wave_order_and_rejects_norm_defects(d):
    ok = _norm_failures(d, None)
    assert not ok, "\n".join(ok)
    for defect in ("drop_last_chunk", "double_chunk", "divisor", "ignore_tail"):
        bad = _norm_failures(d, defect)
        print(f"d={d} {defect}: {len(bad)} lines, e.g. {bad[:1]}")
        assert bad, f"d={d}: the acceptance does not notice `{defect}`"


def _finish_failures(d: int, defect):
    out = []
    for c in R.finish_cases(d):
        o = R.finish_inputs(c)
        x1, _ = R.finish_reference(c, o)
        got = R.emulate_finish(o["h32"], c.n_part, bool(c.pairs), d, o.get("b"), c.scale, o["x"], defect)
        out += R.same_rows(got, x1, c.id + ": x_out")
    return out


def test_acceptance_rejects_finish_defects():
    d = 2056
    ok = _finish_failures(d, None)
    assert not ok, "\n".join(ok)
    for defect in ("pairs_in_sequence", "odd_partner_p0", "xa_previous_row"):
        bad = _finish_failures(d, defect)
        print(f"{defect}: {len(bad)} lines, e.g. {bad[:1]}")
        assert bad, f"the acceptance does not notice `{defect}`"


def test_acceptance_rejects_amax_without_the_last_chunk():
    K = 520
    x = R.quant_sweep(K)
    q_ref, s_ref = R.quant_rows(x)
    for defect, rejected in ((None, False), ("amax_without_last_chunk", True)):
        q, s = R.emulate_quant(x, defect)
        bad = R.same_rows(q, q_ref, "bytes") + R.same_rows(s.view(-1, 1), s_ref.view(-1, 1), "scale")
        assert bool(bad) == rejected, (defect, bad[:3])
    # fused with the norm: the spike row whose largest output sits in the last chunk
    c = R.NormQuantCase(2056, "spike", len(R.spike_positions(2056)), "none", True)
    o = R.norm_quant_inputs(c)
    want = R.norm_want(o["x"], o["w"], R.EPS, None, True, quant=True)
    xn = R.emulate_norm(o["x"], o["w"], R.EPS, None)
    for defect, rejected in ((None, False), ("amax_without_last_chunk", True)):
        q, s = R.emulate_quant(xn, defect)
        assert bool(R.norm_accept(want, xn, c.id, q, s)) == rejected, defect
        assert bool(R.norm_accept(want, None, c.id, q, s)) == rejected, defect
