"""The exact references of the quantised GEMMs on their own (tests/qgemm_exact_reference.py; CPU only): every case meets the
exactness condition and survives its format, the reference agrees bit for bit with two independent restatements, the table
reaches every route, instantiation, shape class and threshold it is there for, and deliberately wrong "kernels" are rejected."""
import re
from pathlib import Path

import pytest
import torch

import gemm_exact_reference as R
import mxfp4_reference as MX
import qgemm_exact_reference as Q

REPO = Path(__file__).resolve().parent.parent
GROUPS = sorted({(c.family, c.group) for c in Q.CASES})
NEW_ROUTES = tuple(r for r in R.ROUTES if r.startswith(("fp8_", "mx4_")))
F8 = torch.float8_e4m3fn


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        if c.data_key not in seen:
            seen.add(c.data_key)
            out.append(c)
    return out


@pytest.mark.parametrize("family,group", GROUPS, ids=[f"{f}/{g}" for f, g in GROUPS])
def test_every_case_is_exact_and_survives_its_format(family, group):
    """reference() raises InexactCase where a sum could round (it never clips); encode() where a value is not of its format"""
    for c in _distinct(Q.cases_of(family, group)):
        o = Q.operands(c)
        enc = Q.encode(c, o)
        assert torch.equal(enc["xq"].view(F8).double(), o["x"]) and enc["xq"].shape == (c.M, c.K)
        assert not bool(((enc["xq"] & 0x7F) == 0x7F).any()), f"{c.id}: x holds the e4m3 NaN"
        for s in ("", "2"):
            if c.fmt == "fp8" and "w" + s in o:
                assert torch.equal(enc[f"w{s}q"].view(F8).double(), o["w" + s])
            elif "codes" + s in o:
                codes, sc = MX.unpack(enc[f"w{s}q"], enc[f"w{s}sc"], c.N, c.K)     # the header's layout, index by index
                assert torch.equal(codes, o["codes" + s]) and torch.equal(sc, o["sc" + s]), f"{c.id}: pack / unpack round trip"
                assert 127 - 8 <= int(sc.min()) and int(sc.max()) <= 127 + 8
        ref = Q.reference(c, o)
        for k, v in ref.items():
            assert not torch.isnan(v.float()).any(), f"{c.id}: {k}"
        if c.epi == "swiglu":
            assert set(ref) == {"g", "u", "cand"} and float(ref["g"].float().abs().max()) < 87
        else:
            assert ref["y"].dtype == torch.bfloat16 and ref["y"].shape == (c.M, c.N)


def test_reference_raises_instead_of_clipping():
    c = Q.Case("small", "x", "fp8", "linear", 4, 16, 5248)
    o = Q.operands(c)
    o["x"] = o["x"] * 64                                 # still e4m3 values; sums of |products| beyond 2^24 units
    o["w"] = o["w"] * 32
    with pytest.raises(Q.InexactCase, match="2\\^24"):
        Q.reference(c, o)
    o = Q.operands(c)
    o["x"][0, 1] = 0.25                                  # not a multiple of the unit the case declares
    with pytest.raises(Q.InexactCase, match="unit"):
        Q.reference(c, o)
    o = Q.operands(c)
    o["x"][0, 1] = 17.0                                  # not an e4m3 number
    with pytest.raises(Q.InexactCase, match="e4m3"):
        Q.encode(c, o)
    m = Q.Case("small", "x", "mx4", "linear", 4, 16, 128)
    o = Q.operands(m)
    o["sc"][3, 2] = 255
    with pytest.raises(Q.InexactCase, match="255"):
        Q.encode(m, o)
    s = Q.Case("small", "x", "fp8", "linear", 4, 16, 5248, epi="swiglu")
    o = Q.operands(s)
    o["xs"] = o["xs"] * 64
    with pytest.raises(Q.InexactCase, match="underflow"):
        Q.reference(s, o)


def test_scales_are_real_and_depend_on_their_index():
    o = Q.operands(Q.Case("small", "x", "fp8", "linear", 128, 516, 640, epi="swiglu"))
    for k in ("xs", "ws", "ws2"):
        v = o[k]
        assert v.dtype == torch.float32 and bool((v[1:] != v[:-1]).all()), k
        mant = v.view(torch.int32) & 0x7FFFFF
        assert int((mant == 0).sum()) == 0 and int((mant & 0xFFFF != 0).sum()) > v.numel() // 2, f"{k}: powers of two, or short mantissas"
    m = Q.operands(Q.Case("small", "x", "mx4", "linear", 8, 528, 1152))
    sc = m["sc"].int()
    assert int(sc.min()) == 127 - 8 and int(sc.max()) == 127 + 8
    per_step = sc.view(528, -1, 4)
    assert bool((per_step.amax(-1) - per_step.amin(-1) == 3).all()), "the four blocks of a k-step differ"
    assert bool((per_step[:, 1:] != per_step[:, :-1]).any(-1).all()), "consecutive k-steps differ"
    assert bool((sc[1:] != sc[:-1]).any(-1).all()), "neighbouring rows differ"
    x = o["x"]
    for v in (1.5, 3, 5, 7, 12):
        assert bool((x == v).any()) and bool((x == -v).any()) and bool((o["w"] == v).any()) and bool((o["w"] == -v).any()), v
    assert set(m["codes"].unique().tolist()) == set(range(16))


def test_every_code_cases_hold_every_code():
    for c in _distinct(Q.cases_of("codes", "fp8")):
        o = Q.operands(c)
        walked = o["x"] if c.data == "codes_x" else o["w"]
        by = walked.float().to(F8).view(torch.uint8)
        assert set(by.unique().tolist()) == set(Q.e4m3_bytes().tolist()), "every non-NaN e4m3 byte"
        assert float(walked.abs().max()) == 448 and float(walked[walked != 0].abs().min()) == 2.0 ** -9
        y = Q.reference(c, o)["y"].double()
        assert torch.equal(y, walked if c.data == "codes_x" else walked.T), "each output is the decoded value itself"
    (c,) = _distinct(Q.cases_of("codes", "mx4"))
    o = Q.operands(c)
    pairs = {(int(a), int(b)) for a, b in zip(o["codes"].flatten().tolist(), o["sc"].repeat_interleave(32, 1).flatten().tolist())}
    assert pairs == {(code, s) for code in range(16) for s in range(127 - 8, 127 + 9)}, "16 codes x 17 block scales"
    assert torch.equal(Q.reference(c, o)["y"].double(), MX.dequantize_blocks(o["codes"], o["sc"]).T)


def _plain_sample(fmt):
    cs = [c for c in _distinct(Q.CASES) if c.fmt == fmt and c.epi == "plain" and not c.resid and c.data == "rand" and c.M * c.N <= 1 << 20]
    return cs[::3] +[c for c in _distinct(Q.cases_of("codes", fmt))]


def test_fp8_reference_is_the_oracles_linear_fp8():
    """oracle.ger_oracle.linear_fp8 quantises its bf16 input itself, so the case's x gets a +-448 in column 0 and is multiplied by
    a 4-bit row factor: the oracle's quantiser then returns exactly x, with the scale amax * fp32(1/448), which the reference
    takes as x_scale.  Exact sums on both sides: bit for bit."""
    from oracle import ger_oracle as O
    n = 0
    for c in _plain_sample("fp8"):
        o = Q.operands(c)
        x = o["x"].clone()
        rows = torch.arange(c.M)
        x[:, 0] = 448.0 * (1 - 2 * (rows % 2)).double()
        xb = (x * ((8 + rows % 8).double() / 8 * 2.0 ** -4).view(-1, 1)).bfloat16()
        xq, xs = O.quantize_rows_fp8(xb)
        assert torch.equal(xq.double(), x)
        o.update(x=x, xs=xs.view(-1), x_unit=torch.minimum(o["x_unit"], torch.tensor(0.5, dtype=torch.float64)))
        want = Q.reference(c, o)["y"]
        got = O.linear_fp8(xb, o["w"].float().to(F8), o["ws"])
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), c.id
        n += 1
    assert n >= 40


def test_mxfp4_reference_is_mxfp4_references_linear():
    n = 0
    for c in _plain_sample("mx4"):
        o = Q.operands(c)
        enc = Q.encode(c, o)
        codes, sc = MX.unpack(enc["wq"], enc["wsc"], c.N, c.K)
        got = MX.linear(enc["xq"], o["xs"], codes, sc)
        want = Q.reference(c, o)["y"]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), c.id
        n += 1
    assert n >= 30


def test_dequant4_is_the_products_dequantiser():
    from dualhyp_amd.quant import dequantize_blocks_mxfp4
    o = Q.operands(Q.Case("small", "x", "mx4", "linear", 1, 48, 640))
    assert torch.equal(Q.dequant4(o["codes"], o["sc"]), dequantize_blocks_mxfp4(o["codes"], o["sc"]).double())
    assert torch.equal(Q.dequant4(o["codes"], o["sc"]), MX.dequantize_blocks(o["codes"], o["sc"]))


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def test_route_table_matches_the_library():
    src = (REPO / "dualhyp_amd" / "csrc" / "gemm.h").read_text()
    body = re.search(r"enum DhGemmRoute : int \{(.*?)\};", src, re.S).group(1)
    names = [n.lower() for n in re.findall(r"^\s*DH_ROUTE_(\w+)", body, re.M)]
    assert tuple(names[:-1]) == R.ROUTES and names[-1] == "count" and len(R.ROUTES) <= 64
    assert len(NEW_ROUTES) == 11 and R.ROUTES[-11:] == NEW_ROUTES, "appended, the earlier numbers unchanged"
    assert R.ROUTES.index("chain_tiled") == 23
    assert R.route_names(1 << R.ROUTES.index("fp8_t256")) == {"fp8_t256"}
    with pytest.raises(AssertionError):
        R.route_names(1 << len(R.ROUTES))
    for c in Q.CASES:
        assert len(c.routes) == 1 and c.routes[0] in NEW_ROUTES, c.id
        tile = dict(c.tune).get(19, 0)
        assert c.routes[0] == Q.route_of(c.fmt, c.M, c.N, c.epi, 2 if c.op == "linear_f32" else c.kernel, tile), c.id
        for k, _ in c.tune:
            assert k in Q.TUNING_DEFAULTS, f"{c.id}: key {k} has no default to restore"


def test_the_table_reaches_every_route_instantiation_and_shape_class():
    five = {("plain", False), ("plain", True), ("adapter", False), ("adapter", True), ("swiglu", False)}
    for r in NEW_ROUTES:
        cs = [c for c in Q.CASES if c.routes == (r,) and c.op == "linear"]
        assert {(c.epi, c.resid) for c in cs} == five, f"{r}: (EPI, RESID) instantiations {sorted({(c.epi, c.resid) for c in cs})}"
        if "stream" in r:
            assert any(c.routes == (r,) and c.op == "linear_f32" for c in Q.CASES), f"{r}: no fp32-out case"
    for fmt in Q.FMTS:
        stream = [c for c in Q.CASES if c.fmt == fmt and "stream" in c.routes[0] and c.data == "rand"]
        tiled = [c for c in Q.CASES if c.fmt == fmt and "stream" not in c.routes[0] and c.data == "rand"]
        for epi, resid in five:
            s = [c for c in stream if (c.epi, c.resid) == (epi, resid) and c.op == "linear"]
            t = [c for c in tiled if (c.epi, c.resid) == (epi, resid)]
            assert {(c.M, c.N) for c in s} >= {(M, N) for M in Q.STREAM_M for N in Q.NS[fmt]}, (fmt, epi, resid)
            assert {(c.M, c.N) for c in t} >= {(M, N) for M in Q.STREAM_M + Q.TILED_M for N in Q.NS[fmt]}, (fmt, epi, resid)
            assert {c.K for c in s} == set(Q.KS) and {c.K for c in t} >= set(Q.KS), (fmt, epi, resid)
        f32 = [c for c in stream if c.op == "linear_f32"]
        assert {c.M for c in f32} == set(Q.STREAM_M) and {c.N for c in f32} == set(Q.NS[fmt]) and {c.K for c in f32} == set(Q.KS)
        # every branch of the staged loops: K one to five stages on the 4-stage and on the 2-stage form
        for r in (f"{fmt}_t128_s4", f"{fmt}_t128_s2") + (("fp8_t256",) if fmt == "fp8" else ()):
            assert {c.K for c in Q.CASES if c.routes == (r,)} >= set(Q.K_LOOP), r
        # the streaming loop's second outer trip: 8 waves x CH k-steps (CH 4, SwiGLU 2)
        assert any(c.K // 128 > 16 for c in stream if c.epi == "swiglu") and any(c.K // 128 > 32 for c in stream if c.epi != "swiglu")
        assert any(c.thin for c in stream) and all(c.thin == (c.K >= 4224) for c in stream)


def test_both_sides_of_every_threshold():
    plain = [c for c in Q.CASES if c.family == "dispatch"]
    assert all(c.kernel == 0 and not c.tune and c.op == "linear" for c in plain)
    for fmt in Q.FMTS:
        d = {(c.M, c.N): c.routes[0] for c in plain if c.fmt == fmt}
        n4 = Q.NS[fmt][0]
        assert d[(128, Q.NS[fmt][4])] == f"{fmt}_stream_ng4" and d[(129, Q.NS[fmt][4])] == f"{fmt}_t128_s4"
        assert Q.cdiv(49024, 128) * Q.cdiv(n4, 128) == 383 and d[(49024, n4)] == f"{fmt}_t128_s4"
        assert Q.cdiv(49025, 128) * Q.cdiv(n4, 128) == 384 and d[(49025, n4)] == f"{fmt}_t128_s2"
    d = {(c.M, c.N): c.routes[0] for c in plain if c.fmt == "fp8"}
    assert Q.cdiv(3841, 256) * Q.cdiv(7684, 256) == 496 and d[(3841, 7684)] == "fp8_t128_s2"
    assert Q.cdiv(3841, 256) * Q.cdiv(7940, 256) == 512 and d[(3841, 7940)] == "fp8_t256"
    tune = [c for c in Q.CASES if c.family == "tune"]
    assert {(dict(c.tune)[19], c.epi, c.resid) for c in tune if c.group.startswith("tile-")} == {(t, e, r) for t in (128, 256) for _, e, r in Q.EPIS}
    bands = {(dict(c.tune)[19], Q.cdiv(c.M, dict(c.tune)[19]), dict(c.tune)[20], c.epi) for c in tune if c.group.startswith("band-")}
    assert bands >= {(t, nb, gm, e) for t in (128, 256) for nb in (3, 5) for gm in (0, 1, 2, 4, 8) for e in ("plain", "swiglu")}


# ---- SwiGLU acceptance ------------------------------------------------------------------------------------------------------
def test_candidates_for_any_g_are_the_integer_tables_rule():
    g = torch.arange(-R.SILU_G_MAX, R.SILU_G_MAX + 1, dtype=torch.float64)
    assert torch.equal(Q.silu_candidates_of(g), R.silu_candidates())
    gen = torch.Generator().manual_seed(9)
    g = (torch.randn(4000, generator=gen, dtype=torch.float64) * 20).bfloat16().double()
    cand = Q.silu_candidates_of(g)
    v = g / (1 + torch.exp(-g))
    err = (cand.double() - v[:, None]).abs()
    assert torch.equal(cand.bfloat16().float(), cand) and (err[:, 0] <= err[:, 1]).all() and (err[:, 0] <= err[:, 2]).all()
    assert (cand[:, 1] < cand[:, 0]).all() and (cand[:, 0] < cand[:, 2]).all()
    # adjacent bf16 numbers: nothing lies between a candidate and its neighbours
    o = Q._bf16_ord(cand)
    assert torch.equal(o[:, 1], o[:, 0] - 1) and torch.equal(o[:, 2], o[:, 0] + 1)


def test_acceptance_agrees_with_the_integer_one_and_rejects_two_steps():
    gen = torch.Generator().manual_seed(3)
    g = torch.randint(-40, 41, (33, 64), generator=gen).double()
    u = torch.randint(-40, 41, (33, 64), generator=gen).double()
    cand = Q.silu_candidates_of(g)
    for col in (0, 1, 2):
        got = (cand[..., col] * u.float()).bfloat16()
        a = Q.swiglu_accept(got, g, u, cand)
        b = R.swiglu_accept(got, g, u)
        assert torch.equal(a[0], b[0]) and a[1:] == b[1:] and a[0].all()
    two_off = cand[..., 2] + (cand[..., 2] - cand[..., 0])
    assert not Q.swiglu_accept((two_off * u.float()).bfloat16(), g, u, cand)[0].all()
    assert not Q.swiglu_accept((cand[..., 0] * u.float()).bfloat16().roll(1, 0), g, u, cand)[0].all(), "a result shifted by one row passes"
    zero = torch.zeros_like(g).bfloat16()
    gg = torch.full_like(g, -87.0)
    assert not Q.swiglu_accept(zero, gg, u, Q.silu_candidates_of(gg))[0][u != 0].any(), "a zero above the flush range passes"


# ---- sensitivity: deliberately wrong kernels ----------------------------------------------------------------------------------
BUGS = ("xs_next_row", "ws_next_col", "last_kstep_dropped", "one_wave_dropped", "nibbles_swapped", "neighbour_block_scale", "row_clamp_off_by_one",
        "bias_after_scale", "resid_before_rounding", "operands_swapped_halves")


def _model(c, o, enc, bug=None):
    """A plain restatement of the kernels from the BYTES the library is given, with one planted defect"""
    M, N, K = c.M, c.N, c.K
    x = enc["xq"].view(F8).double()
    if bug == "row_clamp_off_by_one":                    # m < M - 1 ? m : M - 2
        x = x[torch.arange(M).clamp(max=max(M - 2, 0))]
    if bug == "operands_swapped_halves":                 # an e4m3 fragment read as pieces 2kg, 2kg + 1 next to one read as kg, 4 + kg
        x = x.view(M, K // 128, 4, 2, 16).transpose(2, 3).reshape(M, K)
    keep = torch.ones(K, dtype=torch.float64)
    if bug == "last_kstep_dropped":
        keep[K - 128:] = 0
    if bug == "one_wave_dropped":                        # the k-steps of wave 3 of 8
        keep.view(-1, 128)[3::8] = 0

    def wmat(s):
        if c.fmt == "fp8":
            return enc[f"w{s}q"].view(F8).double()
        codes, sc = MX.unpack(enc[f"w{s}q"], enc[f"w{s}sc"], N, K)
        if bug == "nibbles_swapped":
            codes = codes.view(N, K // 2, 2).flip(-1).reshape(N, K)
        if bug == "neighbour_block_scale":
            sc = sc[:, torch.arange(K // 32) ^ 1]
        return MX.dequantize_blocks(codes, sc)

    xs = o["xs"][(torch.arange(M) + 1).clamp(max=M - 1)] if bug == "xs_next_row" else o["xs"]

    def fin(acc, s):
        if c.fmt == "fp8":
            ws = o["ws" + s]
            ws = ws[(torch.arange(N) + 1).clamp(max=N - 1)] if bug == "ws_next_col" else ws
            sc = xs.view(-1, 1) * ws.view(1, -1)
        else:
            sc = xs.view(-1, 1)
        raw = acc.float() * sc
        y = raw.bfloat16().float()
        if c.epi == "adapter":
            a, b = o["a"].float().view(1, -1), o["b"].float().view(1, -1)
            raw = (a * y).bfloat16().float() + b if bug == "bias_after_scale" else a * (y + b).bfloat16().float()
            y = raw.bfloat16().float()
        return raw, y

    raw, y = fin((x * keep) @ wmat("").T, "")
    if c.epi == "swiglu":
        return {"g": y.bfloat16(), "u": fin((x * keep) @ wmat("2").T, "2")[1].bfloat16()}
    if c.resid:
        y = (o["resid"].float() + (raw if bug == "resid_before_rounding" else y)).bfloat16().float()
    return {"y": y.bfloat16()}


def _rejects(ref, got):
    return any(not torch.equal(ref[k].view(torch.int16), got[k].view(torch.int16)) for k in got)


def test_wrong_kernels_are_rejected_and_the_right_one_is_not():
    sample = [c for c in _distinct(Q.CASES) if c.family in ("small", "tiled", "codes") and c.M in (33, 97, 128, 129)][::3]
    assert len(sample) >= 60
    caught = {b: 0 for b in BUGS}
    for c in sample:
        o = Q.operands(c)
        enc = Q.encode(c, o)
        ref = Q.reference(c, o)
        assert not _rejects(ref, _model(c, o, enc)), f"{c.id}: the restatement from the bytes differs from the reference"
        for b in BUGS:
            caught[b] += _rejects(ref, _model(c, o, enc, b))
    print(f"wrong kernels rejected, of {len(sample)} cases: {caught}")
    assert all(caught.values()), f"never rejected: {[b for b, n in caught.items() if not n]}"
