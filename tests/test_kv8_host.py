"""CPU tests of the fp8 KV cache: the scheme's restatement (tests/kv8_reference.py) keeps its promises — every dequantised
value is a bf16 value, the exponent steps where it must, no NaN byte — and the inference harness parses the two new flags."""
import pytest
import torch

import kv8_reference as R


def _vectors(hs):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(257, hs, generator=g) * torch.exp2(torch.randint(-20, 12, (257, 1), generator=g).float())
    return torch.cat([x.to(torch.bfloat16), R.edge_rows(hs)])


@pytest.mark.parametrize("hs", [64, 96, 128])
def test_dequantised_values_are_bf16_values(hs):
    """The representability claim: e4m3 * 2^e has 4 significant bits and an exponent bf16 holds, so rounding it to bf16
    changes nothing — attention over the fp8 cache is the bf16 attention over the dequantised cache."""
    x = _vectors(hs)
    q, e = R.kv8_quantize(x)
    d = R.kv8_dequantize(q, e)
    assert d.dtype == torch.float32 and torch.isfinite(d).all()
    assert torch.equal(d.to(torch.bfloat16).float(), d)
    # quantising a dequantised vector gives it back: its amax is an e4m3 value times 2^e, never above 448 * 2^e
    q2, e2 = R.kv8_quantize(d.to(torch.bfloat16))
    assert torch.equal(R.kv8_dequantize(q2, e2), d)


@pytest.mark.parametrize("hs", [64, 96, 128])
def test_edge_rows(hs):
    x = R.edge_rows(hs)
    q, e = R.kv8_quantize(x)
    val = q.view(torch.float8_e4m3fn).float()
    assert not torch.isnan(val).any() and not ((q & 0x7f) == 0x7f).any(), "a NaN byte"
    assert val.abs().max() <= 448
    amax = x.float().abs().amax(-1)
    e = e.int()
    assert e[0] == 0 and (q[0] == 0).all()                                             # all-zero
    for i, k in ((1, 0), (3, -3), (5, 5)):
        assert amax[i] == 448.0 * 2.0 ** k and e[i] == k and val[i].abs().max() == 448   # amax = 448 * 2^k: the largest byte, exactly
        assert amax[i + 1] > amax[i] and e[i + 1] == k + 1                               # one bf16 step above: the exponent steps
    assert e[7] == -100 and val[7].abs().max() * 2.0 ** -100 == pytest.approx(1e-30, rel=2 ** -4)   # 448 * 2^-108 would hold it: clamped
    assert e[8] == 7 and val[8].abs().max() * 2.0 ** 7 == pytest.approx(3e4, rel=2 ** -4)
    assert e[9] == 100 and val[9].min() == -448                                        # past 448 * 2^100: saturated, not NaN
    assert e[10] == -2 and val[10].min() == -448                                       # the negative extreme is the largest byte
    # e is the SMALLEST exponent that holds amax (rows that the clamp did not touch)
    free = (e > R.E_MIN) & (e < R.E_MAX) & (amax > 0)
    assert (amax[free] <= 448.0 * torch.exp2(e[free].float())).all() and (amax[free] > 448.0 * torch.exp2(e[free].float() - 1)).all()


def test_cli_flags():
    from dualhyp_amd.inference import parse_args
    base = ["--test_path", "x.json"]
    a = parse_args(base)
    assert a.quantize == "none" and a.kv_cache == "bf16" and a.share_prefix == "off" and a.speculate == 0 and a.decode_batch == 640
    a = parse_args(base + ["--quantize", "fp8"])
    assert a.quantize == "fp8" and a.kv_cache == "bf16"
    a = parse_args(base + ["--quantize", "fp8", "--kv_cache", "fp8"])
    assert a.quantize == "fp8" and a.kv_cache == "fp8"
    for bad in (["--kv_cache", "fp8"], ["--kv_cache", "fp8", "--quantize", "none"], ["--kv_cache", "int8"], ["--quantize", "int8"]):
        with pytest.raises(SystemExit) as ex:
            parse_args(base + bad)
        assert ex.value.code == 2


def test_quantize_model_fp8_rejects_an_unknown_kv_cache():
    from dualhyp_amd import GPT, Config, quantize_model_fp8
    m = GPT(Config.from_name("parity-tiny"))
    assert m.kv_cache_dtype == "bf16"
    with pytest.raises(ValueError, match="kv_cache is 'bf16' or 'fp8'"):
        quantize_model_fp8(m, kv_cache="int8")
    assert not getattr(m, "fp8", False) and m.kv_cache_dtype == "bf16"
