"""CPU checks of the MXFP6 activation format (include/dualhyp_hip.h "MXFP6 activations"): the product's fp32 quantiser against the
fp64 reference of tests/mxfp6_reference.py bit for bit, the packer against the unpacker written from the header, the command-line
flag, the exported symbols and quantize_model_mxfp4(activations=...) on a CPU model.  No GPU."""
import pytest
import torch

import mxfp6_reference as R
from dualhyp_amd.synth import uniform, stream_id


def _rows():
    g = torch.Generator().manual_seed(12)
    x = uniform((48, 512), 1.5, stream_id(5, "mx6_host"))
    # rows whose blocks differ by many binades, rows of larger magnitudes, and heavy tails
    x[8:16] = (x[8:16].float() * torch.exp2(torch.randint(-20, 20, (8, 16), generator=g).float()).repeat_interleave(32, dim=1)).bfloat16()
    x[16:24] = (x[16:24].float() * 1000.0).bfloat16()
    x[24:32] = (x[24:32].float() * (1 + 29 * (torch.rand((8, 512), generator=g) < 0.002).float())).bfloat16()
    return x


def test_quantiser_matches_the_fp64_reference_bit_for_bit():
    from dualhyp_amd.quant import quantize_blocks_mxfp6, dequantize_blocks_mxfp6
    for x in (_rows(), R.edge_row().view(1, -1)):
        codes, scales = quantize_blocks_mxfp6(x)
        rc, rs = R.quantize_blocks(x)
        assert torch.equal(scales, rs), "E8M0 bytes differ from the fp64 reference"
        assert torch.equal(codes, rc), f"e2m3 codes differ from the fp64 reference at {(codes != rc).nonzero()[:4].tolist()}"
        assert int(scales.min()) >= 1 and int(scales.max()) <= 254 and int(codes.max()) < 64
        assert not (codes == 32).any(), "-0 is never produced"
        assert torch.equal(dequantize_blocks_mxfp6(codes, scales).double(), R.dequantize_blocks(rc, rs))


def test_every_bf16_value_of_three_binades_rounds_as_the_reference():
    """All 3 x 128 x 2 bf16 values of the binades [1, 8) and a few thousand below, each in a block whose amax is 4 (e = 0) or 7.5."""
    from dualhyp_amd.quant import quantize_blocks_mxfp6
    bits = torch.arange(0x3800, 0x4100, dtype=torch.int32)                  # 2^-15 .. just below 8
    vals = torch.cat((bits, bits | 0x8000)).to(torch.int16).view(torch.bfloat16)
    for top in (4.0, 7.5, 5.0):
        x = torch.zeros((vals.numel(), 32), dtype=torch.bfloat16)
        x[:, 0], x[:, 1] = top, vals
        x[x[:, 1].float().abs() > top, 0] = 7.96875                          # a larger element takes the block's amax over: still e = 0
        codes, scales = quantize_blocks_mxfp6(x)
        rc, rs = R.quantize_blocks(x)
        assert (scales == 127).all() and torch.equal(codes, rc) and torch.equal(scales, rs)


def test_hand_made_row_rounds_as_the_header_says():
    from dualhyp_amd.quant import quantize_blocks_mxfp6
    row = R.edge_row()
    codes, scales = quantize_blocks_mxfp6(row.view(1, -1))
    deq = R.dequantize_blocks(codes, scales)[0]
    c = codes[0].view(12, 32)
    # blocks 0 / 1: every magnitude as it stands: all 32 positive codes, the 31 negative ones, and +0 for -0
    assert int(scales[0, 0]) == 127 and c[0].tolist() == list(range(32))
    assert int(scales[0, 1]) == 127 - 9 and c[1].tolist() == [0] + [32 + i for i in range(1, 32)]
    assert sorted(set(c[0].tolist()) | set(c[1].tolist())) == [i for i in range(64) if i != 32], "every code the quantiser can produce"
    # blocks 2 / 3: amax 4 and every midpoint between neighbouring magnitudes: each goes to the even code
    assert int(scales[0, 2]) == 127 and deq[64:96].tolist() == [4.0] + list(R.MIDPOINT_RESULT)
    assert all(v % 2 == 0 for v in c[2, 1:].tolist())
    assert int(scales[0, 3]) == 134 and deq[96:128].tolist() == [-128.0 * v for v in [4.0] + list(R.MIDPOINT_RESULT)]
    assert (c[3][deq[96:128] == 0] == 0).all(), "a value that rounds to zero is stored as +0"
    # block 4: amax 7.75 = 1.9375 * 4 would round to 8: saturated to 7.5, e stays 0; -7.25 ties to the even code of 7
    assert int(scales[0, 4]) == 127 and deq[128:134].tolist() == [7.5, -7.5, 7.5, 7.5, 7.5, -7.0]
    # all-zero blocks (negative zeros included): s = 127, every code 0
    assert scales[0, 5:7].tolist() == [127, 127] and int(c[5:7].max()) == 0
    # bf16 subnormals alone: s clamps at 1 (2^-126); 2^-130 is exactly half of the smallest step 2^-129 and ties to code 0
    assert int(scales[0, 7]) == 1 and int(c[7].max()) == 0
    # around the clamp: subnormals are the values they are
    assert int(scales[0, 8]) == 1 and c[8, :6].tolist() == [8, 16, 32 + 24, 1, 0, 0]
    assert deq[256:260].tolist() == [2.0 ** -126, 2.0 ** -125, -(2.0 ** -124), 2.0 ** -129]
    # the largest binade of bf16: floor(log2(3.3e38)) = 127 -> s = 252; the upper clamp is out of a finite input's reach
    assert int(scales[0, 9]) == 252 and deq[288].item() == 7.0 * 2.0 ** 125 and deq[292].item() == 7.5 * 2.0 ** 125


def test_pack_unpack_round_trip():
    from dualhyp_amd.quant import quantize_blocks_mxfp6, pack_mxfp6, unpack_mxfp6
    x = _rows()
    for M in (48, 33, 1):
        codes, scales = quantize_blocks_mxfp6(x[:M])
        K = x.size(1)
        G = (M + 15) // 16
        xq, xs = pack_mxfp6(codes, scales, fill=0xFF)
        assert xq.shape == (G, K // 128, 3, 64, 8) and xs.shape == (G, K // 128, 64) and xq.dtype == xs.dtype == torch.uint8
        assert xq.numel() == G * 16 * K * 3 // 4 and xs.numel() == G * 16 * K // 32
        c1, s1 = R.unpack(xq, xs, M, K)                       # the header's index arithmetic
        assert torch.equal(c1, codes) and torch.equal(s1, scales)
        c2, s2 = unpack_mxfp6(xq, xs, M)
        assert torch.equal(c2, codes) and torch.equal(s2, scales)
        if M % 16:                                            # the rows past M exist and hold the fill
            cp, sp = unpack_mxfp6(xq, xs, G * 16)
            assert (cp[M:] == 63).all() and (sp[M:] == 0xFF).all()
    # all 64 codes survive the six-bit packing at every element position
    allc = ((torch.arange(16).view(-1, 1) * 7 + torch.arange(128).view(1, -1) * 5) % 64).to(torch.uint8)
    alls = torch.arange(64, dtype=torch.uint8).view(16, 4) + 100
    assert sorted(allc.unique().tolist()) == list(range(64))
    xq, xs = pack_mxfp6(allc, alls)
    assert torch.equal(R.unpack(xq, xs, 16, 128)[0], allc) and torch.equal(R.unpack(xq, xs, 16, 128)[1], alls)
    with pytest.raises(ValueError, match="multiple of 128"):
        pack_mxfp6(codes[:, :96], scales[:, :3])


def test_dequantised_activations_are_a_fixed_point():
    from dualhyp_amd.quant import quantize_blocks_mxfp6, dequantize_blocks_mxfp6
    x = _rows()
    codes, scales = quantize_blocks_mxfp6(x)
    deq = dequantize_blocks_mxfp6(codes, scales)
    c2, s2 = quantize_blocks_mxfp6(deq)
    assert torch.equal(dequantize_blocks_mxfp6(c2, s2), deq)
    err = ((deq - x.float()).pow(2).mean(-1).sqrt() / x.float().pow(2).mean(-1).sqrt())
    assert err[:8].max().item() < 0.04, "uniform rows: a three-bit mantissa under a shared exponent"


def test_cli_accepts_and_refuses():
    from dualhyp_amd import inference as I
    base = ["--test_path", "x.json", "--llm_checkpoint", "ckpt"]
    a = I.parse_args(base + ["--quantize", "mxfp4"])
    assert a.activations == "fp8"
    a = I.parse_args(base + ["--quantize", "mxfp4", "--activations", "mxfp6", "--kv_cache", "fp8"])
    assert a.quantize == "mxfp4" and a.activations == "mxfp6" and a.kv_cache == "fp8"
    for extra in ([], ["--quantize", "fp8"]):                # the two refusals: no quantisation, and e4m3 weights
        with pytest.raises(SystemExit):
            I.parse_args(base + extra + ["--activations", "mxfp6"])
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--quantize", "mxfp4", "--activations", "mxfp4"])
    assert I.parse_args(base + ["--quantize", "fp8", "--activations", "fp8"]).activations == "fp8"


def test_symbols_are_exported():
    import re
    from pathlib import Path
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    header = (Path(ge.ROOT) / "include" / "dualhyp_hip.h").read_text()
    for n in ("dh_quant_rows_mxfp6", "dh_rmsnorm_quant_mxfp6", "dh_linear_mxfp4a6_ex", "dh_linear_mxfp4a6_f32", "dh_engine_create_qa"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        assert re.search(r"\bint " + n + r"\(", header), f"{n} is not declared in the header"
    assert "MXFP6 activations (csrc/mxfp6.hip)" in header
    assert lib.dh_abi_version() == 6
    # argument checks run before anything touches a device
    assert lib.dh_linear_mxfp4a6_ex(None, None, None, None, None, 1, 16, 128, 0, None, None, None, None, None, 0, None) != 0
    assert b"dh_linear_mxfp4a6" in lib.dh_last_error()
    assert lib.dh_quant_rows_mxfp6(None, None, None, 1, 128, None) != 0 and b"dh_quant_rows_mxfp6" in lib.dh_last_error()
    assert lib.dh_rmsnorm_quant_mxfp6(None, None, None, None, None, 1, 128, 1e-5, None, None) != 0
    assert lib.dh_engine_create_qa(None, 1, 64, 64, 0, 1, 1, None) != 0


def test_quantize_model_mxfp4_activations_on_a_cpu_model():
    from dualhyp_amd import GPT, Config, quantize_model_mxfp4
    from dualhyp_amd.synth import synth_state_dict
    cfg = Config.from_name("parity-tiny", r=4, alpha=8, to_query=True, to_key=True, to_value=True, to_projection=True)
    sd = synth_state_dict(cfg, seed=1337, norm_jitter=0.25, weight_scale=4.0)

    def fresh():
        m = GPT(cfg).to(dtype=torch.bfloat16)
        m.load_state_dict(sd, strict=True)
        return m.eval()
    m = fresh()
    assert m.activation_format == "fp8"
    with pytest.raises(ValueError, match="activations"):
        quantize_model_mxfp4(m, activations="mxfp4")
    assert not getattr(m, "fp8", False), "a refused call leaves the model as it was"
    quantize_model_mxfp4(m, activations="mxfp6")
    assert m.fp8 and m.weight_format == "mxfp4" and m.activation_format == "mxfp6" and m.kv_cache_dtype == "bf16"
    w = m.transformer.h[0].attn.attn.linear.weight_mx4.clone()
    quantize_model_mxfp4(m, kv_cache="fp8", activations="mxfp6")        # a repeat call may change kv_cache ...
    assert m.activation_format == "mxfp6" and m.kv_cache_dtype == "fp8"
    quantize_model_mxfp4(m, kv_cache="fp8")                             # ... and the activation format (the default is fp8)
    assert m.activation_format == "fp8" and m.kv_cache_dtype == "fp8"
    quantize_model_mxfp4(m, activations="mxfp6")
    assert m.activation_format == "mxfp6" and m.kv_cache_dtype == "bf16"
    assert torch.equal(m.transformer.h[0].attn.attn.linear.weight_mx4, w), "the weights are quantised once"
    d = fresh()
    quantize_model_mxfp4(d)
    assert d.activation_format == "fp8"
