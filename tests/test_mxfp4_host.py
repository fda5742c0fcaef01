"""CPU checks of the MXFP4 weight format (include/dualhyp_hip.h "MXFP4 weights"): the product's fp32 quantiser against the fp64
reference of tests/mxfp4_reference.py bit for bit, the packer against the unpacker written from the header, the command-line
flag, the exported symbols and quantize_model_mxfp4 on a CPU model.  No GPU."""
import pytest
import torch

import mxfp4_reference as R
from dualhyp_amd.synth import uniform, stream_id


def _rows():
    g = torch.Generator().manual_seed(11)
    x = uniform((48, 512), 0.07, stream_id(5, "mx4_host"))
    # rows whose blocks differ by many binades, and rows of larger magnitudes
    x[8:16] = (x[8:16].float() * torch.exp2(torch.randint(-20, 20, (8, 16), generator=g).float()).repeat_interleave(32, dim=1)).bfloat16()
    x[16:24] = (x[16:24].float() * 1000.0).bfloat16()
    return x


def test_quantiser_matches_the_fp64_reference_bit_for_bit():
    from dualhyp_amd.quant import quantize_blocks_mxfp4, dequantize_blocks_mxfp4
    for w in (_rows(), R.edge_row().view(1, -1)):
        codes, scales = quantize_blocks_mxfp4(w)
        rc, rs = R.quantize_blocks(w)
        assert torch.equal(scales, rs), "E8M0 bytes differ from the fp64 reference"
        assert torch.equal(codes, rc), "e2m1 codes differ from the fp64 reference"
        assert int(scales.min()) >= 1 and int(scales.max()) <= 254
        assert torch.equal(dequantize_blocks_mxfp4(codes, scales).double(), R.dequantize_blocks(rc, rs))


def test_hand_made_row_rounds_as_the_header_says():
    from dualhyp_amd.quant import quantize_blocks_mxfp4
    row = R.edge_row()
    codes, scales = quantize_blocks_mxfp4(row.view(1, -1))
    deq = R.dequantize_blocks(codes, scales)[0]
    # block 0: amax 4 -> e = 0: [4, the seven ties, 6, 7] and their negatives
    want = [4.0] + list(R.TIE_RESULT) + [6.0, 6.0]
    assert int(scales[0, 0]) == 127 and deq[:10].tolist() == want and deq[10:19].tolist() == [-v for v in want[1:]]
    assert (codes[0, :32] != 8).all(), "a value that rounds to zero is stored as +0"
    # block 1: the same scaled by 2^5 with amax 6 * 2^5 exactly -> e = 5
    assert int(scales[0, 1]) == 132 and deq[32:42].tolist() == [32.0 * v for v in [6.0] + list(R.TIE_RESULT) + [6.0, 6.0]]
    # all-zero blocks (negative zeros included): s = 127, every code 0
    assert scales[0, 2:4].tolist() == [127, 127] and int(codes[0, 64:128].max()) == 0
    # amax 6 * 2^-3 exactly, one bf16 step above (saturates at 6) and one below (rounds up to 6): one exponent, e = -3
    assert scales[0, 4:7].tolist() == [124, 124, 124]
    assert deq[128].item() == 0.75 and deq[160].item() == 0.75 and deq[192].item() == -0.75
    # bf16 subnormals: s clamps at 1 (2^-126); 2^-133 is far below half of the smallest step and becomes zero
    assert int(scales[0, 7]) == 1 and deq[224:227].tolist() == [0.0, 0.0, 0.0]
    assert int(scales[0, 8]) == 1 and deq[256:259].tolist() == [2.0 ** -126, 2.0 ** -125, -(2.0 ** -124)]
    # the largest binade of bf16: floor(log2(3e38)) = 127 -> s = 252, the upper clamp is out of a finite input's reach
    assert int(scales[0, 9]) == 252 and deq[288].item() == 6.0 * 2.0 ** 125


def test_pack_unpack_round_trip():
    from dualhyp_amd.quant import quantize_blocks_mxfp4, pack_mxfp4, unpack_mxfp4
    w = _rows()
    codes, scales = quantize_blocks_mxfp4(w)
    wq, ws = pack_mxfp4(codes, scales)
    N, K = w.shape
    assert wq.shape == (N // 16, K // 128, 64, 16) and ws.shape == (N // 16, K // 128, 64) and wq.dtype == ws.dtype == torch.uint8
    assert wq.numel() == N * K // 2 and ws.numel() == N * K // 32
    c1, s1 = R.unpack(wq, ws, N, K)                       # the header's index arithmetic
    assert torch.equal(c1, codes) and torch.equal(s1, scales)
    c2, s2 = unpack_mxfp4(wq, ws)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    with pytest.raises(ValueError, match="multiple of 16"):
        pack_mxfp4(codes[:40], scales[:40])


def test_dequantised_weights_are_a_fixed_point():
    from dualhyp_amd.quant import quantize_blocks_mxfp4, dequantize_blocks_mxfp4
    for w in (_rows(), R.edge_row().view(1, -1)):
        codes, scales = quantize_blocks_mxfp4(w)
        deq = dequantize_blocks_mxfp4(codes, scales)
        c2, s2 = quantize_blocks_mxfp4(deq)
        assert torch.equal(dequantize_blocks_mxfp4(c2, s2), deq)
        # the bytes too, except where a block below the lowest scale became all zero: its scale byte is then the zero block's
        live = deq.view(deq.size(0), -1, 32).abs().amax(-1) > 0
        assert torch.equal(c2, codes) and torch.equal(s2[live], scales[live]) and (s2[~live] == 127).all()


def test_cli_accepts_and_refuses():
    from dualhyp_amd import inference as I
    base = ["--test_path", "x.json", "--llm_checkpoint", "ckpt"]
    a = I.parse_args(base + ["--quantize", "mxfp4"])
    assert a.quantize == "mxfp4" and a.kv_cache == "bf16"
    a = I.parse_args(base + ["--quantize", "mxfp4", "--kv_cache", "fp8"])
    assert a.quantize == "mxfp4" and a.kv_cache == "fp8"
    for extra in (["--speculate", "2"], ["--num_beams", "2"]):
        with pytest.raises(SystemExit):
            I.parse_args(base + ["--quantize", "mxfp4"] + extra)
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--kv_cache", "fp8"])         # still needs the fp8 serving path


def test_symbols_are_exported():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    for n in ("dh_linear_mxfp4_ex", "dh_linear_mxfp4_f32", "dh_engine_create_q"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.dh_abi_version() == 6
    # argument checks run before anything touches a device
    assert lib.dh_linear_mxfp4_ex(None, None, None, None, None, 1, 16, 128, 0, None, None, None, None, None, 0, None) != 0
    assert b"dh_linear_mxfp4" in lib.dh_last_error()


def test_quantize_model_mxfp4_on_a_cpu_model():
    from dualhyp_amd import GPT, Config, quantize_model_fp8, quantize_model_mxfp4
    from dualhyp_amd.quant import unpack_mxfp4
    from dualhyp_amd.synth import synth_state_dict
    from dualhyp_amd.checkpoint import save_checkpoint
    from oracle import ger_oracle as O
    cfg = Config.from_name("parity-tiny", r=4, alpha=8, to_query=True, to_key=True, to_value=True, to_projection=True)
    sd = synth_state_dict(cfg, seed=1337, norm_jitter=0.25, weight_scale=4.0)

    def fresh():
        m = GPT(cfg).to(dtype=torch.bfloat16)
        m.load_state_dict(sd, strict=True)
        return m.eval()
    m = fresh()
    with pytest.raises(ValueError, match="kv_cache"):
        quantize_model_mxfp4(m, kv_cache="int8")
    assert not getattr(m, "fp8", False)
    quantize_model_mxfp4(m, kv_cache="fp8")
    assert m.fp8 and m.weight_format == "mxfp4" and m.kv_cache_dtype == "fp8"
    d, I_, qkv = cfg.n_embd, cfg.intermediate_size, (cfg.n_head + 2 * cfg.n_query_groups) * cfg.head_size
    blk = m.transformer.h[1]
    merged = O.merged_weights(sd, cfg)
    for lin, key, (N, K) in ((blk.attn.attn.linear, "attn.attn", (qkv, d)), (blk.attn.proj.linear, "attn.proj", (d, d)),
                             (blk.mlp.fc_1.linear, "mlp.fc_1", (I_, d)), (blk.mlp.fc_2.linear, "mlp.fc_2", (I_, d)),
                             (blk.mlp.proj.linear, "mlp.proj", (d, I_))):
        assert lin.weight.numel() == 0 and not hasattr(lin, "weight_fp8")
        assert lin.weight_mx4.dtype == torch.uint8 and lin.weight_mx4.numel() == N * (K // 2)        # K / 2 bytes per row
        assert lin.weight_mx4_scale.dtype == torch.uint8 and lin.weight_mx4_scale.numel() == N * (K // 32)
        codes, scales = unpack_mxfp4(lin.weight_mx4, lin.weight_mx4_scale)
        rc, rs = R.quantize_blocks(merged[f"transformer.h.1.{key}.linear.weight"])
        assert torch.equal(codes, rc) and torch.equal(scales, rs), key
    head = m.lm_head.linear
    assert head.weight_fp8.shape == (cfg.padded_vocab_size, d) and head.weight_scale.dtype == torch.float32 and not hasattr(head, "weight_mx4")
    assert m.transformer.wte.weight.dtype == torch.bfloat16 and m.transformer.wte.weight.numel() > 0
    assert not any("mx4" in k or "fp8" in k for k in m.state_dict()), "the quantised buffers are not persistent"
    quantize_model_mxfp4(m, kv_cache="bf16")                # idempotent apart from kv_cache
    assert m.kv_cache_dtype == "bf16" and m.weight_format == "mxfp4"
    with pytest.raises(RuntimeError, match="mxfp4"):
        quantize_model_fp8(m)
    with pytest.raises(RuntimeError):
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError):
        save_checkpoint(m, "unused.pth")
    f8 = fresh()
    quantize_model_fp8(f8)
    with pytest.raises(RuntimeError, match="fp8"):
        quantize_model_mxfp4(f8)
