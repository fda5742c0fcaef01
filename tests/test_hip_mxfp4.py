"""GPU tests of MXFP4 weights on the fp8 serving path (csrc/mxfp4.hip, dualhyp_amd.quant; include/dualhyp_hip.h "MXFP4 weights").

The operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 operand and block scales, with exact integers through every
kernel; the GEMMs (streaming and tiled, every epilogue) against the fp64 product of tests/mxfp4_reference.py; row invariance;
the decoder end to end against oracle.OracleGPT over the MXFP4 weights restated as e4m3 values with power-of-two channel
scales (exactly the same products); batch invariance, the fp8 KV cache, the command line, and three engines in one process."""
import functools
import json

import pytest
import torch

import mxfp4_reference as R
from conftest import ulp_diff, record_parity
from dualhyp_amd.synth import uniform, stream_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def U(shape, bound, name, seed=78):
    return uniform(shape, bound, stream_id(seed, name))


def dv(t):
    return t.to(DEV)


def _packed(codes, scales):
    from dualhyp_amd.quant import pack_mxfp4
    wq, ws = pack_mxfp4(codes, scales)
    return dv(wq), dv(ws)


# ---------------------------------------------------------------------------------------------- exact integers
@functools.lru_cache(maxsize=None)
def _integer_weights():
    N, K = 80, 384
    n = torch.arange(N).view(-1, 1)
    k = torch.arange(K).view(1, -1)
    q = (k // 32) % 4
    # every code of the grid, both signs; the rule differs between even and odd k and between the four blocks of a k-step
    codes = ((3 * n + 5 * k + (k & 1) * (n + 2) + q * (q + n)) % 16).to(torch.uint8)
    blk = torch.arange(K // 32).view(1, -1)
    scales = (127 + 1 + ((n + 2 * blk + blk // 4) % 4)).to(torch.uint8)          # 2^1 .. 2^4, by (n, block) and by k-step
    assert sorted(codes.unique().tolist()) == list(range(16)) and sorted(scales.unique().tolist()) == [128, 129, 130, 131]
    return codes, scales, R.dequantize_blocks(codes, scales)


@pytest.mark.parametrize("M", [1, 19, 32, 33, 96, 128, 200])
def test_mxfp4_operand_map_exact_integers(M):
    """Every product and partial sum is an integer below 2^24 (384 * 2 * 6 * 16 = 73 728): fp32 is exact in any order, so a wrong
    nibble order, register half or scale byte shows as a wrong integer.  M = 33 and 128 sit on the row-group boundaries of the
    streaming kernel; M = 200 is tiled only."""
    from dualhyp_amd import ops
    codes, scales, wdeq = _integer_weights()
    N, K = codes.shape
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (M, K), generator=g).float()
    x[:, ::7] = 2.0                                       # break the symmetry between k positions
    want = x.double() @ wdeq.T
    assert want.abs().max() < 2 ** 24 and torch.equal(want, want.round())
    want = want.float().bfloat16()
    xq = dv(x.to(torch.float8_e4m3fn).view(torch.uint8))
    ones = torch.ones(M, device=DEV)
    wq, ws = _packed(codes, scales)
    for kernel in (0, 1, 2):
        if kernel == 2 and M > 128:
            continue
        y = ops.linear_mxfp4(xq, ones, wq, ws, kernel=kernel)
        bad = (y.cpu() != want).nonzero()
        assert torch.equal(y.cpu(), want), f"mxfp4 GEMM (M={M}, kernel={kernel}) is not the exact integer product; first at {bad[:4].tolist()}"
    if M <= 128:
        y32 = ops.linear_mxfp4(xq, ones, wq, ws, out32=True)
        assert torch.equal(y32.cpu(), want.float()), f"fp32-out streaming kernel (M={M}) is not the exact integer product"


# ---------------------------------------------------------------------------------------------- real values
@pytest.mark.parametrize("M,N,K", [(7, 512, 512), (40, 256, 384), (96, 1024, 2048), (130, 1024, 4096), (257, 512, 1792)])
def test_linear_mxfp4_matches_the_fp64_product(M, N, K):
    """Same operands on both sides and exact products: only the fp32 summation order differs from the fp64 sum, so the gates are
    those of test_linear_fp8_matches_the_oracle.  Up to 128 rows both kernels are checked, and a row's bits do not depend on how
    many rows ride along."""
    from dualhyp_amd import ops
    F = torch.nn.functional
    x, w, w2 = U((M, K), 1.5, "mx"), U((N, K), 0.05, "mw"), U((N, K), 0.05, "mw2")
    (c1, s1), (c2, s2) = R.quantize_blocks(w), R.quantize_blocks(w2)
    wq, ws = _packed(c1, s1)
    w2q, w2s = _packed(c2, s2)
    xq, xs = ops.quant_rows_fp8(dv(x))
    y0, y2 = R.linear(xq.cpu(), xs.cpu(), c1, s1), R.linear(xq.cpu(), xs.cpu(), c2, s2)
    r = U((M, N), 1.0, "mr")
    sc, bi = (1 + U((N,), 0.5, "ms").float()).bfloat16(), U((N,), 0.5, "mb")

    def chk(got, want, what, floor=1.0 / 16, max_ulp=2, max_frac=0.01):
        u = ulp_diff(got.float().cpu(), want.float(), floor)
        f = (u > 0).float().mean().item()
        record_parity(f"mxfp4_linear.{what}.M{M}N{N}K{K}", max_ulp=u.max().item(), bit_exact_frac=1.0 - f)
        assert u.max().item() <= max_ulp and f <= max_frac, f"{what}: max {u.max().item()} ulp, {f:.3%} differ"
    for kernel, tag in ((2, "stream."), (1, "tiled.")) if M <= 128 else ((0, ""),):
        chk(ops.linear_mxfp4(xq, xs, wq, ws, kernel=kernel), y0, tag + "plain")
        chk(ops.linear_mxfp4(xq, xs, wq, ws, resid=dv(r), kernel=kernel), r + y0, tag + "resid", floor=1.0)
        chk(ops.linear_mxfp4(xq, xs, wq, ws, epilogue=ops.EPI_SWIGLU, w2q=w2q, w2_scale=w2s, kernel=kernel), F.silu(y0) * y2, tag + "swiglu",
            max_ulp=4, max_frac=0.025)
        chk(ops.linear_mxfp4(xq, xs, wq, ws, epilogue=ops.EPI_ADAPTER, scale=dv(sc), bias=dv(bi), kernel=kernel), sc * (y0 + bi), tag + "adapter",
            floor=1.0, max_ulp=4)
    if M <= 128:
        for kernel in (1, 2):
            full = ops.linear_mxfp4(xq, xs, wq, ws, kernel=kernel)
            for rows in {1, min(M, 33), min(M, 65)}:
                part = ops.linear_mxfp4(xq[:rows].contiguous(), xs[:rows].contiguous(), wq, ws, kernel=kernel)
                assert torch.equal(part, full[:rows]), f"kernel {kernel}: rows 0..{rows} depend on the row count ({M} vs {rows})"
        full32 = ops.linear_mxfp4(xq, xs, wq, ws, out32=True)
        assert torch.equal(full32, ops.linear_mxfp4(xq, xs, wq, ws, kernel=2).float()), "the fp32-out kernel differs from the streaming kernel"


@pytest.mark.parametrize("epilogue", ["plain", "swiglu"])
def test_tiled_grid_classes_are_bit_identical(epilogue):
    """Grids of 384 tiles and more run the tiled kernel with two LDS stages and two blocks per CU, smaller ones with four stages;
    both walk k ascending in one accumulator, so a 128-row tile of the big call equals the same rows computed alone (the
    four-stage form the tests above hold against fp64)."""
    from dualhyp_amd import ops
    M, N, K = (1536, 4096, 384) if epilogue == "plain" else (768, 4096, 384)      # 12 x 32 and 6 x 64 tiles
    x, w, w2 = U((M, K), 1.5, "gx"), U((N, K), 0.05, "gw"), U((N, K), 0.05, "gw2")
    wq, ws = _packed(*R.quantize_blocks(w))
    kw = dict(kernel=1)
    if epilogue == "swiglu":
        w2q, w2s = _packed(*R.quantize_blocks(w2))
        kw.update(epilogue=ops.EPI_SWIGLU, w2q=w2q, w2_scale=w2s)
    xq, xs = ops.quant_rows_fp8(dv(x))
    full = ops.linear_mxfp4(xq, xs, wq, ws, **kw)
    for r0 in (0, M - 128):
        part = ops.linear_mxfp4(xq[r0:r0 + 128].contiguous(), xs[r0:r0 + 128].contiguous(), wq, ws, **kw)
        assert torch.equal(part, full[r0:r0 + 128]), f"rows {r0}.. of the {M}-row call differ from the same rows alone"
    assert full.float().abs().max().item() > 0


# ---------------------------------------------------------------------------------------------- decoder end to end
T, G = 40, 10


def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _model(cfg, sd, kv_cache="bf16", how="mxfp4"):
    from dualhyp_amd import GPT, quantize_model_fp8, quantize_model_mxfp4
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    m.eval()
    m.cpu_rsqrt_vec_width = 32
    if how == "mxfp4":
        quantize_model_mxfp4(m, kv_cache=kv_cache)
    elif how == "fp8":
        quantize_model_fp8(m, kv_cache=kv_cache)
    return m


@functools.lru_cache(maxsize=None)
def _tiny():
    """The model of test_fp8_decoder_vs_oracle_restatement (parity-hs128, LoRA r 16, the same synthetic weights)."""
    from dualhyp_amd import Config
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    from oracle import ger_oracle as O
    cfg = Config.from_name("parity-hs128", r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
    sd = synth_state_dict(cfg, seed=3, norm_jitter=0.25, weight_scale=4.0, embed_scale=64.0, head_tie=1.0)
    sdq, blocks = R.oracle_state_dict(sd, cfg, O)          # asserts the 11-binade bound and the exact e4m3 restatement
    idx = synth_prompts(2, T, cfg.padded_vocab_size, seed=9)
    return dict(cfg=cfg, sd=sd, sdq=sdq, blocks=blocks, idx=idx, m=_model(cfg, sd), oq=O.OracleGPT(cfg, sdq),
                o32=O.OracleGPT(cfg, {k: v.float() for k, v in sd.items()}), obf=O.OracleGPT(cfg, sd))


def test_mxfp4_decoder_vs_oracle_restatement():
    from dualhyp_amd import generate
    from dualhyp_amd.quant import unpack_mxfp4
    from oracle import ger_oracle as O
    t = _tiny()
    m, oq, o32, obf, idx, blocks = t["m"], t["oq"], t["o32"], t["obf"], t["idx"], t["blocks"]
    assert m.fp8 and m.weight_format == "mxfp4"
    # the bytes the engine streams are the reference quantiser's; lm_head is the fp8 path's
    for key, lin in (("transformer.h.1.attn.attn.linear.weight", m.transformer.h[1].attn.attn.linear),
                     ("transformer.h.0.mlp.proj.linear.weight", m.transformer.h[0].mlp.proj.linear)):
        codes, scales = blocks[key]
        c, s = R.unpack(lin.weight_mx4, lin.weight_mx4_scale, *codes.shape)
        assert torch.equal(c, codes) and torch.equal(s, scales), key
    assert torch.equal(m.lm_head.linear.weight_fp8.cpu(), t["sdq"]["lm_head.linear.weight"].view(torch.uint8))
    with torch.no_grad():
        got = m(torch.stack(idx).to(DEV)).float().cpu()
        want_q, want_32 = oq(torch.stack(idx)).float(), o32(torch.stack(idx))
    d_hip, d_orc, d_pair = rel_rms(got, want_32), rel_rms(want_q, want_32), rel_rms(got, want_q)
    record_parity("mxfp4_decoder.tiny.nocache", rel_rms_hip_vs_fp32=d_hip, rel_rms_oracle_mxfp4_vs_fp32=d_orc, rel_rms_hip_vs_oracle_mxfp4=d_pair)
    assert d_hip <= 1.1 * d_orc and d_pair <= d_orc
    with torch.no_grad():
        m.reset_cache()
        oq.reset_cache()
        lp = m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV)).float().cpu()
        rp = oq(idx[0].view(1, -1), torch.arange(T)).float()
        assert rel_rms(lp, rp) <= d_orc
        tok = int(rp[0, -1].argmax())
        for sstep in range(3):
            ld = m(torch.tensor([[tok]], device=DEV), torch.tensor([T + sstep], device=DEV))[0, 0].float().cpu()
            rd = oq(torch.tensor([[tok]]), torch.tensor([T + sstep]))[0, 0].float()
            assert rel_rms(ld, rd) <= 1.25 * d_orc and int(ld.argmax()) == int(rd.argmax())
            tok = int(rd.argmax())
        m.reset_cache()
    oq.reset_cache()
    ids_q = O.generate(oq, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    oq.reset_cache()
    ids_bf = O.generate(obf, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    obf.reset_cache()
    got_ids = generate(m, idx[1].to(DEV), T + G, temperature=0.2, top_k=1).cpu()
    record_parity("mxfp4_decoder.tiny.generate_ids", generated=G, equal_to_bf16_oracle=int((got_ids[T:] == ids_bf[T:]).sum()),
                  equal_to_mxfp4_oracle=int((got_ids[T:] == ids_q[T:]).sum()))
    assert torch.equal(got_ids, ids_q)              # four-bit weights are another model: the bf16 oracle's ids are recorded only


@pytest.mark.parametrize("kv_cache", ["bf16", "fp8"])
def test_mxfp4_batch_invariance(kv_cache):
    """generate_batch equals one-at-a-time for 33, 40 and 128 joint rows and for 96 ragged rows, with either KV cache."""
    from dualhyp_amd import generate, generate_batch
    t = _tiny()
    m, idx = (t["m"] if kv_cache == "bf16" else _kv8_model()), t["idx"]
    kw = dict(temperature=0.2, top_k=1)
    p0, p1 = idx[0][:23].to(DEV), idx[1].to(DEV)
    alone = [generate(m, p, p.numel() + 5, **kw).cpu() for p in (p0, p1)]
    assert m._engine.kv_cache_dtype == kv_cache
    both = [o.cpu() for o in generate_batch(m, [p0, p1], 5, **kw)]
    assert all(torch.equal(a, b) for a, b in zip(alone, both))
    for n, pb in ((33, 33), (40, 16), (128, 32)):
        joint = generate_batch(m, [p1] * n, 5, prefill_batch=pb, **kw)
        assert all(torch.equal(o.cpu(), alone[1]) for o in joint), f"{n}-row joint decode differs from the alone run"
    mixed = generate_batch(m, [p0, p1] * 48, 5, prefill_batch=32, **kw)      # 96 ragged rows
    assert all(torch.equal(o.cpu(), alone[i % 2]) for i, o in enumerate(mixed))


@functools.lru_cache(maxsize=None)
def _kv8_model():
    t = _tiny()
    return _model(t["cfg"], t["sd"], kv_cache="fp8")


def test_mxfp4_with_the_fp8_kv_cache_vs_oracle():
    """As tests/test_hip_kv8.py does for fp8 weights: cached prefill and decode steps against the oracle whose attention sees k and v
    through tests/kv8_reference.py's rounding, over the MXFP4 restatement; greedy ids equal that oracle's."""
    import kv8_reference as R8
    from dualhyp_amd import generate
    from oracle import ger_oracle as O
    t = _tiny()
    m, o32, idx = _kv8_model(), t["o32"], t["idx"]
    okv8 = R8.OracleGPTKV8(t["cfg"], t["sdq"])
    assert m.kv_cache_dtype == "fp8" and m.weight_format == "mxfp4"
    with torch.no_grad():
        d_orc = rel_rms(okv8(torch.stack(idx)).float(), o32(torch.stack(idx)))
        m.reset_cache()
        okv8.reset_cache()
        lp = m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV)).float().cpu()
        rp = okv8(idx[0].view(1, -1), torch.arange(T)).float()
        d_prefill = rel_rms(lp, rp)
        tok = int(rp[0, -1].argmax())
        steps = []
        for sstep in range(3):
            ld = m(torch.tensor([[tok]], device=DEV), torch.tensor([T + sstep], device=DEV))[0, 0].float().cpu()
            rd = okv8(torch.tensor([[tok]]), torch.tensor([T + sstep]))[0, 0].float()
            steps.append((rel_rms(ld, rd), int(ld.argmax()), int(rd.argmax())))
            tok = int(rd.argmax())
        m.reset_cache()
        okv8.reset_cache()
    record_parity("mxfp4_kv8_decoder.tiny", rel_rms_prefill_hip_vs_oracle=d_prefill, rel_rms_decode_steps_hip_vs_oracle=[s[0] for s in steps],
                  rel_rms_oracle_vs_fp32=d_orc)
    assert m._engine.kv_cache_dtype == "fp8"
    assert d_prefill <= d_orc
    for d, a, b in steps:
        assert d <= 1.25 * d_orc and a == b
    ids = O.generate(okv8, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    okv8.reset_cache()
    assert torch.equal(generate(m, idx[1].to(DEV), T + G, temperature=0.2, top_k=1).cpu(), ids)


def test_three_weight_formats_in_one_process():
    """An fp8 model, an mxfp4 model and a bf16 model generate in turn: each gives the ids it gives alone."""
    from dualhyp_amd import generate
    t = _tiny()
    cfg, sd, p = t["cfg"], t["sd"], t["idx"][1].to(DEV)
    kw = dict(temperature=0.2, top_k=1)
    alone = {}
    for how in ("fp8", "mxfp4", "bf16"):
        m = _model(cfg, sd, how=how)
        alone[how] = generate(m, p, T + G, **kw).cpu()
        del m
    models = {how: _model(cfg, sd, how=how) for how in ("fp8", "mxfp4", "bf16")}
    for _ in range(2):
        for how, m in models.items():
            assert torch.equal(generate(m, p, T + G, **kw).cpu(), alone[how]), f"the {how} model's ids change next to the other engines"
    assert torch.equal(alone["mxfp4"], generate(t["m"], p, T + G, **kw).cpu())
    with pytest.raises(ValueError, match="fp8 model"):
        generate(models["mxfp4"], p, T + G, speculate=2, **kw)


def test_cli_quantize_mxfp4(tmp_path):
    """`python -m dualhyp_amd.inference --random_init --quantize mxfp4 --kv_cache fp8` on the merged-schema fixture of test_harness.py:
    the predictions of generate_batch on a model quantised through the API with the same settings."""
    from test_harness import merged_items, CAPTIONS
    from dualhyp_amd import GPT, generate_batch, quantize_model_mxfp4
    from dualhyp_amd import inference as I
    from dualhyp_amd.data import HypothesesDataset
    from dualhyp_amd.synth import synth_state_dict
    from dualhyp_amd.tokenizer import ByteTokenizer
    items = merged_items(caps=CAPTIONS)
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    ckpt_dir = tmp_path / "checkpoints" / "parity-harness"
    ckpt_dir.mkdir(parents=True)
    new = 10
    argv = ["--test_path", str(test_json), "--llm_checkpoint", str(ckpt_dir), "--prompts_format", "DualHyp", "--dual_hypotheses",
            "--tokenizer", "byte", "--random_init", "--quantize", "mxfp4", "--kv_cache", "fp8", "--max_new_tokens", str(new),
            "--decode_batch", "4", "--predict_dir", str(tmp_path / "predictions")]
    out = I.main(argv)
    preds = [p["inference"] for p in out["predictions"]]
    assert len(preds) == len(items)
    args = I.parse_args(argv)
    cfg = I.config_from_args(args)
    torch.manual_seed(args.seed)
    m = GPT(cfg)
    m.load_state_dict(synth_state_dict(cfg, seed=args.seed, embed_scale=50.0, head_tie=1.0))
    m = m.to(device=DEV, dtype=torch.bfloat16).eval()
    quantize_model_mxfp4(m, kv_cache="fp8")
    tok = ByteTokenizer()
    ds = HypothesesDataset(str(test_json), tok, prompts_format="DualHyp", seed=args.seed)
    exs = [ds[i] for i in range(len(ds))]
    want = []
    for b in range(0, len(exs), 4):
        ps = [e["input_ids_no_response"].to(DEV) for e in exs[b:b + 4]]
        outs = generate_batch(m, ps, new, temperature=0.2, top_k=1, eos_id=tok.eos_token_id, prefill_batch=4)
        want += [I.extract_answer(tok.decode(o.cpu()), tok.decode(p.cpu())) for o, p in zip(outs, ps)]
    assert m._engine.kv_cache_dtype == "fp8" and m.weight_format == "mxfp4"
    assert preds == want
