"""GPU tests of the fp8 KV cache (csrc/kv8.hip, attn_decode_kernel over a CacheFp8 in csrc/attention.hip, the kv8 mode of csrc/engine.hip).

Op level, bit for bit: the quantising cache writer against tests/kv8_reference.py applied to what the bf16 writer cached, the
expansion against the reference's dequantisation, and decode attention over the fp8 cache against the bf16 kernel over the
expanded cache — the scheme's values are bf16 values, so the last two are equalities by construction.
Engine level, on the tiny hs-128 model of test_hip_fp8.py::test_fp8_decoder_vs_oracle_restatement: logits and greedy ids against
the oracle with the same rounding of k and v (OracleGPTKV8), batch / schedule / prefix-sharing invariance, the cache's contents
and size, and the CLI."""
import functools
import json

import pytest
import torch

import kv8_reference as R
from conftest import record_parity
from dualhyp_amd.synth import uniform, stream_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
i32 = torch.int32

SHAPES = [(128, 8, 2), (64, 4, 4), (96, 2, 2)]
S_MAX, N_SLOTS = 640, 4
LENS, SLOTS = [1, 33, 545], [2, 0, 3]          # one key, a tile boundary, a wave walking more than one tile; permuted slots
EDGE_SEQ, EDGE_POS0 = 2, 100                   # the edge rows of kv8_reference are V vectors of group 0 there


@functools.lru_cache(maxsize=None)
def _ops_case(hs, n_head, n_groups):
    """One run of both cache writers on the same qkv, positions and slots; everything the op tests compare."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    width = (n_head + 2 * n_groups) * hs
    n_tok = sum(LENS)
    qkv = uniform((n_tok, width), 1.0, stream_id(5, f"kv8qkv{hs}"))
    # per-token magnitudes over 2^-12 .. 2^6: exponents on both sides of zero, e4m3 subnormals next to full-range vectors
    qkv = (qkv.float() * torch.exp2(torch.randint(-12, 7, (n_tok, 1), generator=torch.Generator().manual_seed(hs)).float())).bfloat16()
    edge = R.edge_rows(hs)
    t_edge = sum(LENS[:EDGE_SEQ]) + EDGE_POS0
    qkv.view(n_tok, n_groups, n_head // n_groups + 2, hs)[t_edge:t_edge + edge.size(0), 0, -1] = edge
    cos, sin = O.build_rope_cache(S_MAX, hs)
    slot = torch.cat([torch.full((n,), s, dtype=i32) for s, n in zip(SLOTS, LENS)])
    pos = torch.cat([torch.arange(n, dtype=i32) for n in LENS])
    d = lambda t: t.to(DEV)
    kc = torch.zeros((N_SLOTS, n_groups, S_MAX, hs), dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros((N_SLOTS, n_groups, hs, S_MAX), dtype=torch.bfloat16, device=DEV)
    q_bf = ops.qkv_rope_cache(d(qkv), d(cos), d(sin), d(slot), d(pos), kc, vt, n_head, n_groups)
    k8, v8, ke, ve = ops.kv8_alloc(N_SLOTS, n_groups, S_MAX, hs, DEV)
    q_8 = ops.qkv_rope_cache_kv8(d(qkv), d(cos), d(sin), d(slot), d(pos), k8, v8, ke, ve, n_head, n_groups)
    k_plain = ops.kcache_to_plain(kc).cpu()                                  # [slot, group, key, hs]
    v_plain = ops.vcache_to_plain(vt).transpose(-1, -2).contiguous().cpu()   # [slot, group, key, hs]
    # the expansion of the fp8 cache, over the lengths the sequences have
    ke_out, vt_out = torch.zeros_like(kc), torch.zeros_like(vt)
    ops.kv8_expand(k8, v8, ke, ve, torch.tensor(SLOTS, dtype=i32, device=DEV), torch.tensor(LENS, dtype=i32, device=DEV), ke_out, vt_out)
    torch.cuda.synchronize()
    return dict(q_bf=q_bf, q_8=q_8, k8=k8, v8=v8, ke=ke, ve=ve, k_plain=k_plain, v_plain=v_plain, k_exp_out=ke_out, vt_exp_out=vt_out)


@pytest.mark.parametrize("hs,n_head,n_groups", SHAPES)
def test_quantising_cache_writer(hs, n_head, n_groups):
    from dualhyp_amd import ops
    c = _ops_case(hs, n_head, n_groups)
    assert torch.equal(c["q_bf"], c["q_8"]), "rotated q differs from dh_qkv_rope_cache_bf16's"
    kb, vb, ke, ve = (t.cpu() for t in ops.kv8_unpack(c["k8"], c["v8"], c["ke"], c["ve"]))
    written = torch.zeros((N_SLOTS, S_MAX), dtype=torch.bool)
    for s, n in zip(SLOTS, LENS):
        written[s, :n] = True
    for name, got_b, got_e, plain in (("K", kb, ke, c["k_plain"]), ("V", vb, ve, c["v_plain"])):
        want_b, want_e = R.kv8_quantize(plain)                               # of the bf16 values the bf16 op cached
        w = written[:, None, :].expand(N_SLOTS, n_groups, S_MAX)
        assert torch.equal(got_e[w], want_e[w]), f"{name} exponents differ from kv8_quantize"
        assert torch.equal(got_b[w], want_b[w]), f"{name} bytes differ from kv8_quantize"
        assert (got_b[~w] == 0).all() and (got_e[~w] == 0).all(), f"{name}: a position that was not written is not zero"
        assert not ((got_b & 0x7f) == 0x7f).any(), f"{name}: a NaN byte"
    # the edge rows arrived as V vectors, bit for bit those of the host restatement
    edge_b, edge_e = R.kv8_quantize(R.edge_rows(hs))
    n_e = edge_b.size(0)
    assert torch.equal(vb[SLOTS[EDGE_SEQ], 0, EDGE_POS0:EDGE_POS0 + n_e], edge_b)
    assert torch.equal(ve[SLOTS[EDGE_SEQ], 0, EDGE_POS0:EDGE_POS0 + n_e], edge_e)


@pytest.mark.parametrize("hs,n_head,n_groups", SHAPES)
def test_expand_is_the_dequantised_cache(hs, n_head, n_groups):
    from dualhyp_amd import ops
    c = _ops_case(hs, n_head, n_groups)
    kb, vb, ke, ve = (t.cpu() for t in ops.kv8_unpack(c["k8"], c["v8"], c["ke"], c["ve"]))
    got_k = ops.kcache_to_plain(c["k_exp_out"]).cpu()
    got_v = ops.vcache_to_plain(c["vt_exp_out"]).transpose(-1, -2).cpu()
    for name, got, b, e in (("K", got_k, kb, ke), ("V^T", got_v, vb, ve)):
        want = R.kv8_dequantize(b, e)
        assert torch.equal(want.to(torch.bfloat16).float(), want)
        for s in range(N_SLOTS):
            n = LENS[SLOTS.index(s)] if s in SLOTS else 0
            assert torch.equal(got[s, :, :n].float(), want[s, :, :n]), f"{name}: slot {s} is not kv8_dequantize of its bytes"
            assert (got[s, :, n:] == 0).all(), f"{name}: slot {s} is not zero beyond kv_len = {n}"


@pytest.mark.parametrize("hs,n_head,n_groups", SHAPES)
def test_decode_attention_over_the_fp8_cache(hs, n_head, n_groups):
    """dh_attn_decode_kv8 == dh_attn_decode_bf16 over the expanded cache, bit for bit: the same operand values, the same walk over the
    tiles, the same combine.  The query scale makes the softmax anything from flat to one-hot."""
    from dualhyp_amd import ops
    c = _ops_case(hs, n_head, n_groups)
    slots, lens = torch.tensor(SLOTS, dtype=i32, device=DEV), torch.tensor(LENS, dtype=i32, device=DEV)
    for qs in (0.05, 1.0, 8.0):
        q = (uniform((len(LENS), n_head, hs), 1.0, stream_id(6, f"kv8q{hs}")).float() * qs).bfloat16().to(DEV)
        want = ops.attn_decode(q, c["k_exp_out"], c["vt_exp_out"], slots, lens)
        got = ops.attn_decode_kv8(q, c["k8"], c["v8"], c["ke"], c["ve"], slots, lens)
        assert torch.isfinite(want.float()).all()
        assert torch.equal(got, want), f"q scale {qs}: {(got != want).sum().item()} of {got.numel()} outputs differ from the bf16 kernel's"
    # a sequence shorter than its cached positions: the keys behind kv_len are masked, whatever their bytes are
    short = torch.tensor([1, 20, 300], dtype=i32, device=DEV)
    ke2, vt2 = torch.zeros_like(c["k_exp_out"]), torch.zeros_like(c["vt_exp_out"])
    ops.kv8_expand(c["k8"], c["v8"], c["ke"], c["ve"], slots, short, ke2, vt2)
    assert torch.equal(ops.attn_decode_kv8(q, c["k8"], c["v8"], c["ke"], c["ve"], slots, short), ops.attn_decode(q, ke2, vt2, slots, short))
    # ... and the expansion writes them as zero BITS (+0.0), though their bytes are live values of either sign
    for s_, n in zip(SLOTS, short.tolist()):
        assert (ops.kcache_to_plain(ke2)[s_, :, n:].view(torch.int16) == 0).all()
        assert (ops.vcache_to_plain(vt2)[s_, :, :, n:].contiguous().view(torch.int16) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- engine level
def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


T, G = 40, 10


@functools.lru_cache(maxsize=1)
def _tiny():
    """The tiny hs-128 decoder of test_fp8_decoder_vs_oracle_restatement, quantised with an fp8 KV cache, and its oracles."""
    from dualhyp_amd import Config
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    from oracle import ger_oracle as O
    cfg = Config.from_name("parity-hs128", r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
    sd = synth_state_dict(cfg, seed=3, norm_jitter=0.25, weight_scale=4.0, embed_scale=64.0, head_tie=1.0)
    sdq = O.quantize_state_dict_fp8(sd, cfg)
    idx = synth_prompts(2, T, cfg.padded_vocab_size, seed=9)
    return dict(cfg=cfg, sd=sd, idx=idx, m=_model(cfg, sd, "fp8"), okv8=R.OracleGPTKV8(cfg, sdq), oq=O.OracleGPT(cfg, sdq),
                o32=O.OracleGPT(cfg, {k: v.float() for k, v in sd.items()}), obf=O.OracleGPT(cfg, sd))


def _model(cfg, sd, kv_cache):
    from dualhyp_amd import GPT, quantize_model_fp8
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    m.eval()
    m.cpu_rsqrt_vec_width = 32
    if kv_cache is None:
        quantize_model_fp8(m)
    else:
        quantize_model_fp8(m, kv_cache=kv_cache)
    return m


def test_kv8_decoder_vs_oracle():
    """Cached prefill logits and three decode steps against OracleGPTKV8 over the fp8 state dict, with the gates of
    test_fp8_decoder_vs_oracle_restatement: d_orc is the kv8 oracle's distance to the fp32 function, and two implementations of one
    scheme differ by less than either differs from fp32."""
    t = _tiny()
    m, okv8, oq, o32, idx = t["m"], t["okv8"], t["oq"], t["o32"], t["idx"]
    assert m.kv_cache_dtype == "fp8"
    with torch.no_grad():
        want_32 = o32(torch.stack(idx))
        d_orc = rel_rms(okv8(torch.stack(idx)).float(), want_32)
        d_orc_bf = rel_rms(oq(torch.stack(idx)).float(), want_32)
        m.reset_cache()
        okv8.reset_cache()
        lp = m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV)).float().cpu()
        rp = okv8(idx[0].view(1, -1), torch.arange(T)).float()
        d_prefill = rel_rms(lp, rp)
        print(f"kv8 prefill: rel_rms(hip, kv8 oracle) = {d_prefill:.4g}, d_orc = {d_orc:.4g}, fp8 oracle with a bf16 cache vs fp32 = {d_orc_bf:.4g}")
        tok = int(rp[0, -1].argmax())
        steps = []
        for sstep in range(3):
            ld = m(torch.tensor([[tok]], device=DEV), torch.tensor([T + sstep], device=DEV))[0, 0].float().cpu()
            rd = okv8(torch.tensor([[tok]]), torch.tensor([T + sstep]))[0, 0].float()
            steps.append((rel_rms(ld, rd), int(ld.argmax()), int(rd.argmax())))
            tok = int(rd.argmax())
        m.reset_cache()
        okv8.reset_cache()
    print("kv8 decode steps (rel_rms, argmax hip, argmax oracle):", steps)
    record_parity("kv8_decoder.tiny", rel_rms_prefill_hip_vs_oracle_kv8=d_prefill, rel_rms_decode_steps_hip_vs_oracle_kv8=[s[0] for s in steps],
                  rel_rms_oracle_kv8_vs_fp32=d_orc, rel_rms_oracle_fp8_kv_bf16_vs_fp32=d_orc_bf)
    assert d_prefill <= d_orc
    for d, a, b in steps:
        assert d <= 1.25 * d_orc and a == b


def test_kv8_greedy_ids_are_the_oracles():
    from dualhyp_amd import generate
    from oracle import ger_oracle as O
    t = _tiny()
    m, okv8, obf, idx = t["m"], t["okv8"], t["obf"], t["idx"]
    okv8.reset_cache()
    ids_kv8 = O.generate(okv8, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    okv8.reset_cache()
    ids_bf = O.generate(obf, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    obf.reset_cache()
    got = generate(m, idx[1].to(DEV), T + G, temperature=0.2, top_k=1).cpu()
    record_parity("kv8_decoder.tiny.generate_ids", generated=G, equal_to_kv8_oracle=int((got[T:] == ids_kv8[T:]).sum()),
                  equal_to_bf16_oracle=int((got[T:] == ids_bf[T:]).sum()))
    assert torch.equal(got, ids_kv8)


def test_kv8_batch_schedule_and_prefix_invariance():
    from dualhyp_amd import generate, generate_batch
    from dualhyp_amd.generate import generate_stream
    from dualhyp_amd.synth import synth_prompts
    t = _tiny()
    m, idx, V = t["m"], t["idx"], t["cfg"].padded_vocab_size
    kw = dict(temperature=0.2, top_k=1)
    p0, p1 = idx[0][:23].to(DEV), idx[1].to(DEV)
    alone = [generate(m, p, p.numel() + 5, **kw).cpu() for p in (p0, p1)]
    both = [o.cpu() for o in generate_batch(m, [p0, p1], 5, **kw)]
    assert all(torch.equal(a, b) for a, b in zip(alone, both)), "two ragged prompts together differ from the alone runs"
    for n, pb in ((33, 33), (128, 32)):                 # both fp8 GEMM classes of a decode step stay within one call
        joint = generate_batch(m, [p1] * n, 5, prefill_batch=pb, **kw)
        assert all(torch.equal(o.cpu(), alone[1]) for o in joint), f"{n}-row joint decode differs from the alone run"
    prefix = synth_prompts(1, 32, V, seed=21)[0]
    tails = synth_prompts(6, 12, V, seed=22)
    ps = [torch.cat([prefix, tl[:3 + 2 * i]]).to(DEV) for i, tl in enumerate(tails)]
    plain = [o.cpu() for o in generate_batch(m, ps, 6, **kw)]
    shared = [o.cpu() for o in generate_batch(m, ps, 6, share_prefix="auto", **kw)]
    assert all(torch.equal(a, b) for a, b in zip(plain, shared)), "share_prefix='auto' changes the ids"
    for sp in (False, "auto"):
        stream = [o.cpu() for o in generate_stream(m, ps, 6, max_rows=4, prefill_batch=2, check_every=2, share_prefix=sp, **kw)]
        assert all(torch.equal(a, b) for a, b in zip(plain, stream)), f"generate_stream(share_prefix={sp!r}) changes the ids"


def test_kv8_cache_contents_are_fixed_points_of_the_scheme():
    from dualhyp_amd import ops
    t = _tiny()
    m, idx, cfg = t["m"], t["idx"], t["cfg"]
    m.refresh_engine()                 # a fresh, zeroed cache: earlier tests have decoded into this model's
    with torch.no_grad():
        m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV))
    eng = m._engine
    Gq, hs = cfg.n_query_groups, cfg.head_size
    k = ops.kcache_to_plain(eng.read(6, 1, (eng.max_batch, Gq, eng.s_max, hs))).cpu()
    v = ops.vcache_to_plain(eng.read(7, 1, (eng.max_batch, Gq, hs, eng.s_max))).transpose(-1, -2).cpu()
    m.reset_cache()
    for name, x in (("K", k), ("V", v)):
        assert (x[0, :, :T].float().abs().amax(-1) > 0).all(), f"{name}: a prefilled position is empty"
        assert (x[0, :, T:] == 0).all(), f"{name}: a position behind the prompt is not zero"
        assert torch.equal(R.kv8_round_trip(x), x), f"{name}: a cached value does not survive kv8_quantize -> kv8_dequantize"
    with pytest.raises(Exception, match="selector 1 reads a bf16 KV cache"):
        eng.read(1, 0, (eng.max_batch, Gq, eng.s_max, hs))


def test_kv8_cache_size():
    """dh_engine_device_bytes against the bf16-cache engine of the same capacity: the difference stated in include/dualhyp_hip.h."""
    t = _tiny()
    cfg = t["cfg"]
    mb = _model(cfg, t["sd"], "bf16")
    B, S, tokens = 3, 128, 256
    sizes = {}
    for name, mod in (("fp8", t["m"]), ("bf16", mb)):
        mod.set_capacity(B, S, tokens)
        eng = mod.engine()
        assert (eng.max_batch, eng.s_max, eng.max_tokens, eng.kv_cache_dtype) == (B, S, tokens, name)
        sizes[name] = int(eng.lib.dh_engine_device_bytes(eng.handle))
    L, hs = cfg.n_layer, cfg.head_size
    n = B * cfg.n_query_groups * S
    assert sizes["bf16"] - sizes["fp8"] == L * n * (2 * hs - 2) - 4 * n * hs - 16 * L


def test_kv_cache_bf16_is_todays_path():
    from dualhyp_amd import generate, quantize_model_fp8
    t = _tiny()
    cfg, sd, p = t["cfg"], t["sd"], t["idx"][1].to(DEV)
    ids = [generate(_model(cfg, sd, kv), p, T + G, temperature=0.2, top_k=1).cpu() for kv in (None, "bf16")]
    assert torch.equal(ids[0], ids[1])
    # the setting of a quantised model can be changed: the engine is rebuilt with the other cache
    m = _model(cfg, sd, "fp8")
    kv8_ids = generate(m, p, T + G, temperature=0.2, top_k=1).cpu()
    assert m._engine.kv_cache_dtype == "fp8" and torch.equal(kv8_ids, generate(t["m"], p, T + G, temperature=0.2, top_k=1).cpu())
    quantize_model_fp8(m, kv_cache="bf16")
    assert torch.equal(generate(m, p, T + G, temperature=0.2, top_k=1).cpu(), ids[0]) and m._engine.kv_cache_dtype == "bf16"
    with pytest.raises(ValueError, match="fp8 model"):
        generate(t["m"], p, T + G, temperature=0.2, top_k=1, speculate=2)


def test_cli_quantize_fp8_kv_cache_fp8(tmp_path):
    """`python -m dualhyp_amd.inference --random_init --quantize fp8 --kv_cache fp8` on the merged-schema fixture of test_harness.py:
    the predictions of generate_batch on a model quantised through the API with the same settings."""
    from test_harness import merged_items, CAPTIONS
    from dualhyp_amd import GPT, generate_batch, quantize_model_fp8
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
            "--tokenizer", "byte", "--random_init", "--quantize", "fp8", "--kv_cache", "fp8", "--max_new_tokens", str(new),
            "--decode_batch", "4", "--predict_dir", str(tmp_path / "predictions")]
    out = I.main(argv)
    preds = [p["inference"] for p in out["predictions"]]
    assert len(preds) == len(items)
    # the same through the API
    args = I.parse_args(argv)
    cfg = I.config_from_args(args)
    torch.manual_seed(args.seed)
    m = GPT(cfg)
    m.load_state_dict(synth_state_dict(cfg, seed=args.seed, embed_scale=50.0, head_tie=1.0))
    m = m.to(device=DEV, dtype=torch.bfloat16).eval()
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.kv_cache_dtype == "fp8"
    tok = ByteTokenizer()
    ds = HypothesesDataset(str(test_json), tok, prompts_format="DualHyp", seed=args.seed)
    exs = [ds[i] for i in range(len(ds))]
    want = []
    for b in range(0, len(exs), 4):
        ps = [e["input_ids_no_response"].to(DEV) for e in exs[b:b + 4]]
        outs = generate_batch(m, ps, new, temperature=0.2, top_k=1, eos_id=tok.eos_token_id, prefill_batch=4)
        want += [I.extract_answer(tok.decode(o.cpu()), tok.decode(p.cpu())) for o, p in zip(outs, ps)]
    assert m._engine.kv_cache_dtype == "fp8"
    assert preds == want
    written = json.loads((tmp_path / "predictions" / "random_init.json").read_text())
    assert [w["inference"] for w in written[:len(items)]] == want
