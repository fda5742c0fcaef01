"""Prefix sharing on the GPU (share_prefix of generate_batch / generate_stream, dh_engine_copy_prefix): the tokens every prompt of a
call opens with are forwarded once, their K / V copied into the other slots, the rest of each prompt forwarded at position P.
Every check is exact (torch.equal): caches, logits and ids are those of the unshared run; only the tokens forwarded change, and
that number is checked as a count.  Prompts share 80 tokens, so P = 64."""
import json
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import GPT, Config, generate_batch, generate_stream, quantize_model_fp8
from dualhyp_amd._lib import DualHypHipError
from dualhyp_amd.schedule import predict
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
NEW = 24
P = 64
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}


def build(name, fp8=False, seed=11, **over):
    cfg = Config.from_name(name, **LORA, **over)
    assert cfg.head_size == HEAD_SIZES[name]
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.eval()
    if fp8:
        quantize_model_fp8(m)
    return cfg, m


def sharing_prompts(cfg, tails, shared=80, seed=40):
    """len(tails) prompts: the same `shared` tokens, then tails[i] tokens of their own of which the first differs in every prompt"""
    V = cfg.padded_vocab_size
    head = synth_prompts(1, shared, V, seed=seed)[0]
    out = []
    for i, n in enumerate(tails):
        tail = synth_prompts(1, n + 1, V, seed=seed + 1 + i)[0][1:]          # without the BOS
        tail[0] = 3 + i
        out.append(torch.cat([head, tail]).to(DEV))
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def caches(eng, cfg, B, S):
    """[layer][K, V^T] as (B, G, S * hs): a (slot, group) block, positions [0, n) being its first n * hs elements whenever n % 32 == 0"""
    G, hs = cfg.n_query_groups, cfg.head_size
    return [[eng.read(w, l, (B, G, S * hs)).clone() for w in (1, 2)] for l in range(cfg.n_layer)]


# ---- 1. the copy kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HEAD_SIZES))
def test_copy_prefix_kernel(name):
    cfg, m = build(name, n_layer=3)             # a first, a middle and the last layer
    B, S, hs = 8, 128, cfg.head_size
    V = cfg.padded_vocab_size
    m.refresh_engine()
    eng = m.engine(B, S, B * 100, exact=True)
    # a known pattern in every slot: eight different 100-token sequences
    fill = [synth_prompts(1, 100, V, seed=500 + i)[0].to(DEV) for i in range(B)]
    eng.forward(torch.cat(fill), [100] * B, [0] * B, want_all=False, want_last=True)
    src = synth_prompts(1, 80, V, seed=77)[0].to(DEV)
    eng.forward(src, [80], [0], want_all=False, want_last=True)
    before = caches(eng, cfg, B, S)
    eng.copy_prefix(0, [2, 5, 1], P)
    after = caches(eng, cfg, B, S)
    n = P * hs
    for l in range(cfg.n_layer):
        for w in range(2):
            b, a = before[l][w], after[l][w]
            assert b[0, :, :n].any()
            for s in (1, 2, 5):
                assert not torch.equal(b[s, :, :n], b[0, :, :n]), "the pattern equals the source: the check would prove nothing"
                assert torch.equal(a[s, :, :n], a[0, :, :n]), f"layer {l} cache {w}: positions [0, {P}) of slot {s} differ from slot 0's"
                assert torch.equal(a[s, :, n:], b[s, :, n:]), f"layer {l} cache {w}: slot {s} was written at or behind position {P}"
            for s in (0, 3, 4, 6, 7):
                assert torch.equal(a[s], b[s]), f"layer {l} cache {w}: slot {s} is not a destination and was written"
    # the whole cache length, and one tile
    eng.copy_prefix(3, [0], S)
    eng.copy_prefix(4, [7, 6], 32)
    last = caches(eng, cfg, B, S)
    for l in range(cfg.n_layer):
        for w in range(2):
            assert torch.equal(last[l][w][0], after[l][w][3])
            for s in (6, 7):
                assert torch.equal(last[l][w][s, :, :32 * hs], after[l][w][4, :, :32 * hs])
                assert torch.equal(last[l][w][s, :, 32 * hs:], after[l][w][s, :, 32 * hs:])
    for bad in ((0, [1], 48), (0, [1], 0), (0, [1], S + 32), (0, [B], P), (-1, [1], P), (B, [1], P), (0, [1, 0], P), (0, [1, 2, 1], P),
                (0, [-1], P)):
        with pytest.raises(DualHypHipError, match="dh_engine_copy_prefix"):
            eng.copy_prefix(*bad)
    eng.copy_prefix(0, [], P)                   # nothing to do
    assert all(torch.equal(x, y) for a, b in zip(caches(eng, cfg, B, S), last) for x, y in zip(a, b)), "a refused call wrote"


# ---- 2. prefix forward + copy + remainder forward == one packed forward ---------------------------------------------------------
@pytest.mark.parametrize("name,fp8", [("parity-tiny", False), ("parity-hs96", False), ("parity-hs128", False), ("parity-hs128", True)])
def test_forward_behind_a_copied_prefix(name, fp8):
    cfg, m = build(name, fp8=fp8)
    hs = cfg.head_size
    ps = sharing_prompts(cfg, [1, 17, 31, 16, 40])          # lengths 81 .. 120: remainders of 17 .. 56 tokens behind P = 64
    lens = [p.numel() for p in ps]
    B, S = 5, 128

    def fresh():
        m.refresh_engine()                                   # a zeroed cache: whole blocks are compared
        return m.engine(B, S, sum(lens), exact=True)

    eng = fresh()
    _, want = eng.forward(torch.cat(ps), lens, [0] * B, want_all=False, want_last=True)
    want, kv_want = want.clone(), caches(eng, cfg, B, S)
    eng = fresh()
    eng.forward(ps[0][:P], [P], [0], want_all=False, want_last=False)
    eng.copy_prefix(0, [1, 2, 3, 4], P)
    got = eng.forward_slots(torch.cat([p[P:] for p in ps]), [n - P for n in lens], list(range(B)), prompt_phase=True, pos0=P)
    kv_got = caches(eng, cfg, B, S)
    assert torch.equal(got, want), "logits_last behind a copied prefix differ from the packed forward's"
    for l in range(cfg.n_layer):
        for w in range(2):
            for i, n in enumerate(lens):
                # whole tiles up to the sequence's last one: the positions behind its length are zero in both runs
                t = -(-n // 32) * 32 * hs
                assert torch.equal(kv_got[l][w][i, :, :t], kv_want[l][w][i, :, :t]), f"layer {l} cache {w} sequence {i}"
                assert kv_want[l][w][i, :, :t].any()


# ---- 3. generate_batch ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(HEAD_SIZES))
def model(request):
    return build(request.param)


def test_generate_batch_same_ids_fewer_tokens(model):
    cfg, m = model
    ps = sharing_prompts(cfg, [1, 24, 7, 16, 2, 20, 11, 5, 24])          # 9 ragged prompts, 81 .. 104 tokens
    lens = [p.numel() for p in ps]
    for kw in (dict(temperature=0.2, top_k=1), dict(temperature=0.8, top_k=5, seed=4242)):
        t0, t1 = {}, {}
        want = [o.clone() for o in generate_batch(m, ps, NEW, prefill_batch=4, share_prefix=False, timing=t0, **kw)]
        got = [o.clone() for o in generate_batch(m, ps, NEW, prefill_batch=4, share_prefix=True, timing=t1, **kw)]
        assert t1["shared_prefix"] == P and t0["shared_prefix"] == 0
        assert same(want, got), f"{kw}: ids with a shared prefix differ"
        assert all(o.numel() == n + NEW for o, n in zip(got, lens))
        assert t1["prefill_tokens"] == sum(lens) - (len(ps) - 1) * P and t0["prefill_tokens"] == sum(lens)
    assert not same(want, [o.clone() for o in generate_batch(m, ps, NEW, prefill_batch=4, temperature=0.8, top_k=5, seed=4243)])
    # "auto" shares too, and an eos changes nothing about that
    eos = int(want[3][lens[3] + 5])
    t2 = {}
    assert same([o.clone() for o in generate_batch(m, ps, NEW, prefill_batch=4, eos_id=eos, **kw)],
                generate_batch(m, ps, NEW, prefill_batch=4, eos_id=eos, share_prefix="auto", timing=t2, **kw))
    assert t2["shared_prefix"] == P


# ---- 4. generate_stream: the prefix outlives the refills -------------------------------------------------------------------------
def n_generated(free, prompts, eos, new=NEW):
    out = []
    for o, p in zip(free, prompts):
        hit = (o[p.numel():] == eos).nonzero().flatten()
        out.append(int(hit[0]) + 1 if hit.numel() else new)
    return out


def early_eos(free, prompts, vocab):
    """the token of the EOS-free run that ends the most sequences in the first half of the budget while one runs to the end"""
    best, best_n = None, 0
    for eos in range(vocab):
        g = n_generated(free, prompts, eos)
        early = sum(a <= NEW // 2 for a in g)
        if max(g) == NEW and early > best_n:
            best, best_n = eos, early
    return best


@pytest.mark.parametrize("fp8", [False, True])
def test_generate_stream_prefix_survives_refills(fp8):
    cfg, m = build("parity-hs128", fp8=fp8)
    ps = sharing_prompts(cfg, [1 + (7 * i) % 40 for i in range(40)])
    lens = [p.numel() for p in ps]
    free = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1)]
    eos = early_eos(free, ps, cfg.padded_vocab_size)
    assert eos is not None, "no token ends a sequence early"
    g = n_generated(free, ps, eos)
    sim = predict(g, NEW, 8, 4, fp8=fp8)
    print(f"fp8 {fp8}: eos {eos}, tokens generated {sorted(g)}, {sim.prefill_calls} prefills through 8 rows")
    assert min(g) <= NEW // 2 and sim.prefill_calls >= 10, "slots must be refilled several times"
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, share_prefix=False)]
    tm = {}
    got = generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=8, prefill_batch=4, share_prefix=True, timing=tm)
    assert tm["shared_prefix"] == P and tm["prefill_tokens"] == sum(lens) - (len(ps) - 1) * P
    bad = [i for i, (a, b) in enumerate(zip(want, got)) if not torch.equal(a, b)]
    assert not bad, f"sequences {bad} differ from generate_batch(share_prefix=False)"
    assert tm["decode_row_steps"] == sim.decode_row_steps
    # sampled, and against the unshared stream
    kw = dict(temperature=0.8, top_k=5, seed=99, eos_id=eos, max_rows=8, prefill_batch=4)
    assert same([o.clone() for o in generate_stream(m, ps, NEW, **kw)], generate_stream(m, ps, NEW, share_prefix="auto", **kw))


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
def test_edges(model):
    cfg, m = model
    kw = dict(temperature=0.2, top_k=1)
    # one prompt is the first 65 tokens of the others: P = 64, and a one-token remainder for it (alone in its prefill chunk too)
    ps = sharing_prompts(cfg, [1, 9, 25, 12])              # up to 105 tokens: 24 more fit parity-tiny's 128 positions
    ps = [ps[1], ps[2], ps[2][:65], ps[3]]
    for pb in (4, 2, 1):
        tm = {}
        want = [o.clone() for o in generate_batch(m, ps, NEW, prefill_batch=pb, **kw)]
        assert same(want, generate_batch(m, ps, NEW, prefill_batch=pb, share_prefix=True, timing=tm, **kw))
        assert tm["shared_prefix"] == P
        tm = {}
        assert same(want, generate_stream(m, ps, NEW, max_rows=2, prefill_batch=pb, share_prefix=True, timing=tm, **kw))
        assert tm["shared_prefix"] == P
    # a common prefix of 20 tokens: nothing is shared
    ps = sharing_prompts(cfg, [30, 41, 35], shared=20)
    tm, ts = {}, {}
    want = [o.clone() for o in generate_batch(m, ps, NEW, **kw)]
    assert same(want, generate_batch(m, ps, NEW, share_prefix=True, timing=tm, **kw))
    assert same(want, generate_stream(m, ps, NEW, max_rows=2, share_prefix=True, timing=ts, **kw))
    assert tm["shared_prefix"] == 0 == ts["shared_prefix"] and tm["prefill_tokens"] == ts["prefill_tokens"] == sum(p.numel() for p in ps)
    # B = 1: the prompt's own first tokens (101 - 1, whole tiles: 96), nothing to copy
    ps = sharing_prompts(cfg, [21])
    tm, ts = {}, {}
    want = [o.clone() for o in generate_batch(m, ps, NEW, **kw)]
    assert same(want, generate_batch(m, ps, NEW, share_prefix=True, timing=tm, **kw))
    assert same(want, generate_stream(m, ps, NEW, share_prefix=True, timing=ts, **kw))
    assert tm["shared_prefix"] == 96 == ts["shared_prefix"] and tm["prefill_tokens"] == ts["prefill_tokens"] == 101
    # the two refusals of the GPU path: the CPU-rsqrt emulation raises with True and runs unshared with "auto"
    ps = sharing_prompts(cfg, [3, 8])
    m.cpu_rsqrt_vec_width = 32
    try:
        with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
            generate_batch(m, ps, 4, share_prefix=True, **kw)
        tm = {}
        assert same([o.clone() for o in generate_batch(m, ps, 4, **kw)], generate_batch(m, ps, 4, share_prefix="auto", timing=tm, **kw))
        assert tm["shared_prefix"] == 0
    finally:
        m.cpu_rsqrt_vec_width = 0


# ---- 6. the harness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["DualHyp", "GER"])
def test_harness_share_prefix_flag_changes_nothing(tmp_path, fmt):
    """the fixture corpus of tests/test_harness.py (a decoder that answers "up down": corpus WER 9/17) through the CLI with
    --share_prefix auto and without, under both schedules: the same predictions file, the known WER"""
    import subprocess
    sys.path.insert(0, str(ROOT / "tests"))
    import test_harness as H
    from dualhyp_amd.data import HypothesesDataset
    from dualhyp_amd.schedule import shared_prefix_len
    from dualhyp_amd.tokenizer import ByteTokenizer
    items = H.merged_items(caps=H.CAPTIONS)
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    # the corpus does share something: the template's instruction and header, in byte tokens
    ds = HypothesesDataset(str(test_json), ByteTokenizer(), prompts_format=fmt, seed=1337)
    shared = shared_prefix_len([ds[i]["input_ids_no_response"] for i in range(len(ds))])
    print(f"{fmt}: the 7 prompts share {shared} leading byte tokens (whole tiles)")
    assert shared >= 32
    ckpt_dir = tmp_path / "checkpoints" / "parity-harness"
    ckpt_dir.mkdir(parents=True)
    cfg = Config.from_name("parity-harness", r=16, alpha=16, dropout=0.05, to_query=True, to_key=True, to_value=True, to_projection=True)
    files = {}
    for tag, extra in (("off", []), ("auto", ["--share_prefix", "auto"]), ("auto_continuous", ["--share_prefix", "auto", "--schedule", "continuous"])):
        run_dir = tmp_path / "runs" / tag
        run_dir.mkdir(parents=True)
        torch.save({"model": H.speaking_state_dict(cfg, seed=31)}, run_dir / "best_model.pth")
        cmd = [sys.executable, "-m", "dualhyp_amd.inference", "--test_path", str(test_json), "--model_path", str(run_dir / "best_model.pth"),
               "--llm_checkpoint", str(ckpt_dir), "--prompts_format", fmt, "--tokenizer", "byte", "--max_new_tokens", str(H.NEW),
               "--decode_batch", "4"] + extra + (["--dual_hypotheses"] if fmt == "DualHyp" else [])
        out = subprocess.run(cmd, cwd=tmp_path, env=H._env(), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        files[tag] = json.loads((run_dir / "predictions" / "best_model.json").read_text())
    assert files["auto"] == files["off"] and files["auto_continuous"] == files["off"]
    js = files["auto"]
    assert len(js) == 7 + 2 and [p["inference"] for p in js[:7]] == [H.SAYS] * 7
    assert js[-2]["wer"] == pytest.approx(H.WANT_WER) and js[-2]["gtms"] == f"{H.WANT_EXACT}/7"
