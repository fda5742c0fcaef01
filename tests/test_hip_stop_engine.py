"""Stop conditions through the engine on the GPU (include/dualhyp_hip.h, "Stop conditions").  Every check is exact.

generate_batch runs once unstopped; the specification is built from that run's own ids, so dualhyp_amd.stop.first_stop says where every
sequence must stop.  The stopped call's tokens, lengths, log-probabilities and alternatives are the unstopped prefixes through that
position, with nothing behind it and done = 3; then the same state, bit for bit, under the other schedules and features."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, quantize_model_fp8  # noqa: E402
from dualhyp_amd.stop import compile_stop, finish_reasons, first_stop  # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NEW = 16
GREEDY = dict(temperature=1.0, top_k=1)
TOP5 = dict(temperature=0.8, top_k=5, seed=4242)
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
LENS = (1, 31, 33, 47)
FULL = dict(return_logprobs=True, top_logprobs=3, return_state=True)
KEYS = ("tokens", "length", "done", "logprobs", "top_ids", "top_logprobs")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def build(name, seed=11):
    cfg = Config.from_name(name, **LORA)
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=BF)
    m.load_state_dict(sd)
    m.eval()
    return cfg, m


@pytest.fixture(scope="module")
def tiny():
    return build("parity-tiny")


def ragged_prompts(cfg, seed=70):
    return [synth_prompts(1, n, cfg.padded_vocab_size, seed=seed + i)[0].to(DEV) for i, n in enumerate(LENS)]


def state_of(res):
    """the state dict of a (out, logprobs, top, state) result, cloned: the buffers are the call's own"""
    return {k: res[-1][k].clone() for k in KEYS}


def same_state(a, b, what):
    for k in KEYS:
        assert (same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k])), f"{what}: {k}\n{a[k]}\n{b[k]}"


def texts_of(st, lens):
    tok, n = st["tokens"].tolist(), st["length"].tolist()
    return [tok[u][lens[u]:n[u]] for u in range(len(lens))]


def spec_entries(texts):
    """the issue's specification: the token each sequence generated at position 3 + u, and one bigram from positions (6, 7)"""
    return [texts[u][3 + u] for u in range(len(texts))] + [texts[len(texts) - 1][6:8]]


def check_cut(free, got, lens, spec, eos, what):
    """`got` is `free` cut behind first_stop: -> the first stops"""
    stops = []
    B, tok_ld = free["tokens"].shape
    for u, (p, g) in enumerate(zip(lens, texts_of(free, lens))):
        fs = first_stop(g, spec)
        if fs is not None and eos is not None and g[fs] == eos:
            fs = None
        stops.append(fs)
        n = int(free["length"][u]) if fs is None else p + fs + 1
        w = f"{what}: sequence {u}, first stop {fs}"
        assert int(got["length"][u]) == n and int(got["done"][u]) == (int(free["done"][u]) if fs is None else 3), w
        assert torch.equal(got["tokens"][u, :n], free["tokens"][u, :n]) and not got["tokens"][u, n:].any(), w
        assert same_bits(got["logprobs"][u, p:n], free["logprobs"][u, p:n]) and bool(got["logprobs"][u, n:].isnan().all()), w
        assert torch.equal(got["top_ids"][u, p:n], free["top_ids"][u, p:n]) and bool((got["top_ids"][u, n:] == -1).all()), w
        assert same_bits(got["top_logprobs"][u, p:n], free["top_logprobs"][u, p:n]) and bool(got["top_logprobs"][u, n:].isnan().all()), w
        assert not got["logprobs"][u, p:n].isnan().any(), w
    return stops


def check_inputs(stops):
    """the condition on the inputs: at least three of the four sequences stop before their budget, at two or more different steps"""
    early = [s for s in stops if s is not None and s < NEW - 1]
    assert len(early) >= 3 and len(set(early)) >= 2, stops


def check_returned(res, st, lens):
    """the returned lists are the state's rows: the stopping token stays in the ids, with its log-probability and alternatives"""
    out, lp, top = res[0], res[1], res[2]
    for u, p in enumerate(lens):
        n = int(st["length"][u]) - (1 if int(st["done"][u]) == 1 else 0)
        assert torch.equal(out[u], st["tokens"][u, :n])
        assert same_bits(lp[u], st["logprobs"][u, p:int(st["length"][u])]) and torch.equal(top[u][0], st["top_ids"][u, p:int(st["length"][u])])


@pytest.mark.parametrize("kw", (GREEDY, TOP5), ids=("greedy", "top_k=5"))
def test_stopped_call_is_the_unstopped_prefix(tiny, kw):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    free = state_of(generate_batch(m, ps, NEW, **FULL, **kw))
    texts = texts_of(free, lens)
    assert all(len(g) == NEW for g in texts) and all(d in (0, 2) for d in free["done"].tolist())
    entries = spec_entries(texts)
    spec = compile_stop(entries[:-1], entries[-1:], V, DEV)
    res = generate_batch(m, ps, NEW, stop=spec, **FULL, **kw)
    want = state_of(res)
    stops = check_cut(free, want, lens, spec, None, "generate_batch")
    check_inputs(stops)
    check_returned(res, want, lens)
    assert finish_reasons(want["done"]) == ["stop" if s is not None else "length" for s in stops]
    # the list form of the argument is the compiled one
    same_state(want, state_of(generate_batch(m, ps, NEW, stop=entries, **FULL, **kw)), "list form")
    # stop sequences alone, so that a sequence match (not the set) is what ends sequences inside the captured steps: a bigram at (6, 7),
    # a trigram at (2, 3, 4), an eight-token sequence at (4 .. 11)
    seqs = [texts[0][6:8], texts[1][2:5], texts[2][4:12]]
    spec2 = compile_stop([], seqs, V, DEV)
    got = state_of(generate_batch(m, ps, NEW, stop=spec2, **FULL, **kw))
    stops2 = check_cut(free, got, lens, spec2, None, "sequences only")
    assert stops2[0] is not None and stops2[0] <= 7 and stops2[1] is not None and stops2[1] <= 4 and stops2[2] is not None and stops2[2] <= 11
    # continuous batching: fewer rows than prompts, so a stopped sequence hands its slot on
    res = generate_stream(m, ps, NEW, max_rows=2, check_every=3, stop=spec, **FULL, **kw)
    same_state(want, state_of(res), "generate_stream")
    check_returned(res, want, lens)
    same_state(got, state_of(generate_stream(m, ps, NEW, max_rows=2, check_every=3, stop=spec2, **FULL, **kw)), "generate_stream, sequences")
    # a plain call behind them is the call it always was, and nothing is left on the engine
    same_state(free, state_of(generate_batch(m, ps, NEW, **FULL, **kw)), "the plain call behind stopped ones")
    assert m._engine._stop is None
    # generate() forwards the argument
    if kw is GREEDY:
        one = generate(m, ps[2], ps[2].numel() + NEW, stop=spec, **kw)
        assert torch.equal(one, want["tokens"][2, :int(want["length"][2])])


def test_stop_on_the_first_token_and_with_an_eos(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    first = state_of(generate_batch(m, ps, NEW, **FULL, **GREEDY))
    texts = texts_of(first, lens)
    eos = texts[1][5]
    free = state_of(generate_batch(m, ps, NEW, eos_id=eos, **FULL, **GREEDY))
    # the prefill's pick of sequence 0 stops it; the EOS of sequence 1 is a stop id too and wins; sequence 2 stops at 9
    spec = compile_stop([texts[0][0], eos, texts[2][9]], [], V, DEV)
    got = state_of(generate_batch(m, ps, NEW, eos_id=eos, stop=spec, **FULL, **GREEDY))
    stops = check_cut(free, got, lens, spec, eos, "eos and stop")
    assert stops[0] == 0 and int(got["done"][0]) == 3 and int(got["length"][0]) == lens[0] + 1
    assert int(got["done"][1]) == 1 and stops[1] is None
    same_state(got, state_of(generate_stream(m, ps, NEW, eos_id=eos, max_rows=2, check_every=3, stop=spec, **FULL, **GREEDY)), "stream")


@pytest.mark.parametrize("kw", (GREEDY, TOP5), ids=("greedy", "top_k=5"))
def test_share_prefix(tiny, kw):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 33)]
    lens = [int(p.numel()) for p in ps]
    free = state_of(generate_batch(m, ps, NEW, **FULL, **kw))
    entries = spec_entries(texts_of(free, lens))
    spec = compile_stop(entries[:-1], entries[-1:], V, DEV)
    want = state_of(generate_batch(m, ps, NEW, stop=spec, **FULL, **kw))
    check_inputs(check_cut(free, want, lens, spec, None, "unshared"))
    tm = {}
    same_state(want, state_of(generate_batch(m, ps, NEW, stop=spec, share_prefix=True, timing=tm, **FULL, **kw)), "share_prefix")
    assert tm["shared_prefix"] == 32
    same_state(want, state_of(generate_stream(m, ps, NEW, stop=spec, share_prefix=True, max_rows=3, check_every=5, **FULL, **kw)),
               "share_prefix stream")


def test_speculate(tiny):
    """the stop lands inside a verify step: with the right drafts a step would append four tokens, and the stopping one is the last"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    free = state_of(generate_batch(m, ps, NEW, **FULL, **GREEDY))
    texts = texts_of(free, lens)
    entries = spec_entries(texts)
    spec = compile_stop(entries[:-1], entries[-1:], V, DEV)
    want = state_of(generate_batch(m, ps, NEW, stop=spec, **FULL, **GREEDY))
    stops = check_cut(free, want, lens, spec, None, "speculate=0")
    check_inputs(stops)
    assert any(s is not None and s % 4 != 0 for s in stops), "no stop lies inside a verify step of four positions"
    right = torch.tensor(texts, dtype=torch.int64, device=DEV)
    tm = {}
    same_state(want, state_of(generate_batch(m, ps, NEW, stop=spec, speculate=3, drafts=right, timing=tm, **FULL, **GREEDY)), "right drafts")
    assert tm["spec_accepted"] > 0
    wrong = ((right + 1) % V).contiguous()
    tm = {}
    same_state(want, state_of(generate_batch(m, ps, NEW, stop=spec, speculate=3, drafts=wrong, timing=tm, **FULL, **GREEDY)), "wrong drafts")
    assert tm["spec_accepted"] == 0
    same_state(want, state_of(generate_batch(m, ps, NEW, stop=spec, speculate=3, **FULL, **GREEDY)), "prompt lookup")
    # stop sequences across verify steps: the window is loaded from what earlier launches wrote and shifted with each pick
    seqs = [texts[0][6:8], texts[1][2:5], texts[2][4:12], texts[3][3:6]]
    spec2 = compile_stop([], seqs, V, DEV)
    want2 = state_of(generate_batch(m, ps, NEW, stop=spec2, **FULL, **GREEDY))
    check_cut(free, want2, lens, spec2, None, "sequences, speculate=0")
    same_state(want2, state_of(generate_batch(m, ps, NEW, stop=spec2, speculate=3, drafts=right, **FULL, **GREEDY)), "sequences, right drafts")
    same_state(want2, state_of(generate_batch(m, ps, NEW, stop=spec2, speculate=3, drafts=wrong, **FULL, **GREEDY)), "sequences, wrong drafts")
    # the plain verify steps behind them are what they always were (their own budget flags: every sequence has a limit there)
    plain = state_of(generate_batch(m, ps, NEW, speculate=3, drafts=right, **FULL, **GREEDY))
    assert plain["done"].tolist() == [2] * 4
    same_state(dict(free, done=plain["done"]), plain, "the plain verify steps behind them")


def test_token_mask_and_no_repeat_ngram(tiny):
    """the expected result is those features' own unstopped output, cut"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    allowed = np.zeros((len(ps), V), dtype=bool)
    g = np.random.default_rng(3)
    for u in range(len(ps)):
        allowed[u, g.choice(V, 24, replace=False)] = True               # 24 ids each: no fallback under n = 2 within 16 tokens
    mask = CR.pack_bits(allowed).to(DEV)
    more = dict(token_mask=mask, no_repeat_ngram=2)
    for kw in (GREEDY, TOP5):
        free = state_of(generate_batch(m, ps, NEW, **more, **FULL, **kw))
        texts = texts_of(free, lens)
        assert all(allowed[u][t] for u, t_ in enumerate(texts) for t in t_)
        entries = spec_entries(texts)
        spec = compile_stop(entries[:-1], entries[-1:], V, DEV)
        want = state_of(generate_batch(m, ps, NEW, stop=spec, **more, **FULL, **kw))
        check_inputs(check_cut(free, want, lens, spec, None, f"mask and ban {kw}"))
        same_state(want, state_of(generate_stream(m, ps, NEW, max_rows=2, check_every=3, stop=spec, **more, **FULL, **kw)), "stream")


def test_fp8_model_with_fp8_cache():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.fp8 and m.kv_cache_dtype == "fp8"
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    free = state_of(generate_batch(m, ps, NEW, **FULL, **GREEDY))
    texts = texts_of(free, lens)
    entries = spec_entries(texts)
    spec = compile_stop(entries[:-1] , entries[-1:] + [texts[0][1:3]], V, DEV)
    want = state_of(generate_batch(m, ps, NEW, stop=spec, **FULL, **GREEDY))
    check_inputs(check_cut(free, want, lens, spec, None, "fp8"))
    same_state(want, state_of(generate_stream(m, ps, NEW, max_rows=2, check_every=3, stop=spec, **FULL, **GREEDY)), "fp8 stream")


def test_the_saved_steps(tiny):
    """with an EOS that never comes, 40 new tokens take 39 decode steps; when every sequence stops within its first 8 tokens the loop
    ends behind its first EOS_CHECK_EVERY chunk"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    lens = list(LENS)
    first = generate_batch(m, ps, 40, **GREEDY)
    texts = [o[p.numel():].tolist() for o, p in zip(first, ps)]
    eos = next(t for t in range(V) if all(t not in g for g in texts))
    spec = compile_stop([texts[u][3 + u] for u in range(4)], [], V, DEV)
    assert all(first_stop(g, spec) < 8 for g in texts)
    tm_free, tm = {}, {}
    free = generate_batch(m, ps, 40, eos_id=eos, timing=tm_free, **GREEDY)
    free = [o.clone() for o in free]
    out, st = generate_batch(m, ps, 40, eos_id=eos, stop=spec, timing=tm, return_state=True, **GREEDY)
    assert tm_free["decode_steps"] == 39 and tm["decode_steps"] == 16
    assert st["done"].tolist() == [3] * 4
    for o, f, p, g in zip(out, free, ps, texts):
        n = p.numel() + first_stop(g, spec) + 1
        assert torch.equal(o, f[:n])


# ---- the serving CLI ------------------------------------------------------------------------------------------------------------------
def test_inference_cli_stop(tmp_path, monkeypatch):
    """`python -m dualhyp_amd.inference --stop newline --stop_file F --schedule continuous --logprobs` end to end (in this process)
    against the plain run: every utterance's ids are the plain run's cut behind first_stop, every record says why it ended, and the
    text of a record that did not stop is the plain run's"""
    import importlib
    import json
    import test_harness as harness
    from dualhyp_amd import inference
    from dualhyp_amd.tokenizer import ByteTokenizer
    G = importlib.import_module("dualhyp_amd.generate")        # the package's attribute of that name is the function
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    base = ["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
            "DualHyp", "--dual_hypotheses", "--max_new_tokens", "12"]
    seen = {}

    def spy(name):
        real = getattr(G, name)

        def call(model, prompts, max_new, **kw):
            res = real(model, prompts, max_new, **kw)
            outs = res[0] if isinstance(res, tuple) else res
            seen.setdefault(name, []).append(([p.cpu() for p in prompts], kw.get("stop"), [o.cpu() for o in outs]))
            return res
        return call

    monkeypatch.setattr(G, "generate_batch", spy("generate_batch"))
    monkeypatch.setattr(G, "generate_stream", spy("generate_stream"))
    inference.main(base + ["--decode_batch", str(len(items)), "--predict_dir", str(tmp_path / "plain")])
    plain = json.loads((tmp_path / "plain" / "random_init.json").read_text())
    (prompts, no_stop, free), = seen["generate_batch"]
    assert no_stop is None and all("finish_reason" not in rec for rec in plain[:-2])
    texts = [o[p.numel():].tolist() for p, o in zip(prompts, free)]
    # stop ids: what the first utterances generate third; a stop sequence: the bigram another one generates at (4, 5)
    stop_file = tmp_path / "stop.txt"
    ids, bigram = sorted({g[2] for g in texts[:3]}), texts[-1][4:6]
    stop_file.write_text("# test\n" + "".join(f"{t}\n" for t in ids) + " ".join(str(t) for t in bigram) + "\n")
    inference.main(base + ["--decode_batch", "4", "--schedule", "continuous", "--logprobs", "--stop", "newline", "--stop_file", str(stop_file),
                           "--predict_dir", str(tmp_path / "stopped")])
    js = json.loads((tmp_path / "stopped" / "random_init.json").read_text())
    (prompts2, spec, outs), = seen["generate_stream"]
    nl = ByteTokenizer().encode("\n")[-1]
    assert spec.ids == tuple(sorted(set(ids) | {nl})) and spec.sequences == (tuple(bigram),)
    assert len(js) == len(items) + 2 and len(outs) == len(texts)
    n_stop = 0
    for rec, old, p, o, g in zip(js[:-2], plain[:-2], prompts2, outs, texts):
        fs = first_stop(g, spec)
        assert o[p.numel():].tolist() == (g if fs is None else g[:fs + 1])
        # an unstopped utterance ended as in the plain run: on its EOS (which the ids leave out) or on its 12 tokens
        assert rec["finish_reason"] == ("stop" if fs is not None else "eos" if len(g) < 12 else rec["finish_reason"]) and "sum_logprob" in rec
        assert rec["finish_reason"] in ("stop", "eos", "length")
        if fs is None or g[fs] == nl:
            assert rec["inference"] == old["inference"]
        n_stop += fs is not None
    assert n_stop >= 3
