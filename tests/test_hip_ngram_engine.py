"""No-repeat n-grams through the engine on the GPU (include/dualhyp_hip.h, "No-repeat n-grams").  Every check is exact.

The reference is the existing constrained path stepped from the host: the same prefill and first pick, then one eng.decode(..., 1,
first_step=t) per token, the contents of the set_token_mask rows rewritten before each step to "base mask minus banned_t, with the
fallback" (ngram_reference.pick_rows on the tokens read back).  Both sides run the same forward kernels, so ids, log-probabilities and
alternatives are bit-equal, for the greedy pick and for top_k = 5 with a fixed seed.  Then the schedules: generate_stream with fewer
rows than prompts, share_prefix, verify steps with scripted and looked-up drafts — the same ids and log-probabilities."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
import ngram_reference as R  # noqa: E402
from dualhyp_amd import GPT, Config, beam_search_batch, generate, generate_batch, generate_stream, ngram, ops, quantize_model_fp8  # noqa: E402
from dualhyp_amd import _lib  # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NEW = 16
GREEDY = dict(temperature=1.0, top_k=1)
TOP5 = dict(temperature=0.8, top_k=5, seed=4242)
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
LENS = (1, 31, 33, 47)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_lists(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and (same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y))
                                    for x, y in zip(a, b))


def same_top(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and same_bits(x[1], y[1]) for x, y in zip(a, b))


def same_result(want, got):
    return same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])


def clone_all(res):
    return [[o.clone() for o in res[0]], [v.clone() for v in res[1]], [(a.clone(), b.clone()) for a, b in res[2]]]


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


def three_id_masks(m, ps, V):
    """(bool [B, V], eos): sequence u may produce three ids — its three most probable first tokens, so the picks are not ties among
    -inf — and the EOS, an id outside all of them, is never produced."""
    _, _, top = generate_batch(m, ps, 1, return_logprobs=True, top_logprobs=3, **GREEDY)
    allowed = np.zeros((len(ps), V), dtype=bool)
    for u in range(len(ps)):
        allowed[u, top[u][0][0].tolist()] = True
    eos = int(np.flatnonzero(~allowed.any(axis=0))[0])
    return allowed, eos


def host_stepped(m, ps, new, n, base, eos, kw, K):
    """generate_batch(no_repeat_ngram=n, token_mask=base, return_logprobs, top_logprobs=K, return_state) by the constrained path alone:
    -> the state dict of generate_batch (tokens, length, done, logprobs, top_ids, top_logprobs)"""
    B, V = len(ps), m.config.padded_vocab_size
    lens = [int(p.numel()) for p in ps]
    tok_ld = max(lens) + new
    tokens = torch.nn.utils.rnn.pad_sequence(list(ps), batch_first=True)
    tokens = torch.nn.functional.pad(tokens, (0, tok_ld - tokens.size(1))).contiguous()
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    lp = torch.full((B, tok_ld), float("nan"), dtype=torch.float32, device=DEV)
    top = (torch.full((B, tok_ld, K), -1, dtype=torch.int32, device=DEV), torch.full((B, tok_ld, K), float("nan"), dtype=torch.float32, device=DEV))
    seed = kw.get("seed", 1337)
    eng = m.engine(B, max(lens) + new - 1, sum(lens))
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    _, last = eng.forward(torch.cat(list(ps)), lens, [0] * B, want_all=False, want_last=True, slot_base=0)
    mask = CR.pack_bits(R.pick_rows(base, [[]] * B, n, V)).to(DEV)          # nothing generated: the base mask, or all ones
    ops.sample(last, tokens, length, done, temperature=kw["temperature"], top_k=kw["top_k"], eos_id=eos, seed=seed, step=0, logprobs=lp,
               top_logprobs=top, mask=mask)
    eng.set_logprobs(lp)
    eng.set_top_logprobs(*top)
    eng.set_token_mask(mask)
    fallbacks = 0
    try:
        for t in range(new - 1):
            tok_h, len_h = tokens.tolist(), length.tolist()
            texts = [tok_h[u][lens[u]:len_h[u]] for u in range(B)]
            fallbacks += sum(R.pick_row(None if base is None else base[u], texts[u], n, V)[1] for u in range(B))
            mask.copy_(CR.pack_bits(R.pick_rows(base, texts, n, V)).to(DEV))    # the same storage: the captured step reads it when it runs
            eng.decode(tokens, length, done, 1, kw["temperature"], kw["top_k"], eos, seed, first_step=t)
    finally:
        eng.set_logprobs(None)
        eng.set_top_logprobs(None)
        eng.set_token_mask(None)
    m._cache_len = []
    return dict(tokens=tokens, length=length, done=done, logprobs=lp, top_ids=top[0], top_logprobs=top[1], fallbacks=fallbacks)


def check_against_host(m, ps, n, base, eos, kw, what, K=3):
    V = m.config.padded_vocab_size
    want = host_stepped(m, ps, NEW, n, base, eos, kw, K)
    mask = None if base is None else CR.pack_bits(base).to(DEV)
    out, lp, top, st = generate_batch(m, ps, NEW, eos_id=eos, token_mask=mask, no_repeat_ngram=n, return_logprobs=True, top_logprobs=K,
                                      return_state=True, **kw)
    for key in ("tokens", "length", "done", "top_ids"):
        assert torch.equal(st[key], want[key]), f"{what}: {key}\n{st[key]}\n{want[key]}"
    assert same_bits(st["logprobs"], want["logprobs"]) and same_bits(st["top_logprobs"], want["top_logprobs"]), what
    texts = [o[p.numel():].tolist() for o, p in zip(out, ps)]
    return texts, want["fallbacks"]


def check_picks_outside_their_ban_sets(texts, n, base, V, what):
    """no pick lies in its ban set, except where the fallback applied; -> picks with a non-empty ban set"""
    bans = 0
    for u, g in enumerate(texts):
        for t, tok in enumerate(g):
            b = R.banned(g[:t], n)
            bans += bool(b)
            if tok in b:
                assert R.pick_row(None if base is None else base[u], g[:t], n, V)[1], f"{what}: sequence {u} picked the banned {tok} at {t} of {g}"
    return bans


@pytest.mark.parametrize("kw", (GREEDY, TOP5), ids=("greedy", "top_k=5"))
def test_tiny_against_the_host_stepped_constrained_path(tiny, kw):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    # the free-running case: equality only
    for n in (1, 3):
        check_against_host(m, ps, n, None, None, kw, f"unmasked n={n}")
    # three allowed ids, the EOS not among them, n = 2: among the first four tokens an id repeats, so by the fifth pick a ban set is
    # non-empty
    base, eos = three_id_masks(m, ps, V)
    texts, _ = check_against_host(m, ps, 2, base, eos, kw, "three ids n=2")
    texts2 = texts
    for u, g in enumerate(texts):
        assert len(g) == NEW and all(base[u][t] for t in g)
        assert len(ngram.ban_positions(g, 2)) >= 1 and min(ngram.ban_positions(g, 2)) <= 4, f"sequence {u}: {g}"
        assert ngram.ban_positions(g, 2) == R.ban_positions(g, 2)
    assert check_picks_outside_their_ban_sets(texts, 2, base, V, "three ids n=2") >= len(ps)
    # n = 1 over three ids: from the fourth pick on everything allowed is banned — the fallback, step after step
    texts, fallbacks = check_against_host(m, ps, 1, base, eos, kw, "three ids n=1")
    assert fallbacks >= len(ps) * (NEW - 4)
    for g in texts:
        assert len(set(g[:3])) == 3
    check_picks_outside_their_ban_sets(texts, 1, base, V, "three ids n=1")
    # the ban moves picks: the feature-off run under the same masks repeats a bigram somewhere
    off = generate_batch(m, ps, NEW, eos_id=eos, token_mask=CR.pack_bits(base).to(DEV), **kw)
    assert any(o[p.numel():].tolist() != g for o, p, g in zip(off, ps, texts2))


@pytest.mark.parametrize("name", ("parity-hs96", "parity-hs128", "fp8"))
def test_other_engines_against_the_host_stepped_constrained_path(name):
    cfg, m = build("parity-hs128" if name == "fp8" else name)
    if name == "fp8":
        quantize_model_fp8(m, kv_cache="fp8")
        assert m.fp8 and m.kv_cache_dtype == "fp8"
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)[:3]
    base, eos = three_id_masks(m, ps, V)
    texts, _ = check_against_host(m, ps, 2, base, eos, GREEDY, name)
    assert all(len(ngram.ban_positions(g, 2)) >= 1 for g in texts)
    check_picks_outside_their_ban_sets(texts, 2, base, V, name)
    check_against_host(m, ps, 3, None, None, TOP5, f"{name} unmasked")


def test_schedules_agree(tiny):
    """generate_stream with fewer rows than prompts, share_prefix, and verify steps give generate_batch's ids, log-probabilities and
    alternatives"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 33, 50)]
    base, eos = three_id_masks(m, ps, V)
    mask = CR.pack_bits(base).to(DEV)
    for n, tm_kw, what in ((2, dict(token_mask=mask, eos_id=eos), "three ids"), (3, dict(), "unmasked")):
        kw = dict(return_logprobs=True, top_logprobs=3, no_repeat_ngram=n, **tm_kw, **GREEDY)
        want = clone_all(generate_batch(m, ps, NEW, **kw))
        texts = [o[p.numel():].tolist() for o, p in zip(want[0], ps)]
        check_picks_outside_their_ban_sets(texts, n, base if tm_kw else None, V, what)
        runs = {"stream": generate_stream(m, ps, NEW, max_rows=2, check_every=3, **kw)}
        tm = {}
        runs["share_prefix"] = generate_batch(m, ps, NEW, share_prefix=True, timing=tm, **kw)
        assert tm["shared_prefix"] == 32
        runs["share_prefix stream"] = generate_stream(m, ps, NEW, share_prefix=True, max_rows=3, check_every=5, **kw)
        runs["speculate=3 prompt lookup"] = generate_batch(m, ps, NEW, speculate=3, **kw)
        for name, got in runs.items():
            assert same_result(want, got), f"{what}: {name}"
        # a sampled call: the draw is keyed by the sequence, not by where it was scheduled
        kw5 = dict(kw, **TOP5)
        assert same_result(clone_all(generate_batch(m, ps, NEW, **kw5)), generate_stream(m, ps, NEW, max_rows=2, check_every=3, **kw5)), what
    # scripted drafts under the three-id masks, n = 2
    kw = dict(return_logprobs=True, top_logprobs=3, token_mask=mask, eos_id=eos, **GREEDY)
    off = clone_all(generate_batch(m, ps, NEW, **kw))
    want = clone_all(generate_batch(m, ps, NEW, no_repeat_ngram=2, **kw))
    right_off = torch.stack([o[p.numel():] for o, p in zip(off[0], ps)]).contiguous()
    right_on = torch.stack([o[p.numel():] for o, p in zip(want[0], ps)]).contiguous()
    assert not torch.equal(right_off, right_on)                     # the ban bites
    # (a) the feature-off continuation: a banned draft is rejected where the ban bites
    tm = {}
    got = generate_batch(m, ps, NEW, no_repeat_ngram=2, speculate=3, drafts=right_off, timing=tm, **kw)
    assert same_result(want, got) and tm["spec_accepted"] < tm["spec_drafted"]
    accepted_off = tm["spec_accepted"]
    # (b) the feature-on continuation: every draft is accepted (so more than under (a): a wrong draft costs a step).  A verify step appends up to 4 tokens and the first token is the
    # prefill's, so with 16 new tokens the last step's third draft falls behind the budget; with 17 every drafted token has room
    tm = {}
    got = generate_batch(m, ps, NEW, no_repeat_ngram=2, speculate=3, drafts=right_on, timing=tm, **kw)
    assert same_result(want, got) and tm["spec_accepted"] == tm["spec_drafted"] - len(ps) > accepted_off and tm["spec_steps"] == 4
    want17 = clone_all(generate_batch(m, ps, NEW + 1, no_repeat_ngram=2, **kw))
    right17 = torch.stack([o[p.numel():] for o, p in zip(want17[0], ps)]).contiguous()
    tm = {}
    got = generate_batch(m, ps, NEW + 1, no_repeat_ngram=2, speculate=3, drafts=right17, timing=tm, **kw)
    assert same_result(want17, got) and tm["spec_accepted"] == tm["spec_drafted"] > 0 and tm["spec_steps"] == 4
    # with the feature off the same drafts are what they always were
    tm = {}
    got = generate_batch(m, ps, NEW, speculate=3, drafts=right_off, timing=tm, **kw)
    assert same_result(off, got)


def test_zero_is_the_call_without_the_argument(tiny):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    for kw in (GREEDY, TOP5):
        full = dict(return_logprobs=True, top_logprobs=3, **kw)
        want = clone_all(generate_batch(m, ps, NEW, **full))
        assert same_result(want, generate_batch(m, ps, NEW, no_repeat_ngram=0, **full))
        assert same_result(want, generate_stream(m, ps, NEW, max_rows=2, check_every=3, no_repeat_ngram=0, **full))
    one = generate(m, ps[2], ps[2].numel() + NEW, no_repeat_ngram=0, **GREEDY)
    assert torch.equal(one, generate_batch(m, ps, NEW, **GREEDY)[2])
    # generate() forwards the argument
    many = [o.clone() for o in generate_batch(m, ps, NEW, no_repeat_ngram=1, **GREEDY)]
    assert torch.equal(generate(m, ps[2], ps[2].numel() + NEW, no_repeat_ngram=1, **GREEDY), many[2])
    for o, p in zip(many, ps):
        g = o[p.numel():].tolist()
        assert len(set(g)) == len(g) == NEW                             # n = 1: no id twice


def test_graph_keys_and_refusals():
    """(ngram, start) is part of the captured step's key, as the mask pointer is: a plain step, n = 2, n = 3 and n = 2 with other prompt
    lengths capture one step each; asked for again, every step is found; generate_batch leaves the engine with the feature off; beam
    search refuses it"""
    cfg, m = build("parity-tiny")                                      # a model of its own: an engine keeps 8 captured steps
    ps = ragged_prompts(cfg)
    B, lens, steps = len(ps), [int(p.numel()) for p in ps], 8
    tok_ld = max(lens) + steps + 1
    eng = m.engine(B, max(lens) + steps, sum(lens), exact=True)
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    tokens0 = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(ps, batch_first=True), (0, tok_ld - max(lens))).contiguous()
    tokens, length, done = tokens0.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    starts = [torch.tensor(lens, dtype=torch.int32, device=DEV) for _ in range(2)]
    packed = torch.cat(ps)

    def run(n, start):
        tokens.copy_(tokens0)
        length.copy_(torch.tensor(lens, dtype=torch.int32))
        done.zero_()
        _, last = eng.forward(packed, lens, [0] * B, want_all=False, want_last=True, slot_base=0)
        ops.sample(last, tokens, length, done, seed=3, step=0, no_repeat_ngram=n, start=start, **GREEDY)
        eng.set_no_repeat_ngram(n, start)
        try:
            eng.decode(tokens, length, done, steps, GREEDY["temperature"], GREEDY["top_k"], None, 3, first_step=0)
        finally:
            eng.set_no_repeat_ngram(0)
        torch.cuda.synchronize()
        return dict(tokens=tokens.clone(), count=eng.graph_count(0))

    c0 = eng.graph_count(0)
    plain, two, three, other = run(0, None), run(2, starts[0]), run(3, starts[0]), run(2, starts[1])
    assert [x["count"] - c0 for x in (plain, two, three, other)] == [1, 2, 3, 4]
    plain2, two2 = run(0, None), run(2, starts[0])
    assert plain2["count"] == two2["count"] == other["count"]            # nothing new was captured: every step was found again
    assert torch.equal(plain2["tokens"], plain["tokens"]) and torch.equal(two2["tokens"], two["tokens"])
    assert torch.equal(other["tokens"], two["tokens"])
    for u, k in enumerate(lens):                                          # the steps picked under their own n
        for n, got in ((2, two), (3, three)):
            g = got["tokens"][u, k:k + steps + 1].tolist()
            assert all(g[t] not in R.banned(g[:t], n) for t in range(len(g))), (u, n, g)
    m.refresh_engine()
    # the serving entry point: a call with the feature, then the plain call it does not disturb, and nothing left behind
    want = [o.clone() for o in generate_batch(m, ps, NEW, **GREEDY)]
    eng = m._engine
    generate_batch(m, ps, NEW, no_repeat_ngram=2, **GREEDY)
    assert m._engine is eng and eng._ngram_start is None
    assert same_lists(want, generate_batch(m, ps, NEW, **GREEDY))
    with pytest.raises(ValueError, match="beam"):
        beam_search_batch(m, ps, 4, num_beams=2, no_repeat_ngram=2)
    start = starts[0]
    with pytest.raises(TypeError):
        eng.set_no_repeat_ngram(2, start.long())
    with pytest.raises(_lib.DualHypHipError, match="0 .. 8"):
        eng.set_no_repeat_ngram(9, start)
    with pytest.raises(_lib.DualHypHipError, match="start"):
        _lib.check(eng.lib.dh_engine_set_no_repeat_ngram(eng.handle, 2, None))
    assert eng._ngram_start is None
    assert same_lists(want, generate_batch(m, ps, NEW, **GREEDY))


# ---- the serving CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", (["--schedule", "batch", "--constrain", "prompt"], ["--schedule", "continuous", "--logprobs"]),
                         ids=("batch constrained", "continuous"))
def test_inference_cli_no_repeat_ngram(tmp_path, monkeypatch, more):
    """`python -m dualhyp_amd.inference --no_repeat_ngram 2` end to end (in this process): the entry point gets the argument, no
    utterance repeats a bigram outside a fallback step, and every record carries the count the host model gives for its ids"""
    import importlib
    import json
    import test_harness as harness
    from dualhyp_amd import inference
    G = importlib.import_module("dualhyp_amd.generate")        # the package's attribute of that name is the function
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    seen = []
    name = "generate_stream" if "continuous" in more else "generate_batch"
    real = getattr(G, name)

    def spy(model, prompts, max_new, **kw):
        res = real(model, prompts, max_new, **kw)
        outs = res[0] if isinstance(res, tuple) else res
        mask = kw.get("token_mask")
        seen.append(([p.cpu() for p in prompts], kw.get("no_repeat_ngram"), None if mask is None else mask.cpu(), [o.cpu() for o in outs]))
        return res

    monkeypatch.setattr(G, name, spy)
    inference.main(["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
                    "DualHyp", "--dual_hypotheses", "--max_new_tokens", "12", "--decode_batch", "4", "--no_repeat_ngram", "2",
                    "--predict_dir", str(tmp_path / "pred")] + more)
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2 and all(rec["no_repeat_ngram"] == 2 for rec in js[:-2])
    assert seen and sum(len(s[0]) for s in seen) == len(items)
    V = Config.from_name("parity-hs96").padded_vocab_size
    counts = []
    for prompts, n, mask, outs in seen:
        assert n == 2 and (mask is not None) == ("--constrain" in more)
        base = None if mask is None else CR.unpack_bits(mask, V)
        texts = [o[p.numel():].tolist() for p, o in zip(prompts, outs)]
        check_picks_outside_their_ban_sets(texts, 2, base, V, " ".join(more))
        counts += [len(R.ban_positions(g, 2)) for g in texts]
    assert sorted(rec["ngram_bans"] for rec in js[:-2]) == sorted(counts)
