"""Automaton constraints through the engine on the GPU (include/dualhyp_hip.h, "Automaton constraints").  Every check is exact.

The reference is the existing constrained path stepped from the host, as in test_hip_ngram_engine.py: the same prefill and first pick,
then one eng.decode(..., 1, first_step=t) per token, the contents of the set_token_mask rows rewritten before each step to the allowed
row of the state the host walked to (automaton_reference).  Both sides run the same forward kernels, so ids, done flags,
log-probabilities, alternatives and final states are equal, for the greedy pick and for top_k = 5 with a fixed seed.  Then the
schedules: generate_stream with fewer rows than prompts, share_prefix, sample_batch, an fp8 engine — the same results."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import automaton_reference as AR  # noqa: E402
import constrain_reference as CR  # noqa: E402
from dualhyp_amd import GPT, Config, beam_search_batch, generate, generate_batch, generate_stream, ops, quantize_model_fp8, sample_batch  # noqa: E402
from dualhyp_amd import _lib  # noqa: E402
from dualhyp_amd import automaton as A  # noqa: E402
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


def arrays(aset):
    return aset.edge_off.tolist(), aset.edge_tok.tolist(), aset.edge_dst.tolist(), aset.init.tolist()


def chain_set(ps, V):
    """(the order-2 chain automaton of the prompts, an eos_id no prompt holds)"""
    used = set(t for p in ps for t in p.tolist())
    eos = next(t for t in range(V) if t not in used)
    return A.from_prompts([p.tolist() for p in ps], order=2, eos_id=eos), eos


def host_stepped(m, ps, new, aset, eos, kw, K):
    """generate_batch(automaton=aset, return_logprobs, top_logprobs=K, return_state) by the constrained path alone -> the state dict of
    generate_batch, with automaton_state and the number of picks that had two or more ids to choose among"""
    B, V = len(ps), m.config.padded_vocab_size
    off, tok, dst, init = arrays(aset)
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

    def rows_of(states):
        return np.stack([AR.allowed_row(off, tok, q, V, eos)[0] for q in states])

    states = list(init)
    rows = rows_of(states)
    choices = int((rows.sum(axis=1) >= 2).sum())
    mask = CR.pack_bits(rows).to(DEV)
    ops.sample(last, tokens, length, done, temperature=kw["temperature"], top_k=kw["top_k"], eos_id=eos, seed=seed, step=0, logprobs=lp,
               top_logprobs=top, mask=mask)
    eng.set_logprobs(lp)
    eng.set_top_logprobs(*top)
    eng.set_token_mask(mask)
    try:
        for t in range(new - 1):
            tok_h, len_h, done_h = tokens.tolist(), length.tolist(), done.tolist()
            states = [AR.walk(off, tok, dst, init[u], tok_h[u][lens[u]:len_h[u]])[-1] for u in range(B)]
            rows = rows_of(states)
            choices += int(sum(rows[u].sum() >= 2 for u in range(B) if not done_h[u]))
            mask.copy_(CR.pack_bits(rows).to(DEV))      # the same storage: the captured step reads it when it runs
            eng.decode(tokens, length, done, 1, kw["temperature"], kw["top_k"], eos, seed, first_step=t)
    finally:
        eng.set_logprobs(None)
        eng.set_top_logprobs(None)
        eng.set_token_mask(None)
    m._cache_len = []
    tok_h, len_h = tokens.tolist(), length.tolist()
    final = [AR.walk(off, tok, dst, init[u], tok_h[u][lens[u]:len_h[u]])[-1] for u in range(B)]
    return dict(tokens=tokens, length=length, done=done, logprobs=lp, top_ids=top[0], top_logprobs=top[1], automaton_state=final,
                choices=choices)


def check_accepted(aset, eos, ps, st, what):
    """every produced text is one its automaton accepts: whole where it ended on the EOS, as a prefix where the budget cut it"""
    tok_h, len_h, done_h = st["tokens"].tolist(), st["length"].tolist(), st["done"].tolist()
    texts = []
    for u, p in enumerate(ps):
        g = tok_h[u][p.numel():len_h[u]]
        if done_h[u] == 1:
            assert g[-1] == eos, what
            g = g[:-1]
        assert A.accepts(aset, u, g, eos, complete=done_h[u] == 1), f"{what}: sequence {u} produced {g}"
        texts.append(g)
    return texts


def check_against_host(m, ps, aset, eos, kw, what, K=3):
    want = host_stepped(m, ps, NEW, aset, eos, kw, K)
    out, lp, top, st = generate_batch(m, ps, NEW, eos_id=eos, automaton=aset, return_logprobs=True, top_logprobs=K, return_state=True, **kw)
    for key in ("tokens", "length", "done", "top_ids"):
        assert torch.equal(st[key], want[key]), f"{what}: {key}\n{st[key]}\n{want[key]}"
    assert same_bits(st["logprobs"], want["logprobs"]) and same_bits(st["top_logprobs"], want["top_logprobs"]), what
    assert st["automaton_state"].tolist() == want["automaton_state"], what
    texts = check_accepted(aset, eos, ps, st, what)
    for o, p, g in zip(out, ps, texts):
        assert o[p.numel():].tolist() == g, what
    return texts, want["choices"], [o.clone() for o in out], [v.clone() for v in lp], [(a.clone(), b.clone()) for a, b in top]


@pytest.mark.parametrize("kw", (GREEDY, TOP5), ids=("greedy", "top_k=5"))
def test_tiny_against_the_host_stepped_constrained_path(tiny, kw):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    aset, eos = chain_set(ps, V)
    texts, choices, *_ = check_against_host(m, ps, aset, eos, kw, "chain order 2")
    assert choices >= 1                                                  # at least one pick had two or more ids to choose among
    off = generate_batch(m, ps, NEW, eos_id=eos, **kw)
    assert any(o[p.numel():].tolist() != g for o, p, g in zip(off, ps, texts))      # the constraint moves picks
    # the one-token prompt: its only id or nothing, and then nothing follows that id in the prompt — the EOS edge
    assert texts[0] in ([], ps[0].tolist())


def test_a_forced_path_into_a_dead_end_ends_with_the_eos(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    eos = 3
    # per sequence u: s0 -a-> s1 -b-> s2 -c-> s3, and s3 has no edge at all
    off, tok, dst, init, paths = [0], [], [], [], []
    for u in range(len(ps)):
        path = [10 + u, 50 + 2 * u, 7]
        base = 4 * u
        init.append(base)
        for i, t in enumerate(path):
            tok.append(t)
            dst.append(base + i + 1)
            off.append(len(tok))
        off.append(len(tok))
        paths.append(path)
    aset = A.AutomatonSet(off, tok, dst, init, V)
    for kw in (GREEDY, TOP5):
        out, st = generate_batch(m, ps, NEW, eos_id=eos, automaton=aset, return_state=True, **kw)
        assert st["done"].tolist() == [1] * len(ps) and st["length"].tolist() == [n + 4 for n in LENS]
        for u, (o, p) in enumerate(zip(out, ps)):
            assert o[p.numel():].tolist() == paths[u] and st["tokens"][u, p.numel() + 3].item() == eos
        assert st["automaton_state"].tolist() == [4 * u + 3 for u in range(len(ps))]       # the dead-end EOS leaves the state where it was


def test_schedules_agree(tiny):
    """generate_stream with fewer rows than prompts, share_prefix and sample_batch give generate_batch's ids, log-probabilities,
    alternatives and states"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    aset, eos = chain_set(ps, V)
    for kw in (GREEDY, TOP5):
        full = dict(eos_id=eos, automaton=aset, return_logprobs=True, top_logprobs=3, return_state=True, **kw)
        res = generate_batch(m, ps, NEW, **full)
        want, want_state = clone_all(res), res[3]["automaton_state"].tolist()
        got = generate_stream(m, ps, NEW, max_rows=2, check_every=3, **full)
        assert same_result(want, got) and got[3]["automaton_state"].tolist() == want_state, kw
        check_accepted(aset, eos, ps, got[3], "stream")
    # a shared 32-token head
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps2 = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 33, 50)]
    aset2, eos2 = chain_set(ps2, V)
    for kw in (GREEDY, TOP5):
        full = dict(eos_id=eos2, automaton=aset2, return_logprobs=True, top_logprobs=3, **kw)
        want = clone_all(generate_batch(m, ps2, NEW, **full))
        tm = {}
        assert same_result(want, generate_batch(m, ps2, NEW, share_prefix=True, timing=tm, **full)), kw
        assert tm["shared_prefix"] == 32
        assert same_result(want, generate_stream(m, ps2, NEW, share_prefix=True, max_rows=3, check_every=5, **full)), kw
    # sample_batch(N = 2) is generate_batch over every prompt twice, row u * 2 + j in utterance u's start state
    twice = [p for p in ps for _ in range(2)]
    out, lp, top, st = generate_batch(m, twice, NEW, eos_id=eos, automaton=aset.repeat(2), return_logprobs=True, top_logprobs=3,
                                      return_state=True, **TOP5)
    cands, st2 = sample_batch(m, ps, NEW, num_samples=2, eos_id=eos, automaton=aset, top_logprobs=3, return_state=True, **TOP5)
    for key in ("tokens", "length", "done", "top_ids", "automaton_state"):
        assert torch.equal(st[key], st2[key]), key
    assert same_bits(st["logprobs"], st2["logprobs"]) and same_bits(st["top_logprobs"], st2["top_logprobs"])
    for u, p in enumerate(ps):
        for j in range(2):
            g = out[u * 2 + j][p.numel():].tolist()
            assert cands[u][j]["tokens"].tolist() == g and A.accepts(aset, u, g, eos, complete=st["done"][u * 2 + j].item() == 1)
    # generate() forwards the argument
    one = A.from_prompts([ps[2].tolist()], order=2, eos_id=eos)
    many = generate_batch(m, ps, NEW, eos_id=eos, automaton=aset, **GREEDY)
    assert torch.equal(generate(m, ps[2], ps[2].numel() + NEW, eos_id=eos, automaton=one, **GREEDY), many[2])


def test_fp8_engine_against_the_host_stepped_constrained_path():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.fp8 and m.kv_cache_dtype == "fp8"
    ps = ragged_prompts(cfg)[:3]
    aset, eos = chain_set(ps, cfg.padded_vocab_size)
    _, choices, *_ = check_against_host(m, ps, aset, eos, GREEDY, "fp8")
    assert choices >= 1


def test_none_is_the_call_without_the_argument_and_the_refusals():
    cfg, m = build("parity-tiny")                                      # a model of its own: the graph counts are this test's
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    aset, eos = chain_set(ps, V)
    # the tokens' addresses are part of a captured step's key, so a repeat of the plain call may or may not find its step again: the call
    # with automaton=None captures what that repeat captures, no more, and the call with a set one step of its own
    cpu = lambda res: [o.cpu() for o in res]
    full = dict(eos_id=eos, **GREEDY)
    want = cpu(generate_batch(m, ps, NEW, **full))
    eng = m._engine
    c1 = eng.graph_count()
    again = cpu(generate_batch(m, ps, NEW, **full))
    c2 = eng.graph_count()
    none = cpu(generate_batch(m, ps, NEW, automaton=None, **full))
    c3 = eng.graph_count()
    assert same_lists(want, again) and same_lists(want, none)
    assert m._engine is eng and c3 - c2 == c2 - c1
    on = cpu(generate_batch(m, ps, NEW, automaton=aset, **full))
    assert m._engine is eng and eng.graph_count() == c3 + 1 and eng._automaton is None       # and nothing is left set
    assert not same_lists(want, on) and same_lists(want, cpu(generate_batch(m, ps, NEW, **full)))
    assert same_lists(cpu(generate_batch(m, ps, NEW, automaton=None, **TOP5, eos_id=eos)), cpu(generate_batch(m, ps, NEW, **TOP5, eos_id=eos)))
    with pytest.raises(ValueError, match="speculate"):
        generate_batch(m, ps, NEW, eos_id=eos, automaton=aset, speculate=3, **GREEDY)
    with pytest.raises(ValueError, match="speculate"):
        generate(m, ps[0], ps[0].numel() + NEW, eos_id=eos, automaton=aset, speculate=3, **GREEDY)
    with pytest.raises(TypeError):
        beam_search_batch(m, ps, 4, num_beams=2, automaton=aset)
    with pytest.raises(ValueError, match="eos_id"):
        generate_batch(m, ps, NEW, automaton=aset, **GREEDY)
    with pytest.raises(ValueError, match="sequences"):
        generate_batch(m, ps[:2], NEW, eos_id=eos, automaton=aset, **GREEDY)
    with pytest.raises(TypeError):
        generate_batch(m, ps, NEW, eos_id=eos, automaton=[[1, 2]], **GREEDY)
    # the engine's own refusals, before anything is captured or launched
    B, lens = len(ps), [int(p.numel()) for p in ps]
    eng = m.engine(B, max(lens) + NEW + 4, sum(lens))
    dev_set = aset.to(DEV)
    start = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tok_ld = max(lens) + NEW
    tokens = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(ps, batch_first=True), (0, tok_ld - max(lens))).contiguous()
    length, done = start.clone(), torch.zeros(B, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="start"):
        eng.set_automaton(dev_set, None)
    with pytest.raises(_lib.DualHypHipError, match="start"):
        _lib.check(eng.lib.dh_engine_set_automaton(eng.handle, __import__("ctypes").byref(dev_set.c_struct()), None))
    eng.set_automaton(dev_set, start)
    try:
        with pytest.raises(_lib.DualHypHipError, match="eos_id"):
            eng.decode(tokens, length, done, 1, 1.0, 1, None, 1, first_step=0)
        with pytest.raises(_lib.DualHypHipError, match="sequences"):
            eng.decode(tokens[:2], length[:2], done[:2], 1, 1.0, 1, eos, 1, first_step=0)
        eng.reserve_rows(B * 3)
        limit = (start + NEW).contiguous()
        counters = torch.zeros(3, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.DualHypHipError, match="automaton"):
            eng.decode_spec(tokens, length, done, limit, NEW, 2, None, counters, 1, 1.0, eos, first_step=0)
        from dualhyp_amd import beam as _beam
        eng.reserve_beams(2, NEW)
        state = _beam.BeamState(2, 2, NEW, torch.device(DEV))            # two utterances x two beams: the engine's four slots
        with pytest.raises(_lib.DualHypHipError, match="automaton"):
            eng.decode_beam(state, start[:2].contiguous(), 1, eos, first_step=1)
    finally:
        eng.set_automaton()
    assert torch.equal(length, start) and not done.any()             # nothing ran
