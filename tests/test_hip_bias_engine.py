"""Contextual biasing through the engine on the GPU (include/dualhyp_hip.h, "Contextual biasing").  Every check is exact.

The reference is stepped on the host with none of the new code: the same prefill, then per token one PLAIN eng.decode(..., 1,
first_step=t) on scratch copies of tokens / length / done — its pick is thrown away; the step is needed for its logits and its KV
write — the step's logits read back, tests/bias_reference.py's adjusted rows, a plain ops.sample(..., step=t + 1) on them into the real
buffers, and ops.token_logprobs / ops.token_top_logprobs on the RAW rows for the reported values.  The first pick is adjusted the same
way (an empty history still proposes every entry's first id).  generate_batch(bias=) must give the same state, bit for bit.

The bias is built from the unbiased run, so that it has to change it: utterance 0 emits (a, b) at steps 2 and 3 and c is the step-3
runner-up; the entry (a, c) carries a boost above the step-3 margin, and a one-id entry takes more than its margin off utterance 1's
first token."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bias_reference as BR  # noqa: E402
import constrain_reference as CR  # noqa: E402
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import GPT, Config, _lib, generate, generate_batch, generate_stream, ops, quantize_model_fp8, sample_batch  # noqa: E402
from dualhyp_amd import beam as B_  # noqa: E402
from dualhyp_amd import bias as Bi  # noqa: E402
from dualhyp_amd import stop as S  # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
NEW = 16
K = 3
LENS = (1, 31, 33, 47)
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
GREEDY = dict(temperature=0.7, top_k=1, seed=1)
TOP5 = dict(temperature=1.5, top_k=5, seed=4242)
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=0.3)
KEYS = ("tokens", "length", "done", "top_ids")
# the tiny model's rows are flat (its step margins are a few bf16 steps of 1/64): a boost of the margin plus 1/16 puts the runner-up a
# few steps above the unbiased pick, and is small enough not to lift the entry's first id, boosted at every step, over earlier picks.
# The test asserts on the reference that both hold.
SLACK = 0.0625


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_state(a, b, done=True):
    """done=False: generate_stream ends every sequence on its own budget (done = 2) where generate_batch, which steps all of its rows
    together, leaves a shorter prompt's flag at 0; the stops (3) are still compared"""
    if not done and not torch.equal(a["done"] == 3, b["done"] == 3):
        return False
    return all(torch.equal(a[k], b[k]) for k in KEYS if done or k != "done") and same_bits(a["logprobs"], b["logprobs"]) and \
        same_bits(a["top_logprobs"], b["top_logprobs"])


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


def batch_state(m, ps, kw, bias, **more):
    bkw = {} if bias is None else dict(bias=bias)
    return generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=K, return_state=True, **kw, **bkw, **more)[-1]


def generated(st, ps):
    return [st["tokens"][u, p.numel():int(st["length"][u])].tolist() for u, p in enumerate(ps)]


def entries_from_the_unbiased_run(m, ps):
    """-> ((ids, boost) pairs, (a, b, c), the unbiased greedy state)"""
    st = batch_state(m, ps, GREEDY, None)
    n0, n1 = int(ps[0].numel()), int(ps[1].numel())
    a, b = (int(t) for t in st["tokens"][0, n0 + 2:n0 + 4])
    ids3, lp3 = st["top_ids"][0, n0 + 3].tolist(), st["top_logprobs"][0, n0 + 3].tolist()
    assert ids3[0] == b and a != ids3[1]
    c = ids3[1]
    first = int(st["tokens"][1, n1])
    lp0 = st["top_logprobs"][1, n1].tolist()
    assert st["top_ids"][1, n1, 0] == first
    entries = [([a, c], (lp3[0] - lp3[1]) + SLACK), ([first], -((lp0[0] - lp0[1]) + SLACK))]
    return entries, (a, b, c), st


@pytest.fixture(scope="module")
def tiny_bias(tiny):
    cfg, m = tiny
    return entries_from_the_unbiased_run(m, ragged_prompts(cfg))


def host_stepped(m, ps, kw, entries, pen={}, *, eos=None, mask=None, ngram=0, stop=None, nuc=None):
    """-> (the state dict generate_batch(return_logprobs, top_logprobs=K, return_state, bias=entries, **kw, **pen) must return, the
    number of picks at which the adjusted rows' pick differed from the raw rows')"""
    B = len(ps)
    lens = [int(p.numel()) for p in ps]
    tok_ld = max(lens) + NEW
    tokens = torch.nn.utils.rnn.pad_sequence(list(ps), batch_first=True)
    tokens = torch.nn.functional.pad(tokens, (0, tok_ld - tokens.size(1))).contiguous()
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    lp = torch.full((B, tok_ld), NAN, dtype=torch.float32, device=DEV)
    top = (torch.full((B, tok_ld, K), -1, dtype=torch.int32, device=DEV), torch.full((B, tok_ld, K), NAN, dtype=torch.float32, device=DEV))
    start = torch.tensor(lens, dtype=torch.int32, device=DEV) if ngram or (stop is not None and stop.sequences) else None
    skw = dict(temperature=kw["temperature"], top_k=kw["top_k"], eos_id=eos, seed=kw["seed"], mask=mask, no_repeat_ngram=ngram, start=start,
               stop=stop, **(nuc or {}))
    eng = m.engine(B, max(lens) + NEW - 1, sum(lens))
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    _, last = eng.forward(torch.cat(list(ps)), lens, [0] * B, want_all=False, want_last=True, slot_base=0)
    scratch = [x.clone() for x in (tokens, length, done)]           # one set: the plain step is captured once
    raw_pick = [x.clone() for x in (tokens, length, done)]
    rows = torch.arange(B, device=DEV)
    decided = 0
    for t in range(NEW):
        if t == 0:
            lg = last
        else:
            for s, x in zip(scratch, (tokens, length, done)):
                s.copy_(x)
            eng.decode(scratch[0], scratch[1], scratch[2], 1, kw["temperature"], kw["top_k"], eos, kw["seed"], first_step=t - 1)
            lg = eng.read_step_logits(B)
        adj = BR.adjusted_rows(lg, PR.histories(tokens, lens, length.tolist()), entries, pen)
        for s, x in zip(raw_pick, (tokens, length, done)):
            s.copy_(x)
        ops.sample(lg, raw_pick[0], raw_pick[1], raw_pick[2], step=t, **skw)
        before = length.clone()
        ops.sample(adj, tokens, length, done, step=t, **skw)
        live = length > before
        at = before.long().clamp(max=tok_ld - 1)
        decided += int((live & (tokens[rows, at] != raw_pick[0][rows, at])).sum())
        # the reported values are the raw rows'
        ids, vals = ops.token_top_logprobs(lg, K)
        val = ops.token_logprobs(lg, tokens[rows, at].clamp(0, lg.size(1) - 1))
        lp[rows[live], at[live]] = val[live]
        top[0][rows[live], at[live]] = ids[live]
        top[1][rows[live], at[live]] = vals[live]
    m._cache_len = []
    return dict(tokens=tokens, length=length, done=done, logprobs=lp, top_ids=top[0], top_logprobs=top[1]), decided


def strong(entries):
    """the same ids with boosts of 4 and -4: a seeded draw over a flat row moves only under a boost that shifts its mass"""
    return [(ids, 4.0 if b > 0 else -4.0) for ids, b in entries]


def first_difference(x, y):
    return next((i for i, (s, t) in enumerate(zip(x, y)) if s != t), None)


# ---- 1. generate_batch against the host-stepped reference ---------------------------------------------------------------------------
def test_generate_batch_is_the_host_stepped_reference(tiny, tiny_bias):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    entries, (a, b, c), off = tiny_bias
    want, decided = host_stepped(m, ps, GREEDY, entries)
    assert decided > 0, "the bias decided no pick: the test would show nothing"
    # by the reference alone: utterance 0 leaves the unbiased ids at step 3, for c; utterance 1 at its first token
    g_off, g_want = generated(off, ps), generated(want, ps)
    assert g_off[0][2:4] == [a, b]
    assert first_difference(g_off[0], g_want[0]) == 3 and g_want[0][3] == c
    assert first_difference(g_off[1], g_want[1]) == 0
    assert BR.hits(g_want[0], entries) >= 1
    got = batch_state(m, ps, GREEDY, entries)
    assert same_state(got, want)
    assert got["length"].tolist() == [n + NEW for n in LENS]
    # and again on the device
    g_got = generated(got, ps)
    assert first_difference(g_off[0], g_got[0]) == 3 and g_got[0][3] == c and first_difference(g_off[1], g_got[1]) == 0
    assert Bi.bias_hits(g_got[0], entries) >= 1
    # a compiled specification is the list
    spec = Bi.compile_bias(entries, cfg.padded_vocab_size, DEV)
    assert same_state(batch_state(m, ps, GREEDY, spec), want)


def test_the_seeded_draw(tiny, tiny_bias):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    entries = strong(tiny_bias[0])
    want, decided = host_stepped(m, ps, TOP5, entries)
    assert decided > 0
    assert same_state(batch_state(m, ps, TOP5, entries), want)


def test_an_fp8_engine_with_an_fp8_cache():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.fp8 and m.kv_cache_dtype == "fp8"
    ps = ragged_prompts(cfg)[:3]
    entries, _, off = entries_from_the_unbiased_run(m, ps)
    want, decided = host_stepped(m, ps, GREEDY, entries)
    assert decided > 0
    got = batch_state(m, ps, GREEDY, entries)
    assert same_state(got, want)
    assert generated(got, ps) != generated(off, ps)


# ---- 2. the schedules ----------------------------------------------------------------------------------------------------------------
def test_stream_shared_prefix_generate_and_samples_agree(tiny, tiny_bias):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    entries = strong(tiny_bias[0])
    assert generated(batch_state(m, ps, TOP5, entries), ps) != generated(batch_state(m, ps, TOP5, None), ps)
    want = batch_state(m, ps, TOP5, entries)
    out = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True, bias=entries, **TOP5)
    assert same_state(out[-1], want, done=False)
    # generate: one prompt, the same ids and log-probabilities as its row of a batch of one
    ids, lp = generate(m, ps[0], LENS[0] + NEW, return_logprobs=True, bias=entries, **{k: v for k, v in GREEDY.items() if k != "seed"})
    one = generate_batch(m, [ps[0]], NEW, return_logprobs=True, bias=entries, **GREEDY)
    assert torch.equal(ids, one[0][0]) and same_bits(lp, one[1][0])
    assert ids[LENS[0]:].tolist() == generated(batch_state(m, ps, GREEDY, entries), ps)[0]
    # a shared head of one tile: the prefix is forwarded once, the ids and values stay
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    shared = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 50)]
    s_entries, _, s_off = entries_from_the_unbiased_run(m, shared)
    x = batch_state(m, shared, GREEDY, s_entries)
    timing = {}
    y = batch_state(m, shared, GREEDY, s_entries, share_prefix="auto", timing=timing)
    assert timing["shared_prefix"] == 32 and same_state(x, y)
    assert generated(x, shared) != generated(s_off, shared)
    # three samples per utterance are the rows of the 3-fold call
    N = 3
    cands, st = sample_batch(m, ps, NEW, num_samples=N, top_logprobs=K, return_state=True, bias=entries, **TOP5)
    rep = batch_state(m, [p for p in ps for _ in range(N)], TOP5, entries)
    assert same_state(st, rep)
    assert len({tuple(cd["tokens"].tolist()) for cd in cands[1]}) > 1          # and they are not N copies


# ---- 3. everything together ------------------------------------------------------------------------------------------------------------
def test_mask_ban_stop_sequence_top_p_and_penalties(tiny, tiny_bias):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    entries, (a, b, c), _ = tiny_bias
    _, _, top = generate_batch(m, ps, 1, return_logprobs=True, top_logprobs=8, temperature=1.0, top_k=1)
    g = torch.Generator().manual_seed(3)
    allowed = np.zeros((len(ps), V), dtype=bool)
    for u in range(len(ps)):
        allowed[u, top[u][0][0][:6].tolist()] = True
        allowed[u, torch.randperm(V, generator=g)[:2].tolist()] = True
    allowed[:, [a, c]] = True
    # boosts that decide picks among the allowed ids, on ids the sequences repeat under the mask
    t0, t1 = (int(t) for t in top[0][0][0][:2])
    more = list(entries) + [([t1, t0], 6.0), ([int(top[2][0][0][3])], 5.0), ([int(top[3][0][0][1])], -5.0)]
    mask = CR.pack_bits(allowed).to(DEV)
    spec = S.as_spec([[t0, t1], [t1, t0]], V, torch.device(DEV))
    kw = dict(temperature=1.5, top_k=None, seed=4242)
    nuc = dict(top_p=0.8, min_p=0.02)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=1.5)
    only_pen, _ = host_stepped(m, ps, kw, (), pen, mask=mask, ngram=3, stop=spec, nuc=nuc)
    want, decided = host_stepped(m, ps, kw, more, pen, mask=mask, ngram=3, stop=spec, nuc=nuc)
    assert decided > 0 and generated(want, ps) != generated(only_pen, ps)
    got = batch_state(m, ps, kw, more, token_mask=mask, no_repeat_ngram=3, stop=spec, **nuc, **pen)
    assert same_state(got, want)
    assert all(allowed[u][t] for u, g_ in enumerate(generated(got, ps)) for t in g_)
    streamed = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True,
                               token_mask=mask, no_repeat_ngram=3, stop=spec, bias=more, **kw, **nuc, **pen)[-1]
    assert same_state(streamed, got, done=False)


# ---- 4. clearing, keys and refusals ----------------------------------------------------------------------------------------------------
def test_a_plain_call_after_a_biased_one_is_plain():
    cfg, m = build("parity-tiny")          # an engine of its own: the counts below start from its first captured step
    ps = ragged_prompts(cfg)
    entries, _, _ = entries_from_the_unbiased_run(m, ps)
    plain = generate_batch(m, ps, NEW, **GREEDY)
    biased = generate_batch(m, ps, NEW, bias=entries, **GREEDY)
    again = generate_batch(m, ps, NEW, **GREEDY)
    assert all(torch.equal(x, y) for x, y in zip(plain, again))
    assert any(not torch.equal(x, y) for x, y in zip(plain, biased))
    for off in (dict(bias=None), dict(bias=[])):
        assert all(torch.equal(x, y) for x, y in zip(plain, generate_batch(m, ps, NEW, **GREEDY, **off)))
    # the spec is part of a captured step's key, and clearing finds the plain step again
    B = len(ps)
    V = cfg.padded_vocab_size
    eng = m.engine(B, max(LENS) + NEW - 1, sum(LENS))
    tokens = torch.zeros((B, 64), dtype=torch.int64, device=DEV)
    length = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    start = torch.full((B,), 1, dtype=torch.int32, device=DEV)
    one, two = Bi.compile_bias(entries, V, DEV), Bi.compile_bias(entries[:1], V, DEV)

    def step():
        length.fill_(3)
        done.zero_()
        eng.decode(tokens, length, done, 1, 1.0, 1, None, 7, first_step=0)
        torch.cuda.synchronize()
        return eng.graph_count(0)

    base = step()
    counts = []
    for spec in (one, two, None, one, None):
        eng.set_bias(spec, start)
        counts.append(step())
    assert counts == [base + 1, base + 2, base + 2, base + 2, base + 2], (base, counts)
    m._cache_len = []


def test_verify_and_beam_steps_refuse_while_a_bias_is_set(tiny, tiny_bias):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    entries = tiny_bias[0]
    Bn = len(ps)
    eng = m.engine(Bn, max(LENS) + NEW, sum(LENS))
    eng.reserve_rows(Bn * 2)
    tok_ld = max(LENS) + NEW
    tokens = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(list(ps), batch_first=True), (0, NEW)).contiguous()
    assert tokens.size(1) == tok_ld
    length = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    done = torch.zeros(Bn, dtype=torch.int32, device=DEV)
    limit = torch.tensor([n + NEW for n in LENS], dtype=torch.int32, device=DEV)
    counters = torch.zeros(3, dtype=torch.int32, device=DEV)
    keep = [x.clone() for x in (tokens, length, done, counters)]
    W = 2
    eng.reserve_beams(W, NEW)
    state = B_.BeamState(Bn // W, W, NEW, torch.device(DEV))
    plen = torch.tensor(LENS[:Bn // W], dtype=torch.int32, device=DEV)
    spec = Bi.compile_bias(entries, cfg.padded_vocab_size, DEV)
    start = length.clone()
    eng.set_bias(spec, start)
    try:
        with pytest.raises(_lib.DualHypHipError, match="a bias of 2 entries is set"):
            eng.decode_spec(tokens, length, done, limit, NEW, 1, None, counters, 1, 0.7, None, first_step=0)
        with pytest.raises(_lib.DualHypHipError, match="a bias of 2 entries is set"):
            eng.decode_beam(state, plen, 1, None, first_step=1)
        # with penalties set as well, the token buffer and the entries' ids share the tables
        eng.set_penalties(1.2, 0.0, 0.0, start=start)
        wide = torch.zeros((Bn, 2046), dtype=torch.int64, device=DEV)
        with pytest.raises(_lib.DualHypHipError, match="2048"):
            eng.decode(wide, length, done, 1, 0.7, 1, None, 1, first_step=0)
    finally:
        eng.set_penalties()
        eng.set_bias()
    with pytest.raises(ValueError, match="needs start"):
        eng.set_bias(spec, None)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(keep, (tokens, length, done, counters))) and not bool(wide.any())
    assert not bool(state.done.any())
    with pytest.raises(ValueError, match="speculate=2 does not go with a bias"):
        generate_batch(m, ps, NEW, top_k=1, speculate=2, bias=entries)
    m._cache_len = []
