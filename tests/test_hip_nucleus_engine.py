"""Nucleus and min-p sampling through the engine on the GPU (include/dualhyp_hip.h, "Nucleus and min-p").  Every check is exact.

The reference is the op itself, which tests/test_hip_nucleus.py pins to the host model: the engine is stepped one
eng.decode(..., 1, first_step=t) at a time under set_nucleus, the logits of the step are read back (dh_engine_read, what 8) and
ops.sample with the same parameters is applied to a copy of the state from before the step.  Token, length, done, log-probability and
alternatives must be equal, which shows that the parameters reach the kernel inside a captured step.  Then: one call of 15 steps, the
schedules, the captured steps' keys, the composition with mask, ban and stop, and an fp8 engine."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, ops, quantize_model_fp8  # noqa: E402
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
# a flat sampler, so that the crop decides many picks: temperature 2, no crop by count
SAMPLED = dict(temperature=2.0, top_k=None, seed=4242)
NUCLEUS = dict(top_p=0.6, min_p=0.1)
KEYS = ("tokens", "length", "done", "top_ids")


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


def stepped(m, ps, kw, nuc, *, eos=None, mask=None, ngram=0, stop=None, one_call=False):
    """generate_batch(return_logprobs, top_logprobs=K, return_state, **kw, **nuc) by hand: the prefill and the first pick, then
    NEW - 1 single steps under set_nucleus, each checked against ops.sample on the step's own logits (one_call: one decode call of
    NEW - 1 steps, unchecked).  -> the state dict of generate_batch"""
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
               stop=stop, **nuc)
    eng = m.engine(B, max(lens) + NEW - 1, sum(lens))
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    _, last = eng.forward(torch.cat(list(ps)), lens, [0] * B, want_all=False, want_last=True, slot_base=0)
    ops.sample(last, tokens, length, done, step=0, logprobs=lp, top_logprobs=top, **skw)
    eng.set_logprobs(lp)
    eng.set_top_logprobs(*top)
    if mask is not None:
        eng.set_token_mask(mask)
    if ngram:
        eng.set_no_repeat_ngram(ngram, start)
    if stop is not None:
        eng.set_stop(stop, start)
    eng.set_nucleus(nuc.get("top_p"), nuc.get("min_p"))
    try:
        if one_call:
            eng.decode(tokens, length, done, NEW - 1, kw["temperature"], kw["top_k"], eos, kw["seed"], first_step=0)
        for t in range(0 if one_call else NEW - 1):
            pre = [x.clone() for x in (tokens, length, done, lp, top[0], top[1])]
            eng.decode(tokens, length, done, 1, kw["temperature"], kw["top_k"], eos, kw["seed"], first_step=t)
            lg = eng.read_step_logits(B)
            ops.sample(lg, pre[0], pre[1], pre[2], step=t + 1, logprobs=pre[3], top_logprobs=(pre[4], pre[5]), **skw)
            assert torch.equal(pre[0], tokens) and torch.equal(pre[1], length) and torch.equal(pre[2], done), f"step {t}"
            assert same_bits(pre[3], lp) and torch.equal(pre[4], top[0]) and same_bits(pre[5], top[1]), f"step {t}"
    finally:
        eng.set_logprobs(None)
        eng.set_top_logprobs(None)
        eng.set_token_mask(None)
        eng.set_no_repeat_ngram(0)
        eng.set_stop(None)
        eng.set_nucleus(None, None)
    m._cache_len = []
    return dict(tokens=tokens, length=length, done=done, logprobs=lp, top_ids=top[0], top_logprobs=top[1])


def batch_state(m, ps, kw, nuc, **more):
    return generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=K, return_state=True, **kw, **nuc, **more)[-1]


def generated(st, ps):
    return [st["tokens"][u, p.numel():int(st["length"][u])].tolist() for u, p in enumerate(ps)]


# ---- 1, 2: single steps against the op, and one call of 15 steps --------------------------------------------------------------------
@pytest.mark.parametrize("nuc", (NUCLEUS, dict(top_p=0.9), dict(min_p=0.05), dict(top_p=0.9, min_p=0.05)), ids=lambda n: str(sorted(n.items())))
def test_single_steps_are_the_op_on_the_steps_logits(tiny, nuc):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    want = stepped(m, ps, SAMPLED, nuc)
    assert want["length"].tolist() == [n + NEW for n in LENS]
    assert same_state(stepped(m, ps, SAMPLED, nuc, one_call=True), want)
    if nuc is NUCLEUS:      # the crop decided picks: the sampler without it goes elsewhere
        off = stepped(m, ps, SAMPLED, {})
        assert generated(off, ps) != generated(want, ps)


# ---- 3. the schedules ---------------------------------------------------------------------------------------------------------------
def test_generate_batch_stream_and_shared_prefix_agree(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    want = stepped(m, ps, SAMPLED, NUCLEUS)
    assert same_state(batch_state(m, ps, SAMPLED, NUCLEUS), want)
    out = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True, **SAMPLED, **NUCLEUS)
    assert same_state(out[-1], want, done=False)
    one = generate(m, ps[2], LENS[2] + NEW, temperature=SAMPLED["temperature"], top_k=None, **NUCLEUS)
    assert one.numel() == LENS[2] + NEW
    # a shared head of one tile: the prefix is forwarded once, the ids and values stay
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    shared = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 50)]
    a = batch_state(m, shared, SAMPLED, NUCLEUS)
    timing = {}
    b = batch_state(m, shared, SAMPLED, NUCLEUS, share_prefix=True, timing=timing)
    assert timing["shared_prefix"] == 32 and same_state(a, b)
    c = generate_stream(m, shared, NEW, max_rows=3, check_every=4, share_prefix=True, return_logprobs=True, top_logprobs=K, return_state=True,
                        **SAMPLED, **NUCLEUS)[-1]
    assert same_state(a, c, done=False)


# ---- 4. the captured steps' keys ----------------------------------------------------------------------------------------------------
def test_graph_keys_and_the_engine_is_left_off():
    cfg, m = build("parity-tiny")          # an engine of its own: the counts below start from its first captured step
    ps = ragged_prompts(cfg)
    B = len(ps)
    plain = generate_batch(m, ps, NEW, **SAMPLED)
    eng = m.engine(B, max(LENS) + NEW - 1, sum(LENS))
    tokens = torch.zeros((B, 64), dtype=torch.int64, device=DEV)
    length = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)

    def step(top_k=None):
        length.fill_(3)
        done.zero_()
        eng.decode(tokens, length, done, 1, 1.0, top_k, None, 7, first_step=0)
        torch.cuda.synchronize()
        return eng.graph_count(0)

    base = step()
    assert step() == base                                   # found again
    counts = []
    for top_p, min_p in ((0.9, 0.0), (0.9, 0.05), (None, None), (0.9, 0.0), (0.9, 0.05), (None, None)):
        eng.set_nucleus(top_p, min_p)
        counts.append(step())
    assert counts == [base + 1, base + 2, base + 2, base + 2, base + 2, base + 2], (base, counts)
    # the arg-max takes neither: its step is the one captured without them
    greedy = step(top_k=1)
    eng.set_nucleus(0.5, 0.5)
    assert step(top_k=1) == greedy
    eng.set_nucleus(None, None)
    m._cache_len = []
    # generate_batch leaves the engine off, and a plain call returns what it returned before
    with_nucleus = generate_batch(m, ps, NEW, **SAMPLED, **NUCLEUS)
    again = generate_batch(m, ps, NEW, **SAMPLED)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert any(not torch.equal(a, b) for a, b in zip(plain, with_nucleus))
    for off in (dict(top_p=1.0, min_p=0.0), dict(top_p=None, min_p=None)):
        assert all(torch.equal(a, b) for a, b in zip(plain, generate_batch(m, ps, NEW, **SAMPLED, **off)))


# ---- 5. with mask, ban and stop -----------------------------------------------------------------------------------------------------
def test_composition_with_mask_ban_and_stop(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    # sequence u may produce the 12 most probable first tokens of its own; the most probable of sequence 0 stops
    _, _, top = generate_batch(m, ps, 1, return_logprobs=True, top_logprobs=8, temperature=1.0, top_k=1)
    g = torch.Generator().manual_seed(3)
    allowed = np.zeros((len(ps), V), dtype=bool)
    for u in range(len(ps)):
        allowed[u, top[u][0][0].tolist()] = True
        allowed[u, torch.randperm(V, generator=g)[:4].tolist()] = True
    stop_id = int(top[0][0][0][1])
    mask = CR.pack_bits(allowed).to(DEV)
    spec = S.as_spec([stop_id], V, torch.device(DEV))
    kw = dict(SAMPLED, temperature=1.5)
    nuc = dict(top_p=0.8, min_p=0.02)
    want = stepped(m, ps, kw, nuc, mask=mask, ngram=2, stop=spec)
    got = batch_state(m, ps, kw, nuc, token_mask=mask, no_repeat_ngram=2, stop=spec)
    assert same_state(got, want)
    texts = generated(got, ps)
    assert all(allowed[u][t] for u, g_ in enumerate(texts) for t in g_)
    for u, g_ in enumerate(texts):              # a stop ends the sequence behind the stopping token
        assert stop_id not in g_[:-1]
        assert (int(got["done"][u]) == 3) == (g_[-1] == stop_id)
    streamed = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True,
                               token_mask=mask, no_repeat_ngram=2, stop=spec, **kw, **nuc)[-1]
    assert same_state(streamed, got, done=False)


# ---- 6. an fp8 engine, weights and cache --------------------------------------------------------------------------------------------
def test_an_fp8_engine_steps_like_the_op():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.fp8 and m.kv_cache_dtype == "fp8"
    ps = ragged_prompts(cfg)[:3]
    want = stepped(m, ps, SAMPLED, NUCLEUS)
    assert same_state(batch_state(m, ps, SAMPLED, NUCLEUS), want)
