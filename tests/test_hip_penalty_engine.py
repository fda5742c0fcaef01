"""Penalties through the engine on the GPU (include/dualhyp_hip.h, "Penalties").  Every check is exact.

The reference is stepped on the host with none of the new code: the same prefill and first pick, then per token one PLAIN
eng.decode(..., 1, first_step=t) on scratch copies of tokens / length / done — its pick is thrown away; the step is needed for its
logits and its KV write, and the token it feeds is the same on both sides — the step's logits read back (dh_engine_read, what 8),
tests/penalty_reference.py's adjusted rows, a plain ops.sample(..., step=t + 1) on them into the real buffers, and
ops.token_logprobs / ops.token_top_logprobs on the RAW rows for the reported values.  generate_batch with penalties must give the same
state, bit for bit.  The reference also counts the steps at which the adjusted rows' pick differs from the raw rows': were it zero the
test would show nothing."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import GPT, Config, _lib, generate, generate_batch, generate_stream, ops, quantize_model_fp8, sample_batch  # noqa: E402
from dualhyp_amd import beam as B_  # noqa: E402
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
# under a three-id mask a sequence has to repeat itself: a presence penalty above the spread of its three logits decides picks
STRONG = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=6.0)
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


def three_id_masks(m, ps, V):
    """(bool [B, V], packed mask): sequence u may produce its three most probable first tokens only, so it repeats itself"""
    _, _, top = generate_batch(m, ps, 1, return_logprobs=True, top_logprobs=3, temperature=1.0, top_k=1)
    allowed = np.zeros((len(ps), V), dtype=bool)
    for u in range(len(ps)):
        allowed[u, top[u][0][0].tolist()] = True
    return allowed, CR.pack_bits(allowed).to(DEV)


def host_stepped(m, ps, kw, pen, *, eos=None, mask=None, ngram=0, stop=None, nuc=None):
    """-> (the state dict generate_batch(return_logprobs, top_logprobs=K, return_state, **kw, **pen) must return, the number of steps
    at which the adjusted rows' pick differed from the raw rows')"""
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
    ops.sample(last, tokens, length, done, step=0, logprobs=lp, top_logprobs=top, **skw)        # an empty history: the plain pick
    scratch = [x.clone() for x in (tokens, length, done)]           # one set: the plain step is captured once
    raw_pick = [x.clone() for x in (tokens, length, done)]
    rows = torch.arange(B, device=DEV)
    decided = 0
    for t in range(NEW - 1):
        for s, x in zip(scratch, (tokens, length, done)):
            s.copy_(x)
        eng.decode(scratch[0], scratch[1], scratch[2], 1, kw["temperature"], kw["top_k"], eos, kw["seed"], first_step=t)
        lg = eng.read_step_logits(B)
        adj = PR.adjusted_rows(lg, PR.histories(tokens, lens, length.tolist()), pen)
        for s, x in zip(raw_pick, (tokens, length, done)):
            s.copy_(x)
        ops.sample(lg, raw_pick[0], raw_pick[1], raw_pick[2], step=t + 1, **skw)
        before = length.clone()
        ops.sample(adj, tokens, length, done, step=t + 1, **skw)
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


def batch_state(m, ps, kw, pen, **more):
    return generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=K, return_state=True, **kw, **pen, **more)[-1]


def generated(st, ps):
    return [st["tokens"][u, p.numel():int(st["length"][u])].tolist() for u, p in enumerate(ps)]


# ---- 1. generate_batch against the host-stepped reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (GREEDY, TOP5), ids=("greedy", "top5"))
def test_generate_batch_is_the_host_stepped_reference(tiny, kw):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    allowed, mask = three_id_masks(m, ps, cfg.padded_vocab_size)
    want, decided = host_stepped(m, ps, kw, STRONG, mask=mask)
    assert decided > 0, "the penalties decided no pick: the test would show nothing"
    got = batch_state(m, ps, kw, STRONG, token_mask=mask)
    assert same_state(got, want)
    assert got["length"].tolist() == [n + NEW for n in LENS]
    off = batch_state(m, ps, kw, {}, token_mask=mask)
    assert any(a != b for a, b in zip(generated(got, ps), generated(off, ps))), "the penalised ids are the unpenalised ones"
    assert all(allowed[u][t] for u, g in enumerate(generated(got, ps)) for t in g)


def test_free_running_without_a_mask(tiny):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    want, _ = host_stepped(m, ps, TOP5, PEN)
    assert same_state(batch_state(m, ps, TOP5, PEN), want)
    for one in (dict(repetition_penalty=1.3), dict(frequency_penalty=0.7), dict(presence_penalty=-0.5)):
        want, _ = host_stepped(m, ps, GREEDY, one)
        assert same_state(batch_state(m, ps, GREEDY, one), want)


def test_an_fp8_engine_with_an_fp8_cache():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    assert m.fp8 and m.kv_cache_dtype == "fp8"
    ps = ragged_prompts(cfg)[:3]
    _, mask = three_id_masks(m, ps, cfg.padded_vocab_size)
    want, decided = host_stepped(m, ps, GREEDY, STRONG, mask=mask)
    assert decided > 0
    assert same_state(batch_state(m, ps, GREEDY, STRONG, token_mask=mask), want)


# ---- 2. the schedules ----------------------------------------------------------------------------------------------------------------
def test_stream_shared_prefix_generate_and_samples_agree(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    _, mask = three_id_masks(m, ps, V)
    want = batch_state(m, ps, TOP5, STRONG, token_mask=mask)
    out = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True, token_mask=mask,
                          **TOP5, **STRONG)
    assert same_state(out[-1], want, done=False)
    # generate: one prompt, the same ids and log-probabilities as its row of a batch of one
    ids, lp = generate(m, ps[2], LENS[2] + NEW, return_logprobs=True, token_mask=mask[2:3], **{k: v for k, v in GREEDY.items() if k != "seed"},
                       **STRONG)
    one = generate_batch(m, [ps[2]], NEW, return_logprobs=True, token_mask=mask[2:3], **GREEDY, **STRONG)
    assert torch.equal(ids, one[0][0]) and same_bits(lp, one[1][0])
    # a shared head of one tile: the prefix is forwarded once, the ids and values stay
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    shared = [torch.cat([head, synth_prompts(1, k, V, seed=40 + k)[0].to(DEV)]) for k in (1, 2, 31, 50)]
    _, smask = three_id_masks(m, shared, V)
    a = batch_state(m, shared, TOP5, STRONG, token_mask=smask)
    timing = {}
    b = batch_state(m, shared, TOP5, STRONG, token_mask=smask, share_prefix="auto", timing=timing)
    assert timing["shared_prefix"] == 32 and same_state(a, b)
    # three samples per utterance are the rows of the 3-fold call
    N = 3
    cands, st = sample_batch(m, ps, NEW, num_samples=N, top_logprobs=K, return_state=True, token_mask=mask, **TOP5, **STRONG)
    rep = batch_state(m, [p for p in ps for _ in range(N)], TOP5, STRONG, token_mask=mask.repeat_interleave(N, dim=0).contiguous())
    assert same_state(st, rep)
    assert len({tuple(c["tokens"].tolist()) for c in cands[1]}) > 1          # and they are not N copies


# ---- 3. everything together ------------------------------------------------------------------------------------------------------------
def test_mask_ban_stop_sequence_top_p_and_penalties(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    _, _, top = generate_batch(m, ps, 1, return_logprobs=True, top_logprobs=8, temperature=1.0, top_k=1)
    g = torch.Generator().manual_seed(3)
    allowed = np.zeros((len(ps), V), dtype=bool)
    for u in range(len(ps)):
        allowed[u, top[u][0][0][:6].tolist()] = True
        allowed[u, torch.randperm(V, generator=g)[:2].tolist()] = True
    mask = CR.pack_bits(allowed).to(DEV)
    a, b = (int(t) for t in top[0][0][0][:2])
    spec = S.as_spec([[a, b], [b, a]], V, torch.device(DEV))
    kw = dict(temperature=1.5, top_k=None, seed=4242)
    nuc = dict(top_p=0.8, min_p=0.02)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=1.5)
    want, decided = host_stepped(m, ps, kw, pen, mask=mask, ngram=3, stop=spec, nuc=nuc)
    assert decided > 0
    got = batch_state(m, ps, kw, pen, token_mask=mask, no_repeat_ngram=3, stop=spec, **nuc)
    assert same_state(got, want)
    assert all(allowed[u][t] for u, g_ in enumerate(generated(got, ps)) for t in g_)
    streamed = generate_stream(m, ps, NEW, max_rows=2, check_every=4, return_logprobs=True, top_logprobs=K, return_state=True,
                               token_mask=mask, no_repeat_ngram=3, stop=spec, **kw, **nuc, **pen)[-1]
    assert same_state(streamed, got, done=False)


# ---- 4. clearing, keys and refusals ----------------------------------------------------------------------------------------------------
def test_a_plain_call_after_a_penalised_one_is_plain():
    cfg, m = build("parity-tiny")          # an engine of its own: the counts below start from its first captured step
    ps = ragged_prompts(cfg)
    plain = generate_batch(m, ps, NEW, **TOP5)
    pen = generate_batch(m, ps, NEW, **TOP5, **PEN)
    again = generate_batch(m, ps, NEW, **TOP5)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert any(not torch.equal(a, b) for a, b in zip(plain, pen))
    for off in (dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0), dict(repetition_penalty=None)):
        assert all(torch.equal(a, b) for a, b in zip(plain, generate_batch(m, ps, NEW, **TOP5, **off)))
    # the values are part of a captured step's key, and clearing finds the plain step again
    B = len(ps)
    eng = m.engine(B, max(LENS) + NEW - 1, sum(LENS))
    tokens = torch.zeros((B, 64), dtype=torch.int64, device=DEV)
    length = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    start = torch.full((B,), 1, dtype=torch.int32, device=DEV)

    def step():
        length.fill_(3)
        done.zero_()
        eng.decode(tokens, length, done, 1, 1.0, 1, None, 7, first_step=0)
        torch.cuda.synchronize()
        return eng.graph_count(0)

    base = step()
    counts = []
    for p in ((1.2, 0.0, 0.0), (1.2, 0.5, 0.0), (None, None, None), (1.2, 0.0, 0.0), (1.0, 0.0, 0.0)):
        eng.set_penalties(*p, start=start)
        counts.append(step())
    assert counts == [base + 1, base + 2, base + 2, base + 2, base + 2], (base, counts)
    m._cache_len = []


def test_verify_and_beam_steps_refuse_while_penalties_are_set(tiny):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
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
    eng.set_penalties(1.2, 0.0, 0.0, start=length.clone())
    try:
        with pytest.raises(_lib.DualHypHipError, match="penalties are set"):
            eng.decode_spec(tokens, length, done, limit, NEW, 1, None, counters, 1, 0.7, None, first_step=0)
        with pytest.raises(_lib.DualHypHipError, match="penalties are set"):
            eng.decode_beam(state, plen, 1, None, first_step=1)
        wide = torch.zeros((Bn, 2049), dtype=torch.int64, device=DEV)
        with pytest.raises(_lib.DualHypHipError, match="2048"):
            eng.decode(wide, length, done, 1, 0.7, 1, None, 1, first_step=0)
    finally:
        eng.set_penalties()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (tokens, length, done, counters))) and not bool(wide.any())
    assert not bool(state.done.any())
    with pytest.raises(ValueError, match="speculate=2 does not go with penalties"):
        generate_batch(m, ps, NEW, top_k=1, speculate=2, presence_penalty=0.5)
    m._cache_len = []
