"""Speculative greedy decoding on the GPU (generate_batch(..., speculate=D), dh_engine_decode_spec): a verify step feeds a sequence's
last token and D drafts through the decode kernels at once and keeps what the arg-max confirms.  Every check is exact
(torch.equal): the ids, the token buffer and the KV cache are those of the plain run whatever the drafts say; the number of steps
is the host replay's of the acceptance rule on the known ids."""
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import GPT, Config, generate, generate_batch
from dualhyp_amd.speculate import propose, replay
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
NEW = 24                      # 23 verify-step tokens: not a multiple of D + 1 for D = 1, 2, 3, 7 — the budget ends mid-step
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}
KW = dict(temperature=0.2, top_k=1)
DS = (1, 2, 3, 7)             # (D + 1) * q_per_kv <= 32 allows 7 in all three configs (q_per_kv 2, 1, 2)


def build(name, seed=11, **over):
    cfg = Config.from_name(name, **LORA, **over)
    assert cfg.head_size == HEAD_SIZES[name] and 8 * (cfg.n_head // cfg.n_query_groups) <= 32
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.eval()
    return cfg, m


@pytest.fixture(scope="module", params=list(HEAD_SIZES))
def model(request):
    return build(request.param)


def ragged_prompts(cfg, new=NEW, seed=70):
    """a one-token prompt; 30 .. 33 tokens, so that the first verify steps' positions are 30 .. 33 + j and the appended keys straddle
    the first tile's end in every way; and a prompt whose last generated token sits at the model's last position"""
    V = cfg.padded_vocab_size
    lens = [1, 30, 31, 32, 33, 47, 64, cfg.block_size - new + 1]
    return [synth_prompts(1, n, V, seed=seed + i)[0].to(DEV) for i, n in enumerate(lens)]


def plain_run(m, ps, new, **kw):
    out, st = generate_batch(m, ps, new, return_state=True, **KW, **kw)
    return [o.clone() for o in out], {k: v.clone() for k, v in st.items()}


def generated(st, ps, new):
    """per sequence: the tokens the run produced, the EOS included"""
    ln = st["length"].tolist()
    return [st["tokens"][u, p.numel():min(ln[u], p.numel() + new)].tolist() for u, p in enumerate(ps)]


def scripted(st, ps, new, kind, V, every=3, seed=5):
    """[B, new] drafts: the plain run's continuation (positions it never reached: 0), with every `every`-th token replaced, or random"""
    B = len(ps)
    d = torch.zeros((B, new), dtype=torch.int64, device=DEV)
    for u, p in enumerate(ps):
        d[u] = st["tokens"][u, p.numel():p.numel() + new]
    if kind == "corrupt":
        d[:, every - 1::every] = (d[:, every - 1::every] + 1) % V
    elif kind == "random":
        d = torch.randint(0, V, (B, new), generator=torch.Generator().manual_seed(seed)).to(DEV)
    return d


def same_run(want, st0, got, st1):
    assert len(want) == len(got)
    bad = [i for i, (a, b) in enumerate(zip(want, got)) if not torch.equal(a, b)]
    assert not bad, f"sequences {bad} differ from the speculate=0 run"
    assert torch.equal(st0["tokens"], st1["tokens"]), "the token buffers differ (something was written behind an EOS or a budget)"
    assert torch.equal(st0["length"], st1["length"])
    assert torch.equal(st0["done"] == 1, st1["done"] == 1)


def expected_counts(gen, drafts, D, eos=None):
    tot = dict(steps=0, drafted=0, accepted=0)
    for u, g in enumerate(gen):
        row = drafts[u].tolist() + [-1] * D
        r = replay(g, lambda k: row[k:k + D], D, eos_id=eos)
        tot["steps"] = max(tot["steps"], r["steps"])
        tot["drafted"] += r["drafted"]
        tot["accepted"] += r["accepted"]
    return tot


# ---- 1 + 2. the ids are those of speculate=0, the steps those of the acceptance rule ---------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_ids_and_step_accounting(model, D):
    cfg, m = model
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    want, st0 = plain_run(m, ps, NEW)
    assert all(o.numel() == p.numel() + NEW for o, p in zip(want, ps))
    gen = generated(st0, ps, NEW)
    for kind in ("true", "corrupt", "random"):
        drafts = scripted(st0, ps, NEW, kind, V)
        tm = {}
        got, st1 = generate_batch(m, ps, NEW, speculate=D, drafts=drafts, return_state=True, timing=tm, **KW)
        same_run(want, st0, got, st1)
        exp = expected_counts(gen, drafts, D)
        print(f"{cfg.name} D={D} {kind}: {tm['spec_steps']} steps, {tm['spec_accepted']} of {tm['spec_drafted']} drafts accepted")
        assert (tm["spec_steps"], tm["spec_drafted"], tm["spec_accepted"]) == (exp["steps"], exp["drafted"], exp["accepted"])
        if kind == "true":
            assert tm["spec_steps"] == -(-(NEW - 1) // (D + 1))
            # every draft of a full step is accepted; the final, partial step takes what the budget leaves
            assert tm["spec_accepted"] == len(ps) * (NEW - 1 - tm["spec_steps"])
        if kind == "random":
            assert tm["spec_steps"] > (NEW - 1) // 2            # next to nothing is accepted
    # a single sequence, through generate(), drafted by prompt lookup (a one-token prompt forwarded alone is a decode step, not a
    # prefill row: its plain run is generate()'s own, not the joint run's)
    for i in (0, 3):
        T = ps[i].numel()
        assert torch.equal(generate(m, ps[i], T + NEW, speculate=D, **KW), generate(m, ps[i], T + NEW, **KW).clone())


# ---- 1b. every query column of the MFMA ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HEAD_SIZES))
def test_ids_with_all_32_query_columns(name):
    """The three configs above have q_per_kv <= 2, so even D = 7 leaves query columns 16 .. 31 of the verify kernel's MFMAs at zero,
    as the single-token kernel always does.  8 heads over 2 groups (q_per_kv = 4) at D = 7 fill all 32 columns, the benchmark model's
    occupancy at D = 3, with free-running random-weight logits that a wrong attention row does move; D = 4 fills 20, a count that
    ends inside the upper half."""
    cfg, m = build(name, n_head=8, n_embd=8 * HEAD_SIZES[name], n_query_groups=2)
    assert 8 * (cfg.n_head // cfg.n_query_groups) == 32
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    want, st0 = plain_run(m, ps, NEW)
    gen = generated(st0, ps, NEW)
    for D in (7, 4):
        for kind in ("true", "corrupt", "random"):
            drafts = scripted(st0, ps, NEW, kind, V)
            tm = {}
            got, st1 = generate_batch(m, ps, NEW, speculate=D, drafts=drafts, return_state=True, timing=tm, **KW)
            same_run(want, st0, got, st1)
            exp = expected_counts(gen, drafts, D)
            assert (tm["spec_steps"], tm["spec_drafted"], tm["spec_accepted"]) == (exp["steps"], exp["drafted"], exp["accepted"])


# ---- 3. EOS and budgets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 3))
def test_eos_and_budgets(model, D):
    cfg, m = model
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)
    free, stf = plain_run(m, ps, NEW)
    genf = generated(stf, ps, NEW)
    # an EOS inside an accepted run (true drafts: generated index 2 is draft_2's pick when D = 3, draft_1's of the second step when
    # D = 1), as pick_0 (random drafts: every appended token is a pick_0), and on the very first sample
    for eos in (genf[2][2], genf[5][D + 1], genf[1][0], genf[4][NEW - 1]):
        want, st0 = plain_run(m, ps, NEW, eos_id=eos)
        gen = generated(st0, ps, NEW)
        assert any(g[-1] == eos for g in gen)
        for kind in ("true", "random"):
            drafts = scripted(stf, ps, NEW, kind, V)           # the EOS-free continuation: the drafts run on behind the EOS
            tm = {}
            got, st1 = generate_batch(m, ps, NEW, speculate=D, drafts=drafts, eos_id=eos, return_state=True, timing=tm, **KW)
            same_run(want, st0, got, st1)
            exp = expected_counts(gen, drafts, D, eos=eos)
            assert (tm["spec_steps"], tm["spec_drafted"], tm["spec_accepted"]) == (exp["steps"], exp["drafted"], exp["accepted"])
    # budgets that end on every place of a step, the smallest included
    for new in (1, 2, 3, 4, 5, 6):
        want, st0 = plain_run(m, ps[:6], new)
        drafts = scripted(stf, ps[:6], NEW, "true", V)[:, :new].contiguous()
        got, st1 = generate_batch(m, ps[:6], new, speculate=D, drafts=drafts, return_state=True, **KW)
        same_run(want, st0, got, st1)
        assert all(o.numel() == p.numel() + new for o, p in zip(got, ps))


# ---- 4. the KV cache ----------------------------------------------------------------------------------------------------------------
def cache_prefixes(m, cfg, lens):
    """[layer][K, V^T][sequence]: positions [0, 32 * floor((len - 1) / 32)) of the sequence's slot, every group"""
    eng = m._engine
    G, hs = cfg.n_query_groups, cfg.head_size
    out = []
    for l in range(cfg.n_layer):
        kv = [eng.read(w, l, (eng.max_batch, G, eng.s_max * hs)) for w in (1, 2)]
        out.append([[c[u, :, :32 * ((n - 1) // 32) * hs].clone() for u, n in enumerate(lens)] for c in kv])
    return out


@pytest.mark.parametrize("kind", ("true", "random"))
def test_kv_cache_equals_the_plain_runs(model, kind):
    cfg, m = model
    ps = ragged_prompts(cfg)
    want, st0 = plain_run(m, ps, NEW)
    lens = st0["length"].tolist()
    kv0 = cache_prefixes(m, cfg, lens)
    assert sum(c.numel() for c in kv0[0][0]) > 0 and all(c.any() for c in kv0[-1][1] if c.numel())
    m.refresh_engine()                              # nothing of the plain run is left in the cache
    got, st1 = generate_batch(m, ps, NEW, speculate=3, drafts=scripted(st0, ps, NEW, kind, cfg.padded_vocab_size), return_state=True, **KW)
    same_run(want, st0, got, st1)
    kv1 = cache_prefixes(m, cfg, lens)
    for l in range(cfg.n_layer):
        for w in range(2):
            for u in range(len(ps)):
                assert torch.equal(kv0[l][w][u], kv1[l][w][u]), f"layer {l} cache {w} sequence {u}"


# ---- 5. the proposer kernel ---------------------------------------------------------------------------------------------------------
ALPHABET = list(range(3, 11))


def test_device_proposer_equals_propose(model):
    """The lookup must find something, by construction and not by luck: the logit adapter's bias of this test's own model pushes
    every token outside an 8-token alphabet far below the rest, so whatever the model generates is one of the 8; a prompt opens
    with the alphabet twice (every token of it has an earlier occurrence that a token follows) and goes on with short phrases
    over it in random order, so the longer n-grams recur too."""
    cfg, _ = model
    cfg, m = build(cfg.name)
    bias = m.lm_head.adapter_bias.data
    out = torch.ones_like(bias, dtype=torch.bool)
    out[ALPHABET] = False
    bias[out] -= 30000.0
    m.refresh_engine()
    g = torch.Generator().manual_seed(9)
    ps = []
    for i in range(12):
        phrases = [torch.tensor(ALPHABET)[torch.randint(0, 8, (int(n),), generator=g)] for n in torch.randint(2, 6, (6,), generator=g)]
        order = torch.randint(0, 6, (10 + i,), generator=g).tolist()
        ps.append(torch.cat([torch.tensor(ALPHABET * 2)] + [phrases[k] for k in order])[: 90].to(DEV))
    ps.append(torch.tensor([5], device=DEV))        # nothing to look up behind a one-token prompt's first token, unless it repeats
    ps.append(torch.tensor([7, 8, 7, 8, 7], device=DEV))
    by_n = {1: 0, 2: 0, 3: 0}
    for D, new in ((3, 2), (3, 3), (2, 5), (7, 9), (1, 12), (3, 20)):
        want, st0 = plain_run(m, ps, new)
        assert all(t in ALPHABET for u, p in enumerate(ps) for t in want[u][p.numel():].tolist()), "the bias must confine the ids"
        got, st1 = generate_batch(m, ps, new, speculate=D, return_state=True, **KW)
        same_run(want, st0, got, st1)
        drafts, at = st1["spec_drafts"].tolist(), st1["spec_len"].tolist()
        for u in range(len(ps)):
            row = st1["tokens"][u, :at[u]].tolist()
            exp = propose(row, D)
            assert drafts[u] == exp, f"D={D} new={new} sequence {u}: the device drafted {drafts[u]} behind {row[-6:]}, propose() {exp}"
            if u < 12:
                assert at[u] > ps[u].numel() and row[-1] in row[:-1], "a match exists by construction"
                n = max(k for k in (1, 2, 3) if any(row[i:i + k] == row[-k:] for i in range(len(row) - k)))
                by_n[n] += 1
    print(f"{cfg.name}: longest matching n-gram over the 72 proposals of the phrase prompts: {by_n}")
    # the proposer's n = 3 and n = 2 branches are taken, not only its last resort: 8 tokens and recurring phrases make both certain
    assert by_n[2] > 0 and by_n[3] > 0 and sum(by_n.values()) == 72


# ---- 6. real data: the benchmark's shape at full depth -------------------------------------------------------------------------------
def test_full_tinyllama_512_ids(golden):
    """tests/golden/full_tinyllama_512 (22 layers, a 512-token prompt, 64 tokens of the REFERENCE's generate()): with D = 3 — four
    positions of 8 heads per KV group fill the 32 query columns — the ids are the plain run's, and they pass the fixture's
    free-running gates of tests/test_hip_model.py:test_full_tinyllama_512_vs_reference evaluated the same way (product-default rsqrt
    rounding: all 64 ids equal the reference's), alone and as a row of a joint decode, scripted and looked-up drafts."""
    sys.path.insert(0, str(ROOT / "tests"))
    import test_hip_model as TM
    t, meta = golden("full_tinyllama_512")
    cfg, m = TM.build(meta)
    m.cpu_rsqrt_vec_width = 0
    T, G = meta["T"], meta["G"]
    ids, margins = t["generate_ids"], t["generate_margins_ulps"]
    assert G == 64 and T == 512 and float(margins.min()) >= 16, "fixture must be tie-free on every step"
    idx = t["idx"].to(DEV)
    free0 = generate(m, idx, T + G, **KW).cpu()
    tm = {}
    spec = generate_batch(m, [idx], G, speculate=3, timing=tm, **KW)[0].cpu()
    print(f"full_tinyllama_512, prompt lookup, D=3: {tm['spec_steps']} steps for {G - 1} tokens, {tm['spec_accepted']} of {tm['spec_drafted']} accepted")
    assert torch.equal(spec, free0)
    assert TM._equal_prefix(spec[T:], ids[T:]) == G and torch.equal(spec, ids)
    g = torch.Generator().manual_seed(3)
    V = cfg.padded_vocab_size
    prompts = [torch.cat([torch.ones(1, dtype=torch.int64), torch.randint(3, V, (T - 1,), generator=g)]).to(DEV) for _ in range(8)]
    prompts[5] = idx
    want = [o.clone() for o in generate_batch(m, prompts, G, **KW)]
    drafts = torch.stack([o[T:] for o in want])
    tm = {}
    joint = generate_batch(m, prompts, G, speculate=3, drafts=drafts.contiguous(), timing=tm, **KW)
    assert all(torch.equal(a, b) for a, b in zip(want, joint)) and torch.equal(joint[5].cpu(), ids)
    assert tm["spec_steps"] == -(-(G - 1) // 4)


# ---- 7. defaults ----------------------------------------------------------------------------------------------------------------------
def test_speculate_0_captures_what_it_always_did(model):
    cfg, m = model
    ps = ragged_prompts(cfg)[:5]
    m.refresh_engine()
    tm = {}
    want = [o.clone() for o in generate_batch(m, ps, NEW, timing=tm, **KW)]
    eng = m._engine
    n0 = eng.graph_count(-1)
    assert n0 == 1 and eng.graph_count(0) == 1 and not any(eng.graph_count(d) for d in range(1, 8))
    assert not any(k.startswith("spec_") for k in tm) and tm["decode_steps"] == NEW - 1
    assert all(torch.equal(a, b) for a, b in zip(want, generate_batch(m, ps, NEW, speculate=0, **KW)))
    assert m._engine is eng and eng.graph_count(-1) == eng.graph_count(0) <= 2
    # a speculative call keys its step by D and leaves the plain step's key alone
    got = generate_batch(m, ps, NEW, speculate=2, **KW)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    eng = m._engine
    assert eng.graph_count(2) >= 1 and eng.graph_count(3) == 0
    n_plain = eng.graph_count(0)
    assert all(torch.equal(a, b) for a, b in zip(want, generate_batch(m, ps, NEW, **KW)))
    assert m._engine.graph_count(0) >= max(n_plain, 1) and m._engine.graph_count(2) >= 1
