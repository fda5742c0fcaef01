"""Sampled verification on the GPU (generate_batch(..., speculate=D, verify="draw"), dh_engine_decode_spec_draw): a verify position
draws with the key the plain sampled step would have used — (seed, tokens generated so far, sequence) — and a draft is kept exactly when
it equals the draw.  Every check is exact (torch.equal): ids, lengths, done flags, log-probabilities, alternatives and automaton states
are those of the same call with speculate=0 whatever is drafted; the step counters are the host replay's of the acceptance rule."""
import pytest
import torch

from dualhyp_amd import GPT, Config, generate_batch, sample_batch
from dualhyp_amd import automaton as A
from dualhyp_amd.speculate import propose, replay
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = 24                      # 23 verify-step tokens: not a multiple of D + 1 for D = 1, 3, 7 — the budget ends inside a step
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
DS = (1, 3, 7)
T = 1.0                       # with the synthetic weights: hot enough that a quarter of the picks leave the arg-max (test 1 asserts it)
KS = (5, 40)
SEED = 4242
LENS = (20, 31, 33, 47, 64, 70)          # ragged; positions up to 70 + 24 + 7 fit the model's 128
EOS = 2                       # no prompt holds it (synth_prompts: BOS 1, then ids >= 3)


def build():
    cfg = Config.from_name("parity-tiny", **LORA)
    sd = synth_state_dict(cfg, seed=11, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.eval()
    ps = [synth_prompts(1, n, cfg.padded_vocab_size, seed=70 + i)[0].to(DEV) for i, n in enumerate(LENS)]
    return cfg, m, ps


@pytest.fixture(scope="module")
def model():
    return build()


ALPHABET = list(range(3, 11))


@pytest.fixture(scope="module")
def narrow_model():
    """The same model whose logit adapter's bias pushes every token outside an 8-token alphabet far below the rest: 23 bigrams over 64
    possibilities repeat by construction, so no_repeat_ngram=2 has something to ban at temperature 1."""
    cfg, m, ps = build()
    bias = m.lm_head.adapter_bias.data
    out = torch.ones_like(bias, dtype=torch.bool)
    out[ALPHABET] = False
    bias[out] -= 30000.0
    m.refresh_engine()
    return cfg, m, ps


def run(m, ps, new=NEW, **kw):
    """One call -> dict(out, lp, top_ids, top_lp: per-sequence tensors; tokens, length, done[, aut]: the state; tm: the timing)"""
    kw = dict(dict(temperature=T, seed=SEED), **kw)
    tm = {}
    out, lp, top, st = generate_batch(m, ps, new, return_logprobs=True, top_logprobs=1, return_state=True, timing=tm, **kw)
    r = dict(out=[o.clone() for o in out], lp=[v.clone() for v in lp], top_ids=[a.clone() for a, _ in top], top_lp=[b.clone() for _, b in top],
             tokens=st["tokens"].clone(), length=st["length"].clone(), done=st["done"].clone(), tm=tm)
    if "automaton_state" in st:
        r["aut"] = st["automaton_state"].clone()
    return r


_REFS = {}


def reference(model, K, new=NEW, **kw):
    """the speculate=0 run of a call, computed once per distinct call and never changed"""
    cfg, m, ps = model
    key = (K, new, repr(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = run(m, ps, new, top_k=K, **kw)
    return _REFS[key]


def generated(r, ps):
    """per sequence: the tokens the run produced, the EOS included"""
    ln = r["length"].tolist()
    return [r["tokens"][u, p.numel():ln[u]].tolist() for u, p in enumerate(ps)]


def flags(done):
    """The done flags with the budget's two spellings as one: the plain step flags a spent budget (2) only at the end of the token
    buffer, so a prompt shorter than the call's longest ends on its budget with its flag still 0, where a verify step (either mode,
    by its contract) writes 2 — stop.finish_reasons reads both as "length".  1 (EOS) and 3 (stop) are compared as they are."""
    return torch.where(done == 0, torch.full_like(done, 2), done)


def same(want, got, what=""):
    for name in ("out", "lp", "top_ids", "top_lp"):
        bad = [u for u, (a, b) in enumerate(zip(want[name], got[name])) if not torch.equal(a, b)]
        assert not bad, f"{what}: {name} of sequences {bad} differ from the speculate=0 run"
    for name in ("tokens", "length") + (("aut",) if "aut" in want else ()):
        assert torch.equal(want[name], got[name]), f"{what}: the state's {name} differs from the speculate=0 run"
    assert torch.equal(flags(want["done"]), flags(got["done"])), f"{what}: the done flags differ from the speculate=0 run"
    assert all(v.numel() == 0 or not bool(torch.isnan(v).any()) for v in got["lp"])


def scripted(gen, kind, V, new=NEW):
    """[B, new] drafts from the reference's generated ids: drafts[u, i] is proposed as generated token i"""
    d = torch.zeros((len(gen), new), dtype=torch.int64)
    for u, g in enumerate(gen):
        d[u, :len(g)] = torch.tensor(g[:new], dtype=torch.int64)
    if kind == "wrong":
        d = (d + 1) % V
    elif kind == "prefix":                  # right up to a per-sequence position, then wrong
        for u in range(len(gen)):
            d[u, 3 + 2 * u:] = (d[u, 3 + 2 * u:] + 1) % V
    elif kind == "shifted":                 # the right ids, one place early
        d = torch.cat([d[:, 1:], d[:, -1:]], dim=1)
    else:
        assert kind == "right"
    return d.to(DEV).contiguous()


def expected_counts(ps, gen, drafts, D, eos=None):
    tot = dict(steps=0, drafted=0, accepted=0)
    for u, g in enumerate(gen):
        if drafts is None:                  # prompt lookup on the sequence's own text
            text = ps[u].tolist() + g
            fn = lambda k, text=text, n=ps[u].numel(): propose(text[:n + k], D)
        else:
            row = drafts[u].tolist() + [-1] * D
            fn = lambda k, row=row: row[k:k + D]
        r = replay(g, fn, D, eos_id=eos)
        tot["steps"] = max(tot["steps"], r["steps"])
        tot["drafted"] += r["drafted"]
        tot["accepted"] += r["accepted"]
    return tot


def counters(r):
    return dict(steps=r["tm"]["spec_steps"], drafted=r["tm"]["spec_drafted"], accepted=r["tm"]["spec_accepted"])


# ---- 1. the reference really samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_reference_leaves_the_argmax(model, K):
    cfg, m, ps = model
    ref = reference(model, K)
    off = [int((torch.tensor(g) != ref["top_ids"][u][:, 0].cpu()).sum()) for u, g in enumerate(generated(ref, ps))]
    print(f"top_k={K} T={T}: picks off the arg-max per sequence {off} of {NEW}")
    assert all(o.numel() == p.numel() + NEW for o, p in zip(ref["out"], ps))
    assert sum(off) * 4 >= len(ps) * NEW, "at least a quarter of the generated tokens differ from the row's arg-max"
    assert all(n >= 1 for n in off), "every sequence has such a token"


# ---- 2. exact, whatever is drafted ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_ids_logprobs_and_step_accounting(model, D, K):
    cfg, m, ps = model
    V = cfg.padded_vocab_size
    ref = reference(model, K)
    gen = generated(ref, ps)
    for kind in ("right", "wrong", "prefix", "shifted", None):
        drafts = None if kind is None else scripted(gen, kind, V)
        got = run(m, ps, top_k=K, speculate=D, verify="draw", drafts=drafts)
        same(ref, got, f"D={D} K={K} {kind}")
        exp = expected_counts(ps, gen, drafts, D)
        print(f"D={D} K={K} {kind}: {counters(got)}")
        assert counters(got) == exp, kind
        if kind == "right":                 # drafts are really being accepted: the step count is the rule's ceiling
            assert exp["steps"] == -(-(NEW - 1) // (D + 1)) and exp["accepted"] == len(ps) * (NEW - 1 - exp["steps"])
        if kind == "wrong":
            assert exp["accepted"] == 0 and exp["steps"] == NEW - 1


# ---- 3. ends ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 3))
def test_ends(model, D):
    cfg, m, ps = model
    V = cfg.padded_vocab_size
    K = 5
    free = reference(model, K)
    genf = generated(free, ps)
    # an EOS the reference emits mid-sequence (as draft_2's pick of the second step when D = 3), and an EOS on the first pick
    for eos in (genf[2][6], genf[1][0]):
        ref = reference(model, K, eos_id=eos)
        gen = generated(ref, ps)
        assert any(g[-1] == eos and len(g) < NEW for g in gen)
        for kind in ("right", "wrong", None):
            drafts = None if kind is None else scripted(genf, kind, V)      # the EOS-free continuation: the drafts run on behind the EOS
            got = run(m, ps, top_k=K, eos_id=eos, speculate=D, verify="draw", drafts=drafts)
            same(ref, got, f"eos={eos} {kind}")
            assert counters(got) == expected_counts(ps, gen, drafts, D, eos=eos)
    # budgets that end on every place of a step, the smallest included
    for new in (1, 2, 3, 4, 6):
        ref = reference(model, K, new=new)
        got = run(m, ps, new, top_k=K, speculate=D, verify="draw", drafts=scripted(genf, "right", V)[:, :new].contiguous())
        same(ref, got, f"new={new}")
        assert all(o.numel() == p.numel() + new for o, p in zip(got["out"], ps))
    # a stop id and a stop sequence of 2 ids whose last id falls at position j > 0 of a step: with the right drafts generated token i
    # is position (i - 1) % (D + 1) of its step
    for stop, u in (([genf[3][6]], 3), ([[genf[4][5], genf[4][6]]], 4)):     # i = 6: position 1 of its step for D = 1 and for D = 3
        ref = reference(model, K, stop=stop)
        i = int(ref["length"][u]) - ps[u].numel() - 1
        assert int(ref["done"][u]) == 3 and i >= 1 and (i - 1) % (D + 1) > 0, (stop, i)
        for kind in ("right", "wrong", None):
            got = run(m, ps, top_k=K, stop=stop, speculate=D, verify="draw", drafts=None if kind is None else scripted(genf, kind, V))
            same(ref, got, f"stop={stop} {kind}")


# ---- 4. the sampler's options -----------------------------------------------------------------------------------------------------------
BIAS = [([17, 45, 99], 12.0), ([200], -4.0)]


def controls(ps):
    V = 256
    allowed = [[t for t in range(V) if t % 4 != 0 or t == EOS] for _ in ps]
    return dict(
        nucleus=dict(top_p=0.9, min_p=0.05),
        penalties=dict(repetition_penalty=1.3, frequency_penalty=0.4, presence_penalty=0.3),
        bias=dict(bias=BIAS),
        ngram=dict(no_repeat_ngram=2),
        mask=dict(token_mask=allowed),
        automaton=dict(automaton=lambda: A.from_prompts([p.tolist() for p in ps], order=2, eos_id=EOS)),
    )


@pytest.mark.parametrize("name", ("nucleus", "penalties", "bias", "ngram", "mask", "automaton", "all"))
def test_controls(model, narrow_model, name):
    cfg, m, ps = narrow_model if name == "ngram" else model
    V = cfg.padded_vocab_size
    K, D = 40, 3
    cs = controls(ps)
    kw = dict(eos_id=EOS)
    for k in (cs if name == "all" else (name,)):
        kw.update(cs[k])
    opts = lambda: {k: (v() if callable(v) else v) for k, v in kw.items()}     # a fresh automaton set (its state buffer) per call
    plain = run(m, ps, top_k=K, eos_id=EOS) if name == "ngram" else reference(model, K, eos_id=EOS)
    ref = run(m, ps, top_k=K, **opts())
    gen = generated(ref, ps)
    assert any(not torch.equal(a, b) for a, b in zip(plain["out"], ref["out"])), f"{name} changed no token: the case proves nothing"
    if name in ("automaton", "all"):
        assert "aut" in ref
    if name == "bias":
        # the entry's continuation is proposed at j > 0 from a pick of the same step: somewhere 17 was generated at index i - 1 and 45 at
        # i, with i at position j = (i - 1) % (D + 1) > 0 of its step under the right drafts
        hits = [(u, i) for u, g in enumerate(gen) for i in range(2, len(g)) if g[i - 1] == 17 and g[i] == 45 and (i - 1) % (D + 1) > 0]
        assert hits, "the bias entry never continued inside a step"
    for kind in ("right", "prefix", "wrong", None):
        drafts = None if kind is None else scripted(gen, kind, V)
        got = run(m, ps, top_k=K, speculate=D, verify="draw", drafts=drafts, **opts())
        same(ref, got, f"{name} {kind}")
        assert counters(got) == expected_counts(ps, gen, drafts, D, eos=EOS), (name, kind)
        if kind == "right":
            assert got["tm"]["spec_accepted"] > 0


# ---- 5. top_k = 1 is the arg-max verification ---------------------------------------------------------------------------------------------
def test_top_k_1_equals_argmax_verification(model):
    cfg, m, ps = model
    ref = reference(model, 1)
    gen = generated(ref, ps)
    for D in DS:
        for drafts in (None, scripted(gen, "right", cfg.padded_vocab_size), scripted(gen, "prefix", cfg.padded_vocab_size)):
            a = run(m, ps, top_k=1, speculate=D, drafts=drafts)
            b = run(m, ps, top_k=1, speculate=D, drafts=drafts, verify="draw")
            same(ref, a, "argmax")
            same(ref, b, "draw")
            assert counters(a) == counters(b) == expected_counts(ps, gen, drafts, D)


# ---- 6. keys --------------------------------------------------------------------------------------------------------------------------
def test_seeds_and_modes_never_replay_one_another(model):
    cfg, m, ps = model
    K, D = 5, 3
    r1, r2 = reference(model, K, seed=101), reference(model, K, seed=202)
    assert any(not torch.equal(a, b) for a, b in zip(r1["out"], r2["out"])), "two seeds, two texts"
    greedy = run(m, ps, top_k=1, speculate=D)
    for order in ((101, 202), (202, 101), (101, 202)):
        for s in order:
            got = run(m, ps, top_k=K, seed=s, speculate=D, verify="draw")
            same(r1 if s == 101 else r2, got, f"seed {s}")
            assert any(not torch.equal(a, b) for a, b in zip(got["out"], (r2 if s == 101 else r1)["out"]))
    # top_k and top_p are part of the key as well
    same(reference(model, 40, seed=101), run(m, ps, top_k=40, seed=101, speculate=D, verify="draw"), "top_k 40")
    same(reference(model, 40, seed=101, top_p=0.5), run(m, ps, top_k=40, seed=101, top_p=0.5, speculate=D, verify="draw"), "top_p")
    again = run(m, ps, top_k=1, speculate=D)
    same(greedy, again, "the arg-max call behind the draw calls")
    assert counters(greedy) == counters(again)
    same(reference(model, 1), greedy, "the arg-max call")


# ---- 7. sampled candidates ----------------------------------------------------------------------------------------------------------------
def test_sample_batch(model):
    cfg, m, ps = model
    kw = dict(num_samples=3, temperature=T, top_k=40, top_p=0.95, seed=SEED, eos_id=EOS, top_logprobs=2, repetition_penalty=1.2)
    want = sample_batch(m, ps[:4], NEW, **kw)
    tm = {}
    got = sample_batch(m, ps[:4], NEW, speculate=3, verify="draw", timing=tm, **kw)
    assert len(want) == len(got) == 4
    for u, (a, b) in enumerate(zip(want, got)):
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["token_logprobs"], y["token_logprobs"]), u
            assert x["sum_logprob"] == y["sum_logprob"] and x["avg_logprob"] == y["avg_logprob"] and x["finish_reason"] == y["finish_reason"]
            assert torch.equal(x["top_logprobs"][0], y["top_logprobs"][0]) and torch.equal(x["top_logprobs"][1], y["top_logprobs"][1])
        assert any(not torch.equal(a[0]["tokens"], s["tokens"]) for s in a[1:]), "the candidates of an utterance differ"
    assert tm["spec_steps"] >= 1 and tm["spec_drafted"] >= 3 * 12 and tm["spec_drafted"] % 3 == 0
    # scripted drafts: every row is handed its own continuation, so the steps are the rule's ceiling for the longest row
    rows = [s["token_logprobs"].numel() for a in want for s in a]
    drafts = torch.zeros((12, NEW), dtype=torch.int64)
    st = sample_batch(m, ps[:4], NEW, return_state=True, **kw)[1]
    for r in range(12):
        n = ps[r // 3].numel()
        drafts[r] = st["tokens"][r, n:n + NEW].cpu()
    tm = {}
    got = sample_batch(m, ps[:4], NEW, speculate=3, verify="draw", drafts=drafts, timing=tm, **kw)
    assert all(torch.equal(x["tokens"], y["tokens"]) for a, b in zip(want, got) for x, y in zip(a, b))
    assert tm["spec_steps"] == -(-(max(rows) - 1) // 4) and tm["spec_accepted"] > 0
