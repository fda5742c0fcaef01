"""Shared-prompt attention through the engine (dh_engine_set_shared_prompt; include/dualhyp_hip.h, "Shared-prompt attention"):
sample_batch(shared_prompt=True) and beam_search_batch(shared_prompt=True) give what the calls without the flag give — every id,
log-probability, alternative, parent, score, pool entry and flag, bit for bit — while the steps launch the shared kernel; with
the flag off the steps launch what they always launched; and the setter and the calls refuse what the kernel does not serve.
The op itself, against the single-token op: tests/test_hip_shared_attn.py."""
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import _lib, beam_search_batch, sample_batch
from dualhyp_amd._lib import DualHypHipError
from dualhyp_amd.synth import synth_prompts

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_hip_prefix import DEV, build, sharing_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
N = 3
NEW = 40                                # every row crosses a tile edge: 31 .. 70 prompt tokens + 40
LENS = [31, 32, 33, 50, 64, 70]
KW = dict(temperature=0.8, top_k=5, seed=99)
MODELS = ("parity-tiny", "parity-hs96", "parity-hs128")


def launches():
    return int(_lib.load().dh_attn_shared_launch_count())


def bits(t):
    """NaN-filled float buffers compare by their bits"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def prompts_of(cfg, lens=LENS):
    return [synth_prompts(1, n, cfg.padded_vocab_size, seed=300 + i)[0].to(DEV) for i, n in enumerate(lens)]


def same_samples(a, b, what):
    (out_a, st_a), (out_b, st_b) = a, b
    assert set(st_a) == set(st_b)
    for key in st_a:            # the device state: ids, lengths, done flags, log-probabilities, alternatives, automaton states
        assert torch.equal(bits(st_a[key]), bits(st_b[key])), f"{what}: state[{key!r}] differs under shared_prompt"
    for u, (sa, sb) in enumerate(zip(out_a, out_b)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert set(x) == set(y)
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(bits(x["token_logprobs"]), bits(y["token_logprobs"])), f"{what}: ({u}, {j})"
            assert x["sum_logprob"] == y["sum_logprob"] and x["avg_logprob"] == y["avg_logprob"] and x["finish_reason"] == y["finish_reason"]
            if "top_logprobs" in x:
                assert all(torch.equal(bits(p), bits(q)) for p, q in zip(x["top_logprobs"], y["top_logprobs"])), f"{what}: alternatives of ({u}, {j})"


def run_samples(m, prompts, shared, **kw):
    m.refresh_engine()          # a zeroed cache: a slot nobody filled cannot hold the right bytes by chance
    c0 = launches()
    tm = {}
    out, st = sample_batch(m, prompts, NEW, num_samples=N, return_state=True, timing=tm, shared_prompt=shared, **kw)
    st = {k: v.clone() for k, v in st.items()}
    assert tm["shared_prompt"] is shared
    return (out, st), launches() - c0


def ragged_eos(state, lens):
    """a token of the EOS-free run that ends some rows in the first half of the budget while one row runs to the end"""
    tokens = state["tokens"].cpu()
    best, best_n = None, 0
    gen = [tokens[r, lens[r // N]:lens[r // N] + NEW] for r in range(tokens.size(0))]
    for eos in range(int(tokens.max()) + 1):
        n = [int((g == eos).nonzero()[0]) + 1 if (g == eos).any() else NEW for g in gen]
        early = sum(a <= NEW // 2 for a in n)
        if max(n) == NEW and early > best_n:
            best, best_n = eos, early
    return best


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    cfg, m = build(request.param)
    return cfg, m, prompts_of(cfg)


def test_sample_batch_shared_equals_unshared(setup):
    cfg, m, prompts = setup
    free, d0 = run_samples(m, prompts, False, **KW)
    assert d0 == 0, "without the flag a step launches the kernels it always launched"
    eos = ragged_eos(free[1], LENS)
    assert eos is not None, "no token ends a row early"
    want, d0 = run_samples(m, prompts, False, eos_id=eos, top_logprobs=2, **KW)
    got, d1 = run_samples(m, prompts, True, eos_id=eos, top_logprobs=2, **KW)
    assert d0 == 0 and d1 >= cfg.n_layer and d1 % cfg.n_layer == 0, f"the shared step holds the new kernel once per layer: {d1} launches"
    done = want[1]["done"].tolist()
    assert 1 in done and set(done) & {0, 2}, "rows must finish raggedly"
    same_samples(got, want, "eos + top_logprobs")
    # without an EOS: one decode call of 39 steps
    got, d1 = run_samples(m, prompts, True, **KW)
    assert d1 >= cfg.n_layer
    same_samples(got, free, "no eos")


def test_sample_batch_shared_composes(setup):
    """share_prefix, a token mask, no_repeat_ngram, a penalty and top_p together."""
    cfg, m, _ = setup
    V = cfg.padded_vocab_size
    prompts = sharing_prompts(cfg, [1, 9, 25, 12, 30], shared=40)           # 41 .. 70 tokens behind a shared tile: P = 32
    mask = [sorted(set(range(u % 3, V, 3)) | {7}) for u in range(len(prompts))]
    kw = dict(share_prefix=True, token_mask=mask, no_repeat_ngram=3, repetition_penalty=1.3, top_p=0.9, eos_id=7, **KW)
    want, d0 = run_samples(m, prompts, False, **kw)
    got, d1 = run_samples(m, prompts, True, **kw)
    assert d0 == 0 and d1 >= cfg.n_layer
    same_samples(got, want, "share_prefix + mask + ngram + penalty + top_p")


def run_beams(m, prompts, W, shared, **kw):
    m.refresh_engine()
    c0 = launches()
    tm = {}
    out, st = beam_search_batch(m, prompts, NEW, num_beams=W, return_state=True, timing=tm, shared_prompt=shared, **kw)
    assert tm["shared_prompt"] is shared
    blocks = {str(k): v.clone() for k, v in st["beam"]._blocks.items()}
    return (out, blocks, st["host"]), launches() - c0


@pytest.mark.parametrize("history", ("host", "device"))
@pytest.mark.parametrize("W", (2, 4))
def test_beam_search_shared_equals_unshared(setup, W, history):
    cfg, m, prompts = setup
    free, d0 = run_beams(m, prompts, W, False, history=history)
    assert d0 == 0
    # an EOS the free run's best hypothesis of utterance 0 produces mid-way: pool entries, and utterances that end at different steps
    eos = int(free[0][0][0]["tokens"][LENS[0] + 10])
    kw = dict(eos_id=eos, history=history, **(dict(no_repeat_ngram=3) if history == "device" else {}))
    want, d0 = run_beams(m, prompts, W, False, **kw)
    got, d1 = run_beams(m, prompts, W, True, **kw)
    assert d0 == 0 and d1 >= cfg.n_layer and d1 % cfg.n_layer == 0
    assert any(n > 0 for n in want[2]["n_fin"]), "no hypothesis ended on the EOS"
    assert len(set(want[2]["n_steps"])) > 1 or max(want[2]["n_steps"]) == NEW
    for key in want[1]:             # every token, parent, score and pool entry of the state, by its bits
        assert torch.equal(bits(got[1][key]), bits(want[1][key])), f"W {W} history {history}: the beam state's {key} block differs"
    if history == "device":
        assert got[2]["history"] == want[2]["history"]
    for u, (ha, hb) in enumerate(zip(got[0], want[0])):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(bits(x["token_logprobs"]), bits(y["token_logprobs"]))
            assert x["sum_logprob"] == y["sum_logprob"] and x["finished"] == y["finished"] and x["finish_reason"] == y["finish_reason"], u


def test_flag_is_part_of_the_step_key():
    """The same engine, flag off, on, off: the shared step is a capture of its own that holds the new kernel once per layer, and the
    step captured behind it (a call's buffers are new, so its step is captured anew) holds none: nothing is left set."""
    cfg, m = build("parity-tiny")
    prompts = prompts_of(cfg)
    m.refresh_engine()
    off = sample_batch(m, prompts, NEW, num_samples=N, return_state=True, **KW)
    eng = m._engine
    g0, c0 = eng.graph_count(0), launches()
    on = sample_batch(m, prompts, NEW, num_samples=N, return_state=True, shared_prompt=True, **KW)
    assert m._engine is eng and eng.graph_count(0) == g0 + 1 and launches() == c0 + cfg.n_layer
    off2 = sample_batch(m, prompts, NEW, num_samples=N, return_state=True, **KW)
    assert m._engine is eng and launches() == c0 + cfg.n_layer, "nothing is left set: the plain step holds the kernels it always held"
    same_samples(on, off, "on")
    same_samples(off2, off, "off again")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_setter_and_calls_refuse():
    cfg, m = build("parity-tiny")
    m.refresh_engine()
    R, T = 6, 64
    eng = m.engine(R, T, R * 8, exact=True)
    plen = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    c0 = launches()
    for n, word in ((1, "group_rows=1"), (9, "group_rows=9"), (-2, "group_rows=-2")):
        with pytest.raises(DualHypHipError, match=word):
            eng.set_shared_prompt(n, plen)
    with pytest.raises(TypeError):
        eng.set_shared_prompt(3, plen.long())
    # the CPU rsqrt emulation and dh_set_tuning key 10
    eng.set_rsqrt_emulation(32, whole_call=False)
    with pytest.raises(DualHypHipError, match="rsqrt"):
        eng.set_shared_prompt(3, plen)
    eng.set_rsqrt_emulation(0, whole_call=False)
    lib = _lib.load()
    _lib.check(lib.dh_set_tuning(10, 4))
    try:
        with pytest.raises(DualHypHipError, match="key 10"):
            eng.set_shared_prompt(3, plen)
    finally:
        _lib.check(lib.dh_set_tuning(10, 0))
    # set: the calls that cannot run under it say so before they launch anything
    eng.set_shared_prompt(3, plen)
    tokens = torch.zeros((R, T), dtype=torch.int64, device=DEV)
    length, done, limit = torch.full((R,), 6, **i32), torch.zeros(R, **i32), torch.full((R,), 20, **i32)
    try:
        with pytest.raises(DualHypHipError, match="no multiple"):
            eng.decode(tokens[:4], length[:4], done[:4], 1, 1.0, 5, None, 1)
        eng.set_rsqrt_emulation(32, whole_call=False)           # set behind the setter's back: the call checks again
        with pytest.raises(DualHypHipError, match="rsqrt"):
            eng.decode(tokens, length, done, 1, 1.0, 5, None, 1)
        eng.set_rsqrt_emulation(0, whole_call=False)
        with pytest.raises(DualHypHipError, match="row list"):
            eng.decode_rows(tokens, length, done, limit, 8, R, 1, 1.0, 5, None, 1)
        eng.reserve_rows(2 * R)
        with pytest.raises(DualHypHipError, match="verify step"):
            eng.decode_spec(tokens, length, done, limit, 8, 1, None, torch.zeros(3, **i32), 1, 1.0, None)
        from dualhyp_amd.beam import BeamState
        eng.reserve_beams(2, 8)
        with pytest.raises(DualHypHipError, match="W=2"):
            eng.decode_beam(BeamState(2, 2, 8, DEV), plen, 1, None, first_step=1)
    finally:
        eng.set_shared_prompt()
    assert launches() == c0 and eng.graph_count(-1) == 0
    # off again: the plain call runs
    eng.decode(tokens[:4], length[:4], done[:4], 1, 1.0, 5, None, 1)
    assert launches() == c0


def test_fp8_engine_refuses():
    cfg, m = build("parity-hs128", fp8=True)
    m.refresh_engine()
    eng = m.engine(6, 64, 48, exact=True)
    plen = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    with pytest.raises(DualHypHipError, match="fp8"):
        eng.set_shared_prompt(3, plen)
    with pytest.raises(ValueError, match="fp8"):
        sample_batch(m, prompts_of(cfg)[:2], 4, num_samples=N, shared_prompt=True, **KW)
    # and an fp8 KV cache, which only an fp8 engine has
    from dualhyp_amd import quantize_model_fp8
    quantize_model_fp8(m, kv_cache="fp8")
    eng = m.engine(6, 64, 48, exact=True)
    with pytest.raises(DualHypHipError, match="fp8"):
        eng.set_shared_prompt(3, plen)


def test_python_refusals_launch_nothing():
    cfg, m = build("parity-tiny")
    prompts = prompts_of(cfg)[:2]
    c0 = launches()
    with pytest.raises(ValueError, match="shared_prompt"):
        beam_search_batch(m, prompts, 4, num_beams=1, shared_prompt=True)
    with pytest.raises(ValueError, match="shared_prompt"):
        sample_batch(m, prompts, 4, num_samples=N, shared_prompt=1, **KW)
    m.cpu_rsqrt_vec_width = 32
    try:
        with pytest.raises(ValueError, match="rsqrt"):
            sample_batch(m, prompts, 4, num_samples=N, shared_prompt=True, **KW)
    finally:
        m.cpu_rsqrt_vec_width = 0
    assert launches() == c0
