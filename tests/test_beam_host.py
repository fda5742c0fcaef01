"""Host side of beam search (beam_search_batch, include/dualhyp_hip.h "Beam search"): the definition's worked example and its rules
on scripted candidate lists (tests/beam_reference.py), the host's backtracking and ranking (dualhyp_amd/beam.py) on states written
by hand, the refusals that are raised before anything touches the GPU, the CLI flags and record fields, and the C-ABI entries
(header, exports, ctypes table)."""
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_reference as R  # noqa: E402

G = importlib.import_module("dualhyp_amd.generate")
B = importlib.import_module("dualhyp_amd.beam")
NEW_ENTRIES = ("dh_beam_select_bf16", "dh_engine_reserve_beams", "dh_engine_decode_beam")


def utt(W, max_new, eos, cum, hist=None):
    u = R.Utterance(W, max_new, eos)
    u.cum = [np.float32(c) for c in cum]
    u.hist = hist if hist is not None else [([100 + b], [np.float32(c)]) for b, c in enumerate(cum)]
    u.n_steps = 1
    u.records = [[dict(parent=0, tok=100 + b, lp=np.float32(c), cum=np.float32(c)) for b, c in enumerate(cum)]]
    return u


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def test_worked_example():
    u = utt(2, 8, 2, [-1.0, -1.5])
    rows = [[(7, -0.5), (2, -1.0), (3, -2.0), (9, -3.0)], [(2, -0.25), (5, -0.5), (1, -4.0), (0, -5.0)]]
    order = u.ordered(rows)
    assert [(c["b"], c["tok"], float(c["score"])) for c in order[:4]] == [(0, 7, -1.5), (1, 2, -1.75), (0, 2, -2.0), (1, 5, -2.0)]
    u.step(rows)
    assert [(r["parent"], r["tok"], float(r["cum"])) for r in u.records[-1]] == [(0, 7, -1.5), (1, 5, -2.0)]
    assert [(h["step"], h["parent"], float(h["score"])) for h in u.pool] == [(1, 1, -1.75)]      # position 2's EOS was dropped
    assert u.done == 0 and [float(c) for c in u.cum] == [-1.5, -2.0]


def test_ties_across_beams_and_ranks():
    # every score ties at -2: the order is beam, then rank
    u = utt(2, 8, None, [-1.0, -1.0])
    u.step([[(4, -1.0), (5, -1.0), (6, -1.0), (7, -1.0)], [(4, -1.0), (8, -1.0), (9, -1.0), (3, -1.0)]])
    assert [(r["parent"], r["tok"]) for r in u.records[-1]] == [(0, 4), (0, 5)]
    # beam 1's rank 0 ties with beam 0's rank 1: the lower beam goes first, whatever the rank
    u = utt(2, 8, None, [-1.0, -2.0])
    u.step([[(4, -0.5), (5, -1.5), (6, -3.0), (7, -4.0)], [(8, -0.5), (9, -3.0), (1, -3.5), (3, -4.0)]])
    assert [(r["parent"], r["tok"], float(r["cum"])) for r in u.records[-1]] == [(0, 4, -1.5), (0, 5, -2.5)]
    # fp32: the add rounds.  -2^24 - 1 and -2^24 - 0.5 both round to -2^24, so beam 1's better lp only ties and beam 0 goes first
    u = utt(2, 8, None, [-16777216.0, -16777216.0])
    u.step([[(4, -1.0), (5, -1.5), (6, -3.0), (7, -4.0)], [(8, -0.5), (9, -3.0), (1, -3.5), (3, -4.0)]])
    assert [(r["parent"], r["tok"], float(r["cum"])) for r in u.records[-1]] == [(0, 4, -16777216.0), (1, 8, -16777216.0)]


def test_pool_cap_and_eos_behind_w_dropped():
    # W = 2, pool one short of full: two EOS candidates at p = 0 and p = 1, only the first fits
    u = utt(2, 8, 2, [-1.0, -1.0])
    u.pool = [dict(step=0, parent=0, score=np.float32(-0.5), lp=np.float32(-0.5), tokens=[], token_logprobs=[np.float32(-0.5)], finished=True)]
    u.step([[(2, -0.1), (5, -1.0), (6, -3.0), (7, -4.0)], [(2, -0.2), (9, -3.0), (1, -3.5), (3, -4.0)]])
    assert len(u.pool) == 2 and u.pool[1]["parent"] == 0 and u.done == 1
    assert [(r["parent"], r["tok"]) for r in u.records[-1]] == [(0, 5), (0, 6)]      # the ending step still records W live beams; -4 ties, beam 0 first
    # EOS at p = W - 1 is kept, at p = W dropped
    u = utt(2, 8, 2, [-1.0, -1.0])
    u.step([[(5, -0.1), (2, -0.2), (6, -3.0), (7, -4.0)], [(9, -0.3), (2, -0.4), (1, -3.5), (3, -4.0)]])
    assert [(h["parent"], float(h["score"])) for h in u.pool] == [(0, np.float32(-1.0) + np.float32(-0.2))]
    u = utt(2, 8, 2, [-1.0, -1.0])
    u.step([[(5, -0.1), (6, -0.2), (2, -0.3), (7, -4.0)], [(9, -3.0), (2, -3.4), (1, -3.5), (3, -4.0)]])
    assert u.pool == [] and [(r["parent"], r["tok"]) for r in u.records[-1]] == [(0, 5), (0, 6)]
    # a done utterance is frozen
    before = (list(u.cum), len(u.records))
    u.done = 1
    u.step([[(5, -0.1), (6, -0.2), (2, -0.3), (7, -4.0)]] * 2)
    assert (list(u.cum), len(u.records)) == before


def test_budget_end_and_no_eos():
    for eos in (None, -1):
        u = R.Utterance(2, 3, eos)
        u.step([[(2, -0.1), (5, -1.0), (6, -3.0), (7, -4.0)]])        # step 0: one live row; token 2 is no EOS here
        assert [(r["parent"], r["tok"]) for r in u.records[0]] == [(0, 2), (0, 5)] and u.done == 0
        u.step([[(2, -0.1), (5, -1.0), (6, -3.0), (7, -4.0)]] * 2)
        assert u.done == 0
        u.step([[(2, -0.1), (5, -1.0), (6, -3.0), (7, -4.0)]] * 2)
        assert u.done == 2 and u.n_steps == 3 and u.pool == []
        hyps = u.ranked()
        assert len(hyps) == 2 and not any(h["finished"] for h in hyps) and hyps[0]["tokens"] == [2, 2, 2]
    # pool full and budget spent in the same step: done = 1
    u = R.Utterance(1, 1, 2)
    u.step([[(2, -0.1), (5, -1.0)]])
    assert u.done == 1 and u.pool[0]["tokens"] == [] and u.records[0][0]["tok"] == 5


def test_w1_is_argmax_with_the_lowest_index():
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        row = torch.randint(-3, 4, (37,), generator=g).float()           # many equal maxima
        order = sorted(range(37), key=lambda i: (-float(row[i]), i))[:2]
        lse = torch.logsumexp(row, 0)
        u = R.Utterance(1, 4, None)
        u.step([[(i, float(row[i] - lse)) for i in order]])
        assert u.records[0][0]["tok"] == int((row == row.max()).nonzero()[0]) == order[0]


# ---- the host's half: backtracking, completing, ranking ------------------------------------------------------------------------------
host_state = R.host_state


def same_hyps(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a["tokens"]) == list(b["tokens"]) and a["finished"] == b["finished"] and a["sum_logprob"] == b["sum_logprob"]
        assert torch.equal(a["token_logprobs"], torch.tensor([float(v) for v in b["token_logprobs"]], dtype=torch.float32))


def scripted_run(W, max_new, eos, seed, vocab=12):
    """a run on random scripted candidates with many ties (lps are multiples of 1/4): swaps, fan-out and EOS all occur"""
    g = np.random.default_rng(seed)
    u = R.Utterance(W, max_new, eos)
    while not u.done:
        rows = []
        for _ in u.cum:
            toks = g.permutation(vocab)[:2 * W]
            lps = -np.sort(g.integers(1, 12, 2 * W)) / 4.0
            rows.append([(int(t), float(l)) for t, l in zip(toks, lps)])
        u.step(rows)
    return u


def test_backtracking_through_swapped_parents():
    # a hand-written swap: step 1 continues beam 1 first, then beam 0
    recs = [[dict(parent=0, tok=10), dict(parent=0, tok=11)], [dict(parent=1, tok=20), dict(parent=0, tok=21)],
            [dict(parent=1, tok=30), dict(parent=1, tok=31)]]
    par = [[r["parent"] for r in rec] for rec in recs]
    assert B.backtrack(par, 2, 0) == [0, 1, 0] and R.backtrack_tokens(recs, 2, 0) == [10, 21, 30]
    assert B.backtrack(par, 1, 0) == [1, 0] and R.backtrack_tokens(recs, 1, 0) == [11, 20]
    # scripted runs: the host's hypotheses from the records alone are the reference's, which keeps whole histories
    seen_swap = False
    for W in (1, 2, 3, 4):
        for seed in range(6):
            for eos in (None, 3):
                u = scripted_run(W, 9, eos, seed)
                seen_swap |= any(r["parent"] != w for rec in u.records[1:] for w, r in enumerate(rec))
                for pen in (0.0, 1.0, 2.0):
                    same_hyps(B.hypotheses(host_state([u], W, 9), 0, W, pen), u.ranked(pen))
    assert seen_swap


def test_ranking_with_length_penalty():
    mk = lambda s, n, fin=True: dict(tokens=[1] * (n - fin), token_logprobs=torch.zeros(n), sum_logprob=s, finished=fin)
    pool = [mk(-4.0, 2), mk(-6.0, 4), mk(-3.0, 1), mk(-4.0, 2)]
    for rank in (B.rank, R.rank):
        assert [id(h) for h in rank(pool, 0.0)] == [id(pool[i]) for i in (2, 0, 3, 1)]       # by the sum; the tie keeps pool order
        assert [id(h) for h in rank(pool, 1.0)] == [id(pool[i]) for i in (1, 0, 3, 2)]       # -1.5, -2, -2, -3
        assert [id(h) for h in rank(pool, 2.0)] == [id(pool[i]) for i in (1, 0, 3, 2)]       # -0.375, -1, -1, -3
    assert B.check_length_penalty(2) == 2.0
    for bad in (None, "1", True, float("nan")):
        with pytest.raises(ValueError, match="length_penalty"):
            B.check_length_penalty(bad)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _cpu_model(name="parity-tiny", **over):
    from dualhyp_amd import GPT, Config
    return GPT(Config.from_name(name, **over))


def test_refusals_before_the_gpu():
    m = _cpu_model()
    ps = [torch.arange(3, 20), torch.arange(3, 9)]
    for bad in (0, 5, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="num_beams"):
            G.beam_search_batch(m, ps, 8, num_beams=bad)
    with pytest.raises(ValueError, match="2048"):
        G.beam_search_batch(m, [ps[0]] * 600, 8, num_beams=4)
    m.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        G.beam_search_batch(m, ps, 8, num_beams=2)
    del m.fp8
    m.kv_cache_dtype = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        G.beam_search_batch(m, ps, 8, num_beams=2)
    m.kv_cache_dtype = "bf16"
    m.cpu_rsqrt_vec_width = 32
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.beam_search_batch(m, ps, 8, num_beams=2)
    m.cpu_rsqrt_vec_width = 0
    from dualhyp_amd.relprompt import GPT as RelGPT
    rel = object.__new__(RelGPT)
    object.__setattr__(rel, "cpu_rsqrt_vec_width", 0)
    object.__setattr__(rel, "config", m.config)
    with pytest.raises(ValueError, match="RelPrompt"):
        B.check_arguments(rel, 2, 4)
    assert B.check_arguments(m, 3, 4) == 3
    with pytest.raises(ValueError, match="length_penalty"):
        G.beam_search_batch(m, ps, 8, num_beams=2, length_penalty="1")
    # what is left is a model on the CPU: the engine says that there is no CPU path
    with pytest.raises(Exception, match="GPU"):
        G.beam_search_batch(m, ps, 8, num_beams=2)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_refusals(capsys):
    from dualhyp_amd import inference
    base = ["--test_path", "/nonexistent/none.json", "--random_init", "--tokenizer", "byte"]
    a = inference.parse_args(base)
    assert a.num_beams == 1 and a.length_penalty == 1.0
    a = inference.parse_args(base + ["--num_beams", "3", "--length_penalty", "0.5", "--logprobs"])
    assert a.num_beams == 3 and a.length_penalty == 0.5 and a.logprobs
    for extra, word in ((["--num_beams", "5"], "2..4"), (["--num_beams", "0"], "2..4"),
                        (["--num_beams", "2", "--schedule", "continuous"], "--schedule continuous"),
                        (["--num_beams", "2", "--speculate", "2"], "--speculate 2"),
                        (["--num_beams", "2", "--quantize", "fp8"], "--quantize fp8"),
                        (["--num_beams", "2", "--share_prefix", "auto"], "--share_prefix auto"),
                        (["--num_beams", "2", "--top_logprobs", "3"], "--top_logprobs 3")):
        with pytest.raises(SystemExit) as ex:
            inference.main(base + extra)          # ends at the parser: nothing has been loaded
        assert ex.value.code == 2 and word in capsys.readouterr().err
    # W = 1 leaves every other combination alone
    assert inference.parse_args(base + ["--schedule", "continuous", "--share_prefix", "auto", "--top_logprobs", "3"]).num_beams == 1


def test_record_fields_from_a_scripted_engine():
    """run_inference over a generate_fn that answers as beam_search_batch does: the prediction is the best hypothesis, every record
    carries the ranked beams, --logprobs reports the best beam's sums"""
    from dualhyp_amd.inference import run_inference
    decode = lambda t: "".join(chr(int(c)) for c in t)
    enc = lambda s: torch.tensor([ord(c) for c in s], dtype=torch.int64)
    examples = [dict(input_ids_no_response=enc("ab:"), ground_truth="hello"), dict(input_ids_no_response=enc("cd:"), ground_truth="you")]
    answers = [[("hello", [-0.5, -0.25, -0.25, -0.5, -0.5, -1.0], True), ("hallo", [-1.0] * 5, False)],
               [("yew", [-1.0, -1.0, -2.0, -0.5], True), ("you", [-2.0, -2.0, -1.0, -0.5], True)]]
    calls = []

    def make(want_lp):
        def gen(prompts):
            calls.append(len(prompts))
            beams = []
            for p in prompts:
                k = 0 if decode(p) == "ab:" else 1
                beams.append([dict(tokens=torch.cat([p, enc(t)]), token_logprobs=torch.tensor(lp, dtype=torch.float32),
                                   sum_logprob=float(sum(lp)), finished=fin) for t, lp, fin in answers[k]])
            return {"beams": beams, "logprobs": want_lp}
        return gen

    out = run_inference(make(False), examples, decode, batch_size=1)
    assert calls == [1, 1]
    p0, p1 = out["predictions"]
    assert p0["inference"] == "hello" and p1["inference"] == "yew" and "sum_logprob" not in p0
    assert [b["text"] for b in p0["beams"]] == ["hello", "hallo"] and [b["finished"] for b in p0["beams"]] == [True, False]
    assert p0["beams"][0]["sum_logprob"] == -3.0 and p0["beams"][0]["avg_logprob"] == -0.5 and p0["beams"][1]["avg_logprob"] == -1.0
    assert set(p1["beams"][1]) == {"text", "sum_logprob", "avg_logprob", "finished"}
    assert out["gtms"] == 0.5
    out = run_inference(make(True), examples, decode, batch_size=2)
    assert out["predictions"][1]["sum_logprob"] == -4.5 and out["predictions"][1]["avg_logprob"] == -4.5 / 4
    src = (REPO / "dualhyp_amd" / "inference.py").read_text()
    assert "args.decode_batch // beams" in src and '"--num_beams"' in src and '"--length_penalty"' in src


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_beam_entries_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    import ctypes as C
    from dualhyp_amd import _lib
    lib = _lib.load()
    raw = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text))
    for n in NEW_ENTRIES:
        assert n in declared, f"{n} is not declared in include/dualhyp_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is missing from the ctypes table"
        assert n in raw.split("#define DH_ABI_VERSION")[0], f"{n} is missing from the list of what ABI 6 gained"
        decl = text[text.index(f"int {n}("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_lib.SIGNATURES[n][1])
    assert declared == set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6 and "#define DH_ABI_VERSION 6" in raw and "#define DH_MAX_BEAMS 4" in raw
    assert B.MAX_BEAMS == 4 and 2 * B.MAX_BEAMS <= 8
    # the struct's fields, in the header's order
    body = text[text.index("typedef struct dh_beam_state {"):text.index("} dh_beam_state;")]
    assert re.findall(r"\*\s*([a-z_]+);", body) == [n for n, _ in _lib.BeamState._fields_]
    # refused before anything is read through a pointer
    st = _lib.BeamState()
    assert lib.dh_beam_select_bf16(None, 64, 1, 1, 2, 4, -1, 0, None, C.byref(st), None, None, None) != 0
    assert b"null argument" in lib.dh_last_error()
    assert lib.dh_beam_select_bf16(None, 64, 1, 1, 2, 4, -1, 0, None, None, None, None, None) != 0 and b"null beam state" in lib.dh_last_error()
    assert lib.dh_engine_reserve_beams(None, 2, 8) != 0 and b"null engine" in lib.dh_last_error()
    assert lib.dh_engine_decode_beam(None, None, None, 1, 2, 8, 1, -1, 1, None) != 0 and b"null argument" in lib.dh_last_error()
