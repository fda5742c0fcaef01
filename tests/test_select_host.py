"""Host side of sampled candidates (generate.sample_batch, dualhyp_amd.select, --num_samples / --select): the selection rules on
hand-made candidates, the refusals of sample_batch and of the parser, run_inference's records with a stub generate function, and
the C-ABI entry dh_engine_fork_slots (header, export, ctypes table, the refusals that need no engine)."""
import ctypes as C
import importlib
import math
from pathlib import Path

import pytest
import torch

from dualhyp_amd import select as select_fn
from dualhyp_amd.inference import parse_args, run_inference
from dualhyp_amd.select import mbr_risks, select, words
from dualhyp_amd.wer import edit_counts

REPO = Path(__file__).resolve().parent.parent
G = importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function


def cand(avg, total=None):
    return dict(avg_logprob=avg, sum_logprob=avg if total is None else total)


# ---- 1. select ---------------------------------------------------------------------------------------------------------------
def test_mbr_picks_the_text_the_others_agree_with():
    texts = ["a b c", "a b c", "a x c d"]
    cands = [cand(-2.0), cand(-1.0), cand(-0.1)]              # the odd one out is the most probable: mbr does not follow the score
    best, keys = select(cands, texts, "mbr")
    assert best == 1                                           # the two equal texts tie on risk; the higher avg_logprob wins
    # 0 and 1: edits against "a b c" 0, against "a x c d" (4 reference words) 2 -> 2 / 7; 2: 2 + 2 edits over 3 + 3 words
    assert keys == [2 / 7, 2 / 7, 4 / 6]
    assert select(cands, texts, "avg_logprob")[0] == 2 and select_fn is select


def test_mbr_risk_equals_a_direct_computation():
    texts = ["the cat sat", "The cat, sat.", "a cat sat down", "", "the the cat", "dog"]
    w = [t.lower().translate(str.maketrans("", "", ".,-?'")).split() for t in texts]
    assert [words(t) for t in texts] == w
    want = []
    for i in range(len(texts)):
        err = sum(sum(edit_counts(w[j], w[i])) for j in range(len(texts)) if j != i)
        want.append(err / max(1, sum(len(w[j]) for j in range(len(texts)) if j != i)))
    assert mbr_risks(texts) == want
    best, keys = select([cand(-1.0)] * len(texts), texts, "mbr")
    assert keys == want and best == min(range(len(texts)), key=lambda i: (want[i], i))
    # the edit count is directed: the other sample is the reference.  One candidate against an empty one: max(1, 0) words
    assert mbr_risks(["a b", ""]) == [2.0, 1.0] and mbr_risks(["only"]) == [0.0]


def test_tie_rules():
    # log-probability rules: ties go to the lower index
    assert select([cand(-1.0), cand(-0.5), cand(-0.5)], None, "avg_logprob") == (1, [-1.0, -0.5, -0.5])
    assert select([cand(0, -3.0), cand(0, -3.0)], None, "sum_logprob")[0] == 0
    # sum and avg disagree: each rule reads its own field
    c = [cand(-0.5, -10.0), cand(-1.0, -4.0)]
    assert select(c, None, "avg_logprob")[0] == 0 and select(c, None, "sum_logprob")[0] == 1
    # mbr: equal risks -> the higher avg_logprob; equal there too -> the lower index
    t = ["x y", "x y", "x y"]
    assert select([cand(-3.0), cand(-1.0), cand(-2.0)], t, "mbr")[0] == 1
    assert select([cand(-1.0), cand(-1.0), cand(-2.0)], t, "mbr")[0] == 0
    assert select([cand(-2.0), cand(-1.0), cand(-1.0)], t, "mbr")[0] == 1


def test_non_finite_scores_rank_last():
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf, None):
        assert select([cand(bad), cand(-50.0), cand(-60.0)], None, "avg_logprob")[0] == 1
        assert select([cand(bad, bad), cand(0, -50.0)], None, "sum_logprob")[0] == 1
        # an mbr tie is not won on a score that is no number
        assert select([cand(bad), cand(-50.0)], ["a", "a"], "mbr")[0] == 1
    best, keys = select([cand(nan), cand(nan)], None, "avg_logprob")
    assert best == 0 and all(math.isnan(k) for k in keys)      # nothing finite: the lower index


def test_select_refuses_what_it_cannot_rank():
    with pytest.raises(ValueError, match="how is one of"):
        select([cand(-1.0)], ["a"], "best")
    with pytest.raises(ValueError, match="no candidates"):
        select([], [], "mbr")
    with pytest.raises(ValueError, match="one text per candidate"):
        select([cand(-1.0), cand(-2.0)], ["a"], "mbr")
    with pytest.raises(ValueError, match="one text per candidate"):
        select([cand(-1.0)], None, "mbr")


# ---- 2. sample_batch's refusals: each before anything is launched --------------------------------------------------------------
class NoEngineModel:
    """A model whose engine must never be asked for"""
    max_seq_length = 4096
    cpu_rsqrt_vec_width = 0

    def engine(self, *a, **k):
        raise AssertionError("a refused call reached the engine")


def test_sample_batch_refusals():
    ps = [torch.arange(3, 40)]
    m = NoEngineModel()
    for bad in (1, 0, 9, -2, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="num_samples"):
            G.sample_batch(m, ps, 4, num_samples=bad, temperature=0.8, top_k=5)
    with pytest.raises(ValueError, match="top_k=1"):
        G.sample_batch(m, ps, 4, num_samples=3, temperature=0.8, top_k=1)
    with pytest.raises(ValueError, match="speculate"):
        G.sample_batch(m, ps, 4, num_samples=3, temperature=0.8, top_k=5, speculate=2)
    from dualhyp_amd.relprompt import GPT as RelGPT
    rel = RelGPT.__new__(RelGPT)                               # the type is what the check reads
    with pytest.raises(ValueError, match="RelPrompt"):
        G.sample_batch(rel, ps, 4, num_samples=3, temperature=0.8, top_k=5)
    assert G.MAX_SAMPLES == 8 and "#define DH_MAX_SAMPLES 8" in (REPO / "include" / "dualhyp_hip.h").read_text()


# ---- 3. the parser -------------------------------------------------------------------------------------------------------------
BASE = ["--test_path", "x.json"]


def test_flags_parse():
    a = parse_args(BASE)
    assert a.num_samples == 1 and a.select is None             # the path it always was
    a = parse_args(BASE + ["--num_samples", "3", "--top_k", "5", "--temperature", "0.8"])
    assert a.num_samples == 3 and a.select == "avg_logprob"
    for how in ("avg_logprob", "sum_logprob", "mbr"):
        assert parse_args(BASE + ["--num_samples", "8", "--top_k", "0", "--select", how]).select == how
    # what it goes with
    a = parse_args(BASE + ["--num_samples", "2", "--top_k", "5", "--quantize", "fp8", "--kv_cache", "fp8", "--share_prefix", "auto",
                           "--constrain", "prompt", "--no_repeat_ngram", "2", "--stop", "newline", "--top_logprobs", "2", "--top_p", "0.9"])
    assert a.num_samples == 2 and a.logprobs


@pytest.mark.parametrize("argv,why", [
    (["--num_samples", "3", "--top_k", "5", "--num_beams", "2"], "--num_beams 2"),
    (["--num_samples", "3", "--speculate", "2"], "--speculate 2"),
    (["--num_samples", "3", "--top_k", "5", "--schedule", "continuous"], "--schedule continuous"),
    (["--num_samples", "3"], "--top_k 1"),
    (["--num_samples", "3", "--top_k", "1", "--temperature", "0.8"], "--top_k 1"),
    (["--select", "mbr"], "--num_samples N > 1"),
    (["--select", "avg_logprob", "--num_samples", "1"], "--num_samples N > 1"),
    (["--num_samples", "9", "--top_k", "5"], "N is 1"),
    (["--num_samples", "0"], "N is 1"),
    (["--num_samples", "3", "--top_k", "5", "--select", "vote"], "invalid choice"),
])
def test_parser_refusals(argv, why, capsys):
    with pytest.raises(SystemExit):
        parse_args(BASE + argv)
    assert why in capsys.readouterr().err


# ---- 4. run_inference with a stub ----------------------------------------------------------------------------------------------
def byte_decode(t):
    return bytes(int(x) for x in t.reshape(-1).tolist()).decode()


def enc(s):
    return torch.tensor(list(s.encode()), dtype=torch.int64)


def sample(text, lps, reason="eos"):
    lp = torch.tensor(lps, dtype=torch.float32)
    total = float(lp.double().sum())
    return dict(tokens=enc(text), token_logprobs=lp, sum_logprob=total, avg_logprob=total / max(len(lps), 1), finish_reason=reason)


@pytest.mark.parametrize("how,want", [("avg_logprob", [2, 0]), ("sum_logprob", [1, 0]), ("mbr", [1, 1])])
def test_run_inference_records(how, want):
    prompt = "### Response:\n"
    examples = [dict(input_ids_no_response=enc(prompt), ground_truth="up down"),
                dict(input_ids_no_response=enc(prompt), ground_truth="sit down")]
    cands = [[sample("up down", [-1.0, -1.0, -1.0]), sample("up down", [-1.0, -0.5]), sample("up town now", [-0.1] * 20, "length")],
             [sample("sit down", [-0.5]), sample("sit", [float("nan")], "stop")]]
    calls = []

    def gen(prompts):
        calls.append(len(prompts))
        return {"samples": cands, "select": how, "logprobs": True}

    gen.stop = True
    gen.sampling = dict(temperature=0.8, top_k=5, top_p=1.0, min_p=0.0, seed=1337)
    out = run_inference(gen, examples, byte_decode, batch_size=4)
    assert calls == [2]
    recs = out["predictions"]
    assert [r["selected"] for r in recs] == want
    for r, cs, k in zip(recs, cands, want):
        assert r["inference"] == r["samples"][k]["text"]
        assert [s["text"] for s in r["samples"]] == [byte_decode(c["tokens"]) for c in cs]
        assert [s["finish_reason"] for s in r["samples"]] == [c["finish_reason"] for c in cs]
        assert r["finish_reason"] == cs[k]["finish_reason"] and r["sampling"] == gen.sampling
        for key in ("sum_logprob", "avg_logprob"):              # --logprobs: the chosen candidate's, as run_inference always wrote them
            assert r[key] == cs[k][key] or (math.isnan(r[key]) and math.isnan(cs[k][key]))
        for s, c in zip(r["samples"], cs):
            assert set(s) == {"text", "sum_logprob", "avg_logprob", "finish_reason", "key"}
            if math.isfinite(c["sum_logprob"]):
                assert s["sum_logprob"] == c["sum_logprob"] and s["avg_logprob"] == c["avg_logprob"]
            else:
                assert s["sum_logprob"] is None and s["avg_logprob"] is None       # JSON has no NaN
    keys0 = [s["key"] for s in recs[0]["samples"]]
    if how == "mbr":
        assert keys0 == mbr_risks(["up down", "up down", "up town now"])
    else:
        assert keys0 == [c[how] for c in cands[0]]
        assert recs[1]["samples"][1]["key"] is None
    # the metrics are those of the chosen answers: avg_logprob keeps "up town now" for the first utterance; with two candidates mbr
    # keeps the shorter one (one edit over the other's two words, against one edit over its one word)
    assert out["n"] == 2 and out["gtms"] == (1.0 if how == "sum_logprob" else 0.5)


# ---- 5. the C-ABI entry --------------------------------------------------------------------------------------------------------
def test_fork_slots_is_declared_exported_and_bound():
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    n = "dh_engine_fork_slots"
    assert "Sampled candidates" in head and f"int {n}(dh_engine* e, const int32_t* d_prompt_len, int n_utt, int n_copies, int max_len," in head
    assert n in head.split("#define DH_ABI_VERSION")[0], f"{n} is missing from the list of what ABI 6 gained"
    assert n in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.dh_abi_version() == 6
    fn = getattr(lib, n)
    lens = (C.c_int32 * 2)(5, 40)       # never read: every call below is refused before it
    err = lambda: lib.dh_last_error().decode()
    assert fn(None, lens, 2, 2, 40, None) != 0 and "null engine" in err()
    assert fn(None, lens, 2, 1, 40, None) != 0 and "n_copies=1" in err() and "2 .. 8" in err()
    assert fn(None, lens, 2, 9, 40, None) != 0 and "n_copies=9" in err()
    assert fn(None, lens, 2, 2, 0, None) != 0 and "max_len=0" in err()
    foreign = (C.c_char * 4096)()       # memory that is no engine
    assert fn(C.cast(foreign, C.c_void_p), lens, 2, 2, 40, None) != 0 and "is not an engine" in err()
