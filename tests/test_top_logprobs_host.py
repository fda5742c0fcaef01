"""The host side of the token alternatives, without a GPU: the reference's closed forms, the argument refusals of the generation
entry points (before anything is launched: on a CPU model), the --top_logprobs flag, run_inference with a generate_fn that returns
(ids, logprobs, top), and the new entries of the C ABI in the header and the ctypes table."""
import inspect
import json
import re
from pathlib import Path

import pytest
import torch

import top_logprob_reference as T
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, inference as I, ops, score_batch
from dualhyp_amd.tokenizer import ByteTokenizer

REPO = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
NEW_ENTRIES = ("dh_token_top_logprobs_bf16", "dh_sample_bf16_top", "dh_sample_rows_bf16_top", "dh_engine_set_top_logprobs")


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (8, 320, 1001))
@pytest.mark.parametrize("K", T.KS)
def test_reference_closed_forms(V, K):
    ramp = torch.arange(0x3F80, 0x3F80 + V, dtype=torch.int16).view(BF)[None]   # consecutive bf16 values from 1.0 up: strictly ascending
    assert bool((ramp[0, 1:].double() > ramp[0, :-1].double()).all())
    assert T.top_ids(ramp, K).tolist() == [list(range(V - 1, V - 1 - K, -1))]
    assert T.top_ids(torch.full((2, V), 1.5, dtype=BF), K).tolist() == [list(range(K))] * 2
    zeros = T.make_row("zeros_alternating_sign", V, 0, K)
    assert bool(torch.signbit(zeros[0])) and not bool(torch.signbit(zeros[1])) and not bool(zeros.any())
    assert T.top_ids(zeros[None], K).tolist() == [list(range(K))]              # -0 == +0: index order
    inf = torch.full((V,), -float("inf"), dtype=BF)
    inf[5] = -3.0
    assert T.top_ids(inf[None], K).tolist() == [([5] + [i for i in range(V) if i != 5])[:K]]


@pytest.mark.parametrize("K", T.KS)
def test_reference_sorts_agree_on_every_kind(K):
    """numpy's stable sort of the negated values against the plain-Python sort of (-float(value), index)"""
    for V in (8, 320, 1000):
        rows, kinds = T.case(V, 37, K)
        assert set(kinds) == set(T.KINDS)
        got = T.top_ids(rows, K).tolist()
        for r in range(rows.size(0)):
            assert got[r] == T.top_ids_row(rows[r].tolist(), K), (V, kinds[r])
    rows, kinds = T.case(9000, 37, K)
    r = kinds.index("equal_maxima")
    assert int((rows[r] == rows[r].max()).sum()) == max(K + 3, 6)             # at 0, 7, 8, 8191, 8192 and 8999, and K - 3 more
    assert all(float(rows[r, i]) == 17.0 for i in (0, 7, 8, 8191, 8192, 8999))
    ids = T.top_ids(rows[r:r + 1], K).tolist()[0]
    assert ids == sorted(ids) and ids[:min(K, 3)] == [0, 7, 8][:K] and all(float(rows[r, i]) == 17.0 for i in ids)
    r = kinds.index("mostly_minus_inf")
    assert int(torch.isfinite(rows[r]).sum()) == max(K - 2, 1)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    return GPT(Config.from_name("parity-tiny"))


def test_arguments_are_refused_before_any_launch(cpu_model):
    """on a CPU model nothing can be launched: every refusal below comes from the argument checks"""
    m = cpu_model
    p = torch.tensor([1, 2, 3], dtype=torch.int64)
    calls = (lambda **kw: generate_batch(m, [p], 4, **kw), lambda **kw: generate_stream(m, [p], 4, **kw),
             lambda **kw: generate(m, p, 7, **kw))
    for call in calls:
        for bad in (-1, 9, 100):
            with pytest.raises(ValueError, match="top_logprobs"):
                call(return_logprobs=True, top_logprobs=bad)
        for bad in (True, False, 2.0, "3", None):
            with pytest.raises(TypeError, match="top_logprobs"):
                call(return_logprobs=True, top_logprobs=bad)
        for k in (1, 8):
            with pytest.raises(ValueError, match="return_logprobs"):
                call(top_logprobs=k)
    for bad, exc in ((9, ValueError), (-1, ValueError), (True, TypeError), (1.0, TypeError)):
        with pytest.raises(exc, match="top_logprobs"):
            score_batch(m, [p], [p], top_logprobs=bad)
    for bad, exc in ((0, ValueError), (9, ValueError), (True, TypeError), (2.0, TypeError)):
        with pytest.raises(exc):
            ops.check_top_logprobs(bad, 32000, lowest=1)
    with pytest.raises(ValueError):
        ops.check_top_logprobs(8, 7)                                            # K <= vocab
    assert ops.check_top_logprobs(7, 7) == 7 and ops.check_top_logprobs(0) == 0 and ops.MAX_TOP_LOGPROBS == 8


def test_public_names():
    import dualhyp_amd
    assert callable(ops.token_top_logprobs)
    for fn in (dualhyp_amd.generate_batch, dualhyp_amd.generate_stream, dualhyp_amd.generate, dualhyp_amd.score_batch):
        assert inspect.signature(fn).parameters["top_logprobs"].default == 0
    for fn in (ops.sample, ops.sample_rows):
        assert inspect.signature(fn).parameters["top_logprobs"].default is None


def test_new_entries_are_declared_and_bound():
    """tests/test_capi.py would fail on a mismatch between the header and the table; this states which names the feature adds"""
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _lib.SIGNATURES
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
    # the extended entries: the _ex argument lists plus K and the two buffers
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_top"][1] == _lib.SIGNATURES[old + "_ex"][1] + [_lib.I, _lib.P, _lib.P]
    assert "#define DH_ABI_VERSION 6" in head and "#define DH_MAX_TOP_LOGPROBS 8" in head
    assert "Token alternatives" in head and "index ascending" in head and "-0 == +0" in head


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
def test_top_logprobs_flag_parses():
    base = ["--test_path", "x.json", "--random_init"]
    a = I.parse_args(base)
    assert a.top_logprobs == 0 and a.logprobs is False
    a = I.parse_args(base + ["--top_logprobs", "3"])
    assert a.top_logprobs == 3 and a.logprobs is True
    a = I.parse_args(base + ["--top_logprobs", "8", "--schedule", "continuous"])
    assert a.top_logprobs == 8 and a.logprobs is True
    assert I.parse_args(base + ["--logprobs"]).top_logprobs == 0
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            I.parse_args(base + ["--top_logprobs", bad])


EOS = 10        # "\n" of the byte tokenizer: the stub's sequence 1 ends on it


def _examples(tok, K):
    texts = [("fix: teh cat\nanswer: ", "the cat"), ("fix: a dgo\nanswer: ", "a dog"), ("fix: helo\nanswer: ", "hello")]
    exs, table, lps, tops = [], {}, {}, {}
    for k, (prompt, truth) in enumerate(texts):
        p = torch.tensor(tok.encode(prompt), dtype=torch.int64)
        gen = torch.tensor(tok.encode(truth), dtype=torch.int64)
        key = tuple(p.tolist())
        table[key] = torch.cat([p, gen])
        n = gen.numel() + (1 if k == 1 else 0)                                  # sequence 1 met its EOS: one entry more than ids
        lps[key] = torch.tensor([-0.25 * (j + 1) - k for j in range(n)], dtype=torch.float32)
        ids = torch.arange(n * K, dtype=torch.int32).view(n, K) + 100 * k
        lp = -torch.arange(n * K, dtype=torch.float32).view(n, K) / 8 - k
        if k == 2:
            lp[1, K - 1] = -float("inf")
            lp[2, 0] = float("nan")
            lps[key][0] = -float("inf")
        tops[key] = (ids, lp)
        exs.append({"input_ids_no_response": p, "ground_truth": truth})
    return exs, table, lps, tops


@pytest.mark.parametrize("K", (1, 3))
def test_run_inference_takes_the_triple(K):
    tok = ByteTokenizer()
    exs, table, lps, tops = _examples(tok, K)
    key = lambda p: tuple(p.tolist())
    plain = I.run_inference(lambda ps: [table[key(p)] for p in ps], exs, tok.decode, batch_size=2)
    pair = I.run_inference(lambda ps: ([table[key(p)] for p in ps], [lps[key(p)] for p in ps]), exs, tok.decode, batch_size=2)
    three = I.run_inference(lambda ps: ([table[key(p)] for p in ps], [lps[key(p)] for p in ps], [tops[key(p)] for p in ps]), exs,
                            tok.decode, batch_size=2, eos_id=EOS)
    for k in ("WER", "gtms", "post_ST_wer", "post_gtms", "n"):
        assert plain[k] == pair[k] == three[k]
    # the list and the pair write exactly what they wrote before
    assert all(set(r) == {"inference", "ground_truth"} for r in plain["predictions"])
    assert all(set(r) == {"inference", "ground_truth", "sum_logprob", "avg_logprob"} for r in pair["predictions"])
    assert "token_ids" not in json.dumps(pair["predictions"]) and "top_logprobs" not in json.dumps(pair["predictions"])
    for k, (ex, b, c) in enumerate(zip(exs, pair["predictions"], three["predictions"])):
        assert set(c) == set(b) | {"token_ids", "token_logprobs", "top_logprobs"}
        if k != 2:                                                              # sequence 2 holds a -inf: its sum is -inf in both
            assert {x: c[x] for x in b} == b
        p = ex["input_ids_no_response"]
        want_lp, (want_ids, want_top) = lps[key(p)], tops[key(p)]
        n = want_lp.numel()
        gen = table[key(p)][p.numel():].tolist()
        assert c["token_ids"] == gen + ([EOS] if k == 1 else [])
        assert len(c["token_ids"]) == len(c["token_logprobs"]) == len(c["top_logprobs"]) == n       # aligned
        for j in range(n):
            v = float(want_lp[j])
            assert c["token_logprobs"][j] == (v if v == v and abs(v) != float("inf") else None)
            assert len(c["top_logprobs"][j]) == K
            for r in range(K):
                i, v = c["top_logprobs"][j][r]
                w = float(want_top[j, r])
                assert isinstance(i, int) and i == int(want_ids[j, r])
                assert v == (w if w == w and abs(w) != float("inf") else None)
    new = [{k: r[k] for k in ("token_ids", "token_logprobs", "top_logprobs")} for r in three["predictions"]]
    text = json.dumps(new, allow_nan=False)                                     # strict JSON: no NaN, no Infinity in the new fields
    assert text.count("null") == 3                                              # the -inf log-probability, the -inf and the NaN alternative


def test_strict_json_of_the_new_fields_only():
    """what --top_logprobs adds is strict JSON even where a value is not finite (the fields of --logprobs stay as they were)"""
    assert I._finite_or_none(float("nan")) is None and I._finite_or_none(-float("inf")) is None and I._finite_or_none(-1.5) == -1.5
