"""The host side of token log-probabilities, without a GPU: run_inference with a generate_fn that returns (ids, logprobs), the
--logprobs flag, and the new entries of the C ABI in the header and the ctypes table."""
import json
import re
from pathlib import Path

import pytest
import torch

from dualhyp_amd import inference as I
from dualhyp_amd.tokenizer import ByteTokenizer

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("dh_token_logprobs_bf16", "dh_sample_bf16_ex", "dh_sample_rows_bf16_ex", "dh_engine_set_logprobs")


def _examples(tok):
    texts = [("fix: teh cat\nanswer: ", "the cat"), ("fix: a dgo\nanswer: ", "a dog"), ("fix: helo\nanswer: ", "hello")]
    exs, table, lps = [], {}, {}
    for k, (prompt, truth) in enumerate(texts):
        p = torch.tensor(tok.encode(prompt), dtype=torch.int64)
        answer = truth if k != 1 else "a dgo"                                  # one wrong prediction: a WER strictly inside (0, 1)
        table[tuple(p.tolist())] = torch.cat([p, torch.tensor(tok.encode(answer + "\nrest"), dtype=torch.int64)])
        lps[tuple(p.tolist())] = torch.tensor([-0.25 * (j + 1) - k for j in range(3 + k)], dtype=torch.float32)
        exs.append({"input_ids_no_response": p, "ground_truth": truth})
    return exs, table, lps


def test_run_inference_takes_ids_and_logprobs():
    tok = ByteTokenizer()
    exs, table, lps = _examples(tok)
    plain = I.run_inference(lambda ps: [table[tuple(p.tolist())] for p in ps], exs, tok.decode, batch_size=2)
    both = I.run_inference(lambda ps: ([table[tuple(p.tolist())] for p in ps], [lps[tuple(p.tolist())] for p in ps]), exs, tok.decode,
                           batch_size=2)
    assert 0 < plain["WER"] < 1
    for key in ("WER", "gtms", "post_ST_wer", "post_gtms", "n"):
        assert plain[key] == both[key]
    assert all(set(r) == {"inference", "ground_truth"} for r in plain["predictions"])
    assert [r["inference"] for r in plain["predictions"]] == ["the cat", "a dgo", "hello"]
    for k, (a, b) in enumerate(zip(plain["predictions"], both["predictions"])):
        assert set(b) == {"inference", "ground_truth", "sum_logprob", "avg_logprob"}
        assert {x: b[x] for x in a} == a
        want = [-0.25 * (j + 1) - k for j in range(3 + k)]
        assert b["sum_logprob"] == pytest.approx(sum(want), rel=1e-6)
        assert b["avg_logprob"] == pytest.approx(sum(want) / len(want), rel=1e-6)
    # the plain list form writes what it always wrote: the records serialise to the same text
    again = I.run_inference(lambda ps: [table[tuple(p.tolist())] for p in ps], exs, tok.decode, batch_size=2)
    assert json.dumps(plain["predictions"], indent=4) == json.dumps(again["predictions"], indent=4)
    assert "logprob" not in json.dumps(plain["predictions"])
    json.dumps(both["predictions"])                                            # plain floats, not tensors


def test_logprobs_flag_parses():
    base = ["--test_path", "x.json", "--random_init"]
    assert I.parse_args(base).logprobs is False
    assert I.parse_args(base + ["--logprobs"]).logprobs is True
    assert I.parse_args(base + ["--logprobs", "--schedule", "continuous"]).logprobs is True


def test_new_entries_are_declared_and_bound():
    """tests/test_capi.py would fail on a mismatch between the header and the table; this states which names the feature adds"""
    from dualhyp_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "dualhyp_hip.h").read_text(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _lib.SIGNATURES
    # the extended entries: the old argument lists plus one trailing pointer
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_ex"][1] == _lib.SIGNATURES[old][1] + [_lib.P]
    assert "#define DH_ABI_VERSION 6" in (REPO / "include" / "dualhyp_hip.h").read_text()


def test_public_names():
    import inspect
    import dualhyp_amd
    from dualhyp_amd import ops
    assert callable(dualhyp_amd.score_batch) and callable(ops.token_logprobs)
    for fn in (dualhyp_amd.generate_batch, dualhyp_amd.generate_stream, dualhyp_amd.generate):
        assert inspect.signature(fn).parameters["return_logprobs"].default is False
    for fn in (ops.sample, ops.sample_rows):
        assert inspect.signature(fn).parameters["logprobs"].default is None
