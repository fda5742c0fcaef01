"""Nucleus and min-p sampling on the host: dualhyp_amd.nucleus, the refusals of the entry points (before anything is launched: on a
CPU model), the --temperature / --top_k / --top_p / --min_p flags, run_inference's sampling field, and the new entries of the C ABI
(include/dualhyp_hip.h, "Nucleus and min-p")."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, ops  # noqa: E402
from dualhyp_amd import inference as I  # noqa: E402
from dualhyp_amd import nucleus as N  # noqa: E402
from dualhyp_amd.tokenizer import ByteTokenizer  # noqa: E402

NAN = float("nan")
BAD_TOP_P = (0.0, -0.1, 1.0001, 2, NAN, math.inf)
BAD_MIN_P = (-0.001, 1.5, NAN, -math.inf)


def test_check_top_p_and_min_p():
    assert N.check_top_p(None) == 1.0 and N.check_top_p(1) == 1.0 and N.check_top_p(0.9) == 0.9 and N.check_top_p(1e-9) == 1e-9
    assert N.check_min_p(None) == 0.0 and N.check_min_p(0) == 0.0 and N.check_min_p(0.05) == 0.05 and N.check_min_p(1) == 1.0
    for bad in BAD_TOP_P:
        with pytest.raises(ValueError, match=r"top_p=.* is not in \(0, 1\]"):
            N.check_top_p(bad)
    for bad in BAD_MIN_P:
        with pytest.raises(ValueError, match=r"min_p=.* is not in \[0, 1\]"):
            N.check_min_p(bad)
    for bad in ("0.9", True, [0.9], 1j):
        with pytest.raises(TypeError):
            N.check_top_p(bad)
        with pytest.raises(TypeError):
            N.check_min_p(bad)
    assert N.check_nucleus(None, None) == (1.0, 0.0)
    assert not N.nucleus_on(None, None) and not N.nucleus_on(1.0, 0.0) and N.nucleus_on(0.9, None) and N.nucleus_on(None, 0.05)
    with pytest.raises(ValueError, match="0.0"):
        N.check_top_p(0.0)                      # the value is in the message


def test_entry_points_refuse_before_anything_is_launched():
    """on a CPU model: a call that got as far as the engine would fail for another reason"""
    cfg = Config.from_name("parity-tiny")
    m = GPT(cfg)
    ps = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    for fn in (generate_batch, generate_stream):
        for bad in BAD_TOP_P:
            with pytest.raises(ValueError, match="top_p"):
                fn(m, ps, 4, top_k=40, top_p=bad)
        for bad in BAD_MIN_P:
            with pytest.raises(ValueError, match="min_p"):
                fn(m, ps, 4, top_k=40, min_p=bad)
        with pytest.raises(TypeError):
            fn(m, ps, 4, top_p="0.9")
        with pytest.raises(ValueError, match="top_p"):
            fn(m, ps, 4, top_k=1, top_p=0.0)    # the arg-max takes neither, and still refuses what is no top_p at all
    with pytest.raises(ValueError, match="top_p"):
        generate(m, ps[0], 8, top_p=1.5)
    with pytest.raises(ValueError, match="min_p"):
        generate(m, ps[0], 8, min_p=-1.0)
    # the ops: CPU tensors, which the HIP path refuses for another reason once the values have passed
    lg = torch.zeros(2, 8, dtype=torch.bfloat16)
    tokens = torch.zeros(2, 4, dtype=torch.int64)
    length = torch.ones(2, dtype=torch.int32)
    done = torch.zeros(2, dtype=torch.int32)
    for kw, what in ((dict(top_p=0.0), "top_p"), (dict(top_p=NAN), "top_p"), (dict(min_p=1.01), "min_p"), (dict(min_p=NAN), "min_p")):
        with pytest.raises(ValueError, match=what):
            ops.sample(lg, tokens, length, done, **kw)
        with pytest.raises(ValueError, match=what):
            ops.sample_rows(lg, tokens, length, done, length, length, 2, **kw)
    assert int(tokens.sum()) == 0 and length.tolist() == [1, 1]


def test_new_entries_are_declared_and_bound():
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    assert "Nucleus and min-p" in head and head.index("Stop conditions") < head.index("Nucleus and min-p")
    for phrase in ("kept WHOLE", "(float)log((double)min_p)", "A(v) < top_p * T", "text-generation stacks", "what 8"):
        assert phrase in head, phrase
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in ("dh_sample_bf16_nucleus", "dh_sample_rows_bf16_nucleus", "dh_engine_set_nucleus"):
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert decl and hasattr(lib, name), name
        assert decl.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
    assert "#define DH_ABI_VERSION 6" in head and lib.dh_abi_version() == 6
    # the _nucleus samplers: the _stop argument lists plus the two floats
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_nucleus"][1][:-2] == _lib.SIGNATURES[old + "_stop"][1]
        assert _lib.SIGNATURES[old + "_nucleus"][1][-2:] == [C.c_float, C.c_float]
    assert _lib.SIGNATURES["dh_engine_set_nucleus"][1][1:] == [C.c_float, C.c_float]


def test_c_entries_refuse_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)                # a non-null pointer that is never read

    def sample(top_p, min_p):
        return lib.dh_sample_bf16_nucleus(p, 8, p, 4, p, p, 1, 1.0, 0, -1, 0, 0, None, None, 0, None, None, None, 0, 0, None, None, top_p, min_p)

    def rows(top_p, min_p):
        return lib.dh_sample_rows_bf16_nucleus(p, 8, p, 4, p, p, p, p, 1, 1, 2, 1.0, 0, -1, 0, None, None, 0, None, None, None, 0, 0, None,
                                               None, top_p, min_p)

    for call in (sample, rows):
        for top_p, min_p, why in ((0.0, 0.0, "top_p=0 is not in (0, 1]"), (1.5, 0.0, "top_p=1.5 is not in (0, 1]"), (-0.25, 0.0, "top_p=-0.25"),
                                  (NAN, 0.0, "nan is not in (0, 1]"), (0.9, -0.5, "min_p=-0.5 is not in [0, 1]"), (0.9, 1.25, "min_p=1.25"),
                                  (1.0, NAN, "nan is not in [0, 1]")):
            assert call(top_p, min_p) != 0
            err = lib.dh_last_error().lower()
            assert (b"dh_sample_rows_bf16_nucleus" if call is rows else b"dh_sample_bf16_nucleus") in err, err
            assert why.encode() in err, (why, err)
    assert lib.dh_engine_set_nucleus(None, 0.9, 0.0) != 0 and b"null engine" in lib.dh_last_error()


def test_sampling_flags_parse_and_refuse():
    base = ["--test_path", "x.json", "--random_init"]
    args = I.parse_args(base)
    assert (args.temperature, args.top_k, args.top_p, args.min_p) == (0.2, 1, 1.0, 0.0)
    assert I.sampling_from_args(args) is None
    args = I.parse_args(base + ["--top_k", "40", "--top_p", "0.9", "--min_p", "0.05", "--temperature", "0.7", "--seed", "5"])
    assert I.sampling_from_args(args) == dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05, seed=5)
    assert I.sampling_from_args(I.parse_args(base + ["--top_p", "0.9"])) == dict(temperature=0.2, top_k=1, top_p=0.9, min_p=0.0, seed=1337)
    assert I.sampling_from_args(I.parse_args(base + ["--top_k", "0"]))["top_k"] == 0
    for more in (["--schedule", "continuous"], ["--share_prefix", "auto"], ["--constrain", "prompt"], ["--top_logprobs", "3"],
                 ["--quantize", "fp8", "--kv_cache", "fp8"], ["--no_repeat_ngram", "2"], ["--stop", "newline"], ["--logprobs"]):
        assert I.parse_args(base + ["--top_k", "40", "--top_p", "0.9", "--min_p", "0.05"] + more).top_p == 0.9
    for bad in (["--top_p", "0"], ["--top_p", "1.5"], ["--top_p", "nan"], ["--min_p", "-0.1"], ["--min_p", "2"], ["--min_p", "nan"],
                ["--temperature", "0"], ["--temperature", "-1"], ["--top_k", "-1"],
                ["--top_k", "40", "--speculate", "3"], ["--top_k", "0", "--speculate", "3"], ["--top_k", "40", "--num_beams", "2"]):
        with pytest.raises(SystemExit):
            I.parse_args(base + bad)
    # with the greedy default both still run
    assert I.parse_args(base + ["--speculate", "3"]).speculate == 3 and I.parse_args(base + ["--num_beams", "2"]).num_beams == 2


def test_the_refusals_give_a_reason(capsys):
    base = ["--test_path", "x.json", "--random_init"]
    for bad, why in ((["--top_k", "40", "--speculate", "3"], "arg-max"), (["--top_k", "40", "--num_beams", "2"], "draws nothing"),
                     (["--top_p", "1.5"], "(0, 1]"), (["--min_p", "2"], "[0, 1]")):
        with pytest.raises(SystemExit):
            I.parse_args(base + bad)
        assert why in capsys.readouterr().err


def test_run_inference_records_the_sampling_parameters():
    tok = ByteTokenizer()
    enc = lambda s: torch.tensor(tok.encode(s), dtype=torch.int64)      # noqa: E731
    exs = [{"input_ids_no_response": enc("### Response:\n"), "ground_truth": "one"},
           {"input_ids_no_response": enc("x\n### Response:\n"), "ground_truth": "two"}]

    def gen(prompts):
        return [torch.cat([p, enc("one")[1:]]) for p in prompts]

    plain = I.run_inference(gen, exs, tok.decode, batch_size=2)
    assert all("sampling" not in r for r in plain["predictions"])
    gen.sampling = None
    assert I.run_inference(gen, exs, tok.decode, batch_size=2)["predictions"] == plain["predictions"]
    gen.sampling = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05, seed=5)
    out = I.run_inference(gen, exs, tok.decode, batch_size=2)
    assert all(r["sampling"] == gen.sampling and r["sampling"] is not gen.sampling for r in out["predictions"])
    for a, b in zip(plain["predictions"], out["predictions"]):
        assert {k: v for k, v in b.items() if k != "sampling"} == a
    assert (plain["WER"], plain["gtms"]) == (out["WER"], out["gtms"])
