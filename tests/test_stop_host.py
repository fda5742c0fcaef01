"""Stop conditions on the host: dualhyp_amd.stop against hand-written cases of the definition (include/dualhyp_hip.h, "Stop
conditions"), the refusals of compile_stop and of the entry points (before anything is launched: on a CPU model), the stop-file
parser, the --stop flags, run_inference's finish_reason, and the new entries of the C ABI."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from dualhyp_amd import GPT, Config, beam_search_batch, generate, generate_batch, generate_stream  # noqa: E402
from dualhyp_amd import inference as I  # noqa: E402
from dualhyp_amd import stop as S  # noqa: E402
from dualhyp_amd.tokenizer import ByteTokenizer  # noqa: E402

A, B_, X, Y = 11, 22, 44, 55
V = 515


def test_compile_stop_folds_and_refuses():
    spec = S.compile_stop([Y, A], [[A, A, B_], [X], (X, Y)], V)
    assert spec.ids == (A, X, Y) and spec.sequences == ((A, A, B_), (X, Y))       # the one-token sequence went into the set
    assert bool(spec) and not bool(S.compile_stop([], [], V))
    assert S.compile_stop([A, A], [[X, Y], [X, Y]], V).sequences == ((X, Y),)
    with pytest.raises(ValueError, match="empty"):
        S.compile_stop([], [[]], V)
    with pytest.raises(ValueError, match="at most 8 tokens"):
        S.compile_stop([], [list(range(9))], V)
    with pytest.raises(ValueError, match="at most 8 stop sequences"):
        S.compile_stop([], [[i, i + 1] for i in range(9)], V)
    assert len(S.compile_stop([], [[i, i + 1] for i in range(8)] + [[400]], V).sequences) == 8       # eight, and a folded ninth
    assert len(S.compile_stop([], [list(range(8))], V).sequences[0]) == 8
    for bad in (-1, V, 10 ** 6):
        with pytest.raises(ValueError, match="outside"):
            S.compile_stop([bad], [], V)
        with pytest.raises(ValueError, match="outside"):
            S.compile_stop([], [[A, bad]], V)
    for bad in (2.0, "3", None, True):
        with pytest.raises(TypeError):
            S.compile_stop([bad], [], V)
    with pytest.raises(ValueError, match="vocab"):
        S.compile_stop([1], [], 0)
    # the list form of the generate functions: ints are ids, lists are sequences
    assert S.split_entries([A, [X, Y], B_, (A, A, B_)]) == ([A, B_], [[X, Y], (A, A, B_)])
    with pytest.raises(TypeError):
        S.as_spec("newline", V, "cpu")
    assert S.as_spec(None, V, "cpu") is None and S.as_spec([], V, "cpu") is None
    with pytest.raises(ValueError, match="compiled for"):
        S.as_spec(S.compile_stop([A], [], V), V + 1, "cpu")


def test_first_stop_hand_cases():
    spec = S.compile_stop([], [[A, A, B_]], V)
    assert S.first_stop([A, A, A, B_], spec) == 3                     # overlap: the match begins at the second a
    assert S.first_stop([A, A, B_, A, A, B_], spec) == 2              # the first of two
    assert S.first_stop([A, B_, A, A], spec) is None
    eight = list(range(100, 108))
    spec8 = S.compile_stop([], [eight], V)
    assert S.first_stop([5] + eight + [6], spec8) == 8 and S.first_stop(eight, spec8) == 7
    assert S.first_stop(eight[1:], spec8) is None and S.first_stop([5] + eight[:-1] + [6], spec8) is None
    # a would-be match that begins in the prompt: the generated text alone is looked at
    prompt, generated = [X, A, A], [B_, Y]
    assert S.first_stop(generated, spec) is None and S.first_stop(prompt + generated, spec) == 3
    # the set, the first of several conditions, the pair form of the specification
    both = S.compile_stop([Y], [[X, B_]], V)
    assert S.first_stop([A, X, B_, Y], both) == 2 and S.first_stop([A, Y, X, B_], both) == 1 and S.first_stop([], both) is None
    assert S.first_stop([A, X, B_, Y], ((Y,), ((X, B_),))) == 2
    assert S.first_stop(torch.tensor([A, X, B_]).tolist(), both) == 2


def test_newline_ids_and_finish_reasons():
    tok = ByteTokenizer()
    assert S.newline_ids(tok, 259) == [ord("\n") + 3] == S.newline_ids(tok, 515)
    assert tok.decode(S.newline_ids(tok, 259)) == "\n"
    assert S.finish_reasons([1, 2, 3, 3]) == ["eos", "length", "stop", "stop"]
    assert S.finish_reasons(torch.tensor([3, 1], dtype=torch.int32)) == ["stop", "eos"]
    assert S.finish_reasons([0, 2]) == ["length", "length"]          # generate_batch leaves 0 where the budget ended a shorter prompt
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            S.finish_reasons([bad])
    assert (S.DONE_EOS, S.DONE_LENGTH, S.DONE_STOP) == (1, 2, 3)


def test_stop_file_parser(tmp_path):
    f = tmp_path / "stop.txt"
    f.write_text("# stop ids\n13\n\n  17   # a comment behind an id\n5 6 7\n8 9\n")
    assert S.read_stop_file(f) == ([13, 17], [[5, 6, 7], [8, 9]])
    f.write_text("13\nx\n")
    with pytest.raises(ValueError, match=":2:"):
        S.read_stop_file(f)
    f.write_text("4 -5\n")
    with pytest.raises(ValueError, match="non-negative"):
        S.read_stop_file(f)


def test_entry_points_refuse_before_anything_is_launched():
    """on a CPU model: a call that got as far as the engine would fail for another reason"""
    cfg = Config.from_name("parity-tiny")
    m = GPT(cfg)
    ps = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    nine = [[i, i + 1] for i in range(9)]
    for fn in (generate_batch, generate_stream):
        with pytest.raises(ValueError, match="at most 8 stop sequences"):
            fn(m, ps, 4, stop=nine)
        with pytest.raises(ValueError, match="outside"):
            fn(m, ps, 4, stop=[cfg.padded_vocab_size])
        with pytest.raises(TypeError):
            fn(m, ps, 4, stop=7)
    with pytest.raises(ValueError, match="empty"):
        generate(m, ps[0], 8, stop=[[]])
    with pytest.raises(ValueError, match="histories live on the host"):
        beam_search_batch(m, ps, 4, num_beams=2, stop=[3, [4, 5]])
    with pytest.raises(ValueError, match="histories live on the host"):
        beam_search_batch(m, ps, 4, num_beams=2, stop=S.compile_stop([3], [[4, 5]], cfg.padded_vocab_size))


def test_new_entries_are_declared_and_bound():
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    assert "Stop conditions" in head and head.index("No-repeat n-grams") < head.index("Stop conditions")
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in ("dh_sample_bf16_stop", "dh_sample_rows_bf16_stop", "dh_beam_select_bf16_stop", "dh_engine_set_stop"):
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert decl and hasattr(lib, name), name
        assert decl.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
    assert "#define DH_ABI_VERSION 6" in head
    for define in ("DH_MAX_STOP_SEQS 8", "DH_MAX_STOP_LEN 8", "DH_DONE_EOS 1", "DH_DONE_LENGTH 2", "DH_DONE_STOP 3"):
        assert f"#define {define}" in head, define
    # the _stop samplers: the _ngram argument lists plus the specification
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_stop"][1][:-1] == _lib.SIGNATURES[old + "_ngram"][1]


def test_c_entries_refuse_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)                # a non-null pointer that is never read

    def spec(n, lens, seqs=64, ids=None):
        arr = (C.c_int32 * max(len(lens), 1))(*lens)
        s = _lib.StopSpec(set=ids, seqs=seqs, h_seq_len=C.cast(arr, C.c_void_p).value if lens else None, n_seqs=n)
        s._keep = arr
        return s

    def sample(s, start):
        return lib.dh_sample_bf16_stop(p, 8, p, 4, p, p, 1, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, start, C.byref(s))

    def rows(s):
        return lib.dh_sample_rows_bf16_stop(p, 8, p, 4, p, p, p, p, 1, 1, 2, 1.0, 1, -1, 0, None, None, 0, None, None, None, 0, 0, None, C.byref(s))

    def beam(s):
        st = _lib.BeamState(**{n: 64 for n, _ in _lib.BeamState._fields_})
        return lib.dh_beam_select_bf16_stop(p, 8, 1, 1, 2, 4, -1, 0, None, C.byref(st), p, p, None, 0, C.byref(s), p, None)

    cases = ((lambda: sample(spec(9, [2] * 9), p), "at most 8"), (lambda: sample(spec(1, [1]), p), "2 .. 8"),
             (lambda: sample(spec(2, [2, 9]), p), "stop sequence 1 has 9 tokens"), (lambda: sample(spec(1, [2]), None), "start"),
             (lambda: sample(spec(1, [2], seqs=None), p), "without their ids"), (lambda: sample(spec(-1, []), p), "at most 8"),
             (lambda: rows(spec(9, [2] * 9)), "at most 8"), (lambda: rows(spec(1, [0])), "2 .. 8"),
             (lambda: beam(spec(1, [2])), "histories live on the host"),
             (lambda: lib.dh_engine_set_stop(None, None, None, None), "null engine"))
    for call, why in cases:
        assert call() != 0
        assert why.encode() in lib.dh_last_error(), (why, lib.dh_last_error())


def test_stop_flags_parse(tmp_path):
    base = ["--test_path", "x.json", "--random_init"]
    args = I.parse_args(base)
    assert args.stop == "off" and args.stop_file is None
    assert I.stop_from_args(args, ByteTokenizer(), 259) is None
    args = I.parse_args(base + ["--stop", "newline"])
    spec = I.stop_from_args(args, ByteTokenizer(), 259)
    assert spec.ids == (13,) and spec.sequences == ()
    f = tmp_path / "stop.txt"
    f.write_text("20\n30 31\n")
    spec = I.stop_from_args(I.parse_args(base + ["--stop", "newline", "--stop_file", str(f)]), ByteTokenizer(), 259)
    assert spec.ids == (13, 20) and spec.sequences == ((30, 31),)
    for more in (["--schedule", "continuous"], ["--speculate", "3"], ["--share_prefix", "auto"], ["--constrain", "prompt"],
                 ["--top_logprobs", "3"], ["--quantize", "fp8", "--kv_cache", "fp8"], ["--no_repeat_ngram", "2"], ["--num_beams", "2"]):
        assert I.parse_args(base + ["--stop", "newline"] + more).stop == "newline"
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--stop", "period"])
    # the CLI's refusal of stop sequences with --num_beams; a file of stop ids alone goes with it
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--stop_file", str(f), "--num_beams", "2"])
    f.write_text("20\n21\n")
    assert I.parse_args(base + ["--stop_file", str(f), "--num_beams", "2"]).stop_file == str(f)


def test_run_inference_text_is_unchanged_and_the_reasons_are_recorded():
    """a stub decoder over a ByteTokenizer corpus whose outputs contain newlines: with the stop on newline the harness reads the same
    first line, and every record says why its sequence ended"""
    tok = ByteTokenizer()
    enc = lambda s: torch.tensor(tok.encode(s), dtype=torch.int64)      # noqa: E731
    body = lambda s: enc(s)[1:]                                          # noqa: E731  (without the BOS)
    exs = [{"input_ids_no_response": enc("a\nb ### Response:\n"), "ground_truth": "first line"},
           {"input_ids_no_response": enc("### Response:\n"), "ground_truth": "no newline"},
           {"input_ids_no_response": enc("x\n### Response:\n"), "ground_truth": "ends"},
           {"input_ids_no_response": enc("### Response:\n"), "ground_truth": ""}]
    answers = ["first line\nsecond line\nthird", "no newline at all", "ends on the eos", "\nbehind an empty line"]
    budget = 24
    spec = S.compile_stop(S.newline_ids(tok, 259), [], 259)

    def decoder(stopping):
        def gen(prompts):
            outs, reasons = [], []
            for p, a in zip(prompts, answers):
                g = body(a)[:budget].tolist()
                reason = "eos" if a.startswith("ends") else "length"
                at = S.first_stop(g, spec) if stopping else None
                if at is not None:
                    g, reason = g[:at + 1], "stop"
                outs.append(torch.cat([p, torch.tensor(g, dtype=torch.int64)]))
                reasons.append(reason)
            gen.finish_reasons = reasons
            return outs
        gen.stop = stopping
        return gen

    plain = I.run_inference(decoder(False), exs, tok.decode, batch_size=4)
    stopped = I.run_inference(decoder(True), exs, tok.decode, batch_size=4)
    assert [r["inference"] for r in plain["predictions"]] == ["first line", "no newline at all", "ends on the eos", ""]
    assert [r["inference"] for r in stopped["predictions"]] == [r["inference"] for r in plain["predictions"]]
    assert [r["finish_reason"] for r in stopped["predictions"]] == ["stop", "length", "eos", "stop"]
    assert all("finish_reason" not in r for r in plain["predictions"])
    for a, b in zip(plain["predictions"], stopped["predictions"]):
        assert {k: v for k, v in b.items() if k != "finish_reason"} == a
    assert (plain["WER"], plain["gtms"]) == (stopped["WER"], stopped["gtms"])
    # a generate_fn that says it stops and leaves no reasons is an error, not a silent gap in the records
    bad = decoder(True)

    def forgetful(prompts):
        outs = bad(prompts)
        forgetful.finish_reasons = None
        return outs
    forgetful.stop = True
    with pytest.raises(ValueError, match="finish_reasons"):
        I.run_inference(forgetful, exs, tok.decode, batch_size=4)
    # beams: the best hypothesis' reason, and every entry's own
    def beams(prompts):
        return {"beams": [[dict(tokens=torch.cat([p, body("hi\n")]), token_logprobs=torch.zeros(3), sum_logprob=-1.0, finished=True,
                                finish_reason="stop"),
                           dict(tokens=torch.cat([p, body("ho")]), token_logprobs=torch.zeros(2), sum_logprob=-2.0, finished=False,
                                finish_reason="length")] for p in prompts], "logprobs": False}
    beams.stop = True
    out = I.run_inference(beams, exs, tok.decode, batch_size=4)
    assert all(r["finish_reason"] == "stop" and [b["finish_reason"] for b in r["beams"]] == ["stop", "length"] and r["inference"] == "hi"
               for r in out["predictions"])
