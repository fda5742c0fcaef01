"""Contextual biasing on the host (include/dualhyp_hip.h, "Contextual biasing"): the reference model against bit patterns computed by
hand, the proposal rules case by case, the non-vacuity of the GPU fixtures, the argument and file checks, the CLI, the records, the
refusals that need no GPU, and the library's new entries."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bias_reference as BR  # noqa: E402
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import _lib, beam_search_batch, generate, generate_batch, generate_stream, sample_batch  # noqa: E402
from dualhyp_amd import bias as Bi  # noqa: E402
from dualhyp_amd.tokenizer import ByteTokenizer  # noqa: E402

ALL = (1.3, 0.7, 0.3)
F32 = lambda bits: PR.f32_of_bits([bits])[0]        # noqa: E731


# ---- bf16(y + B) against hand-computed bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, boost, want", [
    (0x3F80, 2.0 ** -8, 0x3F80),        # 1 + 2^-8 lies halfway between 0x3F80 and 0x3F81: the even one
    (0x3F81, 2.0 ** -8, 0x3F82),        # 1 + 2^-7 + 2^-8 lies halfway between 0x3F81 and 0x3F82: the even one
    (0x3F80, 3 * 2.0 ** -8, 0x3F82),
    (0x4020, 0.5, 0x4040),              # 2.5 + 0.5 = 3
    (0x4020, -4.0, 0xBFC0),             # a negative boost: -1.5
    (0x7F7F, 1e36, 0x7F80),             # the largest finite bf16 plus 1e36 is a finite fp32 above the halfway point: bf16 +inf
    (0xFF80, 5.0, 0xFF80),              # -inf stays -inf
    (0xFF80, -5.0, 0xFF80),
    (0x0000, 0.0, 0x0000),
])
def test_boosted_value_gives_the_hand_computed_bits(bits, boost, want):
    assert BR.boosted_value(F32(bits), boost) == want
    row = np.array([bits], dtype=np.uint16)
    assert BR.adjusted_bits(row, [], [((0,), boost)]).tolist() == [want]


def test_a_nan_stays_a_nan():
    out = BR.adjusted_bits(np.array([0x7FC0, 0xFFC0], dtype=np.uint16), [], [((0,), 2.0), ((1,), -2.0)])
    assert all((int(v) & 0x7FFF) > 0x7F80 for v in out)


def test_a_penalised_id_is_boosted_from_z_not_from_the_rounded_value():
    # 2.5 once in the history under ALL: z = fl(fl(fl(2.5 / 1.3) - 0.7) - 0.3) = 0.92307..., a_t = 0x3F6C = 0.921875.
    # z + 2^-9 = 0.92503 lies above 0.923828125, the halfway point of 0x3F6C and 0x3F6D; a_t + 2^-9 is that point, and would stay even
    row = np.array([0x4020, 0x4020], dtype=np.uint16)
    assert PR.adjusted_value(0x4020, 1, *ALL) == 0x3F6C
    out = BR.adjusted_bits(row, [0], [((0,), 2.0 ** -9)], *ALL)
    assert int(out[0]) == 0x3F6D
    assert BR.boosted_value(F32(0x3F6C), 2.0 ** -9) == 0x3F6C
    assert int(out[1]) == 0x4020                                         # neither generated nor proposed


def test_a_boosted_id_that_was_never_generated_takes_no_penalty():
    row = np.array([0x4020, 0x4020, 0xC040], dtype=np.uint16)
    out = BR.adjusted_bits(row, [1], [((0,), 0.5), ((2,), 0.5)], *ALL)
    assert int(out[0]) == 0x4040                                         # 2.5 + 0.5, not fl(2.5 / 1.3) - 0.3 + 0.5 = 2.123 -> 0x4008
    assert BR.boosted_value(BR.penalised_z(0x4020, 0, *ALL), 0.5) == 0x4008
    assert int(out[2]) == 0xC020                                         # -3 + 0.5 = -2.5, not -3 * 1.3 + 0.5
    assert int(out[1]) == PR.adjusted_value(0x4020, 1, *ALL)             # generated, not proposed: a_t as always


def test_the_key_keeps_the_order_of_the_floats():
    vals = [-3.0e38, -6.0, -1.0, -2.0 ** -126, -0.0, 0.0, 2.0 ** -149, 0.5, 3.0, 3.5, 3.0e38]
    keys = [BR.boost_key(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and min(keys) > 0
    for v in vals:
        assert BR.key_boost(BR.boost_key(v)).tobytes() == np.float32(v).tobytes()


# ---- which ids are proposed ---------------------------------------------------------------------------------------------------------------
a, b, c, d = 10, 11, 12, 13


def both(generated, entries):
    """the reference's and the package's model agree; the reference's answer as plain floats"""
    got = {t: float(v) for t, v in BR.proposed(generated, entries).items()}
    assert Bi.proposed(generated, entries) == got
    return got


def test_nothing_generated_proposes_the_first_ids():
    assert both([], [((a, b, c), 2.0), ((d,), -1.0)]) == {a: 2.0, d: -1.0}


def test_a_prompt_tail_does_not_match():
    # the caller hands over what lies behind the prompt: a prompt that ends in a b leaves the history empty
    prompt, generated = [5, a, b], []
    assert both((prompt + generated)[len(prompt):], [((a, b, c), 2.0)]) == {a: 2.0}
    assert both([a, b], [((a, b, c), 2.0)]) == {a: 2.0, c: 2.0}        # generated a b does


def test_depth_7_of_an_8_id_entry():
    ids = tuple(range(20, 28))
    assert both([3] + list(ids[:7]), [(ids, 1.5)]) == {20: 1.5, 27: 1.5}
    assert both(list(ids[:7]), [(ids, 1.5)]) == {20: 1.5, 27: 1.5}      # k = m = 7
    assert both(list(ids[1:7]), [(ids, 1.5)]) == {20: 1.5}


def test_a_completed_phrase_restarts_at_depth_0():
    assert both([a, b, c], [((a, b, c), 2.0)]) == {a: 2.0}
    assert both([a, b, c, a], [((a, b, c), 2.0)]) == {a: 2.0, b: 2.0}


def test_overlapping_entries():
    e = [((a, b, c), 3.0), ((b, c, d), 2.0)]
    assert both([a, b], e) == {a: 3.0, b: 2.0, c: 3.0}                   # c: depth 2 of a b c (3) and depth 1 of b c d (2)
    assert both([a, b, c], e) == {a: 3.0, b: 2.0, d: 2.0}                # b c d goes on where a b c has ended


def test_a_repeated_id():
    e = [((a, a, b), 1.0)]
    assert both([a, a, a], e) == {a: 1.0, b: 1.0}                        # the last two a's are the prefix again
    assert both([a], e) == {a: 1.0}
    assert both([c, a, a], e) == {a: 1.0, b: 1.0}


def test_no_failure_arc_and_the_maximum_of_both_signs():
    e = [((d,), -6.0), ((c, d), 3.0)]
    assert both([c], e) == {c: 3.0, d: 3.0}
    assert both([a], e) == {c: 3.0, d: -6.0}
    assert both([c], [((c, d), -3.0), ((d,), -6.0)]) == {c: -3.0, d: -3.0}
    assert both([c], list(reversed(e))) == both([c], e)                  # any order


def test_bias_hits_counts_continuations():
    e = [((a, b, c), 3.0), ((d,), 1.0)]
    for g in ([a, b, c, d, a, b, 9], [d, d], [], [b, c], [a, a, b]):
        assert Bi.bias_hits(g, e) == BR.hits(g, e)
    assert Bi.bias_hits([a, b, c, d, a, b, 9], e) == 3 and Bi.bias_hits([d, d], e) == 0 and Bi.bias_hits([a, a, b], e) == 1


# ---- the GPU fixtures are not vacuous: decided here, by the reference alone --------------------------------------------------------------
@pytest.mark.parametrize("vocab", (250, 256, 32000, 128256))
def test_every_fixture_row_flips(vocab):
    bits, tokens, length = BR.fixture(vocab)
    hist = BR.histories(tokens, BR.START, length)
    assert hist[BR.ROW_EMPTY] == [] and tokens[BR.ROW_EMPTY, 2:4].tolist() == [BR.A, BR.B]
    for r, (raw, biased) in BR.FLIPS.items():
        assert PR.argmax_bits(bits[r]) == raw != biased
        assert PR.argmax_bits(BR.adjusted_bits(bits[r], hist[r], BR.ENTRIES)) == biased
    out = BR.adjusted_bits(bits[BR.ROW_PHRASE], hist[BR.ROW_PHRASE], BR.ENTRIES)
    assert [int(out[t]) for t in (BR.NINF, BR.TIE, BR.ODD)] == [0xFF80, 0x3F80, 0x3F82]
    assert BR.proposed(hist[BR.ROW_DEEP], BR.ENTRIES)[BR.DEEP[7]] == 5.0


def test_the_full_table_fills_every_pair():
    e = BR.full_table()
    assert len(e) == Bi.MAX_ENTRIES and all(len(ids) == Bi.MAX_LEN for ids, _ in e)
    assert e[0][0][:5] == e[1][0][:5] and e[0][0][5] != e[1][0][5] and e[2][0] == e[3][0]
    assert BR.proposed(list(e[2][0][:4]), e)[e[2][0][4]] == np.float32(e[3][1])      # the duplicate's larger boost


# ---- argument and file checks ------------------------------------------------------------------------------------------------------------
def test_check_bias_accepts_and_rounds_to_fp32():
    got = Bi.check_bias([([1, 2], 0.1), ((3,), -0.0), ([4] * 8, 3)], 100)
    assert got[0] == ((1, 2), float(np.float32(0.1))) and got[2] == ((4,) * 8, 3.0)
    assert got[1][1] == 0.0 and str(got[1][1]) == "0.0"                  # -0 is +0
    spec = Bi.compile_bias([([1, 2], 1.0)], 100)
    assert len(spec) == 1 and spec.n_ids == 2 and spec.device is None
    with pytest.raises(_lib.DualHypHipError, match="without a device"):
        spec.c_struct()
    assert Bi.as_spec(None, 100, "cpu") is None and Bi.as_spec([], 100, "cpu") is None


@pytest.mark.parametrize("entries, vocab, text", [
    ([], 100, "1 .. 256 entries"),
    ([([1], 1.0)] * 257, 100, "got 257"),
    ([([], 1.0)], 100, "holds 0 ids"),
    ([([1] * 9, 1.0)], 100, "holds 9 ids"),
    ([([100], 1.0)], 100, "id 100, outside"),
    ([([-1], 1.0)], 100, "id -1, outside"),
    ([([1], float("inf"))], 100, "not a finite"),
    ([([1], float("nan"))], 100, "not a finite"),
    ([([1], 1e39)], 100, "not a finite"),
    ([([1], 1.0)], 131073, "131072"),
])
def test_check_bias_refuses_with_the_value(entries, vocab, text):
    with pytest.raises(ValueError, match=text):
        Bi.check_bias(entries, vocab)


@pytest.mark.parametrize("entries", [[(1, 1.0)], [([1.5], 1.0)], [([True], 1.0)], [([1], "2")], [([1], True)], [[1, 2, 3]], "ab"])
def test_check_bias_refuses_wrong_types(entries):
    with pytest.raises(TypeError):
        Bi.check_bias(entries, 100)


def test_check_tables_is_the_limit_shared_with_the_penalties():
    Bi.check_tables(2040, 8)
    with pytest.raises(ValueError, match="2048"):
        Bi.check_tables(2041, 8)


def test_read_bias_file_and_the_two_encodings(tmp_path):
    f = tmp_path / "bias.txt"
    f.write_text("# names\n\n65 66 67\n2.5\t68\nAda\n-1.5\tNoor Khan\n")
    lines = Bi.read_bias_file(f, 4.0)
    assert lines == [([65, 66, 67], 4.0), ([68], 2.5), ("Ada", 4.0), ("Noor Khan", -1.5)]
    tok = ByteTokenizer()
    entries = Bi.entries_from_lines(lines, tok)
    plain = lambda s: [x + 3 for x in s.encode()]       # noqa: E731
    assert entries == [([65, 66, 67], 4.0), ([68], 2.5), (plain("Ada"), 4.0), (plain(" Ada"), 4.0), (plain("Noor Khan"), -1.5),
                       (plain(" Noor Khan"), -1.5)]
    assert all(tok.bos_token_id not in ids and tok.eos_token_id not in ids for ids, _ in entries)
    with pytest.raises(ValueError, match="needs the run's tokenizer"):
        Bi.entries_from_lines([("Ada", 1.0)], None)
    with pytest.raises(ValueError, match="holds 9 ids"):
        Bi.check_bias(Bi.entries_from_lines([("Noor Khan", 1.0)], tok), 259)
    for bad, text in (("x\t65\n", "is a boost"), ("inf\t65\n", "not finite"), ("2.0\t \n", "without an entry")):
        f.write_text(bad)
        with pytest.raises(ValueError, match=text):
            Bi.read_bias_file(f)


# ---- refusals before anything touches the GPU --------------------------------------------------------------------------------------------
def test_speculate_and_beams_are_refused_before_the_model_is_touched():
    prompts = [torch.arange(5)]
    e = [([1, 2], 2.0)]
    with pytest.raises(ValueError, match="speculate=2 does not go with a bias of 1 entries"):
        generate_batch(None, prompts, 4, top_k=1, speculate=2, bias=e)
    with pytest.raises(ValueError, match="speculate=3 does not go with a bias"):
        generate(None, prompts[0], 9, top_k=1, speculate=3, bias=e)
    with pytest.raises(ValueError, match="speculate=2 does not go with a bias"):
        generate_stream(None, prompts, 4, top_k=1, speculate=2, bias=Bi.compile_bias(e, 100))
    with pytest.raises(ValueError, match="does not go with beam search"):
        beam_search_batch(None, prompts, 4, num_beams=2, bias=e)
    for fn, kw in ((generate_batch, {}), (generate_stream, {}), (sample_batch, dict(num_samples=2)), (beam_search_batch, dict(num_beams=2))):
        with pytest.raises(TypeError, match="bias is a compiled specification"):
            fn(None, prompts, 4, bias="Ada", **kw)


BASE = ["--test_path", "x.json", "--model_path", "m.pth", "--llm_checkpoint", "ckpt"]


def parse(extra):
    from dualhyp_amd.inference import parse_args
    return parse_args(BASE + list(extra))


def test_cli_defaults_and_accepted_combinations():
    x = parse([])
    assert x.bias_file is None and x.bias_boost == 4.0 == Bi.DEFAULT_BOOST
    x = parse(["--bias_file", "names.txt", "--bias_boost", "-2.5", "--schedule", "continuous", "--share_prefix", "auto", "--constrain", "prompt",
               "--no_repeat_ngram", "3", "--stop", "newline", "--logprobs", "--top_logprobs", "3", "--top_k", "40", "--top_p", "0.9", "--min_p",
               "0.05", "--repetition_penalty", "1.2", "--quantize", "fp8", "--kv_cache", "fp8"])
    assert (x.bias_file, x.bias_boost) == ("names.txt", -2.5)
    x = parse(["--bias_file", "names.txt", "--num_samples", "3", "--top_k", "0", "--quantize", "mxfp4"])
    assert x.num_samples == 3 and x.bias_file == "names.txt"


@pytest.mark.parametrize("extra, text", [
    (["--bias_file", "n.txt", "--speculate", "2"], "--speculate 2 does not go with --bias_file n.txt"),
    (["--bias_file", "n.txt", "--num_beams", "2"], "--num_beams 2 does not go with --bias_file n.txt"),
    (["--bias_file", "n.txt", "--bias_boost", "inf"], "--bias_boost inf: the boost is finite"),
    (["--bias_boost", "nan"], "the boost is finite"),
])
def test_cli_refusals(extra, text, capsys):
    with pytest.raises(SystemExit):
        parse(extra)
    assert text in capsys.readouterr().err


def test_bias_from_args_and_the_default_run(tmp_path):
    from dualhyp_amd.inference import bias_from_args
    assert bias_from_args(parse([]), ByteTokenizer(), 259) == (None, None)
    f = tmp_path / "b.txt"
    f.write_text("Ada\n1.5\t70 71\n")
    entries, rec = bias_from_args(parse(["--bias_file", str(f), "--bias_boost", "3"]), ByteTokenizer(), 259)
    assert rec == {"entries": 3, "default_boost": 3.0}
    assert entries == [([68, 103, 100], 3.0), ([35, 68, 103, 100], 3.0), ([70, 71], 1.5)]


def test_records_gain_the_fields_only_with_the_flag():
    from dualhyp_amd.inference import run_inference
    ex = [dict(input_ids_no_response=torch.tensor([9, 1, 2]), ground_truth="1 2")]

    def gen(prompts):
        return [torch.cat([p, torch.tensor([1, 2, 3, 7])]) for p in prompts]

    def decode(ids):
        return " ".join(str(int(i)) for i in ids)

    plain = run_inference(gen, ex, decode, batch_size=1)
    gen.bias, gen.bias_entries = Bi.record(2, 4.0), [([1, 2, 3], 4.0), ([7], 1.0)]
    biased = run_inference(gen, ex, decode, batch_size=1)
    p0, p1 = plain["predictions"][0], biased["predictions"][0]
    assert "bias" not in p0 and "bias_hits" not in p0
    assert p1["bias"] == {"entries": 2, "default_boost": 4.0} and p1["bias_hits"] == 2       # 2 and 3 continued 1 2 3; the prompt's 1 2 did not count
    assert {k: v for k, v in p1.items() if k not in ("bias", "bias_hits")} == p0


# ---- the library ---------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("dh_sample_bf16_bias", "dh_sample_rows_bf16_bias", "dh_engine_set_bias")


def test_lib_declares_and_exports_the_new_entries():
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["dh_sample_bf16_bias"][1][:-1] == _lib.SIGNATURES["dh_sample_bf16_penalty"][1]
    assert _lib.SIGNATURES["dh_sample_rows_bf16_bias"][1][:-1] == _lib.SIGNATURES["dh_sample_rows_bf16_penalty"][1]
    assert [f[0] for f in _lib.BiasSpec._fields_] == ["ids", "len", "boost", "h_ids", "h_len", "h_boost", "n"]
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None
    assert _lib.load().dh_abi_version() == 6


def test_header_declares_what_lib_declares():
    text = (Path(__file__).resolve().parents[1] / "include" / "dualhyp_hip.h").read_text()
    for name in NEW_ENTRIES:
        assert f"int {name}(" in text
    assert "#define DH_MAX_BIAS_ENTRIES 256" in text and "#define DH_MAX_BIAS_LEN 8" in text
    assert (Bi.MAX_ENTRIES, Bi.MAX_LEN) == (256, 8)
    assert "typedef struct dh_bias_spec" in text and "NO FAILURE ARC" in text


def c_spec(entries):
    """a dh_bias_spec whose device pointers are never read: the calls below are refused, or have no sequence to launch for"""
    n = len(entries)
    rows = [list(ids)[:8] + [-1] * (8 - min(len(ids), 8)) for ids, _ in entries]
    keep = ((ctypes.c_int32 * (8 * n))(*[t for r in rows for t in r]), (ctypes.c_int32 * n)(*[len(ids) for ids, _ in entries]),
            (ctypes.c_float * n)(*[bst for _, bst in entries]))
    addr = [ctypes.cast(k, ctypes.c_void_p).value for k in keep]
    return _lib.BiasSpec(ids=16, len=16, boost=16, h_ids=addr[0], h_len=addr[1], h_boost=addr[2], n=n), keep


def call(lib, spec, vocab=256, tok_ld=8, start=ctypes.c_void_p(16), pen=None):
    return lib.dh_sample_bf16_bias(None, vocab, None, tok_ld, None, None, 0, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, start, None,
                                   1.0, 0.0, pen, None if spec is None else ctypes.byref(spec))


def test_c_entries_refuse_bad_values_without_a_device():
    lib = _lib.load()
    good = [((1, 2, 3), 2.0), ((4,), -1.0)]
    for entries, text in (([((1, 2, 256), 2.0)], b"id 256"), ([((1,) * 9, 2.0)], b"9 ids"), ([((), 2.0)], b"0 ids"),
                          ([((1,), float("inf"))], b"not finite"), ([((1,), float("nan"))], b"not finite"),
                          ([((1,), 1.0)] * 257, b"257 bias entries")):
        spec, keep = c_spec(entries)
        assert call(lib, spec) != 0
        err = lib.dh_last_error()
        assert b"dh_sample_bf16_bias" in err and text in err
    spec, keep = c_spec(good)
    assert call(lib, spec, start=None) != 0 and b"start" in lib.dh_last_error()
    assert call(lib, spec, vocab=131073) != 0 and b"131073" in lib.dh_last_error()
    # with a penalty on, the history and the entries' ids share the tables: 2045 + 4 ids
    on = _lib.PenaltyArgs(1.2, 0.0, 0.0)
    assert call(lib, spec, tok_ld=2045, pen=ctypes.byref(on)) != 0 and b"2048" in lib.dh_last_error()
    assert call(lib, spec, tok_ld=2044, pen=ctypes.byref(on)) == 0
    assert call(lib, spec, tok_ld=4096) == 0                            # a bias alone always fits
    assert call(lib, spec) == 0 and call(lib, None) == 0 and call(lib, None, start=None) == 0
    spec.n = 0                                                          # no entry is off
    assert call(lib, spec, start=None) == 0
    assert lib.dh_engine_set_bias(None, None, None) != 0 and b"null engine" in lib.dh_last_error()
