"""Penalties on the host (include/dualhyp_hip.h, "Penalties"): the reference model against bit patterns computed by hand (exact rational
arithmetic, each operation rounded to 24 bits, the result to 8), the non-vacuity of the GPU fixtures, the argument checks, the refusals
that need no GPU, and the library's new entries."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import penalty_reference as PR  # noqa: E402
from dualhyp_amd import _lib, generate, generate_batch, generate_stream, sample_batch  # noqa: E402
from dualhyp_amd import penalty as P  # noqa: E402

ALL = (1.3, 0.7, 0.3)


# ---- the reference against hand-computed bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, c, pen, want", [
    (0x4020, 1, ALL, 0x3F6C),           # 2.5: fl(2.5 / 1.3) - 0.7 - 0.3
    (0x4020, 3, ALL, 0xBEF4),           # the count matters: - fl(0.7 * 3)
    (0xC040, 1, ALL, 0xC09D),           # -3.0: negative values are multiplied
    (0xC040, 3, ALL, 0xC0CA),
    (0x0000, 1, ALL, 0xBF80),           # +0 / 1.3 = +0; 0 - 0.7f - 0.3f rounds to -1
    (0x8000, 1, ALL, 0xBF80),           # -0 takes the division too
    (0xFF80, 1, ALL, 0xFF80),           # -inf stays -inf
    (0xFF80, 3, ALL, 0xFF80),
    (0xC0D6, 1, ALL, 0xC11B),
    (0x4020, 1, (1.3, 0.0, 0.0), 0x3FF6),
    (0xC040, 1, (1.3, 0.0, 0.0), 0xC07A),
    (0x4020, 1, (1.0, 0.75, 0.0), 0x3FE0),      # 2.5 - 0.75 = 1.75
    (0x4020, 3, (1.0, 0.75, 0.0), 0x3E80),      # 2.5 - 2.25 = 0.25
    (0x4020, 3, (1.0, 0.0, 0.75), 0x3FE0),      # presence does not count
    (0x4020, 2, (1.0, -0.75, 0.0), 0x4080),     # a negative penalty rewards: 2.5 + 1.5 = 4
])
def test_reference_gives_the_hand_computed_bits(bits, c, pen, want):
    assert PR.adjusted_value(bits, c, *pen) == want


def test_separately_rounded_operations_not_an_fma():
    f = PR.FUSED
    assert PR.adjusted_value(f["bits"], f["count"], *ALL) == f["want"] != f["fused"]
    # what a contraction of alpha_f * c into the subtraction would give: the product exact, one rounding
    th, af, ap = (np.float32(v) for v in ALL)
    y = np.float32(PR.f32_of_bits([f["bits"]])[0] * th)
    fused = np.float32(np.float32(np.float64(y) - np.float64(af) * 3.0) - ap)
    assert int(PR.bf16_bits(fused)[0]) == f["fused"]
    assert PR.PENALTIES["all"] == dict(repetition_penalty=ALL[0], frequency_penalty=ALL[1], presence_penalty=ALL[2])


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)   # 1 + 2^-8, 1 + 3 * 2^-8: ties
    assert PR.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x7F80, 0xFF80, 0x0000, 0x8000]
    t = torch.tensor(x).to(torch.bfloat16)
    assert PR.bits_of(t).tolist() == PR.bf16_bits(x).tolist()          # torch's conversion agrees


def test_off_values_are_the_identity_bit_for_bit():
    bits = np.array([0x0000, 0x8000, 0xFF80, 0x7F80, 0x4020, 0xC040, 0x0001, 0x8001, 0x3F80], dtype=np.uint16)
    hist = list(range(bits.size)) * 3
    assert PR.adjusted_bits(bits, hist, 1.0, 0.0, 0.0).tolist() == bits.tolist()
    row = PR.tensor_of(bits)
    assert PR.bits_of(PR.adjusted_row(row, hist)).tolist() == bits.tolist()


def test_only_history_columns_inside_the_vocab_change():
    bits, _, _ = PR.fixture(250)
    row = bits[PR.ROW_SPECIAL]
    out = PR.adjusted_bits(row, [3, 3, 250, -1, 10**6, 249], *ALL)
    changed = np.nonzero(out != row)[0].tolist()
    assert changed == [3, 249]
    assert out[3] == PR.adjusted_value(int(row[3]), 2, *ALL) and out[249] == PR.adjusted_value(int(row[249]), 1, *ALL)
    assert P.counts([3, 3, 250, 3]) == {3: 3, 250: 1} == PR.counts([3, 3, 250, 3])


# ---- the GPU fixtures are not vacuous: decided here, by the reference alone --------------------------------------------------------------
@pytest.mark.parametrize("vocab", (250, 256, 32000, 128256))
@pytest.mark.parametrize("name", sorted(PR.PENALTIES))
def test_fixture_rows_marked_flips_flip(vocab, name):
    bits, tokens, length = PR.fixture(vocab)
    hist = PR.histories(tokens, PR.START, length)
    pen = PR.PENALTIES[name]
    args = (pen.get("repetition_penalty", 1.0), pen.get("frequency_penalty", 0.0), pen.get("presence_penalty", 0.0))
    assert hist[PR.ROW_EMPTY] == [] and len(hist[PR.ROW_ONE]) == 1
    assert length[PR.ROW_FULL] == tokens.size(1) - 1                    # one free place, the pick's
    for r in PR.FLIPS[name]:
        raw = PR.argmax_bits(bits[r])
        assert raw == PR.TOP and hist[r].count(PR.TOP) == (1 if r == PR.ROW_ARGMAX else 3)
        assert PR.argmax_bits(PR.adjusted_bits(bits[r], hist[r], *args)) == PR.RUNNER != raw
    # the empty history changes nothing
    assert PR.adjusted_bits(bits[PR.ROW_EMPTY], hist[PR.ROW_EMPTY], *args).tolist() == bits[PR.ROW_EMPTY].tolist()


@pytest.mark.parametrize("vocab", (250, 128256))
def test_the_count_decides_the_frequency_flip(vocab):
    bits, tokens, length = PR.fixture(vocab)
    hist = PR.histories(tokens, PR.START, length)[PR.ROW_COUNT]
    once = [t for t in hist if t != PR.TOP] + [PR.TOP]
    assert hist.count(PR.TOP) == 3 and once.count(PR.TOP) == 1
    row = bits[PR.ROW_COUNT]
    assert PR.argmax_bits(PR.adjusted_bits(row, hist, 1.0, 0.75, 0.0)) == PR.RUNNER
    assert PR.argmax_bits(PR.adjusted_bits(row, once, 1.0, 0.75, 0.0)) == PR.TOP
    assert PR.argmax_bits(PR.adjusted_bits(row, hist, 1.0, 0.0, 0.75)) == PR.TOP     # presence counts once: no flip


def test_special_row_holds_the_special_values():
    bits, tokens, length = PR.fixture(256)
    hist = PR.histories(tokens, PR.START, length)[PR.ROW_SPECIAL]
    assert [int(bits[PR.ROW_SPECIAL, t]) for t in PR.SPECIAL_IDS] == list(PR.SPECIAL_BITS)
    assert hist.count(PR.SPECIAL_IDS[5]) == PR.FUSED["count"]
    out = PR.adjusted_bits(bits[PR.ROW_SPECIAL], hist, *ALL)
    assert int(out[PR.SPECIAL_IDS[5]]) == PR.FUSED["want"]
    assert int(out[PR.SPECIAL_IDS[0]]) == PR.NEG_INF and int(out[PR.SPECIAL_IDS[1]]) == int(out[PR.SPECIAL_IDS[2]]) == 0xBF80


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_check_penalties_accepts_the_ranges_and_none():
    assert P.check_penalties(None, None, None) == (1.0, 0.0, 0.0)
    assert P.check_penalties(0.125, -8, 8.0) == (0.125, -8.0, 8.0)
    assert P.check_penalties(8, 0, 0) == (8.0, 0.0, 0.0)
    assert not P.penalties_on(1.0, 0.0, -0.0) and P.penalties_on(1.0, 0.0, 0.5) and P.penalties_on(1.2, 0.0, 0.0)
    assert P.record(1.0, 0.0, 0.0) is None
    assert P.record(1.2, 0.0, 0.5) == {"repetition": 1.2, "frequency": 0.0, "presence": 0.5}


@pytest.mark.parametrize("args", [(0.1, 0, 0), (8.5, 0, 0), (0.0, 0, 0), (-1.0, 0, 0), (1.0, 8.5, 0), (1.0, -9, 0), (1.0, 0, 8.01), (1.0, 0, -8.01),
                                  (float("nan"), 0, 0), (1.0, float("nan"), 0), (1.0, 0, float("nan")), (float("inf"), 0, 0),
                                  (1.0, float("inf"), 0), (1.0, 0, float("-inf"))])
def test_check_penalties_refuses_values_out_of_range(args):
    with pytest.raises(ValueError):
        P.check_penalties(*args)


@pytest.mark.parametrize("args", [(True, 0, 0), (1.0, False, 0), (1.0, 0, True), ("1.2", 0, 0), (1.0, "0.5", 0), (1.0, 0, [0.5])])
def test_check_penalties_refuses_bools_and_strings(args):
    with pytest.raises(TypeError):
        P.check_penalties(*args)


def test_check_history_refuses_what_the_tables_cannot_hold():
    P.check_history(P.MAX_HISTORY, P.MAX_VOCAB)
    with pytest.raises(ValueError, match="2048"):
        P.check_history(P.MAX_HISTORY + 1, 32000)
    with pytest.raises(ValueError, match="131072"):
        P.check_history(100, P.MAX_VOCAB + 1)


# ---- refusals before anything touches the GPU --------------------------------------------------------------------------------------------
def test_speculate_with_a_penalty_is_refused_before_the_model_is_touched():
    prompts = [torch.arange(5)]
    with pytest.raises(ValueError, match="speculate=2 does not go with penalties"):
        generate_batch(None, prompts, 4, top_k=1, speculate=2, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="speculate=3 does not go with penalties"):
        generate(None, prompts[0], 9, top_k=1, speculate=3, presence_penalty=0.5)
    for fn, kw in ((generate_batch, {}), (generate_stream, {}), (sample_batch, dict(num_samples=2))):
        with pytest.raises(ValueError, match="frequency_penalty"):
            fn(None, prompts, 4, frequency_penalty=9.0, **kw)
        with pytest.raises(TypeError, match="repetition_penalty"):
            fn(None, prompts, 4, repetition_penalty=True, **kw)


BASE = ["--test_path", "x.json", "--model_path", "m.pth", "--llm_checkpoint", "ckpt"]


def parse(extra):
    from dualhyp_amd.inference import parse_args
    return parse_args(BASE + list(extra))


def test_cli_defaults_and_accepted_combinations():
    a = parse([])
    assert (a.repetition_penalty, a.frequency_penalty, a.presence_penalty) == (1.0, 0.0, 0.0)
    a = parse(["--repetition_penalty", "1.2", "--frequency_penalty", "0.5", "--presence_penalty", "-0.25", "--schedule", "continuous",
               "--share_prefix", "auto", "--constrain", "prompt", "--no_repeat_ngram", "3", "--logprobs", "--top_logprobs", "3",
               "--top_k", "40", "--top_p", "0.9", "--min_p", "0.05", "--quantize", "fp8", "--kv_cache", "fp8"])
    assert (a.repetition_penalty, a.frequency_penalty, a.presence_penalty) == (1.2, 0.5, -0.25)
    a = parse(["--presence_penalty", "0.5", "--num_samples", "3", "--top_k", "0"])
    assert a.num_samples == 3 and a.presence_penalty == 0.5


@pytest.mark.parametrize("extra, text", [
    (["--repetition_penalty", "1.2", "--speculate", "2"], "--speculate 2 does not go with --repetition_penalty 1.2"),
    (["--frequency_penalty", "0.5", "--num_beams", "2"], "--num_beams 2 does not go with"),
    (["--presence_penalty", "0.5", "--num_beams", "3"], "--num_beams 3 does not go with"),
    (["--repetition_penalty", "9"], "is not in [0.125, 8.0]"),
    (["--frequency_penalty", "nan"], "is not in [-8.0, 8.0]"),
    (["--presence_penalty", "-8.5"], "is not in [-8.0, 8.0]"),
])
def test_cli_refusals(extra, text, capsys):
    with pytest.raises(SystemExit):
        parse(extra)
    assert text in capsys.readouterr().err


def test_records_gain_penalties_only_off_the_defaults():
    from dualhyp_amd.inference import run_inference
    ex = [dict(input_ids_no_response=torch.arange(4), ground_truth="1 2")]

    def gen(prompts):
        return [torch.cat([p, torch.tensor([1, 2])]) for p in prompts]

    def decode(ids):
        return " ".join(str(int(i)) for i in ids)

    plain = run_inference(gen, ex, decode, batch_size=1)
    gen.penalties = P.record(1.2, 0.0, 0.5)
    pen = run_inference(gen, ex, decode, batch_size=1)
    p0, p1 = plain["predictions"][0], pen["predictions"][0]
    assert "penalties" not in p0
    assert p1["penalties"] == {"repetition": 1.2, "frequency": 0.0, "presence": 0.5}
    assert {k: v for k, v in p1.items() if k != "penalties"} == p0


# ---- the library ---------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("dh_sample_bf16_penalty", "dh_sample_rows_bf16_penalty", "dh_engine_set_penalties")


def test_lib_declares_and_exports_the_new_entries():
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["dh_sample_bf16_penalty"][1][:-1] == _lib.SIGNATURES["dh_sample_bf16_nucleus"][1]
    assert _lib.SIGNATURES["dh_sample_rows_bf16_penalty"][1][:-1] == _lib.SIGNATURES["dh_sample_rows_bf16_nucleus"][1]
    assert ctypes.sizeof(_lib.PenaltyArgs) == 12 and [f[0] for f in _lib.PenaltyArgs._fields_] == ["repetition", "frequency", "presence"]
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None
    assert _lib.load().dh_abi_version() == 6


def test_header_declares_what_lib_declares():
    text = (Path(__file__).resolve().parents[1] / "include" / "dualhyp_hip.h").read_text()
    for name in NEW_ENTRIES:
        assert f"int {name}(" in text
    assert "#define DH_MAX_PENALTY_HISTORY 2048" in text and P.MAX_HISTORY == 2048
    assert "typedef struct dh_penalty_args" in text


def test_c_entries_refuse_bad_values_without_a_device():
    lib = _lib.load()
    for bad in ((9.0, 0.0, 0.0), (1.0, float("nan"), 0.0), (1.0, 0.0, -9.0)):
        args = _lib.PenaltyArgs(*bad)
        rc = lib.dh_sample_bf16_penalty(None, 256, None, 8, None, None, 0, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, None, None,
                                        1.0, 0.0, ctypes.byref(args))
        assert rc != 0 and b"dh_sample_bf16_penalty" in lib.dh_last_error()
    # a penalty without start, and a token buffer the tables cannot hold
    on = _lib.PenaltyArgs(1.2, 0.0, 0.0)
    rc = lib.dh_sample_bf16_penalty(None, 256, None, 8, None, None, 0, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, None, None,
                                    1.0, 0.0, ctypes.byref(on))
    assert rc != 0 and b"start" in lib.dh_last_error()
    start = ctypes.c_void_p(16)         # never read: the call is refused, or has no sequence to launch for
    rc = lib.dh_sample_bf16_penalty(None, 256, None, 4096, None, None, 0, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, start, None,
                                    1.0, 0.0, ctypes.byref(on))
    assert rc != 0 and b"2048" in lib.dh_last_error()
    assert lib.dh_sample_bf16_penalty(None, 256, None, 8, None, None, 0, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, 0, start, None,
                                      1.0, 0.0, ctypes.byref(on)) == 0
    assert lib.dh_engine_set_penalties(None, None, None) != 0 and b"null engine" in lib.dh_last_error()
