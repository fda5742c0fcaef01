"""No-repeat n-grams on the host: dualhyp_amd.ngram against the hand-written cases of the definition (include/dualhyp_hip.h, "No-repeat
n-grams") and against tests/ngram_reference.py, the argument checks and refusals of the entry points (before anything is launched:
on a CPU model), the --no_repeat_ngram flag, run_inference's record fields, and the new entries of the C ABI."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ngram_reference as R  # noqa: E402
from dualhyp_amd import GPT, Config, beam_search_batch, generate, generate_batch, generate_stream  # noqa: E402
from dualhyp_amd import inference as I  # noqa: E402
from dualhyp_amd import ngram as N  # noqa: E402

A, B_, C_, X, Y = 11, 22, 33, 44, 55

CASES = [
    # (generated, n, ban set, what)
    ([], 1, set(), "m = 0"),
    ([A], 2, set(), "m < n"),
    ([A, B_], 3, set(), "m = n - 1"),
    ([A, B_, C_], 3, set(), "m = n, the one candidate does not match"),
    ([A, B_, C_, X], 2, set(), "m >= n with no earlier occurrence of the suffix"),
    ([A, B_, C_, X, Y, A, B_], 3, {C_}, "one earlier occurrence"),
    ([X, A, X, B_, Y, X, C_, X], 2, {A, B_, C_}, "several earlier occurrences with different followers"),
    ([X, Y, A, X, Y, B_, X, Y], 3, {A, B_}, "several occurrences, n = 3"),
    ([A, A, A, A], 3, {A}, "overlapping occurrences"),
    ([A, A, A], 3, {A}, "the occurrence that ends right before the suffix's last token: i = m - n = 0"),
    ([Y, A, A], 2, {A}, "i = m - n: the candidate's follower is the last token"),
    ([Y, X, A, X], 2, {A}, "the occurrence and its follower end where the suffix starts"),
    ([A, B_, A, C_], 1, {A, B_, C_}, "n = 1: every id already generated"),
    ([A], 1, {A}, "n = 1, m = 1"),
    ([A, B_, C_, X, A, B_, C_], 4, {X}, "n = 4"),
    ([A, B_, C_, A, B_, Y], 3, set(), "the last token breaks the suffix"),
]


@pytest.mark.parametrize("generated,n,want,what", CASES, ids=[c[3] for c in CASES])
def test_banned_hand_written(generated, n, want, what):
    assert N.banned(generated, n) == want, what
    assert R.banned(generated, n) == want, what
    assert N.banned(torch.tensor(generated, dtype=torch.int64).tolist(), n) == want


def test_an_ngram_that_lies_only_in_the_prompt_is_not_banned():
    prompt, generated = [X, Y, A, X, Y, B_], [C_, X, Y]
    assert N.banned(generated, 3) == set()                          # the history is the generated text alone
    assert N.banned(prompt + generated, 3) == {A, B_}               # what a history that began at 0 would ban
    # an n-gram that straddles the prompt's end does not count either
    assert N.banned([X, Y, A, X, Y], 3) == {A} and N.banned([A, X, Y], 3) == set()      # prompt X Y, text A X Y


def test_definitions_agree_on_random_texts():
    g = np.random.default_rng(5)
    some = 0
    for trial in range(300):
        n = int(g.integers(1, 9))
        text = g.integers(0, int(g.integers(2, 5)), int(g.integers(0, 30))).tolist()
        assert N.banned(text, n) == R.banned(text, n), (text, n)
        assert N.ban_positions(text, n) == R.ban_positions(text, n)
        some += bool(N.banned(text, n))
    assert some > 50
    for kind in R.KINDS:
        for n in range(1, 9):
            p, text = R.history(kind, n, [1, 5, 6], 8, seed=n)
            assert all(0 <= t < 8 for t in p + text) and N.banned(text, n) == R.banned(text, n), (kind, n)


def test_ban_positions_counts_the_positions_with_a_ban():
    assert N.ban_positions([], 2) == [] and N.ban_positions([A, B_, C_], 2) == []
    # position t is counted when banned(text[:t]) is non-empty, whatever was picked there
    assert N.ban_positions([A, B_, A, C_, A], 2) == [3]             # behind A B A the suffix A has occurred; behind A B A C it has not
    assert N.ban_positions([A, B_, A, C_, A, X], 2) == [3, 5]
    assert N.ban_positions([A, A, A], 1) == [1, 2]
    assert N.ban_positions([A, B_, C_, A, B_, X, Y], 3) == [5]


def test_pick_row_fallback_in_the_reference():
    allowed = np.zeros(8, dtype=bool)
    allowed[[2, 5]] = True
    row, fell = R.pick_row(allowed, [2, 5], 1, 8)
    assert fell and row.tolist() == allowed.tolist()                # the mask allows exactly the banned ids: the ban is ignored
    row, fell = R.pick_row(allowed, [2], 1, 8)
    assert not fell and row.nonzero()[0].tolist() == [5]
    row, fell = R.pick_row(None, list(range(8)), 1, 8)
    assert fell and bool(row.all())                                 # no mask: every id is banned, every id is allowed
    row, fell = R.pick_row(None, [3, 3], 1, 8)
    assert not fell and row.nonzero()[0].tolist() == [0, 1, 2, 4, 5, 6, 7]


def test_check_ngram():
    assert [N.check_ngram(n) for n in range(9)] == list(range(9))
    assert N.check_ngram(4, 131072) == 4 and N.check_ngram(0, 1 << 20) == 0
    for bad in (-1, 9, 100):
        with pytest.raises(ValueError, match="0 .. 8"):
            N.check_ngram(bad)
    for bad in (2.0, "3", None, True):
        with pytest.raises(TypeError):
            N.check_ngram(bad)
    with pytest.raises(ValueError, match="131072"):
        N.check_ngram(2, 131073)
    with pytest.raises(ValueError):
        N.banned([1, 2], 0)
    with pytest.raises(ValueError):
        N.banned([1, 2], 9)


def test_entry_points_refuse_before_anything_is_launched():
    """on a CPU model: a call that got as far as the engine would fail for another reason"""
    cfg = Config.from_name("parity-tiny")
    m = GPT(cfg)
    ps = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    for fn in (generate_batch, generate_stream):
        for bad in (-1, 9):
            with pytest.raises(ValueError, match="no_repeat_ngram"):
                fn(m, ps, 4, no_repeat_ngram=bad)
        with pytest.raises(TypeError, match="no_repeat_ngram"):
            fn(m, ps, 4, no_repeat_ngram=2.5)
    with pytest.raises(ValueError, match="no_repeat_ngram"):
        generate(m, ps[0], 8, no_repeat_ngram=12)
    with pytest.raises(ValueError, match="beam"):
        beam_search_batch(m, ps, 4, num_beams=2, no_repeat_ngram=2)
    with pytest.raises(ValueError, match="0 .. 8"):
        beam_search_batch(m, ps, 4, num_beams=2, no_repeat_ngram=9)


def test_new_entries_are_declared_and_bound():
    """tests/test_capi.py would fail on a mismatch between the header and the table; this states which names the feature adds"""
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    assert "No-repeat n-grams" in head and head.index("Token masks") < head.index("No-repeat n-grams")
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in ("dh_sample_bf16_ngram", "dh_sample_rows_bf16_ngram", "dh_engine_set_no_repeat_ngram"):
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert decl and hasattr(lib, name), name
        assert decl.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
        at = head.index(f"int {name}(")
        assert "generate/base.py:62-80" in head[head.rfind("/*", 0, at):at], f"{name} cites the reference line it extends"
    # the _ngram samplers: the _mask argument lists plus n and the prompt lengths
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_ngram"][1] == _lib.SIGNATURES[old + "_mask"][1] + [_lib.I, _lib.P]
    assert "#define DH_ABI_VERSION 6" in head


def test_c_entries_refuse_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)                # a non-null pointer that is never read

    def sample(vocab, ngram, start):
        return lib.dh_sample_bf16_ngram(p, vocab, p, 4, p, p, 1, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 0, ngram, start)

    def rows(vocab, ngram):
        return lib.dh_sample_rows_bf16_ngram(p, vocab, p, 4, p, p, p, p, 1, 1, 2, 1.0, 1, -1, 0, None, None, 0, None, None, None, 0, ngram, None)

    for call, why in ((lambda: sample(8, 0, p), "ngram=0"), (lambda: sample(8, 9, p), "0 .. 8"), (lambda: sample(8, 2, None), "start"),
                      (lambda: sample(131073, 2, p), "131072"), (lambda: rows(8, 0), "ngram=0"), (lambda: rows(8, -3), "ngram=-3"),
                      (lambda: rows(200000, 1), "131072"), (lambda: lib.dh_engine_set_no_repeat_ngram(None, 2, p), "null engine")):
        assert call() != 0
        assert why.encode() in lib.dh_last_error(), (why, lib.dh_last_error())


def test_no_repeat_ngram_flag_parses():
    base = ["--test_path", "x.json", "--random_init"]
    assert I.parse_args(base).no_repeat_ngram == 0
    assert I.parse_args(base + ["--no_repeat_ngram", "4"]).no_repeat_ngram == 4
    for more in (["--schedule", "continuous"], ["--speculate", "3"], ["--share_prefix", "auto"], ["--constrain", "prompt"],
                 ["--top_logprobs", "3"], ["--quantize", "fp8", "--kv_cache", "fp8"]):
        assert I.parse_args(base + ["--no_repeat_ngram", "3"] + more).no_repeat_ngram == 3
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            I.parse_args(base + ["--no_repeat_ngram", bad])
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--no_repeat_ngram", "2", "--num_beams", "2"])
    assert I.parse_args(base + ["--num_beams", "2"]).no_repeat_ngram == 0


def test_run_inference_records_the_bans():
    from dualhyp_amd.tokenizer import ByteTokenizer
    tok = ByteTokenizer()
    enc = lambda s: torch.tensor(tok.encode(s), dtype=torch.int64)      # noqa: E731
    exs = [{"input_ids_no_response": enc("### Response:\n"), "ground_truth": "abcab"},
           {"input_ids_no_response": enc("ab ### Response:\n"), "ground_truth": "xyz"}]
    answers = ["abcabd", "xyz"]

    def gen(prompts):
        return [torch.cat([p, enc(a)[-len(a):]]) for p, a in zip(prompts, answers)]

    plain = I.run_inference(gen, exs, tok.decode, batch_size=2)
    assert "ngram_bans" not in plain["predictions"][0] and "no_repeat_ngram" not in plain["predictions"][0]
    gen.no_repeat_ngram = 2
    marked = I.run_inference(gen, exs, tok.decode, batch_size=2)
    for rec, a, p in zip(marked["predictions"], answers, exs):
        ids = enc(a)[-len(a):].tolist()
        assert rec["no_repeat_ngram"] == 2 and rec["ngram_bans"] == len(R.ban_positions(ids, 2))
    assert marked["predictions"][0]["ngram_bans"] == 2 and marked["predictions"][1]["ngram_bans"] == 0   # behind "abca" and "abcab"
    assert {k: v for k, v in marked["predictions"][0].items() if k not in ("no_repeat_ngram", "ngram_bans")} == plain["predictions"][0]
