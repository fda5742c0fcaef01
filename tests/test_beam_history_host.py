"""Beam search over device histories, what needs no GPU: closed-form cases of the host model (tests/beam_history_reference.py), the
crafted cases' coverage (tests/beam_history_cases.py), the C entries' declarations and refusals, the CLI and the Python refusals."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_history_cases as CASES  # noqa: E402
import beam_history_reference as HR  # noqa: E402
from dualhyp_amd import _lib, beam as B, beam_search_batch, inference as I  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def row(*pairs):
    return [(t, lp) for t, lp in pairs]


# ---- the reference, by hand -----------------------------------------------------------------------------------------------------------
def two_beams(**kw):
    """W = 2 behind step 0: beam 0 = [5] (cum -0.25), beam 1 = [6] (cum -0.5)"""
    u = HR.HistUtterance(2, 6, **kw)
    u.step([row((5, -0.25), (6, -0.5), (7, -3.0), (8, -4.0))])
    assert [u.history(b) for b in range(2)] == [[5], [6]]
    return u


def test_a_swap_moves_both_histories():
    u = two_beams()
    u.step([row((1, -1.0), (3, -9.0), (4, -9.5), (9, -9.75)), row((2, -0.25), (3, -9.0), (4, -9.5), (9, -9.75))])
    assert [r["parent"] for r in u.records[1]] == [1, 0] and u.events["swap"] == 1 and u.events["fanout"] == 0
    assert [u.history(b) for b in range(2)] == [[6, 2], [5, 1]]
    for w in range(2):
        assert HR.R.backtrack_tokens(u.records, 1, w) == u.history(w)


def test_a_fan_out_copies_one_history_twice():
    u = two_beams()
    u.step([row((1, -5.0), (3, -9.0), (4, -9.5), (9, -9.75)), row((2, -0.25), (3, -0.5), (4, -9.5), (9, -9.75))])
    assert [r["parent"] for r in u.records[1]] == [1, 1] and u.events["fanout"] == 1 and u.events["swap"] == 0
    assert [u.history(b) for b in range(2)] == [[6, 2], [6, 3]]


def test_the_ban_and_its_fallback_row():
    vals = [1.0, 3.0, 2.0, 3.0, 0.5, -0.0, 0.0]                    # raw order: 1, 3, 2, 0, 4, 5, 6 (-0 == +0: index decides)
    assert HR.candidates(vals, [], 2, 1) == [1, 3, 2, 0]
    assert HR.candidates(vals, [3], 2, 1) == [1, 2, 0, 4]           # 6 survivors
    assert HR.candidates(vals, [3, 1, 2], 2, 1) == [0, 4, 5, 6]     # exactly 2 W = 4 survivors: the ban holds
    assert HR.candidates(vals, [3, 1, 2, 0], 2, 1) == [1, 3, 2, 0]  # 3 survivors: the ban is ignored for the row
    assert HR.effective_ban([3, 1, 2, 0], 7, 2, 1) == set() and HR.effective_ban([3, 1, 2], 7, 2, 1) == {1, 2, 3}
    # n = 2 bans what followed the last token before; n = 3 needs the last two
    assert HR.candidates(vals, [1, 3, 1], 2, 2) == [1, 2, 0, 4] and HR.candidates(vals, [1, 3, 1], 2, 3) == [1, 3, 2, 0]
    assert HR.candidates(vals, [1, 3, 2, 1, 3], 2, 3) == [1, 3, 0, 4]
    # under a mask: the ban counts among the allowed ids only, and the fallback is the mask's row
    allowed = {0, 1, 2, 3, 4}
    assert HR.candidates(vals, [6, 5], 2, 1, allowed) == [1, 3, 2, 0]          # banned ids the mask disallows anyway: nothing is cut
    assert HR.candidates(vals, [3], 2, 1, allowed) == [1, 2, 0, 4]
    assert HR.candidates(vals, [3, 1], 2, 1, allowed) == [1, 3, 2, 0]          # 3 survivors: the mask alone
    u = HR.HistUtterance(2, 6, ngram=1)
    u.step([row((3, -0.25), (1, -0.5), (2, -3.0), (0, -4.0))])
    assert u.row_ban(0, 7) == {3} and u.row_ban(1, 7, allowed) == {1} and u.events["ban_kept"] == 2
    assert u.row_ban(0, 4) == set() and u.events["fallback"] == 1


def test_a_stop_sequence_matches_a_beams_own_text_only():
    # (5, 2): beam 0's text is [5], beam 1's [6]; the candidate 2 comes from beam 1 — through beam 0's text it would match
    u = two_beams(stop_seqs=[(5, 2)])
    u.step([row((1, -1.0), (3, -9.0), (4, -9.5), (9, -9.75)), row((2, -0.25), (3, -9.0), (4, -9.5), (9, -9.75))])
    assert not u.pool and [u.history(b) for b in range(2)] == [[6, 2], [5, 1]]
    # (6, 2) is beam 1's own text: the hypothesis ends into the pool, the id stays, the next candidates fill the beams
    u = two_beams(stop_seqs=[(6, 2)])
    u.step([row((1, -1.0), (3, -9.0), (4, -9.5), (9, -9.75)), row((2, -0.25), (3, -9.0), (4, -9.5), (9, -9.75))])
    assert len(u.pool) == 1 and u.pool[0]["tokens"] == [6, 2] and u.pool[0]["finish_reason"] == "stop" and u.pool[0]["parent"] == 1
    assert u.fin_tok() == [2, -1] and [u.history(b) for b in range(2)] == [[5, 1], [5, 3]]      # -1.25, -9.25 before beam 1's -9.5
    # (9, 5): the text [5] is the sequence's tail; only an id from before the text's start (the prompt's last) could complete it
    u = two_beams(stop_seqs=[(9, 5)])
    assert not u.pool and u.events["near_match"] == 1
    # the EOS wins where both hold: the entry drops the id
    u = two_beams(stop_seqs=[(6, 2)], eos_id=2)
    u.step([row((1, -1.0), (3, -9.0), (4, -9.5), (9, -9.75)), row((2, -0.25), (3, -9.0), (4, -9.5), (9, -9.75))])
    assert u.pool[0]["tokens"] == [6] and u.pool[0]["finish_reason"] == "eos" and u.events["eos_and_seq"] == 1
    # a match behind the W-th live beam is never walked
    u = two_beams(stop_seqs=[(6, 4)])
    u.step([row((1, -0.25), (3, -0.5), (7, -9.5), (9, -9.75)), row((2, -1.0), (4, -1.25), (8, -9.5), (9, -9.75))])
    assert not u.pool and [u.history(b) for b in range(2)] == [[5, 1], [5, 3]]


def test_the_crafted_cases_hold_every_event():
    """the kernel-level GPU test replays these cases: each event it must not miss occurs in them (counted here under fp32 torch
    log-probabilities; the GPU test counts again under the device's own)"""
    total = {k: 0 for k in CASES.EVENTS}
    for params in CASES.small_cases():
        c = CASES.build(*params)
        run = CASES.Run(c["logits"], c["W"], c["vocab"], c["ngram"], c["allow"], stop_seqs=c["stop_seqs"]).finish()
        for k, v in run.events().items():
            total[k] += v
        for ut in run.utts:                 # the histories are the backtracked records, whatever happened
            for w in range(len(ut.hist)):
                assert HR.R.backtrack_tokens(ut.records, ut.n_steps - 1, w) == ut.history(w)
    print(total)
    assert all(total[k] >= 20 for k in CASES.EVENTS), total
    words = CASES.pack_bool(torch.tensor([[True] * 31 + [False, True, False]]))
    assert words.tolist() == [[2 ** 31 - 1, 1]]
    assert CASES.pack_bool(torch.ones((1, 32), dtype=torch.bool)).tolist() == [[-1]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_exported_and_bound():
    head = (ROOT / "include" / "dualhyp_hip.h").read_text()
    assert "Beam histories" in head and "typedef struct dh_beam_hist" in head
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in ("dh_beam_select_bf16_hist", "dh_engine_set_beam_history"):
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert decl and hasattr(lib, name), name
        assert decl.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
    assert "#define DH_ABI_VERSION 6" in head and lib.dh_abi_version() == 6
    # the _hist entry: the _stop argument list with the history before the stream; the state struct is untouched
    stop, hist = _lib.SIGNATURES["dh_beam_select_bf16_stop"][1], _lib.SIGNATURES["dh_beam_select_bf16_hist"][1]
    assert hist[:-2] == stop[:-1] and hist[-1] == stop[-1]
    assert [n for n, _ in _lib.BeamState._fields_] == ["cum", "n_steps", "done", "beam_tok", "beam_parent", "beam_lp", "beam_cum", "fin_step",
                                                       "fin_parent", "fin_score", "fin_lp", "n_fin"]
    assert [n for n, _ in _lib.BeamHist._fields_] == ["tokens", "ngram"]


def test_the_c_entries_refuse_their_arguments_before_any_launch():
    lib = _lib.load()
    p = C.c_void_p(64)                # a non-null pointer that is never read
    st = _lib.BeamState(**{n: 64 for n, _ in _lib.BeamState._fields_})

    def spec(lens):
        arr = (C.c_int32 * max(len(lens), 1))(*lens)
        s = _lib.StopSpec(set=None, seqs=64, h_seq_len=C.cast(arr, C.c_void_p).value, n_seqs=len(lens))
        s._keep = arr
        return s

    def select(tokens, ngram, vocab=64, stop=None, fin_tok=p):
        h = _lib.BeamHist(tokens, ngram)
        return lib.dh_beam_select_bf16_hist(p, vocab, 1, 1, 2, 4, -1, 0, None, C.byref(st), p, p, None, 0,
                                            None if stop is None else C.byref(stop), fin_tok, C.byref(h), None)

    cases = ((lambda: select(64, 9), "ngram=9 is not in 0 .. 8"), (lambda: select(64, -1), "ngram=-1 is not in 0 .. 8"),
             (lambda: select(64, 2, vocab=131073), "vocab=131073"), (lambda: select(None, 2), "ngram=2 without the history planes"),
             (lambda: select(None, 0, stop=spec([2, 3])), "2 stop sequences without the history planes"),
             (lambda: select(64, 0, stop=spec([9])), "stop sequence 0 has 9 tokens"),
             (lambda: select(64, 0, stop=spec([2] * 9)), "at most 8"),
             (lambda: select(64, 0, stop=spec([2]), fin_tok=None), "fin_tok"),
             (lambda: lib.dh_beam_select_bf16_hist(p, 64, 1, 1, 2, 4, -1, 0, None, None, p, p, None, 0, None, None, None, None), "null beam state"),
             (lambda: lib.dh_engine_set_beam_history(None, None, 0), "null engine"),
             (lambda: lib.dh_engine_set_beam_history(None, 64, 2), "null engine"))
    for call, why in cases:
        assert call() != 0
        assert why.encode() in lib.dh_last_error(), (why, lib.dh_last_error())
    # the entry that has no histories keeps refusing sequences, with the words it always used
    assert lib.dh_beam_select_bf16_stop(p, 8, 1, 1, 2, 4, -1, 0, None, C.byref(st), p, p, None, 0, C.byref(spec([2])), p, None) != 0
    assert b"histories live on the host" in lib.dh_last_error()


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_beam_history(tmp_path, capsys):
    base = ["--test_path", "/nonexistent/none.json", "--random_init", "--tokenizer", "byte"]
    assert I.parse_args(base).beam_history == "host"
    a = I.parse_args(base + ["--beam_history", "device", "--num_beams", "2", "--no_repeat_ngram", "2"])
    assert a.beam_history == "device" and a.num_beams == 2 and a.no_repeat_ngram == 2
    seqs = tmp_path / "stop.txt"
    seqs.write_text("7\n3 4\n")
    a = I.parse_args(base + ["--beam_history", "device", "--num_beams", "3", "--stop_file", str(seqs)])
    assert a.stop_file == str(seqs)

    def refused(extra, *words):
        with pytest.raises(SystemExit) as ex:
            I.main(base + extra)               # ends at the parser: nothing has been loaded
        err = capsys.readouterr().err
        assert ex.value.code == 2 and all(w in err for w in words), err

    refused(["--beam_history", "device"], "--beam_history device goes with --num_beams")
    refused(["--beam_history", "device", "--no_repeat_ngram", "2"], "--beam_history device goes with --num_beams")
    refused(["--beam_history", "banana", "--num_beams", "2"], "invalid choice")
    # without the flag, and with its default spelled out: the errors it always gave
    for flag in ([], ["--beam_history", "host"]):
        refused(flag + ["--num_beams", "2", "--no_repeat_ngram", "2"], "--no_repeat_ngram 2 does not go with --num_beams 2",
                "histories live on the host")
        refused(flag + ["--num_beams", "2", "--stop_file", str(seqs)], "histories live on the host")
    # what stays refused under device histories, for what it would mean
    refused(["--beam_history", "device", "--num_beams", "2", "--presence_penalty", "0.5"], "--num_beams 2 does not go with", "rank")
    bias = tmp_path / "bias.txt"
    bias.write_text("hello\n")
    refused(["--beam_history", "device", "--num_beams", "2", "--bias_file", str(bias)], "--num_beams 2 does not go with --bias_file", "rank")
    refused(["--beam_history", "device", "--num_beams", "2", "--no_repeat_ngram", "9"], "1..8")


# ---- Python refusals ------------------------------------------------------------------------------------------------------------------
def test_beam_search_batch_refusals_before_the_gpu():
    from dualhyp_amd import GPT, Config
    m = GPT(Config.from_name("parity-tiny"))
    ps = [torch.arange(3, 20), torch.arange(3, 9)]
    with pytest.raises(ValueError, match="banana"):
        beam_search_batch(m, ps, 8, num_beams=2, history="banana")
    # the host default: the refusals it always had, now naming the switch
    with pytest.raises(ValueError, match='histories live on the host.*history="device"'):
        beam_search_batch(m, ps, 8, num_beams=2, no_repeat_ngram=2)
    with pytest.raises(ValueError, match='histories live on the host.*history="device"'):
        beam_search_batch(m, ps, 8, num_beams=2, stop=[[3, 4]])
    # on the device: what stays refused
    with pytest.raises(ValueError, match="0 .. 8"):
        beam_search_batch(m, ps, 8, num_beams=2, history="device", no_repeat_ngram=9)
    with pytest.raises(ValueError, match="at most 8 tokens"):
        beam_search_batch(m, ps, 8, num_beams=2, history="device", stop=[list(range(9))])
    with pytest.raises(ValueError, match="a bias of 1 entries does not go with beam search.*rank"):
        beam_search_batch(m, ps, 8, num_beams=2, history="device", bias=[([3, 4], 2.0)])
    m.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        beam_search_batch(m, ps, 8, num_beams=2, history="device", no_repeat_ngram=2)
    del m.fp8
    # what is left is a model on the CPU: the engine says that there is no CPU path
    with pytest.raises(Exception, match="GPU"):
        beam_search_batch(m, ps, 8, num_beams=2, history="device", no_repeat_ngram=2, stop=[[3, 4]])
    assert B.HISTORIES == ("host", "device")
