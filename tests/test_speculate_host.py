"""Host side of speculative greedy decoding (generate_batch(..., speculate=D)): the proposer's rule on hand-written cases, the host
replay of the acceptance rule, the argument refusals that are raised before anything touches the GPU, and the C-ABI entries (header,
exports, ctypes table)."""
import importlib
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
G = importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function


def test_propose_hand_written_cases():
    from dualhyp_amd.speculate import propose
    # the longest n wins: the last three tokens (1 2 3) occurred at 0 and are followed by 9 8 7; the last token alone (3) occurred
    # later, at 8, followed by 5
    t = [1, 2, 3, 9, 8, 7, 4, 4, 3, 5, 1, 2, 3]
    assert propose(t, 3) == [9, 8, 7]
    assert propose(t, 2) == [9, 8]
    assert propose(t, 3, ngram_max=1) == [5, 1, 2]
    # the latest occurrence wins: (7 7) at 0 followed by 1, and at 4 followed by 2
    assert propose([7, 7, 1, 0, 7, 7, 2, 0, 7, 7], 2) == [2, 0]
    # the occurrence must be EARLIER than the tail itself and followed by a token: (5 5 5) inside 5 5 5 5 starts at 0, followed by
    # the last 5
    assert propose([5, 5, 5, 5], 3) == [5, 5, 5]
    # n falls back: no earlier (8 2 3), no earlier (2 3)... but 3 alone occurred at 1, followed by 4 6
    assert propose([0, 3, 4, 6, 8, 2, 3], 2) == [4, 6]
    # padding: the continuation is shorter than D (the match is followed by two tokens only, then the sequence ends)
    assert propose([1, 2, 6, 1, 2], 4) == [6, 1, 2, 2]
    assert propose([4, 9, 4], 3) == [9, 4, 4]
    # a continuation of exactly one token
    assert propose([3, 3], 3) == [3, 3, 3]
    # no match at all: the last token, D times
    assert propose([1, 2, 3, 4], 3) == [4, 4, 4]
    assert propose([6], 2) == [6, 6]
    assert propose([1, 2], 1) == [2]
    # tensors' ids are plain ints in a list
    assert propose(torch.tensor([1, 2, 6, 1, 2]).tolist(), 1) == [6]


def test_replay_counts_steps():
    from dualhyp_amd.speculate import replay
    gen = list(range(10, 26))                                   # 16 generated tokens, no EOS
    true = lambda D: (lambda k: (gen + [0] * D)[k:k + D])          # draft_1 stands for the token row 0 picks: gen[k]
    for D in (1, 2, 3, 7):
        r = replay(gen, true(D), D)
        assert r["steps"] == -(-(len(gen) - 1) // (D + 1))
        assert r["drafted"] == D * r["steps"] and r["accepted"] == len(gen) - 1 - r["steps"]
    wrong = replay(gen, lambda k: [999] * 3, 3)
    assert wrong == dict(steps=15, drafted=45, accepted=0)
    # every second draft position wrong: draft_1 right, draft_2 wrong -> two tokens per step
    half = replay(gen, lambda k: [gen[k], 999, 999], 3)
    assert half["steps"] == 8 and half["accepted"] == 7
    # an EOS inside an accepted run ends the sequence there; as the first sample, no step at all
    assert replay([10, 11, 2], true(3), 3, eos_id=2) == dict(steps=1, drafted=3, accepted=1)
    assert replay([2], true(3), 3, eos_id=2) == dict(steps=0, drafted=0, accepted=0)


def _cpu_model(name="parity-tiny", **over):
    from dualhyp_amd import GPT, Config
    return GPT(Config.from_name(name, **over))


def test_refusals_before_the_gpu():
    m = _cpu_model()                                            # 4 heads in 2 groups: q_per_kv = 2
    ps = [torch.arange(3, 20), torch.arange(3, 9)]
    kw = dict(temperature=0.2)
    for top_k in (None, 0, 2, 5):
        with pytest.raises(ValueError, match="top_k"):
            G.generate_batch(m, ps, 8, top_k=top_k, speculate=2, **kw)
    for bad in (-1, 8, 1.5, True, "2"):
        with pytest.raises(ValueError, match="speculate"):
            G.generate_batch(m, ps, 8, top_k=1, speculate=bad, **kw)
    # (D + 1) * q_per_kv > 32: a model with 16 heads per KV group takes D = 1 only
    wide = _cpu_model(n_head=16, n_query_groups=1, n_embd=1024)
    with pytest.raises(ValueError, match="query columns"):
        G.generate_batch(wide, ps, 8, top_k=1, speculate=2, **kw)
    # B * S > 2048 rows
    with pytest.raises(ValueError, match="2048"):
        G.generate_batch(m, [ps[0]] * 600, 8, top_k=1, speculate=3, **kw)
    # fp8, RelPrompt and the CPU rsqrt emulation, each with its reason
    m.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        G.generate_batch(m, ps, 8, top_k=1, speculate=2, **kw)
    del m.fp8
    m.cpu_rsqrt_vec_width = 32
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.generate_batch(m, ps, 8, top_k=1, speculate=2, **kw)
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.generate(m, ps[0], 30, top_k=1, speculate=2, **kw)
    m.cpu_rsqrt_vec_width = 0
    from dualhyp_amd.relprompt import GPT as RelGPT
    from dualhyp_amd.speculate import check_arguments
    rel = object.__new__(RelGPT)
    object.__setattr__(rel, "cpu_rsqrt_vec_width", 0)
    object.__setattr__(rel, "config", m.config)
    with pytest.raises(ValueError, match="RelPrompt"):
        check_arguments(rel, 2, 1, 4)
    assert check_arguments(rel, 0, None, 4) == 0 and check_arguments(m, 3, 1, 4) == 3
    # drafts: with speculate > 0 only, [B, max_new_tokens] int64
    with pytest.raises(ValueError, match="drafts"):
        G.generate_batch(m, ps, 8, top_k=1, drafts=torch.zeros((2, 8), dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="drafts"):
        G.generate_batch(m, ps, 8, top_k=1, speculate=2, drafts=torch.zeros((2, 7), dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="drafts"):
        G.generate_batch(m, ps, 8, top_k=1, speculate=2, drafts=torch.zeros((2, 8), dtype=torch.int32), **kw)
    # continuous batching refuses the combination
    with pytest.raises(ValueError, match="continuous"):
        G.generate_stream(m, ps, 8, top_k=1, speculate=2, **kw)


def test_cli_has_the_flag():
    src = (REPO / "dualhyp_amd" / "inference.py").read_text()
    assert '"--speculate"' in src and "default=0" in src[src.index('"--speculate"'):][:120]


def test_cli_refuses_continuous_before_loading_anything(capsys):
    """--speculate with --schedule continuous, or a D outside 0..7, ends at the argument parser: the test path does not exist and
    nobody has asked for it, no model has been built"""
    from dualhyp_amd import inference
    for extra, word in ((["--speculate", "2", "--schedule", "continuous"], "--schedule batch"), (["--speculate", "8"], "1..7")):
        with pytest.raises(SystemExit) as ex:
            inference.main(["--test_path", "/nonexistent/none.json", "--random_init", "--tokenizer", "byte", *extra])
        assert ex.value.code == 2 and word in capsys.readouterr().err


def test_decode_spec_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    raw = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text))
    for n in ("dh_engine_decode_spec", "dh_engine_reserve_rows", "dh_engine_graph_count"):
        assert n in declared, f"{n} is not declared in include/dualhyp_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is missing from the ctypes table"
    assert declared == set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6
    # the comment in front of the declaration cites the loop it replaces
    head = raw[:raw.index("int dh_engine_decode_spec(")]
    assert "generate/base.py:57-80" in head[head.rindex("/*"):]
    # the ctypes argument list has the declaration's length
    decl = text[text.index("int dh_engine_decode_spec("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SIGNATURES["dh_engine_decode_spec"][1])
    # refused before anything is read through the handle
    assert lib.dh_engine_decode_spec(None, None, 8, None, None, None, 1, 4, 2, None, None, 1, 0.2, -1, 0, None) != 0
    assert b"null argument" in lib.dh_last_error()
    assert lib.dh_engine_reserve_rows(None, 8) != 0 and b"null engine" in lib.dh_last_error()
    assert lib.dh_engine_graph_count(None, 0) == -1
