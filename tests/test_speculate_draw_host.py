"""Host side of sampled verification (generate_batch(..., speculate=D, verify="draw")): the argument checks that are raised before
anything touches the GPU, the command line's --speculate_verify, and the C-ABI entry (header, exports, ctypes table)."""
import importlib
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
G = importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function
BASE = ["--test_path", "/nonexistent/none.json", "--random_init", "--tokenizer", "byte"]


def _cpu_model(name="parity-tiny", **over):
    from dualhyp_amd import GPT, Config
    return GPT(Config.from_name(name, **over))


def test_verify_is_checked_before_the_model_is_touched():
    m = _cpu_model()
    ps = [torch.arange(3, 20), torch.arange(3, 9)]
    kw = dict(temperature=0.8, top_k=5)
    for bad in ("sample", "Draw", "", None, 1, True):
        with pytest.raises(ValueError, match="verify"):
            G.generate_batch(m, ps, 8, speculate=2, verify=bad, **kw)
        with pytest.raises(ValueError, match="verify"):
            G.sample_batch(m, ps, 8, num_samples=2, speculate=2, verify=bad, **kw)
    # "draw" says how a verify step confirms its drafts: without speculate there is none
    for fn, extra in ((G.generate_batch, {}), (G.sample_batch, dict(num_samples=2)), (G.generate_stream, {})):
        with pytest.raises(ValueError, match="speculate > 0"):
            fn(m, ps, 8, verify="draw", **extra, **kw)
    with pytest.raises(ValueError, match="speculate > 0"):
        G.generate(m, ps[0], 30, verify="draw", **kw)
    # the default still refuses what it refused, in the words it used
    with pytest.raises(ValueError, match="needs top_k=1"):
        G.generate_batch(m, ps, 8, speculate=2, **kw)
    with pytest.raises(ValueError, match="needs top_k=1"):
        G.generate_batch(m, ps, 8, speculate=2, verify="argmax", **kw)
    with pytest.raises(ValueError, match="does not go with penalties"):
        G.generate_batch(m, ps, 8, speculate=2, top_k=1, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="confirms drafts against the arg-max"):
        G.sample_batch(m, ps, 8, num_samples=2, speculate=2, **kw)
    # continuous batching steps one token at a time, whatever the mode
    with pytest.raises(ValueError, match="continuous"):
        G.generate_stream(m, ps, 8, speculate=2, verify="draw", **kw)
    # speculate itself is still checked
    for bad in (-1, 8, 1.5, "2"):
        with pytest.raises(ValueError, match="speculate"):
            G.generate_batch(m, ps, 8, speculate=bad, verify="draw", **kw)
    # the verify attention's columns and the streaming step's rows bound a sampled call as they bound a greedy one
    wide = _cpu_model(n_head=16, n_query_groups=1, n_embd=1024)
    with pytest.raises(ValueError, match="query columns"):
        G.generate_batch(wide, ps, 8, speculate=2, verify="draw", **kw)
    with pytest.raises(ValueError, match="2048"):
        G.generate_batch(m, [ps[0]] * 600, 8, speculate=3, verify="draw", **kw)
    with pytest.raises(ValueError, match="2048"):
        G.sample_batch(m, [ps[0]] * 200, 8, num_samples=3, speculate=3, verify="draw", **kw)      # 600 rows x 4 positions
    # fp8, the CPU rsqrt emulation and RelPrompt, each with its reason
    m.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        G.generate_batch(m, ps, 8, speculate=2, verify="draw", **kw)
    with pytest.raises(ValueError, match="fp8"):
        G.sample_batch(m, ps, 8, num_samples=2, speculate=2, verify="draw", **kw)
    del m.fp8
    m.cpu_rsqrt_vec_width = 32
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.generate_batch(m, ps, 8, speculate=2, verify="draw", **kw)
    m.cpu_rsqrt_vec_width = 0
    from dualhyp_amd.relprompt import GPT as RelGPT
    from dualhyp_amd.speculate import check_arguments, check_verify
    rel = object.__new__(RelGPT)
    object.__setattr__(rel, "cpu_rsqrt_vec_width", 0)
    object.__setattr__(rel, "config", m.config)
    with pytest.raises(ValueError, match="RelPrompt"):
        check_arguments(rel, 2, 5, 4, "draw")
    with pytest.raises(ValueError, match="RelPrompt"):
        G.sample_batch(rel, ps, 8, num_samples=2, speculate=2, verify="draw", **kw)
    # shared-prompt attention reads rows of an utterance; a verify step's rows are positions of a sequence
    with pytest.raises(ValueError, match="shared_prompt=True does not go with speculate"):
        G.sample_batch(m, ps, 8, num_samples=2, speculate=2, verify="draw", shared_prompt=True, **kw)
    # drafts: sample_batch's are a row per decode row
    with pytest.raises(ValueError, match="drafts"):
        G.sample_batch(m, ps, 8, num_samples=2, speculate=2, verify="draw", drafts=torch.zeros((2, 8), dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="drafts"):
        G.sample_batch(m, ps, 8, num_samples=2, drafts=torch.zeros((4, 8), dtype=torch.int64), **kw)
    # what the mode opens
    assert check_verify("draw", 3) is True and check_verify("argmax", 3) is False and check_verify("argmax", 0) is False
    for top_k in (None, 0, 1, 2, 40):
        assert check_arguments(m, 3, top_k, 4, "draw") == 3
    assert check_arguments(m, 0, 5, 4) == 0 and check_arguments(m, 3, 1, 4) == 3
    from dualhyp_amd.automaton import from_prompts
    picks = G._Picks.check(speculate=3, verify="draw", top_p=0.9, min_p=0.05, repetition_penalty=1.3, frequency_penalty=0.4,
                           presence_penalty=0.3, bias=[([5, 6, 7], 2.0)], automaton=from_prompts([p.tolist() for p in ps], order=2, eos_id=2),
                           no_repeat_ngram=2, stop=[4], return_logprobs=True, top_logprobs=2)
    assert picks.pen == (1.3, 0.4, 0.3) and picks.bias is not None and picks.aut is not None and picks.top_p == 0.9


OPENED = (["--top_k", "40"], ["--top_k", "0", "--temperature", "0.8"], ["--top_k", "40", "--top_p", "0.9", "--min_p", "0.05"],
          ["--repetition_penalty", "1.3"], ["--frequency_penalty", "0.4", "--presence_penalty", "0.3"], ["--bias_file", "phrases.txt"],
          ["--constrain", "chain"], ["--num_samples", "3", "--top_k", "40"])


@pytest.mark.parametrize("extra", OPENED, ids=lambda e: " ".join(e))
def test_cli_opens_the_sampled_path_with_the_flag_only(extra, capsys):
    from dualhyp_amd import inference
    args = inference.parse_args([*BASE, "--speculate", "3", "--speculate_verify", "draw", *extra])
    assert args.speculate == 3 and args.speculate_verify == "draw"
    for mode in ([], ["--speculate_verify", "argmax"]):
        with pytest.raises(SystemExit) as ex:
            inference.parse_args([*BASE, "--speculate", "3", *mode, *extra])
        err = capsys.readouterr().err.replace("\n", " ")
        assert ex.value.code == 2 and ("--speculate 3 does not go with" in err or "does not go with --speculate 3" in err)


def test_cli_keeps_the_other_refusals(capsys):
    from dualhyp_amd import inference
    assert inference.parse_args(BASE).speculate_verify == "argmax"
    assert inference.parse_args([*BASE, "--speculate", "3"]).speculate_verify == "argmax"
    draw = ["--speculate", "3", "--speculate_verify", "draw"]
    for extra, word in ((["--speculate_verify", "draw"], "goes with --speculate"),
                        ([*draw, "--schedule", "continuous"], "--schedule batch"),
                        ([*draw, "--num_beams", "2"], "--num_beams 2 does not go with --speculate 3"),
                        ([*draw, "--quantize", "fp8"], "--quantize fp8"),
                        ([*draw, "--quantize", "mxfp4"], "--quantize mxfp4"),
                        ([*draw, "--num_samples", "3"], "--top_k 1"),
                        ([*draw, "--num_samples", "3", "--top_k", "40", "--share_prompt_kv"], "--share_prompt_kv does not go with --speculate"),
                        (["--speculate", "3", "--speculate_verify", "sample"], "invalid choice")):
        with pytest.raises(SystemExit) as ex:
            inference.parse_args([*BASE, *extra])
        assert ex.value.code == 2 and word in capsys.readouterr().err.replace("\n", " "), extra


def test_records_name_the_mode():
    src = (REPO / "dualhyp_amd" / "inference.py").read_text()
    assert 'preds[i]["speculate_verify"]' in src and '"--speculate_verify"' in src
    assert 'default="argmax"' in src[src.index('"--speculate_verify"'):][:120]


def test_decode_spec_draw_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    raw = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text))
    n = "dh_engine_decode_spec_draw"
    assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES
    assert declared == set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6
    # the paragraph in front of the declaration states the key and the equality
    head = raw[:raw.index(f"int {n}(")]
    para = head[head.rindex("/*"):]
    assert "Sampled verification" in para and "(seed, step, seq)" in para and "limit[u] - max_new_tokens" in para and "bit for bit" in para

    def arity(name):
        decl = text[text.index(f"int {name}("):]
        return decl[:decl.index(";")].count(",") + 1

    # dh_engine_decode_spec's arguments plus top_k and seed; the greedy entry is what it was
    assert arity(n) == len(_lib.SIGNATURES[n][1]) == arity("dh_engine_decode_spec") + 2
    assert _lib.SIGNATURES["dh_engine_decode_spec"][1] == [_lib.SIGNATURES[n][1][i] for i in range(18) if i not in (13, 15)]
    # refused before anything is read through the handle
    assert lib.dh_engine_decode_spec_draw(None, None, 8, None, None, None, 1, 4, 2, None, None, 1, 0.8, 5, -1, 7, 0, None) != 0
    assert b"dh_engine_decode_spec_draw: null argument" in lib.dh_last_error()
    assert lib.dh_engine_decode_spec(None, None, 8, None, None, None, 1, 4, 2, None, None, 1, 0.2, -1, 0, None) != 0
    assert b"dh_engine_decode_spec: null argument" in lib.dh_last_error()
