"""Host side of shared-prompt attention (include/dualhyp_hip.h, "Shared-prompt attention"; --share_prompt_kv): the argument checks of
the op, of the C entries and of sample_batch / beam_search_batch, each before anything is launched; the parser's flag and its
refusals; the records' `shared_prompt` key with a stub generate function.  No GPU."""
import importlib
from pathlib import Path

import pytest
import torch

from dualhyp_amd.inference import parse_args, run_inference

REPO = Path(__file__).resolve().parent.parent
G = importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function


# ---- 1. argument checks --------------------------------------------------------------------------------------------------------
def test_group_rows_of_the_op():
    from dualhyp_amd import ops
    assert [ops.check_shared_rows(24, n) for n in (2, 3, 4, 8)] == [2, 3, 4, 8]
    for rows, n in ((24, 1), (24, 9), (24, 0), (24, True), (24, 2.0), (24, None), (24, 5), (0, 2), (7, 2)):
        with pytest.raises(ValueError, match="attn_decode_shared"):
            ops.check_shared_rows(rows, n)


def test_op_wrapper_refuses_before_it_loads_anything():
    """CPU tensors: a call that got as far as the library would fail differently."""
    from dualhyp_amd import ops
    q32 = torch.zeros(1, 6, 4 * 64)
    kc, vt = torch.zeros(6, 1, 64, 64, dtype=torch.bfloat16), torch.zeros(6, 1, 64, 64, dtype=torch.bfloat16)
    cs = torch.zeros(64, 64, dtype=torch.bfloat16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    args = (q32, 4 * 64, None, 0.0, (128, 192), cs, cs, i32(0, 1, 2, 3, 4, 5), i32(*[9] * 6), kc, vt, 2)
    for n, plen in ((4, i32(5)), (1, i32(5) ), (3, i32(5)), (3, torch.tensor([5, 5])), (3, i32(5, 5, 5)), (3, [5, 5]), (3, None)):
        with pytest.raises(ValueError, match="attn_decode_shared"):
            ops.attn_decode_shared(*args, n, plen)


def test_c_entries_refuse_without_a_gpu():
    """dh_attn_decode_shared_bf16 checks its arguments before it touches the device: the refusals need no GPU and no real buffer."""
    from dualhyp_amd import _lib
    lib = _lib.load()
    assert {"dh_attn_decode_shared_bf16", "dh_engine_set_shared_prompt", "dh_attn_shared_launch_count"} <= set(_lib.SIGNATURES)
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    assert "Shared-prompt attention" in head and "dh_attn_decode_shared_bf16" in head and "dh_engine_set_shared_prompt" in head
    p = 4096                                                    # any non-null address: a refused call reads none of them

    def call(n_seq=6, N=3, plen=p, hs=64, n_part=2, n_ext=48, qkv_dim=(8 + 4) * 64):
        rc = lib.dh_attn_decode_shared_bf16(p, n_part, 1, n_seq, qkv_dim, n_ext, p, 2.0, 8 * 64, 10 * 64, p, p, p, p, p, p, p, 8, 2, hs, 640, N,
                                            plen, None)
        return rc, lib.dh_last_error().decode(errors="replace")

    c0 = lib.dh_attn_shared_launch_count()
    for kw, word in ((dict(N=1), "group_rows = 1"), (dict(N=9, n_seq=9), "group_rows = 9"), (dict(N=0), "group_rows = 0"),
                     (dict(n_seq=7), "n_seq = 7"), (dict(plen=None), "prompt_len"), (dict(hs=80), "head_size 80"),
                     (dict(n_part=17), "n_part"), (dict(n_ext=16), "48"), (dict(qkv_dim=13 * 64), "qkv_dim")):
        rc, msg = call(**kw)
        assert rc != 0 and "dh_attn_decode_shared_bf16" in msg and word in msg, (kw, msg)
    assert lib.dh_attn_shared_launch_count() == c0
    assert lib.dh_engine_set_shared_prompt(None, 3, p) != 0 and b"null engine" in lib.dh_last_error()
    assert lib.dh_abi_version() == 6


class NoEngineModel:
    """A model whose engine must never be asked for"""
    max_seq_length = 4096
    cpu_rsqrt_vec_width = 0

    def engine(self, *a, **k):
        raise AssertionError("a refused call reached the engine")


def test_python_refusals():
    m = NoEngineModel()
    assert G.check_shared_prompt(m, False, 1, "x") is False and G.check_shared_prompt(m, True, 2, "x") is True
    assert G.check_shared_prompt(m, True, 8, "x") is True
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="shared_prompt is True or False"):
            G.check_shared_prompt(m, bad, 3, "x")
    for rows in (1, 9):
        with pytest.raises(ValueError, match="num_beams=1|2..8"):
            G.check_shared_prompt(m, True, rows, "num_beams=1")
    for attr, value, word in (("fp8", True, "fp8"), ("kv_cache_dtype", "fp8", "fp8 KV cache"), ("cpu_rsqrt_vec_width", 32, "rsqrt")):
        q = NoEngineModel()
        setattr(q, attr, value)
        with pytest.raises(ValueError, match=word):
            G.check_shared_prompt(q, True, 3, "num_samples=3")
        assert G.check_shared_prompt(q, False, 3, "num_samples=3") is False     # off: nothing is asked of the model
        with pytest.raises(ValueError, match=word):
            G.sample_batch(q, [torch.arange(3, 40)], 4, num_samples=3, temperature=0.8, top_k=5, shared_prompt=True)
    with pytest.raises(ValueError, match="shared_prompt"):
        G.sample_batch(m, [torch.arange(3, 40)], 4, num_samples=3, temperature=0.8, top_k=5, shared_prompt="on")


# ---- 2. the parser -------------------------------------------------------------------------------------------------------------
BASE = ["--test_path", "x.json"]


def test_flag_parses():
    assert parse_args(BASE).share_prompt_kv is False              # the path it always was
    a = parse_args(BASE + ["--num_samples", "3", "--top_k", "5", "--temperature", "0.8", "--share_prompt_kv"])
    assert a.share_prompt_kv is True and a.num_samples == 3
    a = parse_args(BASE + ["--num_beams", "4", "--share_prompt_kv", "--beam_history", "device", "--no_repeat_ngram", "3"])
    assert a.share_prompt_kv is True and a.num_beams == 4
    # what it goes with
    a = parse_args(BASE + ["--num_samples", "2", "--top_k", "5", "--share_prompt_kv", "--share_prefix", "auto", "--constrain", "prompt",
                           "--no_repeat_ngram", "2", "--stop", "newline", "--top_logprobs", "2", "--top_p", "0.9", "--repetition_penalty", "1.2"])
    assert a.share_prompt_kv is True and a.logprobs


@pytest.mark.parametrize("argv,why", [
    (["--share_prompt_kv"], "--num_samples N > 1 or --num_beams W > 1"),
    (["--share_prompt_kv", "--num_samples", "1", "--num_beams", "1"], "--num_samples N > 1 or --num_beams W > 1"),
    (["--share_prompt_kv", "--num_samples", "3", "--top_k", "5", "--quantize", "fp8"], "--quantize fp8"),
    (["--share_prompt_kv", "--num_samples", "3", "--top_k", "5", "--quantize", "mxfp4"], "--quantize mxfp4"),
    (["--share_prompt_kv", "--num_samples", "3", "--top_k", "5", "--quantize", "fp8", "--kv_cache", "fp8"], "--quantize fp8"),
])
def test_parser_refusals(argv, why, capsys):
    with pytest.raises(SystemExit):
        parse_args(BASE + argv)
    err = capsys.readouterr().err
    assert "--share_prompt_kv" in err and why in err


# ---- 3. the records --------------------------------------------------------------------------------------------------------------
def byte_decode(t):
    return bytes(int(x) for x in t.reshape(-1).tolist()).decode()


def enc(s):
    return torch.tensor(list(s.encode()), dtype=torch.int64)


@pytest.mark.parametrize("kind", ("samples", "beams"))
def test_records_carry_shared_prompt(kind):
    prompt = "fix: "
    examples = [dict(input_ids_no_response=enc(prompt), ground_truth="up down"), dict(input_ids_no_response=enc(prompt), ground_truth="sit down")]
    lp = torch.tensor([-1.0, -0.5])

    def gen(prompts):
        if kind == "samples":
            c = lambda t: dict(tokens=enc(t), token_logprobs=lp, sum_logprob=-1.5, avg_logprob=-0.75, finish_reason="eos")
            return {"samples": [[c("up down"), c("up")], [c("sit down"), c("sit")]], "select": "avg_logprob", "logprobs": False}
        h = lambda t: dict(tokens=enc(prompt + t), token_logprobs=lp, sum_logprob=-1.5, finished=True, finish_reason="eos")
        return {"beams": [[h("up down"), h("up")], [h("sit down"), h("sit")]], "logprobs": False}

    recs = run_inference(gen, examples, byte_decode, batch_size=4)["predictions"]
    assert [r["inference"] for r in recs] == ["up down", "sit down"] and all("shared_prompt" not in r for r in recs)
    gen.shared_prompt = True
    recs = run_inference(gen, examples, byte_decode, batch_size=4)["predictions"]
    assert [r["inference"] for r in recs] == ["up down", "sit down"] and all(r["shared_prompt"] is True for r in recs)
    assert all(kind in r for r in recs)
    gen.shared_prompt = False
    assert all("shared_prompt" not in r for r in run_inference(gen, examples, byte_decode, batch_size=4)["predictions"])
