"""The host side of constrained decoding, without a GPU: the packing against numpy's, the allowed set of a prompt, every refusal of
check_mask and of the generation entry points (before anything is launched: on a CPU model), the --constrain flags, run_inference's
record mark, and the new entries of the C ABI in the header and the ctypes table."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import constrain_reference as CR
from dualhyp_amd import GPT, Config, beam_search_batch, generate, generate_batch, generate_stream, inference as I, ops
from dualhyp_amd import constrain as K

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("dh_sample_bf16_mask", "dh_sample_rows_bf16_mask", "dh_token_top_logprobs_bf16_mask", "dh_beam_select_bf16_mask",
               "dh_engine_set_token_mask")


# ---- pack_mask -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (8, 33, 1001, 32000))
def test_pack_mask_is_numpy_packbits(V):
    g = np.random.default_rng(V)
    allowed = g.random((5, V)) < 0.4
    allowed[0] = True
    allowed[1] = False
    allowed[2] = False
    allowed[2, [0, V - 1]] = True
    lists = [np.nonzero(r)[0].tolist() for r in allowed]
    lists[3] = lists[3] + lists[3][:3]                    # an id may repeat
    m = K.pack_mask(lists, V)
    assert m.dtype == torch.int32 and tuple(m.shape) == (5, (V + 31) // 32) and m.is_contiguous()
    by = np.packbits(np.pad(allowed, ((0, 0), (0, m.size(1) * 32 - V))), axis=1, bitorder="little")
    assert np.array_equal(m.numpy().view(np.uint32), np.ascontiguousarray(by).view("<u4"))
    assert torch.equal(m, CR.pack_bits(allowed))
    assert np.array_equal(K.unpack_mask(m, V).numpy(), allowed) and np.array_equal(CR.unpack_bits(m, V), allowed)
    assert K.allowed_counts(m, V).tolist() == allowed.sum(1).tolist()
    # tensors of ids are taken as they are
    assert torch.equal(K.pack_mask([torch.tensor(l, dtype=torch.int64) for l in lists], V), m)
    ones = K.all_ones(2, V)
    assert K.allowed_counts(ones, V).tolist() == [V, V] and tuple(ones.shape) == (2, m.size(1))


def test_pack_mask_refuses_ids_outside_the_vocabulary():
    with pytest.raises(ValueError, match="row 1"):
        K.pack_mask([[0], [3, 8]], 8)
    with pytest.raises(ValueError, match="row 0"):
        K.pack_mask([[-1]], 8)
    assert K.pack_mask([[], [7]], 8).tolist() == [[0], [128]]
    assert K.pack_mask([[31], [32]], 33).tolist() == [[-(1 << 31), 0], [0, 1]]      # bit 31 is the int32's sign


def test_allowed_from_prompts():
    ps = [torch.tensor([5, 9, 5, 200]), [3, 3, 1], torch.tensor([], dtype=torch.int64)]
    assert K.allowed_from_prompts(ps, 2) == [[2, 5, 9, 200], [1, 2, 3], [2]]
    assert K.allowed_from_prompts(ps, None) == [[5, 9, 200], [1, 3], []]
    assert K.allowed_from_prompts(ps, 9, extra=(7, 5, 7)) == [[5, 7, 9, 200], [1, 3, 5, 7, 9], [5, 7, 9]]
    m = K.pack_mask(K.allowed_from_prompts(ps, 2), 256)
    assert K.allowed_counts(m, 256).tolist() == [4, 3, 1]


# ---- check_mask ----------------------------------------------------------------------------------------------------------------------
def test_check_mask_refusals():
    V, n = 70, 3
    good = K.pack_mask([list(range(0, 9)) + [69], [5], list(range(V))], V)
    assert K.check_mask(good, n, V, 1) is good
    with pytest.raises(TypeError):
        K.check_mask(good.long(), n, V, 1)                        # wrong dtype
    with pytest.raises(TypeError):
        K.check_mask(good.tolist(), n, V, 1)
    for bad in (good[:2], good[:, :2], torch.cat([good, good], 1), good.view(-1)):      # wrong shape
        with pytest.raises(ValueError, match=r"\[3, 3\]"):
            K.check_mask(bad, n, V, 1)
    with pytest.raises(ValueError, match="contiguous"):
        K.check_mask(torch.cat([good, good], 1)[:, ::2], n, V, 1)
    empty = good.clone()
    empty[1] = 0
    with pytest.raises(ValueError, match="row 1 allows 0"):
        K.check_mask(empty, n, V, 1)                              # an empty row
    behind = good.clone()
    behind[1] = 0
    behind[1, 2] = -(1 << 6)                                      # bits 70 .. 95: nothing below vocab
    with pytest.raises(ValueError, match="row 1 allows 0"):
        K.check_mask(behind, n, V, 1)
    for W in (2, 4):                                              # beams need 2 W candidates per row
        with pytest.raises(ValueError, match=f"row 1 allows 1 ids below vocab=70, at least {2 * W}"):
            K.check_mask(good, n, V, 2 * W)
    assert K.check_mask(good[[0, 2]].contiguous(), 2, V, 8) is not None
    with pytest.raises(ValueError, match="row 0 allows 10"):
        K.check_mask(good[[0, 2]].contiguous(), 2, V, 11)
    with pytest.raises(ValueError, match="lives on"):
        K.check_mask(good, n, V, 1, device="cuda:0")              # a CPU tensor for a GPU model


def test_entry_points_refuse_a_bad_mask_before_anything_is_launched():
    """on a CPU model: a call that got as far as the engine would fail for another reason"""
    cfg = Config.from_name("parity-tiny")
    m = GPT(cfg)
    V = cfg.padded_vocab_size
    ps = [torch.tensor([1, 2, 3]), torch.tensor([4, 5])]
    for fn in (generate_batch, generate_stream):
        assert inspect.signature(fn).parameters["token_mask"].default is None
        with pytest.raises(ValueError, match="row 1 allows 0"):
            fn(m, ps, 4, top_k=1, token_mask=[[1, 2], []])
        with pytest.raises(ValueError, match="3 id lists for 2 prompts"):
            fn(m, ps, 4, top_k=1, token_mask=[[1], [2], [3]])
        with pytest.raises(ValueError, match=r"\[2, 8\]"):
            fn(m, ps, 4, top_k=1, token_mask=K.all_ones(3, V))
        with pytest.raises(TypeError):
            fn(m, ps, 4, top_k=1, token_mask=K.all_ones(2, V).long())
        with pytest.raises(ValueError, match="outside"):
            fn(m, ps, 4, top_k=1, token_mask=[[1], [V]])
    with pytest.raises(ValueError, match="row 0 allows 0"):
        generate(m, ps[0], 6, top_k=1, token_mask=[[]])
    with pytest.raises(ValueError, match="row 1 allows 3 ids below vocab=256, at least 4"):
        beam_search_batch(m, ps, 4, num_beams=2, token_mask=[[1, 2, 3, 4], [1, 2, 3]])
    assert inspect.signature(beam_search_batch).parameters["token_mask"].default is None
    for fn in (ops.sample, ops.sample_rows, ops.beam_select, ops.token_top_logprobs):
        assert inspect.signature(fn).parameters["mask"].default is None


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    """tests/test_capi.py would fail on a mismatch between the header and the table; this states which names the feature adds"""
    from dualhyp_amd import _lib
    head = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    for name in NEW_ENTRIES:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert decl, name
        assert decl.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert name in head.split("#define DH_ABI_VERSION")[0], f"{name} is missing from the list of what ABI 6 gained"
    # the _mask samplers: the _top argument lists plus the mask and its leading dimension
    for old in ("dh_sample_bf16", "dh_sample_rows_bf16"):
        assert _lib.SIGNATURES[old + "_mask"][1] == _lib.SIGNATURES[old + "_top"][1] + [_lib.P, _lib.I]
    assert "#define DH_ABI_VERSION 6" in head
    assert "Token masks" in head and "0xFF80" in head and "lowest ALLOWED index" in head


def test_c_entries_refuse_their_arguments_before_any_launch():
    """no GPU is touched: the checks come first"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)              # a non-null pointer that is never read
    # a null mask at a _mask entry
    assert lib.dh_sample_bf16_mask(one, 64, one, 4, one, one, 1, 1.0, 1, -1, 0, 0, None, None, 0, None, None, None, 2) != 0
    assert b"null mask" in lib.dh_last_error()
    assert lib.dh_sample_rows_bf16_mask(one, 64, one, 4, one, one, one, one, 1, 1, 4, 1.0, 1, -1, 0, None, None, 0, None, None, None, 2) != 0
    assert b"null mask" in lib.dh_last_error()
    assert lib.dh_token_top_logprobs_bf16_mask(one, 64, 2, one, one, 1, None, 2, 1, None) != 0 and b"null mask" in lib.dh_last_error()
    # mask_ld below ceil(vocab / 32)
    assert lib.dh_sample_bf16_mask(one, 65, one, 4, one, one, 1, 1.0, 1, -1, 0, 0, None, None, 0, None, None, one, 2) != 0
    assert b"mask_ld=2 is below the 3 words" in lib.dh_last_error()
    assert lib.dh_sample_rows_bf16_mask(one, 65, one, 4, one, one, one, one, 1, 1, 4, 1.0, 1, -1, 0, None, None, 0, None, None, one, 2) != 0
    assert b"mask_ld=2 is below the 3 words" in lib.dh_last_error()
    assert lib.dh_token_top_logprobs_bf16_mask(one, 65, 2, one, one, 1, one, 2, 1, None) != 0 and b"mask_ld=2" in lib.dh_last_error()
    assert lib.dh_token_top_logprobs_bf16_mask(one, 64, 2, one, one, 1, one, 2, 0, None) != 0 and b"bad shape" in lib.dh_last_error()
    assert lib.dh_beam_select_bf16_mask(one, 64, 1, 1, 2, 4, -1, 0, None, None, one, one, one, 2, None) != 0
    assert b"null beam state" in lib.dh_last_error()
    assert lib.dh_engine_set_token_mask(None, one, 2) != 0 and b"null engine" in lib.dh_last_error()


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
def test_constrain_flags_parse(tmp_path):
    base = ["--test_path", "x.json", "--random_init"]
    a = I.parse_args(base)
    assert a.constrain == "off" and a.constrain_extra is None
    a = I.parse_args(base + ["--constrain", "prompt"])
    assert a.constrain == "prompt" and a.constrain_extra is None
    extra = tmp_path / "extra.txt"
    extra.write_text("# punctuation\n13\n\n 46 \n259  # a comment\n")
    a = I.parse_args(base + ["--constrain", "prompt", "--constrain_extra", str(extra)])
    assert a.constrain_extra == str(extra) and I.read_token_ids(a.constrain_extra) == [13, 46, 259]
    # both schedules, beams, and the flags that expose the distribution
    for more in (["--schedule", "continuous"], ["--num_beams", "3"], ["--speculate", "3"], ["--share_prefix", "auto"],
                 ["--top_logprobs", "4"], ["--quantize", "fp8", "--kv_cache", "fp8"]):
        assert I.parse_args(base + ["--constrain", "prompt"] + more).constrain == "prompt"
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--constrain", "hypotheses"])
    with pytest.raises(SystemExit):
        I.parse_args(base + ["--constrain_extra", str(extra)])               # goes with --constrain prompt
    bad = tmp_path / "bad.txt"
    bad.write_text("12\nx7\n")
    with pytest.raises(ValueError, match="bad.txt:2"):
        I.read_token_ids(bad)


def test_run_inference_marks_constrained_records():
    from dualhyp_amd.tokenizer import ByteTokenizer
    tok = ByteTokenizer()
    enc = lambda s: torch.tensor(tok.encode(s), dtype=torch.int64)
    exs = [{"input_ids_no_response": enc("fix: teh cat\nanswer: "), "ground_truth": "the cat"}]

    def gen(prompts):
        return [torch.cat([p, enc("the cat")]) for p in prompts]

    plain = I.run_inference(gen, exs, tok.decode, batch_size=2)
    assert "constrained" not in plain["predictions"][0]
    gen.constrained = True
    marked = I.run_inference(gen, exs, tok.decode, batch_size=2)
    assert marked["predictions"][0]["constrained"] is True
    assert {k: v for k, v in marked["predictions"][0].items() if k != "constrained"} == plain["predictions"][0]
