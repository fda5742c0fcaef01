"""Phi-3.5's prompt packing (no GPU): --apply_chat_template and the "<|endoftext|>" EOS override of both reference harnesses,
against ids and labels the reference's own get_prompt produced on a tiny tokenizer (tests/golden/make_golden_hs96.py)."""
import json

import pytest

from conftest import GOLDEN
from dualhyp_amd.data import HypothesesDataset, encode_example
from dualhyp_amd.tokenizer import ByteTokenizer, apply_eos_override, load_tokenizer

TOK_DIR = GOLDEN / "phi_chat_tokenizer"


def _record():
    return json.loads((GOLDEN / "phi_chat_packing.json").read_text())


def test_phi_eos_override():
    rec = _record()
    tok = load_tokenizer(TOK_DIR, "hf")
    assert tok.eos_token == "<|end|>"                         # the tokenizer's own EOS
    apply_eos_override(tok, "tiny-llama-1.1b-chat")
    assert tok.eos_token == "<|end|>"
    apply_eos_override(tok, "Phi-3.5-mini-instruct")
    assert (tok.eos_token, tok.eos_token_id) == (rec["eos_token"], rec["eos_token_id"]) == ("<|endoftext|>", tok.tok.convert_tokens_to_ids("<|endoftext|>"))


@pytest.mark.parametrize("fmt", ["GER", "DualHyp"])
def test_chat_template_packing_equals_the_reference(fmt):
    rec = _record()
    tok = load_tokenizer(TOK_DIR, "hf")
    apply_eos_override(tok, "Phi-3.5-mini-instruct")
    ds = HypothesesDataset(rec["items"], tok, prompts_format=fmt, apply_chat_template=True, seed=0)
    assert len(ds) == len(rec[fmt])
    for i, want in enumerate(rec[fmt]):
        ex = ds[i]
        assert ex["input_ids"].tolist() == want["input_ids"], f"{fmt} item {i}: input_ids"
        assert ex["labels"].tolist() == want["labels"], f"{fmt} item {i}: labels"
        assert ex["input_ids_no_response"].tolist() == want["input_ids_no_response"], f"{fmt} item {i}: prompt ids"
        assert ex["input"] == want["input"]
        # the answer is the caption without special tokens, then EOS; the prompt ends with the generation prompt
        assert ex["labels"].tolist()[-1] == tok.eos_token_id


def test_without_the_flag_packing_is_unchanged():
    rec = _record()
    tok = load_tokenizer(TOK_DIR, "hf")
    it = rec["items"][0]
    a = encode_example(tok, "prompt: ", it["Caption"])
    assert a["input_ids_no_response"].tolist() == tok.encode("prompt: ")
    assert a["input_ids"].tolist() == tok.encode("prompt: " + it["Caption"] + tok.eos_token)


def test_byte_tokenizer_refuses_the_chat_template():
    tok = ByteTokenizer()
    apply_eos_override(tok, "Phi-3.5-mini-instruct")        # no <|endoftext|> in the byte vocabulary: its EOS stays
    assert tok.eos_token == "</s>"
    with pytest.raises(ValueError, match="chat template"):
        encode_example(tok, "prompt", "caption", apply_chat_template=True)
