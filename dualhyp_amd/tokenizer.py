"""Tokenizers for the harnesses (inference/ger.py:194-201, finetune/ger.py:88-90).

The reference uses `AutoTokenizer.from_pretrained(checkpoint_dir, use_fast=True)` (HF `LlamaTokenizerFast`)
and only three things of it: `encode(str) -> ids` (BOS prepended), `decode(ids) -> str`, `eos_token` /
`eos_token_id`.  `load_tokenizer` returns that HF object when the checkpoint directory holds tokenizer files;
`ByteTokenizer` is a dependency-free stand-in with the same three members for runs without a checkpoint
(smoke tests, synthetic weights): BOS = 1, EOS = 2, one id per UTF-8 byte (byte + 3), vocabulary 259.
"""
from __future__ import annotations

from pathlib import Path
from typing import Iterable, List, Union


RELIABILITY_TOKENS = ("<<C>>", "<<M>>", "<<N>>")     # inference/relprompt.py:341


class ByteTokenizer:
    bos_token_id, eos_token_id, pad_token_id = 1, 2, 0
    eos_token = "</s>"
    vocab_size = 259

    def __init__(self) -> None:
        self.special = {self.eos_token: self.eos_token_id}

    def add_reliability_tokens(self, first_id: int) -> None:
        """<<C>>/<<M>>/<<N>> -> first_id.. (the rows `resize_token_embeddings(3)` appends to wte)."""
        for i, tok in enumerate(RELIABILITY_TOKENS):
            self.special[tok] = first_id + i

    def encode(self, text: str) -> List[int]:
        ids, rest = [self.bos_token_id], text
        while rest:                                   # special strings in the text become their ids, as with HF
            hits = [(rest.find(s), s) for s in self.special if rest.find(s) >= 0]
            if not hits:
                ids += [b + 3 for b in rest.encode("utf-8")]
                break
            cut, tok = min(hits)
            ids += [b + 3 for b in rest[:cut].encode("utf-8")] + [self.special[tok]]
            rest = rest[cut + len(tok):]
        return ids

    def chat_prompt_ids(self, user_text: str, system_text: str) -> List[int]:
        raise ValueError("--apply_chat_template needs the checkpoint's Hugging Face tokenizer and its chat template; "
                         "the byte-level stand-in tokenizer has none")

    def decode(self, ids: Iterable[int]) -> str:
        """Special tokens are skipped, like `decode(..., skip_special_tokens=True)`; the reference's
        `output[len(tokenizer.decode(encoded)):]` slicing then works on plain text."""
        return bytes(int(i) - 3 for i in ids if 3 <= int(i) < 259).decode("utf-8", errors="replace")


class _HFTokenizer:
    """The three members the harness needs over a Hugging Face tokenizer."""

    def __init__(self, tok) -> None:
        self.tok = tok
        if tok.pad_token is None:                     # inference/ger.py:200-201
            tok.pad_token = tok.eos_token
        self.eos_token, self.eos_token_id = tok.eos_token, tok.eos_token_id

    def add_reliability_tokens(self, first_id: int) -> None:
        self.tok.add_special_tokens({"additional_special_tokens": list(RELIABILITY_TOKENS)})
        got = self.tok.convert_tokens_to_ids(list(RELIABILITY_TOKENS))
        if got != [first_id, first_id + 1, first_id + 2]:
            raise ValueError(f"reliability tokens got ids {got}, the decoder's added wte rows are {first_id}..{first_id + 2}")

    def set_eos_token(self, token: str) -> None:
        """The reference's Phi override (inference/ger.py:196-198, finetune/ger.py:119-120): `eos_token` / `eos_token_id` follow."""
        self.tok.eos_token = token
        self.eos_token, self.eos_token_id = self.tok.eos_token, self.tok.eos_token_id

    def encode(self, text: str) -> List[int]:
        return list(self.tok.encode(text))

    def encode_plain(self, text: str) -> List[int]:
        """`tokenizer(text, add_special_tokens=False)["input_ids"]` (data/av_dataset.py:236)."""
        return list(self.tok(text, add_special_tokens=False)["input_ids"])

    def chat_prompt_ids(self, user_text: str, system_text: str) -> List[int]:
        """`apply_chat_template([system, user], tokenize=True, add_generation_prompt=True)` (data/av_dataset.py:226-235) as a list of
        ids: transformers 4.x returns the list itself, 5.x a BatchEncoding (its "input_ids"), either possibly batched."""
        if not getattr(self.tok, "chat_template", None):
            raise ValueError("--apply_chat_template: the checkpoint's tokenizer has no chat template")
        r = self.tok.apply_chat_template([{"role": "system", "content": system_text}, {"role": "user", "content": user_text}],
                                         tokenize=True, add_generation_prompt=True)
        if hasattr(r, "keys"):
            r = r["input_ids"]
        if hasattr(r, "tolist"):
            r = r.tolist()
        if len(r) and isinstance(r[0], (list, tuple)):
            assert len(r) == 1, "one conversation"
            r = r[0]
        return [int(i) for i in r]

    def decode(self, ids) -> str:
        return self.tok.decode([int(i) for i in ids])


PHI_EOS = "<|endoftext|>"


def apply_eos_override(tokenizer, config_name: str) -> None:
    """Both reference harnesses end Phi's targets and decoding at "<|endoftext|>" (`'phi-' in config.name.lower()`,
    inference/ger.py:196-198, finetune/ger.py:119-120).  The byte-level stand-in has no such token and keeps its EOS."""
    if "phi-" in config_name.lower() and hasattr(tokenizer, "set_eos_token"):
        tokenizer.set_eos_token(PHI_EOS)


def load_tokenizer(checkpoint_dir: Union[str, Path], kind: str = "auto"):
    """kind: 'hf' (tokenizer files in `checkpoint_dir`), 'byte', or 'auto' (hf when the files are there)."""
    d = Path(checkpoint_dir)
    has_files = any((d / n).is_file() for n in ("tokenizer.json", "tokenizer.model", "tokenizer_config.json"))
    if kind == "byte" or (kind == "auto" and not has_files):
        if kind == "auto":
            print(f"[dualhyp_amd] no tokenizer files in {str(d)!r}: using the byte-level stand-in tokenizer")
        return ByteTokenizer()
    if not has_files:
        raise FileNotFoundError(f"{str(d)!r} holds no tokenizer.json / tokenizer.model")
    from transformers import AutoTokenizer
    return _HFTokenizer(AutoTokenizer.from_pretrained(str(d), use_fast=True))
