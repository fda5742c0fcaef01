"""Host model of the token masks (include/dualhyp_hip.h, "Token masks") and the masks of tests/test_hip_constrain.py.  CPU only; it
imports neither the library nor dualhyp_amd.constrain, so the packing under test is held against numpy's.

The model is one sentence of the definition: a disallowed column takes part in the pick as if its logit were bf16 -inf.  So the
reference of a masked pick is the UNMASKED entry (pinned by test_hip_sampling.py) on substitute(logits, mask).
"""
from __future__ import annotations

import zlib
from typing import Dict, List

import numpy as np
import torch

BF = torch.bfloat16
NEG_INF_BITS = 0xFF80


def words(vocab: int) -> int:
    return (vocab + 31) // 32


def pack_bits(allowed: np.ndarray) -> torch.Tensor:
    """bool [n, vocab] -> int32 [n, ceil(vocab / 32)]: numpy.packbits, little bit order, the bytes viewed as little-endian words."""
    allowed = np.asarray(allowed, dtype=bool)
    n, vocab = allowed.shape
    padded = np.zeros((n, words(vocab) * 32), dtype=bool)
    padded[:, :vocab] = allowed
    by = np.packbits(padded, axis=1, bitorder="little")
    return torch.from_numpy(np.ascontiguousarray(by).view("<u4").astype(np.uint32).view(np.int32).copy())


def unpack_bits(mask: torch.Tensor, vocab: int) -> np.ndarray:
    """int32 [n, >= words] (any device) -> bool [n, vocab]; the bits behind vocab are dropped."""
    m = np.ascontiguousarray(mask.detach().cpu().numpy()[:, :words(vocab)]).view(np.uint32)
    by = m.astype("<u4").view(np.uint8)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :vocab].astype(bool)


def substitute(logits: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """A copy of the bf16 rows [n, vocab] with 0xFF80 (bf16 -inf) in every column that mask row n does not allow."""
    assert logits.dtype == BF and logits.dim() == 2 and mask.size(0) == logits.size(0)
    allowed = torch.from_numpy(unpack_bits(mask, logits.size(1))).to(logits.device)
    out = logits.clone()
    out.view(torch.int16)[~allowed] = NEG_INF_BITS - 0x10000
    return out


MASK_KINDS = ("all_ones", "random_half", "alternating", "single_0", "single_31", "single_32", "single_last", "last_partial_word",
              "argmax_forbidden", "garbage_beyond_vocab")


def make_masks(kind: str, logits_cpu: torch.Tensor) -> torch.Tensor:
    """int32 [n, words] of one kind for bf16 rows [n, vocab] on the CPU; deterministic in (kind, shape)."""
    n, V = logits_cpu.shape
    g = np.random.default_rng(zlib.crc32(f"mask/{kind}/{n}/{V}".encode()))
    a = np.zeros((n, V), dtype=bool)
    if kind in ("all_ones", "garbage_beyond_vocab"):
        a[:] = True
    elif kind == "random_half":
        a = g.random((n, V)) < 0.5
        a[np.arange(n), g.integers(0, V, n)] = True            # never an empty row
    elif kind == "alternating":
        a[:, 0::2] = True
        a[1::2] = ~a[1::2]                                      # odd rows allow the odd ids
    elif kind.startswith("single_"):
        at = {"0": 0, "31": min(31, V - 1), "32": min(32, V - 1), "last": V - 1}[kind.split("_")[1]]
        a[:, at] = True
    elif kind == "last_partial_word":                           # the ids of the row's last word only (a whole word when 32 | V)
        a[:, (V - 1) // 32 * 32:] = True
    elif kind == "argmax_forbidden":                            # everything but the raw row's maxima
        f = logits_cpu.double().numpy()
        a = f < f.max(axis=1, keepdims=True)
        a[~a.any(axis=1), 0] = True                             # a constant row: allow id 0 rather than nothing
    else:
        raise ValueError(kind)
    m = pack_bits(a)
    if kind == "garbage_beyond_vocab" and V % 32:
        m[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)      # every bit at or behind vocab set
    if kind in ("single_0", "random_half") and V % 32:
        m[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)      # garbage there too: it must never be picked
    return m


def first_allowed(ids: List[int], allowed_row: np.ndarray) -> int:
    """The first id of `ids` that the row allows, -1 when none is."""
    for i in ids:
        if allowed_row[i]:
            return int(i)
    return -1


def disjoint_masks(n: int, vocab: int, eos: int) -> torch.Tensor:
    """Sequence u allows the ids with id % n == u, plus the EOS: any row / sequence mix-up produces a foreign id."""
    ids = np.arange(vocab)
    a = (ids[None, :] % n) == np.arange(n)[:, None]
    a[:, eos] = True
    return pack_bits(a)


def random_half_masks(n: int, vocab: int, seed: int, always=()) -> torch.Tensor:
    g = np.random.default_rng(seed)
    a = g.random((n, vocab)) < 0.5
    for i in always:
        a[:, i] = True
    return pack_bits(a)
