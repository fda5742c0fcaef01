"""Constrained decoding: per-utterance allowed-token masks (include/dualhyp_hip.h, "Token masks").

A mask is an int32 tensor [n, ceil(vocab / 32)]: bit i & 31 of word i >> 5 of row u is set when token i is allowed for sequence u.
The sampling kernels read it inside the captured decode steps (ops.sample(mask=...), generate_batch(token_mask=...)); everything
here is the host side — packing id lists, the allowed set of a prompt, and the checks made before anything is launched.  None of it
is hot: plain torch.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import torch


def mask_words(vocab: int) -> int:
    """32-bit words of one mask row."""
    return (int(vocab) + 31) // 32


def pack_mask(id_lists: Sequence[Iterable[int]], vocab: int, device="cpu") -> torch.Tensor:
    """int32 [len(id_lists), ceil(vocab / 32)]: row u has the bits of id_lists[u] set (an id may repeat).  An id outside [0, vocab)
    raises ValueError with its row."""
    vocab = int(vocab)
    if vocab <= 0:
        raise ValueError(f"pack_mask: vocab={vocab}")
    n, words = len(id_lists), mask_words(vocab)
    bits = torch.zeros((n, words * 32), dtype=torch.bool)
    for u, ids in enumerate(id_lists):
        t = ids.detach().reshape(-1).to("cpu", torch.int64) if isinstance(ids, torch.Tensor) else torch.tensor(sorted(set(int(i) for i in ids)), dtype=torch.int64)
        if t.numel() == 0:
            continue
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= vocab:
            raise ValueError(f"pack_mask: row {u} holds ids in [{lo}, {hi}], outside [0, {vocab})")
        bits[u, t] = True
    # word w = sum_b bit[32 w + b] << b, in int64 and wrapped to int32 (bit 31 is the sign)
    weights = torch.ones(32, dtype=torch.int64) << torch.arange(32, dtype=torch.int64)
    packed = (bits.view(n, words, 32).to(torch.int64) * weights).sum(-1)
    packed = torch.where(packed >= (1 << 31), packed - (1 << 32), packed).to(torch.int32)
    return packed.to(device).contiguous()


def all_ones(n: int, vocab: int, device="cpu") -> torch.Tensor:
    """The mask that allows everything: n rows of all-ones words."""
    return torch.full((int(n), mask_words(vocab)), -1, dtype=torch.int32, device=device)


def allowed_from_prompts(prompts: Sequence, eos_id: Optional[int], extra: Iterable[int] = ()) -> List[List[int]]:
    """For each prompt (a 1-D id tensor or a sequence of ints) the sorted ids that occur in it, plus eos_id (None: no EOS), plus
    `extra` — the set a generative error correction may copy from: the utterance's own hypotheses and its template."""
    common = set(int(i) for i in extra)
    if eos_id is not None:
        common.add(int(eos_id))
    out = []
    for p in prompts:
        ids = p.reshape(-1).tolist() if isinstance(p, torch.Tensor) else list(p)
        out.append(sorted(common.union(int(i) for i in ids)))
    return out


def check_mask(mask: torch.Tensor, n: int, vocab: int, need: int = 1, device=None) -> torch.Tensor:
    """`mask` as the kernels take it, or an error before anything is launched: an int32 contiguous [n, ceil(vocab / 32)] tensor (on
    `device` when given) whose every row allows at least `need` ids below vocab — 1 for the samplers, 2 W for beam search.  One
    read-back (the per-row counts).  ValueError names the first offending row; a wrong dtype is a TypeError."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"a token mask is an int32 tensor, not {type(mask).__name__}")
    if mask.dtype != torch.int32:
        raise TypeError(f"a token mask is {torch.int32}, got {mask.dtype}")
    words = mask_words(vocab)
    if mask.dim() != 2 or tuple(mask.shape) != (int(n), words):
        raise ValueError(f"a token mask for {n} sequences over {vocab} tokens is [{n}, {words}], got {tuple(mask.shape)}")
    if not mask.is_contiguous():
        raise ValueError("a token mask is contiguous")
    if device is not None and mask.device != torch.device(device):
        raise ValueError(f"the token mask lives on {mask.device}, the model on {torch.device(device)}")
    counts = allowed_counts(mask, vocab).tolist()                 # the one read-back
    for u, c in enumerate(counts):
        if c < need:
            raise ValueError(f"token mask row {u} allows {c} ids below vocab={vocab}, at least {need} are needed")
    return mask


def allowed_counts(mask: torch.Tensor, vocab: int) -> torch.Tensor:
    """int64 [n]: the ids below vocab that each row allows (the bits behind vocab are ignored, whatever they hold)."""
    return unpack_mask(mask, vocab).sum(-1)


def unpack_mask(mask: torch.Tensor, vocab: int) -> torch.Tensor:
    """bool [n, vocab]: True where the token is allowed."""
    shifts = torch.arange(32, dtype=torch.int32, device=mask.device)
    bits = (mask.unsqueeze(-1) >> shifts) & 1                     # arithmetic shift of int32: bit b lands at bit 0 all the same
    return bits.reshape(mask.size(0), -1)[:, :int(vocab)].bool()
