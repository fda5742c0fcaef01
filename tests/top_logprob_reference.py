"""Reference of the token alternatives (include/dualhyp_hip.h, "Token alternatives"; dualhyp_amd/csrc/sampling.hip: row_top) and the
inputs of tests/test_hip_top_logprobs.py.  CPU only, and it does not import the library; tests/test_top_logprobs_host.py checks it
against closed forms.

The ids of a raw bf16 row: alternative j is the index at rank j of a stable sort by (-float(value), index).  The values are compared
as floating-point numbers, so -0 == +0 (two zeros tie, the lower index first) and -inf entries rank last in index order.  The
VALUES have no reference of their own here: lp_j is, by definition, the bits dh_token_logprobs_bf16 gives for (row, id_j), and that
op is gated against fp64 by tests/test_hip_logprobs.py.
"""
from __future__ import annotations

import zlib
from typing import List, Tuple

import numpy as np
import torch

import logprob_reference as R

BF = torch.bfloat16
MAX_TOP = 8
VOCABS = (8, 320, 1000, 8200, 32064, 128256)   # 1000: the scalar loop; 8200: one thread gets a second 8-element chunk
KS = (1, 2, 5, 8)
ROW_COUNTS = (1, 3, 37)
TIE_KINDS = ("constant", "zeros_alternating_sign", "equal_maxima", "quarter_steps", "mostly_minus_inf")
KINDS = R.KINDS + TIE_KINDS
MAXIMA_AT = (0, 7, 8, 8191, 8192, -1)           # -1: vocab - 1


def top_ids_row(values, k: int) -> List[int]:
    """The definition in plain Python: a stable sort of (-float(value), index).  Python's float compare makes -0 == +0."""
    vals = [float(v) for v in values]
    return sorted(range(len(vals)), key=lambda i: (-vals[i], i))[:k]


def top_ids(rows: torch.Tensor, k: int) -> torch.Tensor:
    """int32 [n, k] for bf16 rows [n, V]: numpy's stable sort of the negated float64 values — ties stay in index order, which is the
    sort above (tests/test_top_logprobs_host.py holds the two against each other)."""
    assert rows.dtype == BF and rows.dim() == 2 and 1 <= k <= min(MAX_TOP, rows.size(1))
    r = rows.cpu().to(torch.float64).numpy()
    assert not np.isnan(r).any(), "NaN rows are outside the definition"
    return torch.from_numpy(np.argsort(-r, axis=1, kind="stable")[:, :k].astype(np.int32))


def make_row(kind: str, V: int, seed: int, k: int) -> torch.Tensor:
    """A bf16 row [V] of one kind; deterministic in (kind, V, seed, k).  The kinds of logprob_reference.make_row, and the tie kinds."""
    if kind in R.KINDS:
        return R.make_row(kind, V, seed)[0]
    g = torch.Generator().manual_seed(zlib.crc32(f"top/{kind}/{V}/{seed}/{k}".encode()))
    fill = (torch.randn(V, generator=g, dtype=torch.float64) * 3).to(BF)
    if kind == "constant":                       # ids 0 .. k-1
        return torch.full((V,), -2.5, dtype=BF)
    if kind == "zeros_alternating_sign":         # -0 at the even indices: still ids 0 .. k-1
        row = torch.zeros(V, dtype=BF)
        row[0::2] = -0.0
        return row
    if kind == "equal_maxima":                   # equal maxima at every chunk and block edge of MAXIMA_AT the row has, then anywhere
        at = sorted({i % V for i in MAXIMA_AT if -V <= i < V})           # until there are k + 3 of them (or V)
        n = max(min(k + 3, V), len(at))
        for i in torch.randperm(V, generator=g).tolist():
            if len(at) >= n:
                break
            if i not in at:
                at.append(i)
        row = fill.clamp(max=8.0)
        row[torch.tensor(at)] = 17.0
        return row
    if kind == "quarter_steps":                  # massive ties: a few dozen distinct values over the whole row
        return (torch.round(fill.double() * 4) / 4).to(BF)
    if kind == "mostly_minus_inf":               # max(k - 2, 1) finite entries: the last alternatives are -inf, in index order
        row = torch.full((V,), -float("inf"), dtype=BF)
        keep = torch.randperm(V, generator=g)[: max(k - 2, 1)]
        row[keep] = fill[keep]
        return row
    raise ValueError(kind)


def case(V: int, n_rows: int, k: int) -> Tuple[torch.Tensor, List[str]]:
    """(bf16 rows [n_rows, V], the kind of every row).  The kinds start at a place of their own per row count, so that the 1- and
    3-row cases are tie kinds and the 37-row case holds every kind at least twice."""
    shift = {1: len(R.KINDS) + 2, 3: len(R.KINDS)}.get(n_rows, 0)
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(n_rows)]
    return torch.stack([make_row(kd, V, seed=i, k=k) for i, kd in enumerate(kinds)]), kinds
