"""fp64 reference of the token log-probability (include/dualhyp_hip.h, "Token log-probabilities"; dualhyp_amd/csrc/sampling.hip:
token_logprob) and the inputs of tests/test_hip_logprobs.py.  CPU only, and it does not import the library;
tests/test_logprob_reference.py checks it against closed forms.

    lp(t) = l[t] - m - log(sum_i exp(l[i] - m)),   m = max_i l[i]

of the raw bf16 row l: temperature 1, no top-k crop.  The bf16 values are taken as float64 (exact), the sum and the logarithm
are numpy float64.  -inf entries add 0; a -inf token gives -inf.

The gate on the kernel's fp32 result: |got - ref| <= GATE_ABS + GATE_REL * |ref|.  A thread's chain has at most
ceil(128256 / 8 / 1024) * 8 = 128 fp32 additions, the butterfly over the 1024 chains 10 more: the relative error of the sum is below
about 138 * 2**-24 = 8e-6 plus that of expf, which the logarithm turns into an absolute error; GATE_REL is two fp32 ulps of the
result (the subtraction l[t] - m is exact, the final one rounds once, logf a little more).
"""
from __future__ import annotations

import zlib
from typing import List, Tuple

import numpy as np
import torch

BF = torch.bfloat16
GATE_ABS = 2e-5
GATE_REL = 2.4e-7
VOCABS = (8, 320, 1000, 32000, 128256)
ROW_COUNTS = (1, 3, 37)
KINDS = ("normal0", "normal1", "normal2", "normal3", "dominant", "all_equal", "tenth_minus_inf", "magnitude_3e4", "token_argmax",
         "token_min", "token_minus_inf")


def logprob64(row: np.ndarray, token: int) -> float:
    """The definition above on one row of float64 values (bf16 values widened exactly)."""
    row = np.asarray(row, dtype=np.float64)
    if row[token] == -np.inf:
        return -np.inf
    m = row.max()
    with np.errstate(under="ignore"):
        s = np.exp(row[row != -np.inf] - m).sum()
    return float(row[token] - m - np.log(s))


def logprobs64(rows: torch.Tensor, ids) -> np.ndarray:
    """float64 [n] for bf16 rows [n, V] and n token ids."""
    assert rows.dtype == BF and rows.dim() == 2
    r = rows.cpu().to(torch.float64).numpy()
    return np.array([logprob64(r[i], int(t)) for i, t in enumerate(ids)], dtype=np.float64)


def gate(ref: np.ndarray) -> np.ndarray:
    """The largest accepted |got - ref| per entry (inf where ref is -inf: there got must be -inf itself)."""
    return GATE_ABS + GATE_REL * np.abs(ref)


def within_gate(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    inf = np.isneginf(ref)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= gate(ref)
    return np.where(inf, np.isneginf(got), ok & np.isfinite(got))


def make_row(kind: str, V: int, seed: int) -> Tuple[torch.Tensor, int]:
    """(bf16 row [V], token) of one kind; deterministic in (kind, V, seed)."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{kind}/{V}/{seed}".encode()))
    row = (torch.randn(V, generator=g, dtype=torch.float64) * 3).to(BF)
    token = int(torch.randint(0, V, (1,), generator=g))
    if kind == "dominant":            # one entry far above the rest, the token elsewhere (when there is an elsewhere)
        top = int(torch.randint(0, V, (1,), generator=g))
        row[top] = 60.0
        if V > 1 and token == top:
            token = (top + 1) % V
    elif kind == "all_equal":
        row[:] = 1.5
    elif kind == "tenth_minus_inf":   # 10 % of the entries, never the token
        drop = torch.randperm(V, generator=g)[: max(1, V // 10)]
        row[drop[drop != token]] = -float("inf")
    elif kind == "magnitude_3e4":
        row = (torch.randn(V, generator=g, dtype=torch.float64) * 3e4).to(BF)
    elif kind == "token_argmax":
        token = int(row.float().argmax())
    elif kind == "token_min":
        token = int(row.float().argmin())
    elif kind == "token_minus_inf":
        row[token] = -float("inf")
        if V == 1:
            raise ValueError("token_minus_inf needs a second entry")
    else:
        assert kind.startswith("normal"), kind
    return row, token


def case(V: int, n_rows: int) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
    """(bf16 rows [n_rows, V], int64 ids [n_rows], the kind of every row).  The kinds start at a place of their own per row count, so
    the 1- and 3-row cases are not the first kinds of the 37-row one."""
    shift = {1: 6, 3: 4}.get(n_rows, 0)
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(n_rows)]
    made = [make_row(k, V, seed=i) for i, k in enumerate(kinds)]
    return torch.stack([r for r, _ in made]), torch.tensor([t for _, t in made], dtype=torch.int64), kinds
