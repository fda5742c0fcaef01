"""Speculative decoding (generate_batch(..., speculate=D)): the proposer's rule, the argument checks, and a host replay of the
acceptance rule.

A verify step feeds a sequence's last token and D drafted tokens through the decode kernels at once and keeps the drafts the model's
own arg-max confirms (dh_engine_decode_spec).  The ids never depend on the drafts; the drafts only decide how many tokens a step
yields.  The correction of an ASR hypothesis is mostly a copy of spans of its prompt, so the default proposer looks the continuation
up in the sequence itself.

verify="draw" (the default is "argmax", everything above): a verify position draws as the plain sampled step would — the draw is a
function of (seed, tokens generated so far, sequence) and the row — and a draft is kept exactly when it equals the draw
(dh_engine_decode_spec_draw; include/dualhyp_hip.h, "Sampled verification"), so a sampled call, with any of the sampler's options, gets
the ids of its speculate=0 run in fewer steps.  replay() is the rule of both modes: it only compares drafts with the known ids.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

MAX_DRAFTS = 7            # S = D + 1 positions of a sequence share the 32 query columns of the verify attention's MFMA
VERIFY_COLUMNS = 32
VERIFY_MODES = ("argmax", "draw")
MAX_VERIFY_ROWS = 2048    # the streaming single-token step's row limit (engine.hip MAX_DECODE_ROWS)


def propose(tokens: Sequence[int], D: int, ngram_max: int = 3) -> List[int]:
    """The D tokens drafted behind `tokens` by prompt lookup.  This function is the specification of the device proposer
    (spec_prep_kernel):
      for n = ngram_max .. 1: take the last n tokens and find their latest EARLIER occurrence that at least one token follows;
      draft the up to D tokens behind it, padded to D with the last of them;
      no occurrence for any n: the last token, D times."""
    tokens = list(tokens)
    L = len(tokens)
    assert L >= 1 and D >= 1 and ngram_max >= 1
    for n in range(min(ngram_max, L - 1), 0, -1):
        tail = tokens[L - n:]
        for i in range(L - n - 1, -1, -1):           # i + n <= L - 1: tokens[i + n] exists
            if tokens[i:i + n] == tail:
                cont = tokens[i + n:i + n + D]
                return cont + [cont[-1]] * (D - len(cont))
    return [tokens[-1]] * D


def check_verify(verify, speculate) -> bool:
    """verify of a call: True for "draw", False for "argmax" (the default), or a ValueError.  Needs nothing but the arguments."""
    if not isinstance(verify, str) or verify not in VERIFY_MODES:
        raise ValueError(f'verify is "argmax" (a draft is kept when it is the arg-max) or "draw" (when it is the seeded draw), not {verify!r}')
    if verify == "draw" and not speculate:
        raise ValueError('verify="draw" goes with speculate > 0: it says how a verify step confirms its drafts, and this call has none')
    return verify == "draw"


def check_arguments(model, speculate: int, top_k: Optional[int], n_seq: int, verify: str = "argmax") -> int:
    """D of a generate_batch call, or a ValueError that says why this call cannot speculate.  Nothing here touches the GPU.
    verify="draw": any top_k speculates; the other refusals stand."""
    if isinstance(speculate, bool) or not isinstance(speculate, int) or not 0 <= speculate <= MAX_DRAFTS:
        raise ValueError(f"speculate is the number of drafts per step, 0..{MAX_DRAFTS}, not {speculate!r}")
    D = speculate
    if D == 0:
        return 0
    if top_k != 1 and not check_verify(verify, D):
        raise ValueError(f"speculate={D} needs top_k=1 (greedy): a draft is accepted when it IS the arg-max; top_k={top_k!r} samples")
    cfg = model.config
    q_per_kv = cfg.n_head // cfg.n_query_groups
    if (D + 1) * q_per_kv > VERIFY_COLUMNS:
        raise ValueError(f"speculate={D}: {D + 1} positions x {q_per_kv} heads per KV group exceed the {VERIFY_COLUMNS} query columns "
                         f"of the verify attention (at most speculate={VERIFY_COLUMNS // q_per_kv - 1} for this model)")
    if n_seq * (D + 1) > MAX_VERIFY_ROWS:
        raise ValueError(f"speculate={D}: {n_seq} sequences x {D + 1} positions exceed the {MAX_VERIFY_ROWS} rows of a streaming decode step")
    from .relprompt import GPT as RelGPT
    if getattr(model, "fp8", False):
        raise ValueError(f"speculate={D}: an fp8 model's decode step changes its GEMM kernel with the row count, so a verify step would "
                         "not reproduce the plain step's bits")
    if isinstance(model, RelGPT):
        raise ValueError(f"speculate={D}: the RelPrompt decoder's prompts carry spliced reliability embeddings")
    if model.cpu_rsqrt_vec_width != 0:
        raise ValueError(f"speculate={D}: cpu_rsqrt_vec_width != 0 flags rows by their index within a call; a verify step has other rows")
    return D


def replay(generated: Sequence[int], drafts_for, D: int, eos_id: Optional[int] = None) -> dict:
    """The acceptance rule on the host for one sequence whose generated tokens are known (`generated`, the EOS included when one was
    produced; generated[0] is the pick of the prefill, not of a verify step).  drafts_for(k) -> the D drafts proposed when k tokens
    have been generated.  Returns steps / drafted / accepted as dh_engine_decode_spec counts them."""
    k, n = 1, len(generated)
    steps = drafted = accepted = 0
    if eos_id is not None and generated[0] == eos_id:
        return dict(steps=0, drafted=0, accepted=0)
    while k < n:
        d = list(drafts_for(k))
        steps += 1
        drafted += D
        took = 0
        for j in range(D + 1):
            if j > 0 and d[j - 1] != generated[k - 1]:
                break
            k += 1                                    # pick_j == generated[k]
            took += 1
            if (eos_id is not None and generated[k - 1] == eos_id) or k >= n:
                break
        accepted += took - 1
    return dict(steps=steps, drafted=drafted, accepted=accepted)
