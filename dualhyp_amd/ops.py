"""Tensor-level wrappers over the C ABI (include/dualhyp_hip.h).

Every function takes CUDA (ROCm) bf16/int tensors, launches on torch's current stream and
returns torch tensors.  They are thin: shape checks + pointer passing.  No fallbacks — a CPU
tensor or a missing library raises.
"""
from __future__ import annotations

import os
from typing import Sequence, Optional, Tuple

import torch

from . import _lib
from ._lib import check

EPI_PLAIN, EPI_LORA, EPI_SWIGLU, EPI_ADAPTER = 0, 1, 2, 3


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype=torch.bfloat16, name="tensor") -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.DualHypHipError(f"{name} must live on the GPU: the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


class _Keep(list):
    """Pointer of a validated (contiguous, right dtype, on the GPU) view of `t`, with the view kept alive until the
    wrapper returns: `.contiguous()` may allocate a temporary, and a temporary freed before the launch is enqueued
    could be handed to the next argument by the caching allocator (two kernel arguments would then alias)."""

    def __call__(self, t: Optional[torch.Tensor], dtype=torch.bfloat16, name: str = "tensor"):
        if t is None:
            return None
        t = _dev(t, dtype, name)
        self.append(t)
        return t.data_ptr()


def _out(out: Optional[torch.Tensor], shape, dtype, device, name: str = "out") -> torch.Tensor:
    """The caller's output buffer (checked: on the GPU, contiguous, right dtype and shape), or a fresh one."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    shape = tuple(int(d) for d in shape)
    if not out.is_cuda or out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != shape:
        raise ValueError(f"{name} must be a contiguous {dtype} GPU tensor of shape {shape}, got {tuple(out.shape)} {out.dtype}")
    return out


def embed(ids: torch.Tensor, wte: torch.Tensor) -> torch.Tensor:
    ids = _dev(ids.reshape(-1), torch.int64, "ids")
    wte = _dev(wte, name="wte")
    out = torch.empty((ids.numel(), wte.size(1)), dtype=torch.bfloat16, device=wte.device)
    check(_lib.load().dh_embed_bf16(_p(ids), _p(wte), _p(out), ids.numel(), wte.size(1), wte.size(0), _stream()))
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, resid: Optional[torch.Tensor] = None,
            return_sum: bool = False, row_tail: Optional[torch.Tensor] = None):
    x = _dev(x, name="x")
    w = _dev(w, name="weight")
    d = x.size(-1)
    rows = x.numel() // d
    out = torch.empty_like(x)
    s = torch.empty_like(x) if (resid is not None and return_sum) else None
    if resid is not None:
        resid = _dev(resid, name="resid")
    if row_tail is not None:
        row_tail = _dev(row_tail.reshape(-1), torch.uint8, "row_tail")
        assert row_tail.numel() == rows
    check(_lib.load().dh_rmsnorm_bf16(_p(x), _p(resid), _p(w), _p(out), _p(s), rows, d, float(eps), _p(row_tail),
                                      _stream()))
    return (out, s) if return_sum else out


def linear(x: torch.Tensor, w: torch.Tensor, *, epilogue: int = EPI_PLAIN, w2: Optional[torch.Tensor] = None,
           xa: Optional[torch.Tensor] = None, lora_b: Optional[torch.Tensor] = None, lora_scale: float = 1.0,
           splits: Optional[Tuple[int, int]] = None, scale: Optional[torch.Tensor] = None,
           bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epilogue(x @ w.T); see dh_linear_bf16 in include/dualhyp_hip.h."""
    x = _dev(x, name="x")
    w = _dev(w, name="w")
    K = x.size(-1)
    M = x.numel() // K
    N = w.size(0)
    assert w.size(1) == K, f"weight is {tuple(w.shape)}, input feature size {K}"
    y = _out(out, (*x.shape[:-1], N), torch.bfloat16, x.device)
    s0, s1 = splits if splits is not None else (N, N)
    xa_ld = 0
    if xa is not None:
        xa = _dev(xa, name="xa")
        xa_ld = xa.size(-1)
    for t, nm in ((w2, "w2"), (lora_b, "lora_b"), (scale, "scale"), (bias, "bias"), (resid, "resid")):
        if t is not None:
            _dev(t, name=nm)
            assert t.is_contiguous(), f"{nm} must be contiguous"
    check(_lib.load().dh_linear_bf16(_p(x), _p(w), _p(y), M, N, K, epilogue, _p(w2), _p(xa), xa_ld, _p(lora_b),
                                     float(lora_scale), s0, s1, _p(scale), _p(bias), _p(resid), _stream()))
    return y


def qkv_rope_cache(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, tok_slot: torch.Tensor,
                   tok_pos: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, n_head: int,
                   n_groups: int, k_out: Optional[torch.Tensor] = None, v_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> rotated q [n_tok, n_head, hs]; appends k / v^T into the caches in place (and, for training,
    plain copies into k_out / v_out [n_tok, n_groups, hs])."""
    k = _Keep()
    qkv = _dev(qkv, name="qkv")
    hs = k_cache.size(-1)
    s_max = k_cache.size(-2)
    n_tok = qkv.numel() // ((n_head + 2 * n_groups) * hs)
    q = torch.empty((n_tok, n_head, hs), dtype=torch.bfloat16, device=qkv.device)
    check(_lib.load().dh_qkv_rope_cache_bf16(_p(qkv), k(cos), k(sin), k(tok_slot, torch.int32),
                                             k(tok_pos, torch.int32), _p(q), _p(k_cache), _p(vT_cache), _p(k_out),
                                             _p(v_out), n_tok, n_head, n_groups, hs, s_max, _stream()))
    return q


def linear_qkv_rope_cache(x: torch.Tensor, w: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, tok_slot: torch.Tensor,
                          tok_pos: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, n_head: int, n_groups: int,
                          xa: Optional[torch.Tensor] = None, lora_b: Optional[torch.Tensor] = None,
                          lora_scale: float = 1.0) -> torch.Tensor:
    """QKV projection (+LoRA) with rope and KV-cache append in the GEMM epilogue -> rotated q [M, n_head, hs];
    dh_linear_qkv_rope_cache_bf16 (large M only)."""
    k = _Keep()
    x = _dev(x, name="x")
    K = x.size(-1)
    M = x.numel() // K
    hs, s_max = k_cache.size(-1), k_cache.size(-2)
    q = torch.empty((M, n_head, hs), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().dh_linear_qkv_rope_cache_bf16(_p(x), k(w, name="w"), M, K, k(xa, name="xa"), 0 if xa is None else xa.size(-1),
                                                    k(lora_b, name="lora_b"), float(lora_scale), k(cos), k(sin),
                                                    k(tok_slot, torch.int32), k(tok_pos, torch.int32), _p(q), _p(k_cache),
                                                    _p(vT_cache), n_head, n_groups, hs, s_max, _stream()))
    return q


def linear_lora(x: torch.Tensor, w: torch.Tensor, lora_a: torch.Tensor, lora_b: torch.Tensor, *, lora_scale: float = 1.0,
                splits: Optional[Tuple[int, int]] = None, resid: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, xa_work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x W^T + scale * bf16(x A^T) B^T (+ resid) with the down-projection computed by the library (inside the GEMM's K loop on the
    4-wave 256-tile kernel, else one more launch); lora_a [16 * nseg, K], lora_b [N, 16]; dh_linear_lora_bf16.  `out` [.., N] and
    `xa_work` [M, 16 * nseg] (the down-projection's work buffer): caller-owned contiguous bf16 buffers instead of fresh ones."""
    x, w, lora_a, lora_b = _dev(x, name="x"), _dev(w, name="w"), _dev(lora_a, name="lora_a"), _dev(lora_b, name="lora_b")
    K = x.size(-1)
    M, N = x.numel() // K, w.size(0)
    s0, s1 = splits if splits is not None else (N, N)
    nseg = 1 + (s0 < N) + (s1 < N)
    assert lora_a.shape == (16 * nseg, K) and lora_b.shape == (N, 16), (lora_a.shape, lora_b.shape)
    if resid is not None:
        _dev(resid, name="resid")
    y = _out(out, (*x.shape[:-1], N), torch.bfloat16, x.device)
    work = _out(xa_work, (M, 16 * nseg), torch.bfloat16, x.device, "xa_work")
    check(_lib.load().dh_linear_lora_bf16(_p(x), _p(w), _p(y), M, N, K, _p(lora_a), _p(lora_b), float(lora_scale), s0, s1, _p(resid),
                                          _p(work), _stream()))
    return y


def linear_qkv_lora_rope_cache(x: torch.Tensor, w: torch.Tensor, lora_a: torch.Tensor, lora_b: torch.Tensor, cos: torch.Tensor,
                               sin: torch.Tensor, tok_slot: torch.Tensor, tok_pos: torch.Tensor, k_cache: torch.Tensor,
                               vT_cache: torch.Tensor, n_head: int, n_groups: int, *, lora_scale: float = 1.0) -> torch.Tensor:
    """linear_qkv_rope_cache with the LoRA down-projection computed by the library (dh_linear_qkv_lora_rope_cache_bf16)."""
    k = _Keep()
    M, K = x.shape
    hs = k_cache.size(-1)
    q = torch.empty((M, n_head, hs), dtype=torch.bfloat16, device=x.device)
    work = torch.empty((M, 48), dtype=torch.bfloat16, device=x.device)
    i32 = torch.int32
    check(_lib.load().dh_linear_qkv_lora_rope_cache_bf16(k(x), k(w), M, K, k(lora_a), k(lora_b), float(lora_scale), k(cos), k(sin),
                                                         k(tok_slot, i32), k(tok_pos, i32), _p(q), _p(k_cache), _p(vT_cache), n_head,
                                                         n_groups, hs, k_cache.size(2), _p(work), _stream()))
    return q


def attn_prefill(q: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, seq_slot: torch.Tensor,
                 q_start: torch.Tensor, q_len: torch.Tensor, kv_pos0: torch.Tensor, max_q_len: int,
                 lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    k = _Keep()
    n_tok, n_head, hs = q.shape
    n_groups, s_max = k_cache.size(1), k_cache.size(2)
    y = torch.empty((n_tok, n_head * hs), dtype=torch.bfloat16, device=q.device)
    i32 = torch.int32
    check(_lib.load().dh_attn_prefill_bf16(k(q), _p(k_cache), _p(vT_cache), k(seq_slot, i32),
                                           k(q_start, i32), k(q_len, i32), k(kv_pos0, i32), _p(y), _p(lse),
                                           seq_slot.numel(), int(max_q_len), n_head, n_groups, hs, s_max, _stream()))
    return y


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, seq_slot: torch.Tensor,
                kv_len: torch.Tensor) -> torch.Tensor:
    k = _Keep()
    n_seq, n_head, hs = q.shape
    n_groups, s_max = k_cache.size(1), k_cache.size(2)
    lib = _lib.load()
    work = torch.empty(lib.dh_attn_decode_work_bytes(n_seq, n_head, hs, s_max), dtype=torch.uint8, device=q.device)
    y = torch.empty((n_seq, n_head * hs), dtype=torch.bfloat16, device=q.device)
    i32 = torch.int32
    check(lib.dh_attn_decode_bf16(k(q), _p(k_cache), _p(vT_cache), k(seq_slot, i32),
                                  k(kv_len, i32), _p(y), _p(work), n_seq, n_head, n_groups, hs, s_max, _stream()))
    return y


def _logprobs_buffer(logprobs: Optional[torch.Tensor], tokens: torch.Tensor) -> Optional[torch.Tensor]:
    """The fp32 buffer beside `tokens` that the sampling kernels write in place: refused unless it is exactly that."""
    if logprobs is None:
        return None
    if not logprobs.is_cuda:
        raise _lib.DualHypHipError("logprobs must live on the GPU: the HIP path has no CPU fallback")
    if logprobs.dtype != torch.float32:
        raise TypeError(f"logprobs must be {torch.float32}, got {logprobs.dtype}")
    if tuple(logprobs.shape) != tuple(tokens.shape) or not logprobs.is_contiguous():
        raise ValueError(f"logprobs must be a contiguous {tuple(tokens.shape)} tensor like tokens, got {tuple(logprobs.shape)}")
    return logprobs


MAX_TOP_LOGPROBS = 8       # the header's cap on the alternatives per token


def check_top_logprobs(k, vocab: Optional[int] = None, *, lowest: int = 0) -> int:
    """k as an int in lowest .. min(MAX_TOP_LOGPROBS, vocab); a bool, a float or a value outside raises."""
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"top_logprobs is an int, not {k!r}")
    hi = MAX_TOP_LOGPROBS if vocab is None else min(MAX_TOP_LOGPROBS, int(vocab))
    if not lowest <= k <= hi:
        raise ValueError(f"top_logprobs={k} is outside {lowest} .. {hi}")
    return k


def _top_buffers(top: Optional[Tuple[torch.Tensor, torch.Tensor]], logprobs: Optional[torch.Tensor], tokens: torch.Tensor, vocab: int):
    """(K, ids, lp) of the alternatives' buffers beside `tokens` that the sampling kernels write in place; (0, None, None) without."""
    if top is None:
        return 0, None, None
    if logprobs is None:
        raise ValueError("top_logprobs buffers go with a logprobs buffer")
    ids, lp = top
    if not (ids.is_cuda and lp.is_cuda):
        raise _lib.DualHypHipError("top_logprobs buffers must live on the GPU: the HIP path has no CPU fallback")
    if ids.dtype != torch.int32 or lp.dtype != torch.float32:
        raise TypeError(f"top_logprobs buffers are ({torch.int32}, {torch.float32}), got ({ids.dtype}, {lp.dtype})")
    if ids.dim() != 3 or tuple(ids.shape) != tuple(lp.shape) or tuple(ids.shape[:2]) != tuple(tokens.shape) \
            or not (ids.is_contiguous() and lp.is_contiguous()):
        raise ValueError(f"top_logprobs buffers are contiguous {tuple(tokens.shape)} + (K,) tensors, got {tuple(ids.shape)} and {tuple(lp.shape)}")
    return check_top_logprobs(int(ids.size(2)), vocab, lowest=1), ids, lp


def _mask_arg(mask: Optional[torch.Tensor], n_rows: int, vocab: int, device):
    """(pointer, mask_ld) of a token mask for n_rows sequences (include/dualhyp_hip.h, "Token masks"): int32 [n_rows, >= ceil(vocab /
    32) words] on the logits' device, unit stride within a row, any row stride that holds the words; (None, 0) without one."""
    if mask is None:
        return None, 0
    if not mask.is_cuda:
        raise _lib.DualHypHipError("mask must live on the GPU: the HIP path has no CPU fallback")
    if mask.dtype != torch.int32:
        raise TypeError(f"mask must be {torch.int32}, got {mask.dtype}")
    words = (vocab + 31) // 32
    if mask.dim() != 2 or mask.size(0) != n_rows or mask.size(1) < words:
        raise ValueError(f"mask must be [{n_rows}, >= {words}] for {n_rows} sequences over {vocab} tokens, got {tuple(mask.shape)}")
    if mask.device != device:
        raise ValueError(f"the mask lives on {mask.device}, the logits on {device}")
    ld = int(mask.stride(0)) if n_rows > 1 else max(int(mask.stride(0)), int(mask.size(1)))
    if mask.stride(1) != 1 or ld < words:
        raise ValueError(f"mask rows must have unit stride and a row stride of at least {words} words, got strides {tuple(mask.stride())}")
    return mask.data_ptr(), ld


def _ngram_arg(no_repeat_ngram: int, start: Optional[torch.Tensor], n_seq: int, vocab: int, device, keep, start_optional: bool = False):
    """(ngram, start pointer) of a sampler call (include/dualhyp_hip.h, "No-repeat n-grams"): n in 0 .. 8, and with n > 0 the int32
    [n_seq] prompt lengths on the logits' device (start_optional: None is the row-list sampler's limit - max_new_tokens)."""
    from .ngram import check_ngram
    n = check_ngram(no_repeat_ngram, vocab)
    if n == 0:
        if start is not None:
            raise ValueError("start goes with no_repeat_ngram > 0")
        return 0, None
    if start is None:
        if not start_optional:
            raise ValueError(f"no_repeat_ngram={n} needs start, the int32 [{n_seq}] prompt lengths: the history it bans from begins there")
        return n, None
    if not start.is_cuda:
        raise _lib.DualHypHipError("start must live on the GPU: the HIP path has no CPU fallback")
    if start.dtype != torch.int32 or start.numel() != n_seq:
        raise ValueError(f"start must be {torch.int32} [{n_seq}], got {start.dtype} {tuple(start.shape)}")
    if start.device != device:
        raise ValueError(f"start lives on {start.device}, the logits on {device}")
    return n, keep(start, torch.int32)


def _stop_arg(stop, vocab: int, device):
    """The dh_stop_spec pointer of a sampler call's `stop` (a dualhyp_amd.stop.StopSpec on the logits' device, "Stop conditions" of
    the header), or None when it is off."""
    if stop is None or not stop:
        return None
    from .stop import StopSpec
    if not isinstance(stop, StopSpec):
        raise TypeError(f"stop is a compiled specification (dualhyp_amd.stop.compile_stop), not {stop!r}")
    if stop.vocab != vocab:
        raise ValueError(f"the stop specification was compiled for {stop.vocab} tokens, the logits have {vocab}")
    if stop.device is None:
        raise _lib.DualHypHipError("the stop specification must live on the GPU: the HIP path has no CPU fallback")
    if stop.device != device:
        raise ValueError(f"the stop specification lives on {stop.device}, the logits on {device}")
    import ctypes
    return ctypes.byref(stop.c_struct())


def _start_arg(start: Optional[torch.Tensor], n_seq: int, device, keep):
    """The pointer of `start`, the int32 [n_seq] prompt lengths on the logits' device, beside a stop specification."""
    if start is None:
        return None
    if not start.is_cuda:
        raise _lib.DualHypHipError("start must live on the GPU: the HIP path has no CPU fallback")
    if start.dtype != torch.int32 or start.numel() != n_seq:
        raise ValueError(f"start must be {torch.int32} [{n_seq}], got {start.dtype} {tuple(start.shape)}")
    if start.device != device:
        raise ValueError(f"start lives on {start.device}, the logits on {device}")
    return keep(start, torch.int32)


def _penalty_arg(repetition_penalty, frequency_penalty, presence_penalty, start: Optional[torch.Tensor], tok_ld: int, vocab: int, keep):
    """The dh_penalty_args pointer of a sampler call ("Penalties" of the header), or None when all three are off.  On, the call needs
    start, and a token buffer and a vocab the sampler's LDS tables hold."""
    from .penalty import check_history, check_penalties, penalties_on
    r, f, p = check_penalties(repetition_penalty, frequency_penalty, presence_penalty)
    if not penalties_on(r, f, p):
        return None
    if start is None:
        raise ValueError("penalties need start, the int32 prompt lengths: the history they count begins there")
    check_history(tok_ld, vocab)
    import ctypes
    args = _lib.PenaltyArgs(r, f, p)
    keep.append(args)
    return ctypes.byref(args)


def _bias_arg(bias, pen, start: Optional[torch.Tensor], tok_ld: int, vocab: int, device, keep):
    """The dh_bias_spec pointer of a sampler call ("Contextual biasing" of the header), or None when there is no bias.  bias: a
    dualhyp_amd.bias.BiasSpec or a list of (ids, boost) pairs.  On, the call needs start, and with a penalty on (`pen` not None) tables
    that hold the token buffer and the entries' ids."""
    from .bias import as_spec, check_tables
    spec = as_spec(bias, vocab, device)
    if spec is None:
        return None
    if start is None:
        raise ValueError("a bias needs start, the int32 prompt lengths: a match never reaches back into the prompt")
    if pen is not None:
        check_tables(tok_ld, spec.n_ids)
    import ctypes
    keep.append(spec)
    return ctypes.byref(spec.c_struct())


def _automaton_arg(automaton, start: Optional[torch.Tensor], n_seq: int, vocab: int, device, eos_id, keep):
    """The dh_automaton_spec pointer of a sampler call ("Automaton constraints" of the header), or None when there is none.  automaton: a
    dualhyp_amd.automaton.AutomatonSet with a start state per sequence.  On, the call needs start and an eos_id."""
    from .automaton import as_set
    aset = as_set(automaton, n_seq, vocab, device, eos_id)
    if aset is None:
        return None
    if start is None:
        raise ValueError("an automaton needs start, the int32 prompt lengths: a sequence is in its start state while it has generated nothing")
    import ctypes
    keep.append(aset)
    return ctypes.byref(aset.c_struct())


def token_top_logprobs(logits: torch.Tensor, k: int, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids int32 [rows, k], lp float32 [rows, k]): the k most probable tokens of every raw bf16 row, by value descending, then by
    index ascending, with their log-probabilities — bit-equal to token_logprobs(logits, ids[:, j]) (dh_token_top_logprobs_bf16; the
    definition is in include/dualhyp_hip.h, "Token alternatives").  1 <= k <= min(8, vocab).  mask (int32 [rows, words], "Token
    masks"): the first k ids that the row's mask allows, in that order, with the raw row's values — the beam candidates under a
    mask (dh_token_top_logprobs_bf16_mask)."""
    logits = _dev(logits, name="logits")
    if logits.dim() != 2:
        raise ValueError(f"logits must be [rows, vocab], got {tuple(logits.shape)}")
    rows, vocab = logits.shape
    k = check_top_logprobs(k, vocab, lowest=1)
    ids = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    lp = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    m_ptr, m_ld = _mask_arg(mask, rows, vocab, logits.device)
    if rows and mask is not None:
        check(_lib.load().dh_token_top_logprobs_bf16_mask(_p(logits), vocab, k, _p(ids), _p(lp), rows, m_ptr, m_ld, 1, _stream()))
    elif rows:
        check(_lib.load().dh_token_top_logprobs_bf16(_p(logits), vocab, k, _p(ids), _p(lp), rows, _stream()))
    return ids, lp


def beam_select(logits: torch.Tensor, state, *, rows_per_utt: int, eos_id: Optional[int] = None, step: int = 0,
                mask: Optional[torch.Tensor] = None, stop=None, history: Optional[torch.Tensor] = None,
                no_repeat_ngram: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One beam search step in place on `state` (a dualhyp_amd.beam.BeamState): logits [n_utt * rows_per_utt, vocab], rows_per_utt 1
    (step 0: the one live beam) or state.W; every utterance with done == 0 gets its W next beams, its records of `step` and its pool
    entries (dh_beam_select_bf16; the definition is in include/dualhyp_hip.h, "Beam search").  Returns the rows' candidates
    (ids int32, lp float32, both [rows, 2 W]): token_top_logprobs(logits, 2 W).  mask (int32 [n_utt, words], "Token masks"): row u
    serves every beam row of utterance u; the candidates are the first 2 W allowed ids of each row (dh_beam_select_bf16_mask).
    stop (a compiled specification, its stop set only): a candidate in the set ends its hypothesis into the pool as the EOS does, and
    state.fin_tok_buffer() receives the id that ended each pool entry; stop sequences are refused (dh_beam_select_bf16_stop).
    history (state.history_buffer(), "Beam histories" of the header; None: everything above, unchanged): the step reads plane
    (step - 1) & 1 and writes plane step & 1 of the live beams' tokens; no_repeat_ngram (0 .. 8, needs history) bans on them — the
    candidates are the first 2 W ids that the mask allows and the ban leaves, the ban dropped for a row it leaves fewer than 2 W — and
    stop may carry sequences, matched on a beam's own text (dh_beam_select_bf16_hist).  The candidates of a done utterance's rows
    come back as zeros under a ban."""
    logits = _dev(logits, name="logits")
    if logits.dim() != 2:
        raise ValueError(f"logits must be [rows, vocab], got {tuple(logits.shape)}")
    rows, vocab = logits.shape
    W = state.W
    if rows_per_utt not in (1, W) or rows != state.n_utt * rows_per_utt:
        raise ValueError(f"beam_select: {rows} rows for {state.n_utt} utterances x rows_per_utt={rows_per_utt} (1 or W={W})")
    if vocab < 2 * W:
        raise ValueError(f"beam_select: vocab={vocab} is below the 2 W = {2 * W} candidates of a row")
    if not 0 <= int(step) < state.max_new:
        raise ValueError(f"beam_select: step {step} is outside the {state.max_new} recorded steps")
    if state.device != logits.device:
        raise ValueError(f"beam_select: the state lives on {state.device}, the logits on {logits.device}")
    from .ngram import check_ngram
    ngram = check_ngram(no_repeat_ngram, vocab)
    if history is None and ngram:
        raise ValueError(f"beam_select: no_repeat_ngram={ngram} needs history, the state's history planes (state.history_buffer())")
    if history is not None:
        want = (2, state.n_utt, W, state.max_new)
        if history.dtype != torch.int64 or tuple(history.shape) != want or not history.is_contiguous() or history.device != logits.device:
            raise ValueError(f"beam_select: history must be contiguous {torch.int64} {want} on {logits.device}, got {history.dtype} "
                             f"{tuple(history.shape)} on {history.device}")
    make = torch.zeros if ngram else torch.empty      # under a ban the rows of a done utterance are not written
    ids = make((rows, 2 * W), dtype=torch.int32, device=logits.device)
    lp = make((rows, 2 * W), dtype=torch.float32, device=logits.device)
    m_ptr, m_ld = _mask_arg(mask, state.n_utt, vocab, logits.device)
    st_ptr = _stop_arg(stop, vocab, logits.device)
    if st_ptr is not None and stop.sequences and history is None:
        from .beam import HISTORY_HINT
        from .stop import BEAM_REFUSAL
        raise ValueError(BEAM_REFUSAL + HISTORY_HINT)
    if rows:
        import ctypes
        args = (_p(logits), vocab, state.n_utt, int(rows_per_utt), W, state.max_new, -1 if eos_id is None else int(eos_id), int(step), None,
                ctypes.byref(state.c_struct()), _p(ids), _p(lp))
        if history is not None:
            hist = _lib.BeamHist(_p(history), ngram)
            check(_lib.load().dh_beam_select_bf16_hist(*args, m_ptr, m_ld, st_ptr, None if st_ptr is None else _p(state.fin_tok_buffer()),
                                                       ctypes.byref(hist), _stream()))
        elif st_ptr is not None:
            check(_lib.load().dh_beam_select_bf16_stop(*args, m_ptr, m_ld, st_ptr, _p(state.fin_tok_buffer()), _stream()))
        elif mask is not None:
            check(_lib.load().dh_beam_select_bf16_mask(*args, m_ptr, m_ld, _stream()))
        else:
            check(_lib.load().dh_beam_select_bf16(*args, _stream()))
    return ids, lp


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, *, check_ids: bool = True) -> torch.Tensor:
    """float32 [rows]: log softmax(logits[r])[ids[r]] of the raw bf16 rows (dh_token_logprobs_bf16; the definition is in
    include/dualhyp_hip.h, "Token log-probabilities").  An id outside [0, vocab) raises before anything is launched
    (one read-back of the ids' range; check_ids=False: the caller has checked them, as score_batch does once per call)."""
    logits = _dev(logits, name="logits")
    if logits.dim() != 2:
        raise ValueError(f"logits must be [rows, vocab], got {tuple(logits.shape)}")
    rows, vocab = logits.shape
    ids = _dev(ids.reshape(-1), torch.int64, "ids")
    if ids.numel() != rows:
        raise ValueError(f"{ids.numel()} ids for {rows} logits rows")
    out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    if rows == 0:
        return out
    if check_ids:
        lo, hi = (int(v) for v in torch.aminmax(ids))
        if lo < 0 or hi >= vocab:
            raise ValueError(f"token ids span [{lo}, {hi}], outside [0, {vocab})")
    check(_lib.load().dh_token_logprobs_bf16(_p(logits), vocab, _p(ids), _p(out), rows, _stream()))
    return out


def _sample_tail(k: _Keep, rows: bool, logits: torch.Tensor, tokens: torch.Tensor, logprobs, top_logprobs, mask, no_repeat_ngram: int,
                 start, stop, top_p, min_p, repetition_penalty, frequency_penalty, presence_penalty, bias, automaton=None, eos_id=None):
    """The options of sample() (rows False) and sample_rows() (True), checked: (logits on the device, the suffix of the entry to call,
    its arguments behind `stream`).  The entries form one ladder, each taking the options of the one before and its own behind them
    (_lib.SAMPLE_TAIL, and the _automaton entries behind its last piece); the call goes to the narrowest one that takes every option it
    has on.  rows: start None is limit - max_new_tokens, so neither stop sequences nor a ban need it."""
    from .nucleus import check_nucleus
    top_p, min_p = check_nucleus(top_p, min_p)
    logits = _dev(logits, name="logits")
    vocab = logits.size(1)
    assert tokens.dtype == torch.int64 and tokens.is_contiguous()
    n_seq, tok_ld = tokens.shape
    logprobs = _logprobs_buffer(logprobs, tokens)
    top_n, top_ids, top_lp = _top_buffers(top_logprobs, logprobs, tokens, vocab)
    m_ptr, m_ld = _mask_arg(mask, n_seq, vocab, logits.device)
    st_ptr = _stop_arg(stop, vocab, logits.device)
    if not rows and st_ptr is not None and stop.sequences and start is None:
        raise ValueError("stop sequences need start, the int32 prompt lengths: a match never reaches back into the prompt")
    pen = _penalty_arg(repetition_penalty, frequency_penalty, presence_penalty, start, tok_ld, vocab, k)
    b_ptr = _bias_arg(bias, pen, start, tok_ld, vocab, logits.device, k)
    a_ptr = _automaton_arg(automaton, start, n_seq, vocab, logits.device, eos_id, k)
    if (st_ptr is not None or pen is not None or b_ptr is not None or a_ptr is not None) and not no_repeat_ngram:
        ngram, s_ptr = 0, _start_arg(start, n_seq, logits.device, k)
    else:
        ngram, s_ptr = _ngram_arg(no_repeat_ngram, start, n_seq, vocab, logits.device, k, start_optional=rows and a_ptr is None)
    tail = (_p(logprobs), top_n, _p(top_ids), _p(top_lp), m_ptr, m_ld, ngram, s_ptr, st_ptr, top_p, min_p, pen, b_ptr, a_ptr)
    # (suffix, the call has what the entry adds, the arguments the entry takes), widest first
    for suffix, on, n in (("_automaton", a_ptr is not None, 14), ("_bias", b_ptr is not None, 13), ("_penalty", pen is not None, 12), ("_nucleus", top_p < 1.0 or min_p > 0.0, 11),
                          ("_stop", st_ptr is not None, 9), ("_ngram", ngram, 8), ("_mask", mask is not None, 6), ("_top", True, 4)):
        if on:
            return logits, suffix, tail[:n]


def sample(logits: torch.Tensor, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, *,
           temperature: float = 1.0, top_k: Optional[int] = None, eos_id: Optional[int] = None, seed: int = 0,
           step: int = 0, logprobs: Optional[torch.Tensor] = None,
           top_logprobs: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, mask: Optional[torch.Tensor] = None,
           no_repeat_ngram: int = 0, start: Optional[torch.Tensor] = None, stop=None, top_p: Optional[float] = None,
           min_p: Optional[float] = None, repetition_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
           presence_penalty: Optional[float] = None, bias=None, automaton=None) -> None:
    """Append one token per sequence in place (tokens/length/done); see dh_sample_bf16.  logprobs (float32, the shape of
    tokens): the appended token's log-probability goes to the same place in it (dh_sample_bf16_ex).  top_logprobs (with logprobs:
    int32 ids and float32 values, the shape of tokens + (K,)): the K alternatives of the row the token was picked from go to the
    same place in them (dh_sample_bf16_top).  mask (int32 [n_seq, words], "Token masks" of the header): row u holds the tokens
    sequence u may pick; the log-probabilities and alternatives stay the raw row's (dh_sample_bf16_mask).  no_repeat_ngram (1..8, with
    start: int32 [n_seq] prompt lengths; "No-repeat n-grams" of the header): a token that would complete an n-gram already in
    tokens[u, start[u]:length[u]] is not picked, with or without a mask (dh_sample_bf16_ngram).  stop (a compiled specification,
    dualhyp_amd.stop.compile_stop; "Stop conditions" of the header): a sequence whose appended token is in the stop set, or completes
    a stop sequence within tokens[u, start[u]:], gets done = 3; stop sequences need start (dh_sample_bf16_stop).  top_p (in (0, 1]) and
    min_p (in [0, 1]; "Nucleus and min-p" of the header): the draw is made from the entries top_k keeps, cropped to their nucleus and to
    those within min_p of the best; None, 1.0 and 0.0 are off, and top_k = 1 takes neither (dh_sample_bf16_nucleus).
    repetition_penalty (in [1/8, 8]), frequency_penalty and presence_penalty (in [-8, 8]; "Penalties" of the header; they need start): the
    pick is the same call's pick on a copy of the row in which the column of every id in tokens[u, start[u]:length[u]] holds its adjusted
    value; logits is not written, and the log-probabilities and alternatives stay the raw row's.  None, 1.0 and 0.0 are off
    (dh_sample_bf16_penalty).
    bias (a dualhyp_amd.bias.BiasSpec, or a list of (ids, boost) pairs; "Contextual biasing" of the header; it needs start): the pick is
    the same call's pick on a copy of the row in which every id an entry proposes behind tokens[u, start[u]:length[u]] holds
    bf16(y + boost), y its raw or penalised fp32 value; logits is not written, and the log-probabilities and alternatives stay the raw
    row's.  None and an empty list are off (dh_sample_bf16_bias).
    automaton (a dualhyp_amd.automaton.AutomatonSet with a start state per sequence; "Automaton constraints" of the header; it needs start
    and an eos_id): sequence u picks among the tokens on the edges of its state — its start state while it has generated nothing, else
    automaton.state[u], which the call before left — under the mask as well, the EOS alone where that leaves nothing; the ban, the
    penalties and the bias work on that row, and the pick moves automaton.state[u] along its edge.  Log-probabilities and alternatives
    stay the raw row's.  None is off (dh_sample_bf16_automaton)."""
    k = _Keep()
    logits, suffix, tail = _sample_tail(k, False, logits, tokens, logprobs, top_logprobs, mask, no_repeat_ngram, start, stop, top_p, min_p,
                                        repetition_penalty, frequency_penalty, presence_penalty, bias, automaton, eos_id)
    n_seq, vocab = logits.shape
    assert tokens.size(0) == n_seq
    check(getattr(_lib.load(), "dh_sample_bf16" + suffix)(
        _p(logits), vocab, _p(tokens), tokens.size(1), k(length, torch.int32), k(done, torch.int32), n_seq, float(temperature),
        0 if top_k is None else int(top_k), -1 if eos_id is None else int(eos_id), int(seed) & ((1 << 64) - 1), int(step), _stream(), *tail))


def sample_rows(logits: torch.Tensor, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, limit: torch.Tensor,
                row_seq: torch.Tensor, max_new_tokens: int, *, temperature: float = 1.0, top_k: Optional[int] = None,
                eos_id: Optional[int] = None, seed: int = 0, logprobs: Optional[torch.Tensor] = None,
                top_logprobs: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, mask: Optional[torch.Tensor] = None,
                no_repeat_ngram: int = 0, start: Optional[torch.Tensor] = None, stop=None, top_p: Optional[float] = None,
                min_p: Optional[float] = None, repetition_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                presence_penalty: Optional[float] = None, bias=None, automaton=None) -> None:
    """Append one token to sequence row_seq[r] from logits row r, in place; see dh_sample_rows_bf16.  logprobs, top_logprobs: as
    in sample().  mask: as in sample(), one row per SEQUENCE — logits row r is picked under mask row row_seq[r]
    (dh_sample_rows_bf16_mask).  no_repeat_ngram, start: as in sample(), one entry of start per SEQUENCE; start None is
    limit - max_new_tokens (dh_sample_rows_bf16_ngram).  stop: as in sample(); start None is limit - max_new_tokens here too
    (dh_sample_rows_bf16_stop).  top_p, min_p: as in sample() (dh_sample_rows_bf16_nucleus).  repetition_penalty, frequency_penalty,
    presence_penalty: as in sample(), start included (dh_sample_rows_bf16_penalty).  bias: as in sample(), start included
    (dh_sample_rows_bf16_bias).  automaton: as in sample(), one start state and one state entry per SEQUENCE, and start given
    (dh_sample_rows_bf16_automaton)."""
    k = _Keep()
    logits, suffix, tail = _sample_tail(k, True, logits, tokens, logprobs, top_logprobs, mask, no_repeat_ngram, start, stop, top_p, min_p,
                                        repetition_penalty, frequency_penalty, presence_penalty, bias, automaton, eos_id)
    n_rows, vocab = logits.shape
    n_seq = tokens.size(0)
    assert row_seq.numel() == n_rows
    assert length.numel() == done.numel() == limit.numel() == n_seq
    check(getattr(_lib.load(), "dh_sample_rows_bf16" + suffix)(
        _p(logits), vocab, _p(tokens), tokens.size(1), k(length, torch.int32), k(done, torch.int32), k(limit, torch.int32),
        k(row_seq, torch.int32), n_rows, n_seq, int(max_new_tokens), float(temperature), 0 if top_k is None else int(top_k),
        -1 if eos_id is None else int(eos_id), int(seed) & ((1 << 64) - 1), _stream(), *tail))


def quant_rows_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(uint8 e4m3 [rows, K], fp32 scale [rows]) of bf16 rows; dh_quant_rows_fp8."""
    x = _dev(x, name="x")
    K = x.size(-1)
    rows = x.numel() // K
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device)
    s = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().dh_quant_rows_fp8(_p(x), _p(q), _p(s), rows, K, _stream()))
    return q, s


def rmsnorm_quant_fp8(x: torch.Tensor, w: torch.Tensor, eps: float, row_tail: Optional[torch.Tensor] = None):
    """(bf16 RMSNorm rows, their e4m3 bytes, fp32 scales); dh_rmsnorm_quant_fp8."""
    k = _Keep()
    x = _dev(x, name="x")
    d = x.size(-1)
    rows = x.numel() // d
    xn = torch.empty_like(x)
    q = torch.empty((rows, d), dtype=torch.uint8, device=x.device)
    s = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().dh_rmsnorm_quant_fp8(_p(x), k(w, name="weight"), _p(xn), _p(q), _p(s), rows, d, float(eps),
                                           k(row_tail, torch.uint8, "row_tail"), _stream()))
    return xn, q, s


def linear_fp8(xq: torch.Tensor, x_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor, *, epilogue: int = EPI_PLAIN,
               w2q: Optional[torch.Tensor] = None, w2_scale: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
               bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, kernel: int = 0,
               out32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [M, N] = epilogue((xq . wq^T) * x_scale[m] * w_scale[n]) on the fp8 MFMA; dh_linear_fp8_ex (kernel: 0 by row
    count, 1 tiled, 2 streaming).  out32: dh_linear_fp8_f32, the PLAIN streaming result as fp32.  out: the caller's result
    buffer (bf16, or fp32 with out32)."""
    k = _Keep()
    M, K = xq.shape
    N = wq.size(0)
    assert wq.size(1) == K and xq.dtype == torch.uint8 and wq.dtype == torch.uint8
    if out32:
        assert epilogue == EPI_PLAIN and resid is None and kernel in (0, 2)
        y = _out(out, (M, N), torch.float32, xq.device)
        check(_lib.load().dh_linear_fp8_f32(k(xq, torch.uint8, "xq"), k(x_scale, torch.float32, "x_scale"), k(wq, torch.uint8, "wq"),
                                            k(w_scale, torch.float32, "w_scale"), _p(y), M, N, K, _stream()))
        return y
    y = _out(out, (M, N), torch.bfloat16, xq.device)
    check(_lib.load().dh_linear_fp8_ex(k(xq, torch.uint8, "xq"), k(x_scale, torch.float32, "x_scale"), k(wq, torch.uint8, "wq"),
                                       k(w_scale, torch.float32, "w_scale"), _p(y), M, N, K, epilogue, k(w2q, torch.uint8, "w2q"),
                                       k(w2_scale, torch.float32, "w2_scale"), k(scale, name="scale"), k(bias, name="bias"),
                                       k(resid, name="resid"), int(kernel), _stream()))
    return y


def linear_mxfp4(xq: torch.Tensor, x_scale: torch.Tensor, wq: torch.Tensor, w_scale: torch.Tensor, *, epilogue: int = EPI_PLAIN,
                 w2q: Optional[torch.Tensor] = None, w2_scale: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                 bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, kernel: int = 0,
                 out32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [M, N] = epilogue((xq . dequant(W)^T) * x_scale[m]) with MXFP4 weights as dualhyp_amd.quant.pack_mxfp4 lays them out
    (wq uint8 [N/16, K/128, 64, 16], w_scale uint8 [N/16, K/128, 64]); dh_linear_mxfp4_ex (kernel: 0 by row count, 1 tiled,
    2 streaming).  out32: dh_linear_mxfp4_f32, the PLAIN streaming result as fp32.  out: the caller's result buffer (bf16, or
    fp32 with out32)."""
    k = _Keep()
    M, K = xq.shape
    assert wq.dim() == 4 and wq.shape[2:] == (64, 16) and w_scale.shape == wq.shape[:3] and wq.size(1) * 128 == K
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and w_scale.dtype == torch.uint8
    N = wq.size(0) * 16
    if out32:
        assert epilogue == EPI_PLAIN and resid is None and kernel in (0, 2)
        y = _out(out, (M, N), torch.float32, xq.device)
        check(_lib.load().dh_linear_mxfp4_f32(k(xq, torch.uint8, "xq"), k(x_scale, torch.float32, "x_scale"), k(wq, torch.uint8, "wq"),
                                              k(w_scale, torch.uint8, "w_scale"), _p(y), M, N, K, _stream()))
        return y
    y = _out(out, (M, N), torch.bfloat16, xq.device)
    check(_lib.load().dh_linear_mxfp4_ex(k(xq, torch.uint8, "xq"), k(x_scale, torch.float32, "x_scale"), k(wq, torch.uint8, "wq"),
                                         k(w_scale, torch.uint8, "w_scale"), _p(y), M, N, K, epilogue, k(w2q, torch.uint8, "w2q"),
                                         k(w2_scale, torch.uint8, "w2_scale"), k(scale, name="scale"), k(bias, name="bias"),
                                         k(resid, name="resid"), int(kernel), _stream()))
    return y


# ------------------------------------------------------------------------------------------ MXFP6 activations
def _mxfp6_buffers(rows: int, K: int, device, fill: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    G = (rows + 15) // 16
    mk = torch.empty if fill is None else (lambda *a, **kw: torch.full(*a, fill_value=fill, **kw))
    return (mk((G, K // 128, 3, 64, 8), dtype=torch.uint8, device=device), mk((G, K // 128, 64), dtype=torch.uint8, device=device))


def quant_rows_mxfp6(x: torch.Tensor, fill: Optional[int] = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(uint8 codes [ceil(rows / 16), K / 128, 3, 64, 8], uint8 E8M0 bytes [ceil(rows / 16), K / 128, 64]) of bf16 rows in the layout
    of include/dualhyp_hip.h "MXFP6 activations"; dh_quant_rows_mxfp6.  fill: what the buffers hold before the call (the kernel
    never writes the rows past `rows` of the last group); None leaves them uninitialised."""
    x = _dev(x, name="x")
    K = x.size(-1)
    rows = x.numel() // K
    q, s = _mxfp6_buffers(rows, K, x.device, fill)
    check(_lib.load().dh_quant_rows_mxfp6(_p(x), _p(q), _p(s), rows, K, _stream()))
    return q, s


def rmsnorm_quant_mxfp6(x: torch.Tensor, w: torch.Tensor, eps: float, row_tail: Optional[torch.Tensor] = None, fill: Optional[int] = 0):
    """(bf16 RMSNorm rows, their MXFP6 codes, their E8M0 bytes); dh_rmsnorm_quant_mxfp6."""
    k = _Keep()
    x = _dev(x, name="x")
    d = x.size(-1)
    rows = x.numel() // d
    xn = torch.empty_like(x)
    q, s = _mxfp6_buffers(rows, d, x.device, fill)
    check(_lib.load().dh_rmsnorm_quant_mxfp6(_p(x), k(w, name="weight"), _p(xn), _p(q), _p(s), rows, d, float(eps),
                                             k(row_tail, torch.uint8, "row_tail"), _stream()))
    return xn, q, s


def linear_mxfp4a6(xq: torch.Tensor, x_scale: torch.Tensor, M: int, wq: torch.Tensor, w_scale: torch.Tensor, *, epilogue: int = EPI_PLAIN,
                   w2q: Optional[torch.Tensor] = None, w2_scale: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                   bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, kernel: int = 0,
                   out32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_mxfp4 with MXFP6 activations: bf16 [M, N] = epilogue(dequant(x) . dequant(W)^T), xq / x_scale as quant_rows_mxfp6 or
    dualhyp_amd.quant.pack_mxfp6 lay them out (M is passed: the buffers hold whole groups of 16 rows); dh_linear_mxfp4a6_ex, or
    dh_linear_mxfp4a6_f32 with out32."""
    k = _Keep()
    K = wq.size(1) * 128
    assert wq.dim() == 4 and wq.shape[2:] == (64, 16) and w_scale.shape == wq.shape[:3]
    assert xq.dim() == 5 and xq.shape[1:] == (K // 128, 3, 64, 8) and x_scale.shape == xq.shape[:2] + (64,) and xq.size(0) == (M + 15) // 16
    assert xq.dtype == torch.uint8 and x_scale.dtype == torch.uint8 and wq.dtype == torch.uint8 and w_scale.dtype == torch.uint8
    N = wq.size(0) * 16
    if out32:
        assert epilogue == EPI_PLAIN and resid is None and kernel in (0, 2)
        y = _out(out, (M, N), torch.float32, xq.device)
        check(_lib.load().dh_linear_mxfp4a6_f32(k(xq, torch.uint8, "xq"), k(x_scale, torch.uint8, "x_scale"), k(wq, torch.uint8, "wq"),
                                                k(w_scale, torch.uint8, "w_scale"), _p(y), M, N, K, _stream()))
        return y
    y = _out(out, (M, N), torch.bfloat16, xq.device)
    check(_lib.load().dh_linear_mxfp4a6_ex(k(xq, torch.uint8, "xq"), k(x_scale, torch.uint8, "x_scale"), k(wq, torch.uint8, "wq"),
                                           k(w_scale, torch.uint8, "w_scale"), _p(y), M, N, K, epilogue, k(w2q, torch.uint8, "w2q"),
                                           k(w2_scale, torch.uint8, "w2_scale"), k(scale, name="scale"), k(bias, name="bias"),
                                           k(resid, name="resid"), int(kernel), _stream()))
    return y


# ------------------------------------------------------------------------------------------ fp8 KV cache
def kv8_alloc(n_slots: int, n_groups: int, s_max: int, hs: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """A zeroed fp8 KV cache: (k8 uint8 [slot, group, s_max, hs], v8 uint8 [slot, group, hs, s_max], k_exp, v_exp int8
    [slot, group, s_max]).  The uint8 shapes are nominal, as the bf16 caches' are: the bytes of a (slot, group) block are in the
    fragment order of csrc/common.h k8_off / v8_off (kv8_unpack)."""
    return (torch.zeros((n_slots, n_groups, s_max, hs), dtype=torch.uint8, device=device),
            torch.zeros((n_slots, n_groups, hs, s_max), dtype=torch.uint8, device=device),
            torch.zeros((n_slots, n_groups, s_max), dtype=torch.int8, device=device),
            torch.zeros((n_slots, n_groups, s_max), dtype=torch.int8, device=device))


def _kv8_check(k8: torch.Tensor, v8: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor) -> Tuple[int, int, int, int]:
    B, G, s_max, hs = k8.shape
    for t, dt, shape, nm in ((k8, torch.uint8, (B, G, s_max, hs), "k8"), (v8, torch.uint8, (B, G, hs, s_max), "v8"),
                             (k_exp, torch.int8, (B, G, s_max), "k_exp"), (v_exp, torch.int8, (B, G, s_max), "v_exp")):
        if not t.is_cuda:
            raise _lib.DualHypHipError(f"{nm} must live on the GPU: the HIP path has no CPU fallback")
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError(f"{nm} must be a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    return B, G, s_max, hs


def qkv_rope_cache_kv8(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, tok_slot: torch.Tensor, tok_pos: torch.Tensor,
                       k8: torch.Tensor, v8: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor, n_head: int,
                       n_groups: int) -> torch.Tensor:
    """-> rotated q [n_tok, n_head, hs] (the bits of qkv_rope_cache); k (after rope) and v of every token are quantised into
    the fp8 cache in place; dh_qkv_rope_cache_kv8."""
    k = _Keep()
    qkv = _dev(qkv, name="qkv")
    _, _, s_max, hs = _kv8_check(k8, v8, k_exp, v_exp)
    n_tok = qkv.numel() // ((n_head + 2 * n_groups) * hs)
    q = torch.empty((n_tok, n_head, hs), dtype=torch.bfloat16, device=qkv.device)
    check(_lib.load().dh_qkv_rope_cache_kv8(_p(qkv), k(cos), k(sin), k(tok_slot, torch.int32), k(tok_pos, torch.int32), _p(q),
                                            _p(k8), _p(v8), _p(k_exp), _p(v_exp), n_tok, n_head, n_groups, hs, s_max, _stream()))
    return q


def attn_decode_kv8(q: torch.Tensor, k8: torch.Tensor, v8: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor,
                    seq_slot: torch.Tensor, kv_len: torch.Tensor) -> torch.Tensor:
    """attn_decode over the fp8 cache; dh_attn_decode_kv8."""
    k = _Keep()
    n_seq, n_head, hs = q.shape
    _, n_groups, s_max, hs_c = _kv8_check(k8, v8, k_exp, v_exp)
    assert hs_c == hs, f"q has head size {hs}, the cache {hs_c}"
    lib = _lib.load()
    work = torch.empty(lib.dh_attn_decode_work_bytes(n_seq, n_head, hs, s_max), dtype=torch.uint8, device=q.device)
    y = torch.empty((n_seq, n_head * hs), dtype=torch.bfloat16, device=q.device)
    i32 = torch.int32
    check(lib.dh_attn_decode_kv8(k(q), _p(k8), _p(v8), _p(k_exp), _p(v_exp), k(seq_slot, i32), k(kv_len, i32), _p(y), _p(work),
                                 n_seq, n_head, n_groups, hs, s_max, _stream()))
    return y


def kv8_expand(k8: torch.Tensor, v8: torch.Tensor, k_exp: torch.Tensor, v_exp: torch.Tensor, seq_slot: torch.Tensor,
               kv_len: Optional[torch.Tensor], k_out: torch.Tensor, vT_out: torch.Tensor) -> None:
    """Positions [0, kv_len[i]) of slot seq_slot[i] (kv_len None: every position) dequantised into the bf16 caches k_out
    [slot, group, s_max, hs] / vT_out [slot, group, hs, s_max] in place, whole 32-key tiles; dh_kv8_expand."""
    k = _Keep()
    B, G, s_max, hs = _kv8_check(k8, v8, k_exp, v_exp)
    assert tuple(_dev(k_out, name="k_out").shape) == (B, G, s_max, hs) and k_out.is_contiguous()
    assert tuple(_dev(vT_out, name="vT_out").shape) == (B, G, hs, s_max) and vT_out.is_contiguous()
    i32 = torch.int32
    check(_lib.load().dh_kv8_expand(_p(k8), _p(v8), _p(k_exp), _p(v_exp), k(seq_slot, i32), k(kv_len, i32), None, _p(k_out),
                                    _p(vT_out), seq_slot.numel(), G, hs, s_max, _stream()))


def kv8_unpack(k8: torch.Tensor, v8: torch.Tensor, k_exp: torch.Tensor,
               v_exp: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fp8 cache buffers as stored -> (K bytes, V bytes: uint8 [slot, group, pos, hs]; K exponents, V exponents: int8
    [slot, group, pos]).  Host index math of csrc/common.h k8_off / v8_off; works on any device.  Test/debug helper."""
    B, G, S, hs = k8.shape
    k = k8.reshape(B, G, S // 32, hs // 32, 2, 32, 2, 8)                 # tile, kp, lh, lr, hf, e
    k = k.permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(B, G, S, hs)           # key = (tile, lr); d = 32 kp + 16 hf + 8 lh + e
    v = v8.reshape(B, G, S // 32, hs // 32, 2, 32, 2, 2, 4)              # tile, dt, lh, lr, s2, jh, jl
    v = v.permute(0, 1, 2, 6, 7, 4, 8, 3, 5).reshape(B, G, S, hs)        # key = 32 tile + 16 s2 + 8 jh + 4 lh + jl; d = 32 dt + lr
    return k, v, k_exp, v_exp


def im2col3(x: torch.Tensor, ld: int, relu: bool = False) -> torch.Tensor:
    """[B*T, ld] im2col matrix of a k=3, pad=1 convolution over x [B,T,C] with a ones column at 3C; dh_im2col3_bf16."""
    x = _dev(x, name="x")
    B, T, Cc = x.shape
    out = torch.empty((B * T, ld), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().dh_im2col3_bf16(_p(x), _p(out), B, T, Cc, ld, int(relu), _stream()))
    return out


def pool_head(h: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pool: int) -> torch.Tensor:
    """ReLU -> AvgPool1d(pool, ceil) -> Linear(H, 3) on h [B,T,H]; dh_pool_head_bf16."""
    k = _Keep()
    h = _dev(h, name="h")
    B, T, H = h.shape
    out = torch.empty((B, (T + pool - 1) // pool, 3), dtype=torch.bfloat16, device=h.device)
    check(_lib.load().dh_pool_head_bf16(_p(h), k(w, name="w"), k(bias, name="bias"), _p(out), B, T, H, int(pool),
                                        _stream()))
    return out


def pool_head_bwd(h: torch.Tensor, w: torch.Tensor, dlogits: torch.Tensor, pool: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dh bf16 [B,T,H], pooled bf16 [B*P,H]) from dlogits fp32 [B,P,3]; dh_pool_head_bwd_bf16."""
    k = _Keep()
    h = _dev(h, name="h")
    B, T, H = h.shape
    P = (T + pool - 1) // pool
    assert dlogits.shape == (B, P, 3)
    dh = torch.empty_like(h)
    pooled = torch.empty((B * P, H), dtype=torch.bfloat16, device=h.device)
    check(_lib.load().dh_pool_head_bwd_bf16(_p(h), k(w, name="w"), k(dlogits, torch.float32, "dlogits"), _p(dh), _p(pooled),
                                            B, T, H, int(pool), _stream()))
    return dh, pooled


def col2im3(dcol: torch.Tensor, B: int, T: int, C: int, pre: Optional[torch.Tensor] = None,
            mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx bf16 [B,T,C]: backward of im2col3 through the ReLU of `pre` and the dropout `mask` in front of it; dh_col2im3_bf16."""
    k = _Keep()
    dcol = _dev(dcol, name="dcol")
    assert dcol.dim() == 2 and dcol.size(0) == B * T and dcol.size(1) >= 3 * C
    dx = torch.empty((B, T, C), dtype=torch.bfloat16, device=dcol.device)
    check(_lib.load().dh_col2im3_bf16(_p(dcol), k(pre, name="pre"), k(mask, name="mask"), _p(dx), B, T, C, dcol.size(1), _stream()))
    return dx


def cross_entropy_fwd(logits: torch.Tensor, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss_per_row fp32 [rows], lse fp32 [rows]); ignored rows (target -1) give 0; dh_cross_entropy_fwd."""
    assert logits.dtype in (torch.bfloat16, torch.float32), f"logits must be bf16 or fp32, got {logits.dtype}"
    lg = _dev(logits.reshape(-1, logits.size(-1)), logits.dtype, "logits")
    tg = _dev(targets.reshape(-1), torch.int64, "targets")
    assert tg.numel() == lg.size(0), f"{tg.numel()} targets for {lg.size(0)} rows"
    loss = torch.empty(lg.size(0), dtype=torch.float32, device=lg.device)
    lse = torch.empty_like(loss)
    check(_lib.load().dh_cross_entropy_fwd(_p(lg), int(lg.dtype == torch.float32), _p(tg), _p(loss), _p(lse), lg.size(0),
                                           lg.size(1), _stream()))
    return loss, lse


def cross_entropy_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, grad_row: torch.Tensor) -> torch.Tensor:
    """dlogits (same shape / dtype as logits); dh_cross_entropy_bwd."""
    k = _Keep()
    lg = _dev(logits.reshape(-1, logits.size(-1)), logits.dtype, "logits")
    tg = _dev(targets.reshape(-1), torch.int64, "targets")
    out = torch.empty_like(lg)
    check(_lib.load().dh_cross_entropy_bwd(_p(lg), int(lg.dtype == torch.float32), _p(tg), k(lse, torch.float32, "lse"),
                                           k(grad_row, torch.float32, "grad_row"), _p(out), lg.size(0), lg.size(1),
                                           _stream()))
    return out.view(logits.shape)


def linear_partial(x: torch.Tensor, w: torch.Tensor, w_ext: Optional[torch.Tensor] = None, ksplit: int = 1,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 partial sums [ksplit, M, n_main+n_ext] of x @ [w; w_ext].T (decode rows, M <= 4096); dh_linear_partial_bf16."""
    x, w = _dev(x, name="x"), _dev(w, name="w")
    K = x.size(-1)
    M = x.numel() // K
    n_ext = 0 if w_ext is None else _dev(w_ext, name="w_ext").size(0)
    y = _out(out, (ksplit, M, w.size(0) + n_ext), torch.float32, x.device)
    check(_lib.load().dh_linear_partial_bf16(_p(x), _p(w), _p(w_ext), _p(y), M, w.size(0), n_ext, K, ksplit, _stream()))
    return y


def linear_partial_pairs(x: torch.Tensor, w: torch.Tensor, w_ext: Optional[torch.Tensor] = None, ksplit: int = 1,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [(ksplit+1)//2, M, n_main+n_ext]: sums of adjacent pairs of `linear_partial`'s slices, from the tiled split-K
    kernel; dh_linear_partial_pairs_bf16."""
    x, w = _dev(x, name="x"), _dev(w, name="w")
    K = x.size(-1)
    M = x.numel() // K
    n_ext = 0 if w_ext is None else _dev(w_ext, name="w_ext").size(0)
    y = _out(out, ((ksplit + 1) // 2, M, w.size(0) + n_ext), torch.float32, x.device)
    check(_lib.load().dh_linear_partial_pairs_bf16(_p(x), _p(w), _p(w_ext), _p(y), M, w.size(0), n_ext, K, ksplit, _stream()))
    return y


def combine_partials(parts: torch.Tensor, pairs: bool = True) -> torch.Tensor:
    """The decode family's K-slice combine order on the fp32 partials [n, M, N] (include/dualhyp_hip.h): adjacent slices in
    pairs, pair sums in index order (`pairs=False`: the inputs already are pair sums).  torch fp32 adds: test helper."""
    if pairs:
        n = parts.size(0)
        parts = torch.stack([parts[i] + parts[i + 1] if i + 1 < n else parts[i] for i in range(0, n, 2)])
    out = parts[0].clone()
    for p in parts[1:]:
        out = out + p
    return out


def linear_chain(x: torch.Tensor, w: torch.Tensor, w_ext: Optional[torch.Tensor] = None, ksplit: int = 1,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [M, n_main+n_ext]: the ksplit slices of `linear_partial` combined in the family's order (`combine_partials`)
    by one launch of the tiled kernel (M >= 65); dh_linear_chain_bf16."""
    x, w = _dev(x, name="x"), _dev(w, name="w")
    K = x.size(-1)
    M = x.numel() // K
    n_ext = 0 if w_ext is None else _dev(w_ext, name="w_ext").size(0)
    y = _out(out, (M, w.size(0) + n_ext), torch.float32, x.device)
    check(_lib.load().dh_linear_chain_bf16(_p(x), _p(w), _p(w_ext), _p(y), M, w.size(0), n_ext, K, ksplit, _stream()))
    return y


def finish_norm(h32: torch.Tensor, d: int, x_resid: torch.Tensor, w_norm: torch.Tensor, eps: float,
                lora_b: Optional[torch.Tensor] = None, lora_scale: float = 1.0,
                row_tail: Optional[torch.Tensor] = None, pairs: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x_out, xn_out) = LoRA finish + residual + RMSNorm of fp32 partials (`pairs`: they are K-slices, to be added in
    adjacent pairs first; False: pair sums / the total); dh_finish_norm_bf16."""
    k = _Keep()
    n_part, rows, ld = h32.shape
    x_resid = _dev(x_resid, name="x_resid")
    x_out, xn_out = torch.empty_like(x_resid), torch.empty_like(x_resid)
    check(_lib.load().dh_finish_norm_bf16(_p(h32), n_part, int(pairs), rows, d, ld - d, _p(lora_b), float(lora_scale), _p(x_resid),
                                          k(w_norm), _p(x_out), _p(xn_out), float(eps), _p(row_tail), _stream()))
    return x_out, xn_out


def attn_decode_fused(qkv32: torch.Tensor, qkv_dim: int, lora_b: Optional[torch.Tensor], lora_scale: float,
                      splits: Tuple[int, int], cos: torch.Tensor, sin: torch.Tensor, seq_slot: torch.Tensor,
                      kv_len: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, n_head: int,
                      pairs: bool = True) -> torch.Tensor:
    """Decode-step attention sub-layer from fp32 qkv partials (`pairs` as in finish_norm); dh_attn_decode_fused_bf16."""
    k = _Keep()
    n_part, n_seq, ld = qkv32.shape
    n_groups, s_max, hs = k_cache.size(1), k_cache.size(2), k_cache.size(3)
    y = torch.empty((n_seq, n_head * hs), dtype=torch.bfloat16, device=qkv32.device)
    i32 = torch.int32
    check(_lib.load().dh_attn_decode_fused_bf16(_p(qkv32), n_part, int(pairs), n_seq, qkv_dim, ld - qkv_dim, _p(lora_b),
                                                float(lora_scale), splits[0], splits[1], k(cos), k(sin),
                                                k(seq_slot, i32), k(kv_len, i32), _p(k_cache), _p(vT_cache),
                                                _p(y), n_head, n_groups, hs, s_max, _stream()))
    return y


def attn_verify_fused(qkv32: torch.Tensor, qkv_dim: int, lora_b: Optional[torch.Tensor], lora_scale: float,
                      splits: Tuple[int, int], cos: torch.Tensor, sin: torch.Tensor, seq_slot: torch.Tensor,
                      kv_len: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, n_head: int, S: int,
                      p_max: Optional[int] = None, pairs: bool = True) -> torch.Tensor:
    """`attn_decode_fused` for S consecutive positions per sequence in one launch (the verify step of speculative decoding):
    qkv32 [n_part, n_seq * S, ld], row seq * S + j at position kv_len[seq] - 1 + j; -> [n_seq * S, n_head * hs].  Rows at
    positions >= p_max (default s_max) append nothing; dh_attn_verify_fused_bf16."""
    k = _Keep()
    n_part, n_rows, ld = qkv32.shape
    if S <= 0 or n_rows % S:
        raise ValueError(f"attn_verify_fused: {n_rows} rows are not S = {S} per sequence")
    n_groups, s_max, hs = k_cache.size(1), k_cache.size(2), k_cache.size(3)
    y = torch.empty((n_rows, n_head * hs), dtype=torch.bfloat16, device=qkv32.device)
    i32 = torch.int32
    check(_lib.load().dh_attn_verify_fused_bf16(_p(qkv32), n_part, int(pairs), n_rows // S, S, qkv_dim, ld - qkv_dim, _p(lora_b),
                                                float(lora_scale), splits[0], splits[1], k(cos), k(sin),
                                                k(seq_slot, i32), k(kv_len, i32), _p(k_cache), _p(vT_cache),
                                                _p(y), n_head, n_groups, hs, s_max, s_max if p_max is None else int(p_max), _stream()))
    return y


def check_shared_rows(n_rows: int, group_rows, name: str = "attn_decode_shared") -> int:
    """group_rows of a shared-prompt attention call over n_rows rows, or a ValueError."""
    if isinstance(group_rows, bool) or not isinstance(group_rows, int) or not 2 <= group_rows <= 8:
        raise ValueError(f"{name}: group_rows is the number of rows that share a prompt, an int in 2..8, not {group_rows!r}")
    if n_rows <= 0 or n_rows % group_rows:
        raise ValueError(f"{name}: {n_rows} rows are not group_rows = {group_rows} per utterance")
    return group_rows


def attn_decode_shared(qkv32: torch.Tensor, qkv_dim: int, lora_b: Optional[torch.Tensor], lora_scale: float,
                       splits: Tuple[int, int], cos: torch.Tensor, sin: torch.Tensor, seq_slot: torch.Tensor,
                       kv_len: torch.Tensor, k_cache: torch.Tensor, vT_cache: torch.Tensor, n_head: int, group_rows: int,
                       prompt_len: torch.Tensor, pairs: bool = True, tile_tab: Optional[torch.Tensor] = None,
                       step_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`attn_decode_fused` over rows that share prompts (include/dualhyp_hip.h, "Shared-prompt attention"): rows u * group_rows + j
    are the candidates or beams of utterance u, prompt_len int32 [n_seq / group_rows] on the GPU; the whole prompt tiles are read
    once per block, from the slot of the utterance's row 0.  Same bits and caches as attn_decode_fused; dh_attn_decode_shared_bf16.
    tile_tab (None: the call above, unchanged): the rows' tile table, contiguous int32 [2, n_seq, NT] on the GPU ("Beam KV tile table"
    of the header) — private tile prompt_len[u] // 32 + j of row r is read from the slot of the sibling that entry [plane, r, j] names;
    step_dev (a one-element int32 tensor, the device step counter t) selects plane (t - 1) & 1, None plane 0;
    dh_attn_decode_shared_tab_bf16."""
    k = _Keep()
    n_part, n_seq, ld = qkv32.shape
    N = check_shared_rows(n_seq, group_rows)
    if (not isinstance(prompt_len, torch.Tensor) or prompt_len.dtype != torch.int32 or prompt_len.dim() != 1
            or prompt_len.numel() != n_seq // N or not prompt_len.is_contiguous()):
        raise ValueError(f"attn_decode_shared: prompt_len is a contiguous 1-D int32 tensor of {n_seq // N} utterances")
    n_groups, s_max, hs = k_cache.size(1), k_cache.size(2), k_cache.size(3)
    y = torch.empty((n_seq, n_head * hs), dtype=torch.bfloat16, device=qkv32.device)
    i32 = torch.int32
    if tile_tab is not None:
        if (not isinstance(tile_tab, torch.Tensor) or tile_tab.dtype != i32 or tile_tab.dim() != 3 or tile_tab.size(0) != 2
                or tile_tab.size(1) != n_seq or not tile_tab.is_contiguous() or tile_tab.device != qkv32.device):
            raise ValueError(f"attn_decode_shared: tile_tab is a contiguous int32 tensor [2, {n_seq}, NT] on {qkv32.device}")
        if step_dev is not None and (step_dev.dtype != i32 or step_dev.numel() != 1 or step_dev.device != qkv32.device):
            raise ValueError("attn_decode_shared: step_dev is a one-element int32 tensor on the GPU")
        check(_lib.load().dh_attn_decode_shared_tab_bf16(_p(qkv32), n_part, int(pairs), n_seq, qkv_dim, ld - qkv_dim, _p(lora_b),
                                                         float(lora_scale), splits[0], splits[1], k(cos), k(sin),
                                                         k(seq_slot, i32), k(kv_len, i32), _p(k_cache), _p(vT_cache),
                                                         _p(y), n_head, n_groups, hs, s_max, N, k(prompt_len, i32), _p(tile_tab),
                                                         tile_tab.size(2), _p(step_dev), _stream()))
        return y
    if step_dev is not None:
        raise ValueError("attn_decode_shared: step_dev selects a plane of tile_tab, which is None")
    check(_lib.load().dh_attn_decode_shared_bf16(_p(qkv32), n_part, int(pairs), n_seq, qkv_dim, ld - qkv_dim, _p(lora_b),
                                                 float(lora_scale), splits[0], splits[1], k(cos), k(sin),
                                                 k(seq_slot, i32), k(kv_len, i32), _p(k_cache), _p(vT_cache),
                                                 _p(y), n_head, n_groups, hs, s_max, N, k(prompt_len, i32), _stream()))
    return y


def beam_retile(k_cache: torch.Tensor, vT_cache: torch.Tensor, tile_tab: torch.Tensor, beam_parent: torch.Tensor,
                n_steps: torch.Tensor, prompt_len: torch.Tensor, step: int, scratch: Optional[torch.Tensor] = None) -> None:
    """The KV step of a beam call under a tile table, alone and in place ("Beam KV tile table" of the header; dh_beam_retile): behind
    the selection of `step` (1 .. max_new - 1), plane step & 1 of tile_tab (int32 [2, n_utt * W, NT]) receives the rows' entries and
    the open tile of every row that continues another beam is copied from its parent's slot.  k_cache [n_utt * W, G, s_max, hs] and
    vT_cache [n_utt * W, G, hs, s_max] are one layer's pair as stored; beam_parent int32 [n_utt, max_new, W], n_steps and prompt_len
    int32 [n_utt], all on the GPU.  scratch: bf16, at least rows * 2 * G * hs * 32 elements (made here when None)."""
    i32 = torch.int32
    dev = k_cache.device
    if beam_parent.dim() != 3 or beam_parent.dtype != i32 or not beam_parent.is_contiguous():
        raise ValueError("beam_retile: beam_parent is a contiguous int32 tensor [n_utt, max_new, W]")
    n_utt, max_new, W = beam_parent.shape
    rows = n_utt * W
    if (k_cache.dim() != 4 or k_cache.dtype != torch.bfloat16 or k_cache.size(0) != rows or not k_cache.is_contiguous()
            or vT_cache.dtype != torch.bfloat16 or not vT_cache.is_contiguous()):
        raise ValueError(f"beam_retile: k_cache is a contiguous bf16 [{rows}, G, s_max, hs] and vT_cache its [{rows}, G, hs, s_max]")
    G, s_max, hs = k_cache.size(1), k_cache.size(2), k_cache.size(3)
    if tuple(vT_cache.shape) != (rows, G, hs, s_max):
        raise ValueError(f"beam_retile: vT_cache must be {(rows, G, hs, s_max)}, got {tuple(vT_cache.shape)}")
    if (tile_tab.dtype != i32 or tile_tab.dim() != 3 or tile_tab.size(0) != 2 or tile_tab.size(1) != rows
            or not tile_tab.is_contiguous()):
        raise ValueError(f"beam_retile: tile_tab is a contiguous int32 tensor [2, {rows}, NT]")
    for name, t in (("n_steps", n_steps), ("prompt_len", prompt_len)):
        if t.dtype != i32 or t.dim() != 1 or t.numel() != n_utt or not t.is_contiguous():
            raise ValueError(f"beam_retile: {name} is a contiguous int32 tensor of {n_utt} utterances")
    for t in (vT_cache, tile_tab, beam_parent, n_steps, prompt_len):
        if t.device != dev:
            raise ValueError("beam_retile: every tensor lives on the caches' device")
    need = rows * 2 * G * hs * 32
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.bfloat16, device=dev)
    elif scratch.dtype != torch.bfloat16 or scratch.numel() < need or not scratch.is_contiguous() or scratch.device != dev:
        raise ValueError(f"beam_retile: scratch holds at least {need} contiguous bf16 elements on {dev}")
    check(_lib.load().dh_beam_retile(_p(k_cache), _p(vT_cache), _p(scratch), _p(tile_tab), tile_tab.size(2), _p(beam_parent), _p(n_steps),
                                     _p(prompt_len), n_utt, W, max_new, int(step), None, G, hs, s_max, _stream()))


def kcache_to_plain(kc: torch.Tensor) -> torch.Tensor:
    """K cache [slot, group, s_max, hs] as stored (MFMA-fragment order, csrc/common.h kfrag_off)
    -> plain [slot, group, key, channel].  Test/debug helper."""
    B, G, S, hs = kc.shape
    v = kc.reshape(B, G, S // 32, hs // 16, 2, 32, 8)            # tile, ks, lh, lr, e
    return v.permute(0, 1, 2, 5, 3, 4, 6).reshape(B, G, S, hs)


def vcache_to_plain(vt: torch.Tensor) -> torch.Tensor:
    """V^T cache [slot, group, hs, s_max] as stored (fragment order, vfrag_off) -> plain
    [slot, group, channel, key].  Test/debug helper."""
    B, G, hs, S = vt.shape
    v = vt.reshape(B, G, S // 32, hs // 32, 2, 2, 32, 2, 4)      # tile, dt, s2, lh, lr, jh, jl
    return v.permute(0, 1, 3, 6, 2, 4, 7, 5, 8).reshape(B, G, hs, S)


# ------------------------------------------------------------------------------------------ training backward
def dropout(x: torch.Tensor, p: float, seed: int, call_id: int, step: Optional[torch.Tensor] = None):
    """(bf16(x * m), m): LoRA-branch dropout with the mask drawn in the kernel (Philox keyed by seed / call_id, counted by the
    device counter `step` — an int64 tensor of one element — and the element index); dh_dropout_bf16."""
    x = _dev(x, name="x")
    y, m = torch.empty_like(x), torch.empty_like(x)
    check(_lib.load().dh_dropout_bf16(_p(x), _p(y), _p(m), x.numel(), float(p), int(seed) & (2 ** 64 - 1), int(call_id) & 0xffffffff,
                                      _p(step) if step is not None else None, _stream()))
    return y, m


def swiglu_fwd(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    k = _Keep()
    act = torch.empty_like(g)
    check(_lib.load().dh_swiglu_fwd_bf16(k(g), k(u), _p(act), g.numel(), _stream()))
    return act


def linear_swiglu_train(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """-> (act, g, u): the training forward of fc_1 / fc_2 (ger/model.py:313-315) in one GEMM launch that also keeps the rounded
    pre-activations for the backward; the bits of linear(x, w1), linear(x, w2), swiglu_fwd(g, u)."""
    k = _Keep()
    M, K = x.shape
    I = w1.size(0)
    oa, og, ou = out if out is not None else (None, None, None)       # `out`: caller-owned (act, g, u)
    act = _out(oa, (M, I), torch.bfloat16, x.device, "out[0]")
    g, u = _out(og, (M, I), torch.bfloat16, x.device, "out[1]"), _out(ou, (M, I), torch.bfloat16, x.device, "out[2]")
    check(_lib.load().dh_linear_swiglu_train_bf16(k(x), k(w1), k(w2), _p(act), _p(g), _p(u), M, I, K, _stream()))
    return act, g, u


def linear_mul(x: torch.Tensor, w: torch.Tensor, mul: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16(bf16(x @ w.T) * mul): the multiply inside the GEMM's epilogue for large shapes (dh_linear_mul_bf16), else linear then *."""
    M, K = x.shape
    N = w.size(0)
    if (M >= 256 and N >= 256 and -(-M // 256) * -(-N // 256) >= 128 and mul.is_contiguous() and mul.shape == (M, N)
            and not os.environ.get("DUALHYP_NO_LINEAR_MUL")):        # (the variable: same-box A/B of the fused multiply)
        k = _Keep()
        y = _out(out, (M, N), torch.bfloat16, x.device)
        check(_lib.load().dh_linear_mul_bf16(k(x), k(w), _p(y), M, N, K, k(mul), _stream()))
        return y
    if out is not None:
        return torch.mul(linear(x, w), mul, out=_out(out, (M, N), torch.bfloat16, x.device))
    return linear(x, w) * mul


def swiglu_bwd(dact: torch.Tensor, g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    k = _Keep()
    rows, I = g.shape
    out = torch.empty((rows, 2 * I), dtype=torch.bfloat16, device=g.device)
    check(_lib.load().dh_swiglu_bwd_bf16(k(dact), k(g), k(u), _p(out), rows, I, _stream()))
    return out


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, dres: Optional[torch.Tensor] = None) -> torch.Tensor:
    k = _Keep()
    d = x.size(-1)
    dx = torch.empty_like(x)
    check(_lib.load().dh_rmsnorm_bwd_bf16(k(dy), k(x), k(w), k(dres, name="dres"), _p(dx), x.numel() // d, d,
                                          float(eps), _stream()))
    return dx


def qkv_rope_bwd(dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 tok_pos: torch.Tensor) -> torch.Tensor:
    k = _Keep()
    n_tok, n_head, hs = dq.shape
    n_groups = dk.size(1)
    out = torch.empty((n_tok, (n_head + 2 * n_groups) * hs), dtype=torch.bfloat16, device=dq.device)
    check(_lib.load().dh_qkv_rope_bwd_bf16(k(dq), k(dk), k(dv), k(cos), k(sin),
                                           k(tok_pos, torch.int32), _p(out), n_tok, n_head, n_groups, hs, _stream()))
    return out


def tn_accum(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, scale: float = 1.0, accumulate: bool = True,
             splits: Optional[Tuple[int, int]] = None) -> None:
    """out[M,N] (+)= scale * a[T,M].T @ b[T,N]; a/b may be column slices of wider row-major matrices.
    splits = (s0, s1): out[M,16], rows m of segment seg(m) = (m >= s0) + (m >= s1) contract with b[:, 16 seg : 16 seg + 16]."""
    assert a.stride(1) == 1 and b.stride(1) == 1 and out.dtype == torch.float32 and out.stride(1) == 1
    T, M = a.shape
    N = b.size(1) if splits is None else 16
    lib = _lib.load()
    wb = lib.dh_tn_accum_work_bytes(T, M, N)       # packed micro-batches: the token loop is split over the grid
    work = torch.empty(wb // 4, dtype=torch.float32, device=a.device) if wb else None
    if splits is not None:
        check(lib.dh_tn_accum_seg_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
                                      T, M, int(splits[0]), int(splits[1]), float(scale), int(accumulate), _p(work), _stream()))
        return
    check(lib.dh_tn_accum_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
                              T, M, N, float(scale), int(accumulate), _p(work), _stream()))


def attn_bwd_plan(q_start: torch.Tensor, q_len: torch.Tensor, n_tok: int, lens: Sequence[int]) -> dict:
    """Index tensors of the padded, fragment-ordered copies dh_attn_bwd_bf16 reads — the same for every layer of a micro-step, so the
    training step builds them once: pad_start[i] (sequence i starts at a multiple of 32), n_pad, and the inverse map
    pad_tok[p] = token of padded position p (-1 = padding)."""
    dev = q_len.device
    n_pad = sum(-(-n // 32) * 32 for n in lens)
    pads_dev = (q_len + 31) // 32 * 32
    pad_start = (torch.cumsum(pads_dev, 0) - pads_dev).to(torch.int32)
    tok_seq = torch.repeat_interleave(torch.arange(len(lens), dtype=torch.int64, device=dev), q_len.to(torch.int64), output_size=n_tok)
    tok = torch.arange(n_tok, dtype=torch.int64, device=dev)
    pp = pad_start.to(torch.int64)[tok_seq] + (tok - q_start.to(torch.int64)[tok_seq])
    pad_tok = torch.full((n_pad,), -1, dtype=torch.int32, device=dev)
    pad_tok[pp] = tok.to(torch.int32)
    return {"n_pad": n_pad, "pad_start": pad_start, "pad_tok": pad_tok, "n_seq": len(lens)}


def attn_bwd(q, k, v, out, dout, lse, q_start, q_len, max_q_len: int, lens: Optional[Sequence[int]] = None, plan: Optional[dict] = None):
    """-> (dq, dk, dv) of the causal GQA attention of a packed batch (sequences attend to themselves).
    `lens` = q_len on the host; when given nothing here touches the host (hipGraph capture of a training step).
    `plan` = attn_bwd_plan(...) of the same batch (built once per micro-step by the caller; built here when absent)."""
    keep = _Keep()
    n_tok, H, hs = q.shape
    G = k.size(1)
    lib = _lib.load()
    dev = q.device
    if plan is None:
        if lens is None:
            lens = q_len.tolist()
        plan = attn_bwd_plan(q_start, q_len, n_tok, lens)
    n_pad, pad_start, pad_tok = plan["n_pad"], plan["pad_start"], plan["pad_tok"]
    dout = _dev(dout.reshape(n_tok, H, hs))
    dsum = torch.empty((n_tok, H), dtype=torch.float32, device=dev)
    check(lib.dh_rowdot_f32(_p(dout), keep(out.reshape(n_tok, H, hs)), _p(dsum), n_tok * H, hs, _stream()))

    def tpad(src, heads):
        dst = torch.empty((heads, hs, n_pad), dtype=torch.bfloat16, device=dev)      # padding is written (zeros) by the kernel
        check(lib.dh_transpose_frag_bf16(keep(src), _p(dst), _p(pad_tok), heads, hs, n_pad, _stream()))
        return dst
    need = lib.dh_attn_bwd_transposes(H, G, hs, n_pad)      # hs 64: the dk/dv kernel transposes its q / dO tiles in LDS
    qT, doT = (tpad(q, H), tpad(dout, H)) if need & 1 else (None, None)
    kT = tpad(k, G)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(lib.dh_attn_bwd_bf16(keep(q, name="q"), keep(k, name="k"), keep(v, name="v"), _p(dout), _p(qT), _p(doT), _p(kT), _p(lse), _p(dsum), _p(q_start),
                               _p(q_len), _p(pad_start), _p(dq), _p(dk), _p(dv), plan["n_seq"], int(max_q_len), H, G, hs,
                               n_pad, _stream()))
    return dq, dk, dv
