"""The decode loop of the reference (generate/base.py:19-82), batched and kept on the device.

`generate()` has the reference's signature and semantics for one prompt (EOS excluded from the
result, quirk Q7; `top_k=1` is a deterministic lowest-index arg-max instead of a sampled tie
break, quirk Q6).  `generate_batch()` runs many ragged prompts at once — equal to running each
alone — with one packed prefill and one hipGraph launch per generated token; the host reads the
device state back once at the end instead of once per token (generate/base.py:79).
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import List, Optional, Sequence, Union

import torch

from . import automaton as _automaton
from . import beam as _beam
from . import bias as _bias
from . import constrain as _constrain
from . import ngram as _ngram
from . import nucleus as _nucleus
from . import penalty as _penalty
from . import ops
from . import stop as _stop
from .gpt import GPT
from .schedule import shared_prefix_len
from .speculate import check_arguments as _check_speculate, check_verify as _check_verify


EOS_CHECK_EVERY = 16     # decode steps between two "has every sequence finished" read-backs (generate_batch with an eos_id)


def _shared_prefix(model: GPT, prompts: Sequence[torch.Tensor], share_prefix: Union[bool, str], dev) -> int:
    """P of a call: the leading tokens forwarded once for all of its prompts (schedule.shared_prefix_len), 0 = each prompt whole.
    share_prefix False: 0.  True: P, or an error where sharing would change bits.  "auto": P, or 0 there."""
    if share_prefix is False:
        return 0
    if share_prefix is not True and share_prefix != "auto":
        raise ValueError(f"share_prefix is False, True or 'auto', not {share_prefix!r}")
    from .relprompt import GPT as RelGPT
    why = None
    if model.cpu_rsqrt_vec_width != 0:
        # dh_engine_set_cpu_rsqrt_emulation(whole_call=0): the rsqrt tail rows are the last len % width rows of a sequence within
        # its own forward, so a prompt forwarded in two pieces has other tail rows than the prompt forwarded whole
        why = "cpu_rsqrt_vec_width != 0 flags rows by their index within a call; a prompt split at the prefix would move them"
    elif isinstance(model, RelGPT):
        why = "the RelPrompt decoder's prompts carry spliced reliability embeddings"
    if why is not None:
        if share_prefix is True:
            raise ValueError(f"share_prefix=True: {why} (share_prefix='auto' runs such a call unshared)")
        return 0
    return shared_prefix_len([p.to(dev).reshape(-1) for p in prompts])


def _token_mask(model: GPT, token_mask, n: int, need: int, dev) -> Optional[torch.Tensor]:
    """The call's token mask on the device, checked before anything is launched (constrain.check_mask: one read-back), or None.
    token_mask: an int32 [n, ceil(vocab / 32)] tensor on the model's device, or a list of n id lists, packed here."""
    if token_mask is None:
        return None
    vocab = model.config.padded_vocab_size
    if not isinstance(token_mask, torch.Tensor):
        if len(token_mask) != n:
            raise ValueError(f"token_mask holds {len(token_mask)} id lists for {n} prompts")
        token_mask = _constrain.pack_mask(token_mask, vocab, dev)
    return _constrain.check_mask(token_mask, n, vocab, need, device=dev)


def _top_buffers(shape, K: int, dev):
    """The alternatives' buffers beside a token buffer of `shape`: ids -1 and values NaN where no token was produced."""
    return (torch.full(tuple(shape) + (K,), -1, dtype=torch.int32, device=dev),
            torch.full(tuple(shape) + (K,), float("nan"), dtype=torch.float32, device=dev))


def _forward_prefix(eng, prompt: torch.Tensor, P: int, slot: int, other_slots: Sequence[int]) -> None:
    """The call's first P tokens through the layers once, into KV slot `slot` (a prompt-phase forward, no logits), and their K / V
    of every layer from there into other_slots."""
    eng.forward(prompt[:P].to(eng.device), [P], [0], want_all=False, want_last=False, slot_base=slot)
    if other_slots:
        eng.copy_prefix(slot, list(other_slots), P)


def _check_penalties(repetition_penalty, frequency_penalty, presence_penalty, speculate: int = 0):
    """The checked (repetition, frequency, presence) of a call, or None when all three are off.  Needs nothing but the arguments."""
    pen = _penalty.check_penalties(repetition_penalty, frequency_penalty, presence_penalty)
    if not _penalty.penalties_on(*pen):
        return None
    if speculate:
        raise ValueError(f"speculate={speculate} does not go with penalties (repetition={pen[0]}, frequency={pen[1]}, presence={pen[2]}): "
                         "a verify position's history would have to include the picks of its own step")
    return pen


def _check_bias(bias, speculate: int = 0):
    """`bias=` looked at before the model is touched: its type, and what it does not go with.  Needs nothing but the arguments; the
    entries themselves are checked against the model's vocabulary by bias.as_spec."""
    if bias is None or (isinstance(bias, (list, tuple)) and len(bias) == 0):
        return None
    if not isinstance(bias, (_bias.BiasSpec, list, tuple)):
        raise TypeError(f"bias is a compiled specification (dualhyp_amd.bias.compile_bias) or a list of (ids, boost) pairs, not {bias!r}")
    if speculate:
        raise ValueError(f"speculate={speculate} does not go with a bias of {len(bias)} entries: {_bias.SPEC_REFUSAL}")
    return bias


def _check_automaton(automaton, speculate: int = 0):
    """`automaton=` looked at before the model is touched: its type, and what it does not go with.  Needs nothing but the arguments; the
    set is checked against the call (sequences, vocabulary, eos_id) by _automaton.as_set."""
    if automaton is None:
        return None
    if not isinstance(automaton, _automaton.AutomatonSet):
        raise TypeError(f"automaton is a dualhyp_amd.automaton.AutomatonSet (from_sequences, from_prompts), not {automaton!r}")
    if speculate:
        raise ValueError(f"speculate={speculate} does not go with an automaton of {automaton.n_states} states: {_automaton.SPEC_REFUSAL}")
    return automaton


@contextlib.contextmanager
def _engine_settings(settings, take_back=None):
    """What a call hands the engine for its captured decode steps, and takes back behind them: the buffers are the call's.  settings:
    (on, set, reset) triples, set in their order and reset in take_back's (None: the same), each only where the call uses it — every
    one is part of a captured step's key, so without it the call runs the steps it always ran."""
    try:
        for on, set_, _ in settings:      # a setter that refuses leaves nothing set: the ones before it are taken back below
            if on:
                set_()
        yield
    finally:
        for on, _, reset in settings if take_back is None else take_back:
            if on:
                reset()


def _shared_prompt_setting(eng, on: bool, rows_per_utt: int, plen: torch.Tensor):
    """Shared-prompt attention for the decode steps of a call, as an entry of _engine_settings."""
    return on, lambda: eng.set_shared_prompt(rows_per_utt, plen), lambda: eng.set_shared_prompt()


@dataclasses.dataclass
class _Picks:
    """The pick options of one call, in one place for its three consumers: the first pick (kw), the captured decode steps (engine) and
    the returned state (state).  check() builds it from the arguments alone; compile() puts the model and the call's shape to it."""
    want_logprobs: bool
    K: int                                  # top_logprobs
    mask: object                            # token_mask as given; compiled: the int32 mask, a row per decode row, or None
    ngram: int
    stop: object                            # as given; compiled: a StopSpec on the device, or None
    top_p: float
    min_p: float
    pen: Optional[tuple]                    # (repetition, frequency, presence), None: all three off
    bias: object                            # as given; compiled: a BiasSpec on the device, or None
    aut: object                             # as given; compiled: the AutomatonSet on the device, a start state per decode row, or None
    lp_buf: Optional[torch.Tensor] = None   # compile(): float32 [rows, tok_ld] beside the token buffer, NaN where no token was produced
    top_buf: Optional[tuple] = None         # compile(): _top_buffers
    start: Optional[torch.Tensor] = None    # compile(): the rows' prompt lengths, where an option reads a row's generated text

    @classmethod
    def check(cls, *, speculate: int = 0, verify: str = "argmax", return_logprobs: bool = False, top_logprobs: int = 0, token_mask=None, no_repeat_ngram: int = 0,
              stop=None, top_p=None, min_p=None, repetition_penalty=None, frequency_penalty=None, presence_penalty=None, bias=None,
              automaton=None) -> "_Picks":
        """Stage one: what the arguments alone decide, refused before the model is touched.  verify="draw": a verify step forms every
        position's history itself, so the three readers of a row's generated text go with speculate."""
        if _check_verify(verify, speculate):
            speculate = 0
        pen = _check_penalties(repetition_penalty, frequency_penalty, presence_penalty, speculate)
        bias = _check_bias(bias, speculate)
        automaton = _check_automaton(automaton, speculate)
        top_p, min_p = _nucleus.check_nucleus(top_p, min_p)
        K = ops.check_top_logprobs(top_logprobs)
        if K and not return_logprobs:
            raise ValueError(f"top_logprobs={K} needs return_logprobs=True: the alternatives are returned beside the tokens' own log-probabilities")
        return cls(bool(return_logprobs), K, token_mask, _ngram.check_ngram(no_repeat_ngram), stop, top_p, min_p, pen, bias, automaton)

    def compile(self, model: GPT, lens: Sequence[int], tok_ld: int, dev, eos_id, repeat: int = 1, dummy: bool = False) -> "_Picks":
        """Stage two: the options checked against the model and compiled for the call's len(lens) sequences, and the buffers of its
        decode rows — `repeat` rows per sequence (sample_batch's candidates), and with `dummy` one row more, generate_stream's dummy
        sequence of one token, which never picks."""
        n = len(lens)
        # only an option that is on asks the model for its vocabulary; token_mask asks in _token_mask
        uses_vocab = self.K or self.ngram or self.pen or any(o is not None for o in (self.bias, self.aut, self.stop))
        vocab = model.config.padded_vocab_size if uses_vocab else None
        if self.K:
            ops.check_top_logprobs(self.K, vocab)
        if self.ngram:
            _ngram.check_ngram(self.ngram, vocab)
        if self.pen:
            _penalty.check_history(tok_ld, vocab)
        self.bias = _bias.as_spec(self.bias, vocab, dev)
        if self.bias is not None and self.pen:
            _bias.check_tables(tok_ld, self.bias.n_ids)
        self.aut = _automaton.as_set(self.aut, n, vocab, dev, eos_id)
        self.mask = _token_mask(model, self.mask, n, 1, dev)
        self.stop = _stop.as_spec(self.stop, vocab, dev)
        if self.aut is not None and (repeat > 1 or dummy):
            # a start state and a state per decode row; the dummy's is valid, and a refilled row starts over by itself: its sequence
            # has generated nothing, so its pick reads the start state
            self.aut = self.aut.padded() if dummy else self.aut.repeat(repeat)
        if self.mask is not None and repeat > 1:
            self.mask = self.mask.repeat_interleave(repeat, dim=0).contiguous()
        if self.mask is not None and dummy:     # an all-ones row
            self.mask = torch.cat([self.mask, torch.full_like(self.mask[:1], -1)]).contiguous()
        row_lens = [t for t in lens for _ in range(repeat)] + [1] * dummy
        if self.want_logprobs:
            self.lp_buf = torch.full((len(row_lens), tok_ld), float("nan"), dtype=torch.float32, device=dev)
        if self.K:
            self.top_buf = _top_buffers((len(row_lens), tok_ld), self.K, dev)
        # the ban's and the penalties' history, and a stop sequence's, a bias entry's or the automaton's text, begin behind the prompt
        if self.ngram or self.pen or self.bias is not None or self.aut is not None or (self.stop is not None and self.stop.sequences):
            self.start = torch.tensor(row_lens, dtype=torch.int32, device=dev)
        return self

    def kw(self) -> dict:
        """The keywords of the call's first picks (ops.sample, ops.sample_rows)."""
        pen = self.pen or (None, None, None)
        return dict(logprobs=self.lp_buf, top_logprobs=self.top_buf, mask=self.mask, no_repeat_ngram=self.ngram, start=self.start,
                    stop=self.stop, top_p=self.top_p, min_p=self.min_p, repetition_penalty=pen[0], frequency_penalty=pen[1],
                    presence_penalty=pen[2], bias=self.bias, automaton=self.aut)

    def engine(self, eng, inner=()):
        """The same options on the engine for the captured steps inside the `with` (_engine_settings), and `inner`, further settings
        of the call, inside them.  The three readers of a row's generated text are taken back first, then the others in the order
        they were set."""
        plain = [(self.lp_buf is not None, lambda: eng.set_logprobs(self.lp_buf), lambda: eng.set_logprobs(None)),
                 (self.top_buf is not None, lambda: eng.set_top_logprobs(*self.top_buf), lambda: eng.set_top_logprobs(None)),
                 (self.mask is not None, lambda: eng.set_token_mask(self.mask), lambda: eng.set_token_mask(None)),
                 (self.ngram, lambda: eng.set_no_repeat_ngram(self.ngram, self.start), lambda: eng.set_no_repeat_ngram(0)),
                 (self.stop is not None, lambda: eng.set_stop(self.stop, self.start), lambda: eng.set_stop(None)),
                 (self.top_p < 1.0 or self.min_p > 0.0, lambda: eng.set_nucleus(self.top_p, self.min_p), lambda: eng.set_nucleus(None, None))]
        text = [(self.pen, lambda: eng.set_penalties(*self.pen, start=self.start), lambda: eng.set_penalties()),
                (self.bias is not None, lambda: eng.set_bias(self.bias, self.start), lambda: eng.set_bias()),
                (self.aut is not None, lambda: eng.set_automaton(self.aut, self.start), lambda: eng.set_automaton())]
        inner = list(inner)
        return _engine_settings(plain + text + inner, inner[::-1] + text[::-1] + plain)

    def state(self, n: Optional[int] = None) -> dict:
        """The entries of a return_state dict: the call's buffers, or their first n rows."""
        rows = (lambda t: t) if n is None else (lambda t: t[:n])
        st = {}
        if self.lp_buf is not None:
            st["logprobs"] = rows(self.lp_buf)
        if self.top_buf is not None:
            st["top_ids"], st["top_logprobs"] = rows(self.top_buf[0]), rows(self.top_buf[1])
        if self.aut is not None:
            st["automaton_state"] = rows(self.aut.state)
        return st


def _prompt_shape(model: GPT, prompts: Sequence[torch.Tensor], max_new_tokens: int, prefill_batch: int):
    """(lens, T_max, need_pos, chunks) of a call: the prompt lengths, the longest, the last position a sequence writes, and the
    (first, behind-last) prompt indices of its prefills of prefill_batch prompts."""
    lens = [int(p.numel()) for p in prompts]
    T_max = max(lens)
    need_pos = T_max + max_new_tokens - 1
    if model.max_seq_length < need_pos:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {need_pos}")
    return lens, T_max, need_pos, [(c, min(c + prefill_batch, len(lens))) for c in range(0, len(lens), prefill_batch)]


def _prefill(eng, prompts, lens, chunks, P: int, slots: Sequence[int], dev, whole=None) -> torch.Tensor:
    """The prompts into KV slots `slots`, a chunk at a time, behind their P shared tokens, which go through the layers once: the
    last-position logits, bf16 [len(prompts), vocab].  whole(packed, a, b): how the call forwards a chunk of prompts that share
    nothing (None: by forward_slots, as it forwards what follows a prefix)."""
    last = torch.empty((len(prompts), eng.vocab), dtype=torch.bfloat16, device=dev)
    if P:
        _forward_prefix(eng, prompts[0], P, slots[0], slots[1:])
    for a, b in chunks:
        packed = torch.cat([p.to(dev).reshape(-1)[P:] for p in prompts[a:b]])
        if P or whole is None:      # prompt_phase: a chunk of one-token remainders is still a piece of a prompt forward, not a decode step
            last[a:b] = eng.forward_slots(packed, [n - P for n in lens[a:b]], slots[a:b], prompt_phase=bool(P), pos0=P)
        else:
            last[a:b] = whole(packed, a, b)
    return last


def _decode(eng, picks: _Picks, step, done: torch.Tensor, n: int, early: bool, inner=()) -> int:
    """The decode phase of a call: n steps under the call's settings, issued by step(count, first_step); the steps issued.  early (an
    EOS or a stop specification can end a sequence, or a verify step yields several tokens): issued EOS_CHECK_EVERY at a time, until
    every sequence has finished (generate/base.py:79-80 returns at the EOS; the harness asks for up to 150 tokens,
    inference/ger.py:71, and a correction is usually 20-40): one 4-byte read-back per chunk instead of up to 5x the steps."""
    steps_run = 0
    with picks.engine(eng, inner):
        while steps_run < n:
            c = min(EOS_CHECK_EVERY, n - steps_run) if early else n
            step(c, steps_run)
            steps_run += c
            if steps_run < n and bool((done != 0).all()):
                break
    return steps_run


def _add_timing(timing: dict, **amounts) -> None:
    """The amounts of one call onto the keys of a timing dict that several calls share."""
    for key, v in amounts.items():
        timing[key] = timing.get(key, 0) + v


def _row_result(r: int, n_prompt: int, length_h, done_h, max_new_tokens: int, tokens, lp_buf, top_buf, lo: int = 0):
    """Row r of a finished call out of its buffers, as views (640 clone launches per 20-batch group otherwise): its tokens from place
    `lo`, cut before an EOS (generate/base.py:80 returns idx[:input_pos]), and what was produced, the EOS included — the
    log-probabilities and the alternatives, None where the call keeps none (lp_buf, top_buf None)."""
    end = min(length_h[r], n_prompt + max_new_tokens)
    return (tokens[r, lo:end - 1 if done_h[r] == 1 else end], None if lp_buf is None else lp_buf[r, n_prompt:end],
            None if top_buf is None else tuple(t[r, n_prompt:end] for t in top_buf))


def _batch_result(rows, picks: _Picks, state: Optional[dict]):
    """generate_batch's return value from its rows' results: out, or (out[, logprobs][, top][, state])."""
    out, logprobs, top = (list(col) for col in zip(*rows))
    res = (out,) + ((logprobs,) if picks.lp_buf is not None else ()) + ((top,) if picks.top_buf is not None else ())
    if state is not None:
        res += (state,)
    return res if len(res) > 1 else out


def _token_buffer(prompts, lens, tok_ld: int, dev) -> torch.Tensor:
    """[len(prompts), tok_ld] int64: every prompt at the start of its row, zeros behind."""
    T_max = max(lens)
    if min(lens) == T_max:             # equal lengths: one copy
        tokens = torch.nn.functional.pad(torch.stack([p.to(dev) for p in prompts]), (0, tok_ld - T_max))
    else:                              # ragged: right-pad with 0 (pad_sequence), then out to the buffer width
        tokens = torch.nn.utils.rnn.pad_sequence([p.to(dev) for p in prompts], batch_first=True)
        tokens = torch.nn.functional.pad(tokens, (0, tok_ld - tokens.size(1)))
    return tokens.contiguous()


@torch.inference_mode()
def generate_batch(model: GPT, prompts: Sequence[torch.Tensor], max_new_tokens: int, *, temperature: float = 1.0,
                   top_k: Optional[int] = None, eos_id: Optional[int] = None, seed: int = 1337,
                   return_state: bool = False, prefill_batch: int = 32, timing: Optional[dict] = None,
                   share_prefix: Union[bool, str] = False, speculate: int = 0, drafts: Optional[torch.Tensor] = None,
                   return_logprobs: bool = False, top_logprobs: int = 0, token_mask=None, no_repeat_ngram: int = 0,
                   stop=None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                   repetition_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                   presence_penalty: Optional[float] = None, bias=None, automaton=None, verify: str = "argmax"):
    """prompts: 1-D int64 tensors (any lengths).  Returns a list of 1-D tensors prompt+generated,
    cut before the EOS token when one was produced.

    More than `prefill_batch` prompts are prefilled `prefill_batch` at a time (each prefill is
    MFMA-bound and fills the chip on its own) into consecutive KV-cache slots of one engine and then
    decoded TOGETHER: a decode step streams the weights once for all rows (up to 256 rows take the
    streaming kernels), which is where the time of a small-batch decode goes.  A sequence's tokens do
    not depend on how many others ride along (every kernel's per-row summation order is fixed by the
    phase, not by the packing); only the multinomial draw is keyed by the row index in the call.

    share_prefix (True, or "auto": only where it changes no bit): the P leading tokens every prompt of the call opens with
    (whole 32-token tiles, each prompt keeping a token of its own) go through the layers once, their K / V are copied into
    every slot (dh_engine_copy_prefix), and the prefill forwards each prompt's tokens [P:] at position P.  Same ids.

    speculate=D (1..7, top_k=1 only): a decode step verifies D drafted tokens per sequence next to its last one and appends those
    the arg-max confirms plus one (dh_engine_decode_spec) — the same ids as speculate=0, bit for bit, in fewer steps where the
    drafts are right.  drafts None: drafted by prompt lookup (speculate.propose); a [B, max_new_tokens] int64 tensor: drafts[u, i]
    is proposed as the i-th generated token of sequence u (a scripted proposer for tests and tools/bench_speculate.py).
    timing gains spec_steps (verify steps until the last sequence finished), spec_drafted and spec_accepted.

    verify ("argmax", the default: everything above and every refusal below; or "draw", with speculate > 0; include/dualhyp_hip.h,
    "Sampled verification"): a verify position picks as the plain step of this call would pick the token at its place — top_k, the
    draw keyed by (seed, tokens generated so far, sequence), top_p / min_p, and the penalties, the bias, the no-repeat ban and the
    automaton on a history that includes the picks of the same step — and a draft is kept exactly when it equals that pick
    (dh_engine_decode_spec_draw).  The ids, log-probabilities, alternatives, done flags and automaton states are those of the same
    call with speculate=0, bit for bit, whatever is drafted.  It opens speculate to any top_k (top_k=1 is the arg-max verification)
    and to top_p, min_p, the three penalties, bias and automaton, beside what speculate already goes with.  fp8 / MXFP4 and RelPrompt
    models, the CPU rsqrt emulation and generate_stream stay refused.

    return_logprobs: the call returns (out, logprobs[, state]); logprobs[i] is a 1-D float32 tensor with the log-probability of every
    token the model produced for sequence i, in order, the EOS token's last when the sequence ended on one (so its length is
    len(out[i]) - len(prompts[i]), plus 1 behind an EOS).  It is log softmax of the raw logits row the token was picked from
    (temperature 1, no top-k crop: the model's distribution, whatever the call samples with; include/dualhyp_hip.h, "Token
    log-probabilities"), written by the sampling kernels into a NaN-filled float32 buffer beside the token buffer
    (state["logprobs"]): the first token's by the prefill's sample call, the others inside the captured decode steps.  Ids, steps
    and read-backs are those of the call without the flag; the values do not depend on the schedule (speculate, share_prefix,
    generate_stream).

    top_logprobs=K (1..8, with return_logprobs): the call returns (out, logprobs, top[, state]); top[i] = (ids [n_i, K] int32,
    lp [n_i, K] float32), aligned with logprobs[i]: at every produced token, the EOS included, the K most probable tokens of the
    raw logits row it was picked from — by value descending, then by index ascending (-0 == +0) — and their log-probabilities by
    the definition above, sharing its m and its sum (include/dualhyp_hip.h, "Token alternatives").  Written by the same kernels
    into [B, tok_ld, K] buffers filled with -1 / NaN (state["top_ids"], state["top_logprobs"]).  Ids, logprobs, steps and
    read-backs are those of the call without it.

    token_mask (constrained decoding; include/dualhyp_hip.h, "Token masks"): an int32 [B, ceil(vocab / 32)] tensor on the model's
    device (constrain.pack_mask), or a list of B id lists that is packed here — sequence i produces only ids that row i allows
    (allow the EOS if the sequence is to end on it), as if every other logit were -inf, with whatever sampler the call uses.  Every
    row allows at least one id (checked with one read-back before anything is launched).  The pick happens inside the sampling
    kernels — the prefill's first pick and every captured decode or verify step — and the log-probabilities and alternatives stay
    the raw row's.  It goes with speculate, share_prefix, return_logprobs and top_logprobs, none of which it touches.

    no_repeat_ngram=n (1..8; include/dualhyp_hip.h, "No-repeat n-grams"): a sequence never produces a token that would complete an
    n-gram its GENERATED text already holds (the prompt's n-grams stay free: a correction copies its prompt) — as if the logit were
    -inf, with whatever sampler the call uses, and on top of token_mask; where that would leave nothing to pick, the ban is ignored
    for the step.  The ban set is built inside the sampling kernels from the token buffer, per sequence and step, with no launch or
    read-back of its own; the first pick of a prompt is unaffected, and log-probabilities and alternatives stay the raw row's.  It
    goes with token_mask, speculate (a banned draft is simply not confirmed), share_prefix, return_logprobs and top_logprobs, and
    with fp8 weights and an fp8 KV cache.  0 (the default): the call it always was.

    stop (include/dualhyp_hip.h, "Stop conditions"): a compiled specification (stop.compile_stop), or a list whose ints are stop ids
    and whose lists are stop sequences of 2..8 ids (at most 8 of them).  A sequence ends, with done = 3 in the returned state, right
    behind the first token it GENERATES that is a stop id or completes a stop sequence (a match never reaches into the prompt); that
    token is an ordinary produced token and stays in the result, with its log-probability and alternatives — only an EOS is cut.
    The EOS wins where both hold, and a stop on the last place of the budget is a stop.  The test sits behind the pick in the
    sampling kernels (the prefill's first pick and every captured decode or verify step) and never changes a pick: tokens,
    log-probabilities and alternatives are the unstopped call's up to and including that token, bit for bit, with every sampler.  What
    it saves are steps: the EOS_CHECK_EVERY loop runs whenever an EOS or a stop can end a sequence early.  It goes with speculate,
    share_prefix, return_logprobs, top_logprobs, token_mask, no_repeat_ngram and fp8.  None (the default): the call it always was.

    top_p (in (0, 1]) and min_p (in [0, 1]; include/dualhyp_hip.h, "Nucleus and min-p"): a sampled call (top_k != 1) draws from the
    entries top_k keeps, cropped to their nucleus — values from the best down until the mass above a value reaches top_p of the kept
    mass, the crossing value kept whole, ties together — and to the entries whose scaled logit is within log(min_p) of the best.  The
    crop is taken on the row the sampler uses, after temperature, token_mask and no_repeat_ngram, inside the sampling kernels: the
    prefill's first pick and every captured decode step, with no launch or read-back of its own.  Log-probabilities and alternatives
    stay the raw row's.  It goes with share_prefix, return_logprobs, top_logprobs, token_mask, no_repeat_ngram, stop and fp8; the
    arg-max (top_k = 1, and with it speculate) takes neither.  None, 1.0 and 0.0 (the defaults) are off: the call it always was.

    repetition_penalty (theta in [1/8, 8]), frequency_penalty and presence_penalty (alpha_f, alpha_p in [-8, 8]; include/dualhyp_hip.h,
    "Penalties"): a token the sequence has already GENERATED (the prompt stays free, as for no_repeat_ngram) becomes less likely, with
    whatever sampler the call uses, the arg-max included — the pick is the same call's pick on a copy of the logits row in which the
    column of every such id t, generated c_t times, holds bf16(((x < 0 ? x * theta : x / theta) - alpha_f * c_t) - alpha_p), each
    operation rounded to fp32.  The values are computed inside the sampling kernels from the token buffer, per sequence and step, with
    no launch or read-back of their own and without writing the logits; the first pick of a prompt is unaffected, a masked or banned
    column stays -inf, and log-probabilities and alternatives stay the raw row's.  It goes with share_prefix, return_logprobs,
    top_logprobs, token_mask, no_repeat_ngram, stop, top_p, min_p and fp8; speculate is refused, and the token buffer (the longest
    prompt plus max_new_tokens) may have at most 2048 places.  None, 1.0 and 0.0 (the defaults) are off: the call it always was.

    bias (a dualhyp_amd.bias.BiasSpec from compile_bias, or a list of (ids, boost) pairs: 1 .. 256 entries of 1 .. 8 token ids and a finite
    boost of either sign, shared by all prompts; include/dualhyp_hip.h, "Contextual biasing"): the continuations of the listed phrases
    become more (or less) likely, with whatever sampler the call uses, the arg-max included.  An entry proposes its id at depth k when the
    sequence's last k GENERATED tokens are the entry's first k (the prompt neither starts nor continues a match; depth 0, the first id,
    is always proposed); the pick is the same call's pick on a copy of the logits row in which every proposed id holds bf16(y + B), B
    the largest boost of its proposers and y the column's raw — or, where the id is in the penalised history, penalised — fp32 value.
    The columns are built inside the sampling kernels from the token buffer, per sequence and step, with no launch or read-back of their
    own and without writing the logits; a masked or banned column stays -inf, and log-probabilities and alternatives stay the raw
    row's.  It goes with share_prefix, return_logprobs, top_logprobs, token_mask, no_repeat_ngram, stop, top_p, min_p, the penalties
    (then the token buffer's places plus the entries' ids may be at most 2048) and fp8; speculate is refused.  None (the default) and
    an empty list are off: the call it always was.

    automaton (a dualhyp_amd.automaton.AutomatonSet with a start state per prompt — from_sequences, from_prompts; it needs an eos_id;
    include/dualhyp_hip.h, "Automaton constraints"): a sequential constraint, the general form of token_mask — sequence i produces only
    texts its automaton can follow.  At every pick the allowed ids are the tokens on the edges of the sequence's state (its start state
    while it has generated nothing), under token_mask as well; a state that may end the text has an edge on the eos_id, and a state left
    with nothing to pick ends the sequence with the EOS.  no_repeat_ngram, the penalties and the bias work on that row, with whatever
    sampler the call uses.  The row is built, and the state moved along the picked edge, inside the sampling kernels — the prefill's first
    pick and every captured decode step — with no launch or read-back of their own; log-probabilities and alternatives stay the raw
    row's.  It goes with share_prefix, return_logprobs, top_logprobs, token_mask, no_repeat_ngram, stop, top_p, min_p, the penalties, bias
    and fp8; speculate is refused.  return_state gains automaton_state, the int32 [B] states behind the last picks.  None (the default)
    is off: the call it always was."""
    picks = _Picks.check(speculate=speculate, verify=verify, return_logprobs=return_logprobs, top_logprobs=top_logprobs,
                         token_mask=token_mask, no_repeat_ngram=no_repeat_ngram, stop=stop, top_p=top_p, min_p=min_p,
                         repetition_penalty=repetition_penalty, frequency_penalty=frequency_penalty, presence_penalty=presence_penalty,
                         bias=bias, automaton=automaton)
    B = len(prompts)
    assert B > 0 and max_new_tokens > 0
    D = _check_speculate(model, speculate, top_k, B, verify)
    if drafts is not None and (D == 0 or drafts.dtype != torch.int64 or tuple(drafts.shape) != (B, max_new_tokens)):
        raise ValueError(f"drafts goes with speculate > 0 and is a [{B}, {max_new_tokens}] int64 tensor")
    lens, T_max, need_pos, chunks = _prompt_shape(model, prompts, max_new_tokens, prefill_batch)
    dev = model.transformer.wte.weight.device
    tok_ld = T_max + max_new_tokens
    picks.compile(model, lens, tok_ld, dev, eos_id)
    P = _shared_prefix(model, prompts, share_prefix, dev)
    # a verify step writes K / V up to D positions behind the last token (as far as the model has positions) and runs D + 1 rows per
    # sequence through the row workspaces; the cache keeps B slots
    spec_pos = min(need_pos + D, -(-model.config.block_size // 64) * 64)
    eng = model.engine(B, spec_pos, max(P, B * (D + 1) if D else 0, max(sum(lens[a:b]) - (b - a) * P for a, b in chunks)),
                       exact=B > prefill_batch)
    if D:
        eng.reserve_rows(B * (D + 1))
    tokens = _token_buffer(prompts, lens, tok_ld, dev)
    if D:   # lengths, flags and the three counters side by side: one read-back
        state = torch.cat([torch.tensor(lens, dtype=torch.int32), torch.zeros(B + 3, dtype=torch.int32)]).to(dev)
        length, done, counters = state[:B], state[B:2 * B], state[2 * B:]
        limit = torch.tensor([n + max_new_tokens for n in lens], dtype=torch.int32, device=dev)
        drafts = None if drafts is None else drafts.to(dev).contiguous()
    else:
        length = torch.tensor(lens, dtype=torch.int32, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev)
    eng.set_rsqrt_emulation(model.cpu_rsqrt_vec_width, whole_call=False)   # B independent batch-1 runs
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing is not None else None
    if ev:
        ev[0].record()
    last = _prefill(eng, prompts, lens, chunks, P, list(range(B)), dev,
                    whole=lambda packed, a, b: eng.forward(packed, lens[a:b], [0] * (b - a), want_all=False, want_last=True, slot_base=a)[1])
    ops.sample(last, tokens, length, done, temperature=temperature, top_k=top_k, eos_id=eos_id, seed=seed, step=0, **picks.kw())
    if ev:
        ev[1].record()
    if D and verify == "draw":
        step = lambda c, first: eng.decode_spec_draw(tokens, length, done, limit, max_new_tokens, D, drafts, counters, c, temperature,
                                                     top_k, eos_id, seed, first_step=first)
    elif D:   # a step yields 1 .. D + 1 tokens per live sequence, so at most max_new_tokens - 1 steps are needed
        step = lambda c, first: eng.decode_spec(tokens, length, done, limit, max_new_tokens, D, drafts, counters, c, temperature, eos_id,
                                                first_step=first)
    else:
        step = lambda c, first: eng.decode(tokens, length, done, c, temperature, top_k, eos_id, seed, first_step=first)
    steps_run = _decode(eng, picks, step, done, max_new_tokens - 1, early=bool(D) or eos_id is not None or picks.stop is not None)
    if ev:
        ev[2].record()
    model._cache_len = []  # slots now hold these sequences; a later cached forward must start at 0
    if D:
        state_h = state.tolist()        # the one host read-back
        length_h, done_h, counters_h = state_h[:B], state_h[B:2 * B], state_h[2 * B:]
    else:
        length_h = length.tolist()          # the one host read-back
        done_h = done.tolist()
    if ev:   # the read-back above has synchronised the stream
        _add_timing(timing, prefill_ms=ev[0].elapsed_time(ev[1]), decode_ms=ev[1].elapsed_time(ev[2]), decode_steps=steps_run,
                    decode_row_steps=B * steps_run, prefill_tokens=sum(lens) - (B - 1) * P)
        timing["shared_prefix"] = P
        if D:
            _add_timing(timing, spec_steps=counters_h[0], spec_drafted=counters_h[1], spec_accepted=counters_h[2])
    st = None
    if return_state:
        st = dict(tokens=tokens, length=length, done=done, **picks.state())
        if D and steps_run:             # the last verify step's drafts and the lengths they were proposed from
            st["spec_drafts"], st["spec_len"] = eng.read_spec(B, D)
    rows = [_row_result(i, lens[i], length_h, done_h, max_new_tokens, tokens, picks.lp_buf, picks.top_buf) for i in range(B)]
    return _batch_result(rows, picks, st)


def check_shared_prompt(model, shared_prompt, rows_per_utt: int, what: str) -> bool:
    """shared_prompt of a sample_batch / beam_search_batch call (`what`) whose utterances decode rows_per_utt rows each, or a ValueError
    with the reason the engine's setter would give (include/dualhyp_hip.h, dh_engine_set_shared_prompt)."""
    if not isinstance(shared_prompt, bool):
        raise ValueError(f"shared_prompt is True or False, not {shared_prompt!r}")
    if not shared_prompt:
        return False
    if not 2 <= rows_per_utt <= 8:
        raise ValueError(f"shared_prompt=True: {what} decodes {rows_per_utt} row per utterance; 2..8 rows share a prompt")
    if getattr(model, "fp8", False):
        raise ValueError(f"shared_prompt=True does not go with an fp8 or MXFP4 model: its decode step does not run the streaming layers "
                         "that launch the shared-prompt attention kernel")
    if getattr(model, "kv_cache_dtype", "bf16") != "bf16":
        raise ValueError("shared_prompt=True does not go with an fp8 KV cache: the kernel reads bf16 cache tiles")
    if getattr(model, "cpu_rsqrt_vec_width", 0):
        raise ValueError("shared_prompt=True does not go with the CPU rsqrt emulation (cpu_rsqrt_vec_width), which flags rows by their "
                         "place in a call")
    return True


MAX_SAMPLES = 8           # DH_MAX_SAMPLES: the slots dh_engine_fork_slots gives an utterance, its own included


def check_num_samples(num_samples) -> int:
    """N of a sample_batch call, or a ValueError."""
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 2 <= num_samples <= MAX_SAMPLES:
        raise ValueError(f"num_samples is the number of sampled candidates per utterance, an int in 2..{MAX_SAMPLES}, not {num_samples!r} "
                         "(one candidate is generate_batch's call)")
    return num_samples


@torch.inference_mode()
def sample_batch(model: GPT, prompts: Sequence[torch.Tensor], max_new_tokens: int, *, num_samples: int, temperature: float = 1.0,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None, seed: int = 1337,
                 eos_id: Optional[int] = None, prefill_batch: int = 32, share_prefix: Union[bool, str] = False, token_mask=None,
                 no_repeat_ngram: int = 0, stop=None, top_logprobs: int = 0, timing: Optional[dict] = None,
                 return_state: bool = False, speculate: int = 0, repetition_penalty: Optional[float] = None,
                 frequency_penalty: Optional[float] = None, presence_penalty: Optional[float] = None, bias=None, automaton=None,
                 shared_prompt: bool = False, verify: str = "argmax", drafts: Optional[torch.Tensor] = None):
    """num_samples = N (2..8) sampled candidates per prompt from ONE prefill of it (include/dualhyp_hip.h, "Sampled candidates").

    DEFINITION: sample j of utterance u is row u * N + j of generate_batch over [p for p in prompts for _ in range(N)] with the same
    keyword arguments and return_logprobs=True — the same ids, log-probabilities, alternatives and done flags, bit for bit.  It holds
    by construction: the draw is keyed by (seed, step, row); utterance u is prefilled into KV slot u * N (prefill_batch utterances at
    a time; with share_prefix the shared positions go into the source slots first) and one dh_engine_fork_slots launch copies every
    prompt's tiles into the N - 1 slots behind, the bytes a prefill of their own would have written, since a prefill row's bits do
    not depend on the rows beside it; the first pick is ops.sample on the last-position logits repeated N times per utterance; the
    decode steps are generate_batch's over B * N rows.  (A chunk of one-token prompts alone is forwarded by the single-token
    kernels, as generate_batch forwards it; the chunks here hold utterances, there rows.)

    token_mask: one row, or id list, per UTTERANCE, serving its N samples.  automaton: one start state per UTTERANCE — row u * N + j
    starts in utterance u's — and a state per row (return_state's automaton_state, B * N entries).  The other arguments are
    generate_batch's.

    Returns, per utterance, the list of its N samples in sample order, each a dict of
      tokens          1-D int64 CPU tensor, the generated ids, cut before the EOS as generate_batch cuts,
      token_logprobs  1-D float32 CPU tensor, one value per produced token, the EOS's included (generate_batch's return_logprobs),
      sum_logprob     their sum in double precision, as a float (NaN-free: every produced token has a value),
      avg_logprob     sum_logprob / max(1, the number of produced tokens),
      finish_reason   "eos", "length" or "stop" (dualhyp_amd.stop.finish_reasons of the row's done flag),
      top_logprobs    with top_logprobs=K: (ids [n, K] int32, values [n, K] float32) CPU tensors, generate_batch's.
    return_state: (that, the dict of the call's device state: tokens, length, done, logprobs[, top_ids, top_logprobs], B * N rows).

    shared_prompt: the decode steps' attention reads an utterance's whole 32-key prompt tiles once per block of its N rows, from
    slot u * N, where every row streamed its own copy (include/dualhyp_hip.h, "Shared-prompt attention") — the same bits, so the
    same everything; it goes with every other argument.  The fork still fills the copies.  False (the default): the launches the
    call always made.  Refused for fp8 / MXFP4 models, an fp8 KV cache and the CPU rsqrt emulation.

    timing gains generate_batch's keys, with prefill_tokens counting every prompt once, fork_ms: the fork launch between its own
    two events, inside prefill_ms, and shared_prompt.

    speculate=D with verify="draw" (generate_batch's; "Sampled verification" of the header): the decode steps are verify steps over
    the B * N rows behind the fork, each position drawing with its row's key, so the definition above holds unchanged — every sample,
    score and flag is the speculate=0 call's, in fewer steps where the drafts (prompt lookup on the row's own text, or `drafts`, a
    [B * N, max_new_tokens] int64 tensor) are right.  timing gains generate_batch's spec_* counters.  shared_prompt=True is refused
    with it: a verify step's rows are positions of one sequence, not rows of an utterance.

    Refused with a ValueError before anything is launched: num_samples outside 2..8; top_k == 1 (the arg-max gives N equal rows);
    speculate without verify="draw" (a verify step confirms drafts against the arg-max); RelPrompt models (their prompts carry spliced
    embeddings)."""
    N = check_num_samples(num_samples)
    if top_k is not None and int(top_k) == 1:
        raise ValueError(f"num_samples={N} does not go with top_k=1: the arg-max gives {N} equal rows; sample with top_k != 1")
    draw = _check_verify(verify, speculate)
    if speculate and not draw:
        raise ValueError(f"num_samples={N} does not go with speculate={speculate}: a verify step confirms drafts against the arg-max, "
                         "and sampled candidates are not greedy")
    from .relprompt import GPT as RelGPT
    if isinstance(model, RelGPT):
        raise ValueError(f"num_samples={N}: the RelPrompt decoder's prompts carry spliced reliability embeddings, which a prefill by "
                         "ids into the source slots does not hold")
    shared_prompt = check_shared_prompt(model, shared_prompt, N, f"num_samples={N}")
    if shared_prompt and speculate:
        raise ValueError(f"shared_prompt=True does not go with speculate={speculate}: a verify step's rows are positions of one sequence, "
                         "not rows of an utterance")
    picks = _Picks.check(speculate=speculate, verify=verify, return_logprobs=True, top_logprobs=top_logprobs, token_mask=token_mask, no_repeat_ngram=no_repeat_ngram, stop=stop,
                         top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty, frequency_penalty=frequency_penalty,
                         presence_penalty=presence_penalty, bias=bias, automaton=automaton)
    B = len(prompts)
    assert B > 0 and max_new_tokens > 0
    R = B * N
    D = _check_speculate(model, speculate, top_k, R, verify)
    if drafts is not None and (D == 0 or drafts.dtype != torch.int64 or tuple(drafts.shape) != (R, max_new_tokens)):
        raise ValueError(f"drafts goes with speculate > 0 and is a [{R}, {max_new_tokens}] int64 tensor")
    lens, T_max, need_pos, chunks = _prompt_shape(model, prompts, max_new_tokens, prefill_batch)
    dev = model.transformer.wte.weight.device
    tok_ld = T_max + max_new_tokens
    picks.compile(model, lens, tok_ld, dev, eos_id, repeat=N)       # a mask row and a start state per utterance, serving its N rows
    P = _shared_prefix(model, prompts, share_prefix, dev)
    # D: a verify step's positions and rows, as in generate_batch
    eng = model.engine(R, min(need_pos + D, -(-model.config.block_size // 64) * 64),
                       max(P, R * (D + 1) if D else R, max(sum(lens[a:b]) - (b - a) * P for a, b in chunks)), exact=R > prefill_batch)
    if D:
        eng.reserve_rows(R * (D + 1))
    row_lens = [n for n in lens for _ in range(N)]
    tokens = _token_buffer([p for p in prompts for _ in range(N)], row_lens, tok_ld, dev)
    length = torch.tensor(row_lens, dtype=torch.int32, device=dev)
    done = torch.zeros(R, dtype=torch.int32, device=dev)
    if D:
        counters = torch.zeros(3, dtype=torch.int32, device=dev)
        limit = torch.tensor([n + max_new_tokens for n in row_lens], dtype=torch.int32, device=dev)
        drafts = None if drafts is None else drafts.to(dev).contiguous()
    plen = torch.tensor(lens, dtype=torch.int32, device=dev)      # what the fork reads
    eng.set_rsqrt_emulation(model.cpu_rsqrt_vec_width, whole_call=False)   # independent batch-1 runs
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timing is not None else None
    if ev:
        ev[0].record()
    last = _prefill(eng, prompts, lens, chunks, P, [u * N for u in range(B)], dev)
    if ev:
        ev[3].record()
    # positions at or behind a prompt's end in its last tile are overwritten before causality lets anything read them
    eng.fork_slots(plen, N, T_max)
    if ev:
        ev[4].record()
    ops.sample(last.repeat_interleave(N, dim=0), tokens, length, done, temperature=temperature, top_k=top_k, eos_id=eos_id, seed=seed,
               step=0, **picks.kw())
    if ev:
        ev[1].record()
    if D:
        step = lambda c, first: eng.decode_spec_draw(tokens, length, done, limit, max_new_tokens, D, drafts, counters, c, temperature,
                                                     top_k, eos_id, seed, first_step=first)
    else:
        step = lambda c, first: eng.decode(tokens, length, done, c, temperature, top_k, eos_id, seed, first_step=first)
    steps_run = _decode(eng, picks, step, done, max_new_tokens - 1, early=bool(D) or eos_id is not None or picks.stop is not None,
                        inner=[_shared_prompt_setting(eng, shared_prompt, N, plen)])
    if ev:
        ev[2].record()
    model._cache_len = []  # slots now hold these sequences; a later cached forward must start at 0
    length_h = length.tolist()          # the read-back: lengths, flags, tokens and log-probabilities
    done_h = done.tolist()
    tokens_h, lp_h = tokens.cpu(), picks.lp_buf.cpu()
    top_h = tuple(t.cpu() for t in picks.top_buf) if picks.K else None
    if ev:   # the read-back above has synchronised the stream
        _add_timing(timing, prefill_ms=ev[0].elapsed_time(ev[1]), fork_ms=ev[3].elapsed_time(ev[4]), decode_ms=ev[1].elapsed_time(ev[2]),
                    decode_steps=steps_run, decode_row_steps=R * steps_run, prefill_tokens=sum(lens) - (B - 1) * P)
        timing["shared_prefix"] = P
        timing["shared_prompt"] = shared_prompt
        if D:
            _add_timing(timing, **dict(zip(("spec_steps", "spec_drafted", "spec_accepted"), counters.tolist())))
    reasons = _stop.finish_reasons(done_h)
    out = []
    for u in range(B):
        samples = []
        for r in range(u * N, (u + 1) * N):
            toks, lp, top = _row_result(r, lens[u], length_h, done_h, max_new_tokens, tokens_h, lp_h, top_h, lo=lens[u])
            total = float(lp.double().sum())
            smp = dict(tokens=toks, token_logprobs=lp, sum_logprob=total, avg_logprob=total / max(int(lp.numel()), 1),
                       finish_reason=reasons[r])
            if picks.K:
                smp["top_logprobs"] = top
            samples.append(smp)
        out.append(samples)
    if return_state:
        return out, dict(tokens=tokens, length=length, done=done, **picks.state())
    return out


@torch.inference_mode()
def beam_search_batch(model: GPT, prompts: Sequence[torch.Tensor], max_new_tokens: int, *, num_beams: int, eos_id: Optional[int] = None,
                      length_penalty: float = 1.0, prefill_batch: int = 32, timing: Optional[dict] = None, return_state: bool = False,
                      token_mask=None, no_repeat_ngram: int = 0, stop=None, bias=None, history: str = "host",
                      shared_prompt: bool = False, kv: str = "copy"):
    """Beam search over num_beams = W (1..4) hypotheses per prompt, exact by definition (include/dualhyp_hip.h, "Beam search";
    tests/beam_reference.py is the host model): result[i] is the ranked list of at most W hypotheses of prompt i, each a dict of
      tokens          1-D int64 CPU tensor, prompt + generated, cut before the EOS,
      token_logprobs  1-D float32 CPU tensor, one value per generated token, the EOS's included — generate_batch's return_logprobs,
      sum_logprob     the device's fp32 cumulative score (their sequential fp32 sum), as a float,
      finished        True when the hypothesis ended on the EOS or a stop id; False for a live beam that completed the pool at the budget,
      finish_reason   "eos", "stop" (it ended on an id of the stop set, which stays in tokens and counts in n) or "length" (a live beam).
    Ranked by sum_logprob / n ** length_penalty in Python floats, n = generated tokens with the EOS counted, descending, stable on
    pool order.  The scores compare directly with score_batch and with generate_batch(return_logprobs=True).

    The prompts are prefilled as generate_batch prefills them, prompt i into KV slot i * W, and forked into the W - 1 slots behind
    (dh_engine_copy_prefix, whole tiles).  Step 0 selects from the prefill's last-position logits; every later step is one captured
    chain — ids of the W live beams, the single-token step over all n * W rows, the selection, the KV re-parenting — replayed
    EOS_CHECK_EVERY at a time until every utterance is done (dh_engine_decode_beam).  A decode row's bits do not depend on the rows
    beside it, so a hypothesis has the scores it would have alone; num_beams=1 gives generate_batch(temperature=1.0, top_k=1)'s ids
    and log-probabilities.  The cache holds one position more per slot than generate_batch's: the rows of a finished utterance keep
    stepping at the position behind their last one.

    The fork is one dh_engine_copy_prefix call per utterance (a source slot each): a host synchronisation, a small upload and two
    launches per utterance inside the window timed as prefill_ms — a first version; one launch over a list of (source, destinations)
    is open.

    timing gains prefill_ms, decode_ms, decode_steps, decode_row_steps, and beam_step_rows / beam_copied_rows: the rows of the steps
    that utterances took, and those among them that continued another beam and were copied.

    token_mask (as in generate_batch, one row per utterance, serving all of its W beams): a beam row's 2 W candidates are the first
    2 W allowed ids of its raw row's order, each with the raw row's log-probability ("Token masks" of the header), so every row
    allows at least 2 W ids (checked before anything is launched); everything behind the candidates is unchanged.

    no_repeat_ngram: with history="host" refused unless 0 — a beam's history is re-parented on the host, so the device cannot form
    a beam's ban set; see `history`.

    stop (as in generate_batch, the stop set only): a candidate whose id is in the set ends its hypothesis into the pool exactly as
    the EOS does — same place rule, score and pool order — and the id stays in the hypothesis.  With history="host" stop sequences
    are refused before anything is launched: the beams' histories live on the host; see `history`.

    bias: refused unless None or empty, for the same reason.

    history: "host" (the default: everything above, the launches and the refusals it always had) or "device" ("Beam histories" of
    the header): the live beams' tokens are kept in two int64 planes on the device, re-parented by the selection kernel itself, and
    the two refusals above are lifted — no_repeat_ngram 1 .. 8 bans on a beam's own generated tokens (its candidates are the first
    2 W ids that the mask allows and the ban leaves; a row left with fewer than 2 W ignores the ban at that step), and stop
    sequences end a hypothesis whose own text completes one ("stop", the ids stay in its tokens).  The state of return_state carries
    the planes (host["history"][u][w][:n_steps[u]] is live beam w's text).  A bias and penalties stay refused: they would change
    what a candidate's rank and a beam's score mean.

    shared_prompt (W >= 2, either `history`): the beam steps' attention reads an utterance's whole 32-key prompt tiles once per block
    of its W rows, from slot u * W (include/dualhyp_hip.h, "Shared-prompt attention"; the re-parenting moves only the tiles behind
    them) — the same bits, so the same tokens, parents, scores and pool.  False (the default): the launches the call always made.
    Refused for W = 1 and, as the whole call is, for fp8 models.

    kv: "copy" (the default: the re-parenting above, the launches the call always made) or "table" (include/dualhyp_hip.h, "Beam KV
    tile table"; needs shared_prompt=True and W >= 2, a ValueError otherwise): two int32 planes name, per row and tile, the sibling
    slot that holds the tile; a beam step's attention reads every closed tile where it was written and the re-parenting copies only
    the open tile of the rows that continue another beam — the same keys, so the same tokens, parents, scores and pool.  timing gains
    beam_kv and beam_copied_tiles (the (row, tile) pairs the re-parenting copied, each through every layer, both caches and every
    group); the state of return_state carries the planes (host["tiles"][u][w] is live beam w's row of the plane the last step
    wrote; beam.resolve_slot reads a position's slot off it)."""
    if history not in _beam.HISTORIES:
        raise ValueError(f'history is "host" or "device", not {history!r}')
    on_device = history == "device"
    if _check_bias(bias) is not None:
        raise ValueError(f"a bias of {len(bias)} entries does not go with beam search: " +
                         ("a boosted logit would change what a candidate's rank and a beam's score mean" if on_device else _bias.BEAM_REFUSAL) +
                         "; it runs under generate_batch and generate_stream")
    B = len(prompts)
    assert B > 0 and max_new_tokens > 0
    if stop is not None and not isinstance(stop, _stop.StopSpec):
        stop = _stop.compile_stop(*_stop.split_entries(stop), vocab=model.config.padded_vocab_size)
    if stop is not None and stop.sequences and not on_device:
        raise ValueError(_stop.BEAM_REFUSAL + _beam.HISTORY_HINT)
    ngram = _ngram.check_ngram(no_repeat_ngram, model.config.padded_vocab_size if on_device else 0)
    if ngram and not on_device:
        raise ValueError(f"no_repeat_ngram={no_repeat_ngram} does not go with beam search: the beams' histories live on the host, so the "
                         "sampling kernels cannot form a beam's ban set; it runs under generate_batch and generate_stream" + _beam.HISTORY_HINT)
    W = _beam.check_arguments(model, num_beams, B)
    shared_prompt = check_shared_prompt(model, shared_prompt, W, f"num_beams={W}")
    kv = _beam.check_kv(kv, W, shared_prompt)
    length_penalty = _beam.check_length_penalty(length_penalty)
    lens = [int(p.numel()) for p in prompts]
    T_max = max(lens)
    need_pos = T_max + max_new_tokens
    if model.max_seq_length < need_pos:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {need_pos}")
    dev = model.transformer.wte.weight.device
    mask = _token_mask(model, token_mask, B, 2 * W, dev)
    stop = None if stop is None else _stop.as_spec(stop, model.config.padded_vocab_size, dev)
    chunks = [(c, min(c + prefill_batch, B)) for c in range(0, B, prefill_batch)]
    rows = B * W
    eng = model.engine(rows, need_pos, max(rows, max(sum(lens[a:b]) for a, b in chunks)), exact=rows > prefill_batch)
    eng.set_rsqrt_emulation(0, whole_call=False)
    state = _beam.BeamState(B, W, max_new_tokens, dev)
    tiles = None
    if kv == "table":
        n_tiles = _beam.beam_tiles(max_new_tokens, eng.s_max)
        if n_tiles > _beam.MAX_BEAM_TILES:
            raise ValueError(f'kv="table": {max_new_tokens} new tokens span {n_tiles} tiles, a tile table holds {_beam.MAX_BEAM_TILES} per row')
        eng.reserve_beam_tiles(W, max_new_tokens)
        tiles = state.tile_table(n_tiles)
    else:
        eng.reserve_beams(W, max_new_tokens)
    hist = state.history_buffer() if on_device else None
    plen = torch.tensor(lens, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing is not None else None
    if ev:
        ev[0].record()
    on_dev = [p.to(dev).reshape(-1) for p in prompts]
    last = torch.empty((B, eng.vocab), dtype=torch.bfloat16, device=dev)
    for a, b in chunks:
        last[a:b] = eng.forward_slots(torch.cat(on_dev[a:b]), lens[a:b], [u * W for u in range(a, b)])
    if W > 1:
        for u in range(B):      # positions at or behind the prompt's end are overwritten before causality lets anything read them
            eng.copy_prefix(u * W, list(range(u * W + 1, (u + 1) * W)), -(-lens[u] // 32) * 32)
    ops.beam_select(last, state, rows_per_utt=1, eos_id=eos_id, step=0, mask=mask, stop=stop, history=hist, no_repeat_ngram=ngram)
    if ev:
        ev[1].record()
    step = 1
    with _engine_settings([
            (mask is not None, lambda: eng.set_token_mask(mask), lambda: eng.set_token_mask(None)),
            (stop is not None, lambda: eng.set_stop(stop, plen if stop.sequences else None, state.fin_tok_buffer()), lambda: eng.set_stop(None)),
            (on_device, lambda: eng.set_beam_history(hist, ngram), lambda: eng.set_beam_history(None)),
            (tiles is not None, lambda: eng.set_beam_tiles(tiles), lambda: eng.set_beam_tiles(None)),
            _shared_prompt_setting(eng, shared_prompt, W, plen)]):
        while step < max_new_tokens:
            c = max_new_tokens - step if eos_id is None and stop is None else min(EOS_CHECK_EVERY, max_new_tokens - step)
            eng.decode_beam(state, plen, c, eos_id, first_step=step)
            step += c
            if step < max_new_tokens and bool((state.done != 0).all()):
                break
    if ev:
        ev[2].record()
    model._cache_len = []  # slots now hold these hypotheses; a later cached forward must start at 0
    h = state.host()        # the read-back: two copies
    prompts_h = torch.cat(on_dev).cpu().split(lens)
    if ev:
        took = sum(W * (n - 1) for n in h["n_steps"])
        moved = sum(p != w for u in range(B) for t in range(1, h["n_steps"][u]) for w, p in enumerate(h["beam_parent"][u][t]))
        _add_timing(timing, prefill_ms=ev[0].elapsed_time(ev[1]), decode_ms=ev[1].elapsed_time(ev[2]), decode_steps=step - 1,
                    decode_row_steps=rows * (step - 1), prefill_tokens=sum(lens), beam_step_rows=took, beam_copied_rows=moved)
        timing["shared_prompt"] = shared_prompt
        timing["beam_kv"] = kv
        # the (row, tile) pairs copied: under the table the open tile of a row that continues another beam, unless the step closed it;
        # under the copy every tile that holds a generated key
        timing["beam_copied_tiles"] = sum(
            (1 if (lens[u] + t) >> 5 == (lens[u] + t - 1) >> 5 else 0) if kv == "table" else ((lens[u] + t - 1) >> 5) - (lens[u] >> 5) + 1
            for u in range(B) for t in range(1, h["n_steps"][u]) for w, p in enumerate(h["beam_parent"][u][t]) if p != w)
    out = []
    for u in range(B):
        hyps = _beam.hypotheses(h, u, W, length_penalty, eos_id=eos_id)
        for hyp in hyps:
            hyp["tokens"] = torch.cat([prompts_h[u], torch.tensor(hyp["tokens"], dtype=torch.int64)])
        out.append(hyps)
    if return_state:
        return out, dict(beam=state, host=h, prompt_len=plen)
    return out


class _StreamBackend:
    """What StreamScheduler.run drives: one engine, one token buffer for every sequence of the call."""

    def __init__(self, eng, prompts, lens, max_new_tokens, sample_kw, picks: _Picks, timing, prefix: int = 0) -> None:
        N, dev = len(prompts), eng.device
        self.eng, self.prompts, self.lens, self.max_new, self.kw = eng, prompts, lens, max_new_tokens, sample_kw
        self.picks = picks                   # compiled with the dummy sequence's row (_Picks.compile, dummy=True)
        self.prefix = prefix                 # every slot but the spare one holds the call's first `prefix` positions (share_prefix)
        self.prefill_tokens = 0
        tok_ld = max(lens) + max_new_tokens
        # row N is the dummy sequence of the padding rows: one token, finished, owner of the spare slot
        self.tokens = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence([p.to(dev) for p in prompts], batch_first=True),
                                              (0, 0, 0, 1))
        self.tokens = torch.nn.functional.pad(self.tokens, (0, tok_ld - self.tokens.size(1))).contiguous()
        self.length = torch.tensor(lens + [1], dtype=torch.int32, device=dev)
        self.limit = torch.tensor([n + max_new_tokens for n in lens] + [1], dtype=torch.int32, device=dev)
        self.done = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        self.done[N] = 2
        self.row_seq, self.row_slot = eng.row_arrays()
        self.events = {"prefill_ms": [], "decode_ms": []} if timing is not None else None

    def _timed(self, key):
        if self.events is None:
            return None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.events[key].append(ev)
        ev[0].record()
        return ev[1]

    def prefill(self, seqs, slots) -> None:
        end = self._timed("prefill_ms")
        dev = self.eng.device
        P = self.prefix
        packed = torch.cat([self.prompts[u].to(dev).reshape(-1)[P:] for u in seqs])
        self.prefill_tokens += packed.numel()
        # a chunk of one-token prompts only is still a prompt forward (the engine would take it for a decode step) — unless the whole
        # call is one-token prompts, where generate_batch's one packed prefill is that decode step too
        last = self.eng.forward_slots(packed, [self.lens[u] - P for u in seqs], list(slots), prompt_phase=max(self.lens) > 1, pos0=P)
        ops.sample_rows(last, self.tokens, self.length, self.done, self.limit, torch.tensor(seqs, dtype=torch.int32, device=dev),
                        self.max_new, **self.picks.kw(), **self.kw)
        if end:
            end.record()

    def decode(self, row_seq, row_slot, n_steps) -> None:
        n = len(row_seq)
        rows = torch.tensor([row_seq, row_slot], dtype=torch.int32).to(self.eng.device)   # one upload per chunk
        end = self._timed("decode_ms")
        self.row_seq[:n].copy_(rows[0])
        self.row_slot[:n].copy_(rows[1])
        self.eng.decode_rows(self.tokens, self.length, self.done, self.limit, self.max_new, n, n_steps, self.kw["temperature"],
                             self.kw["top_k"], self.kw["eos_id"], self.kw["seed"])
        if end:
            end.record()

    def finished(self, seqs):
        flags = self.done.tolist()          # the one small read-back per chunk (it synchronises the stream)
        return [u for u in seqs if flags[u]]


@torch.inference_mode()
def generate_stream(model: GPT, prompts: Sequence[torch.Tensor], max_new_tokens: int, *, temperature: float = 1.0,
                    top_k: Optional[int] = None, eos_id: Optional[int] = None, seed: int = 1337, max_rows: int = 640,
                    prefill_batch: int = 64, check_every: int = EOS_CHECK_EVERY, timing: Optional[dict] = None,
                    share_prefix: Union[bool, str] = False, speculate: int = 0, return_logprobs: bool = False,
                    top_logprobs: int = 0, token_mask=None, no_repeat_ngram: int = 0, stop=None, return_state: bool = False,
                    top_p: Optional[float] = None, min_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
                    frequency_penalty: Optional[float] = None, presence_penalty: Optional[float] = None, bias=None, automaton=None,
                    verify: str = "argmax"):
    """generate_batch's result for any number of prompts — the same ids, bit for bit, in prompt order — through at most
    `max_rows` decode rows that change hands: every `check_every` steps the sequences that have finished (EOS, or their own
    budget of max_new_tokens) leave their rows, the next prompts are prefilled into the KV slots they held, and the step is
    launched over the live rows only (rounded up to one of at most 8 row counts).  generate_batch steps all of its rows until
    the last one has finished and starts nothing meanwhile.

    A sequence's ids do not depend on the schedule: no kernel's per-row arithmetic depends on the row count or the packing
    (an fp8 engine's two row classes are never mixed within a call), and the multinomial draw is keyed by
    (seed, sequence index, tokens generated so far).

    share_prefix: as in generate_batch.  The shared positions are forwarded once and copied into every slot the scheduler
    hands out before the first prefill; no sequence of the call writes below position P, so they outlive every refill, and a
    refill is a prefill of the tokens [P:] at position P.  The scheduler's decisions are those of the unshared call.

    return_logprobs, top_logprobs: as in generate_batch — (out, logprobs[, top]), the same values bit for bit.

    token_mask: as in generate_batch, one row per prompt; a sequence is picked under its own row wherever it is scheduled (the
    row-list sampler reads mask row row_seq[r]); the dummy sequence of the padding rows gets an all-ones row.

    no_repeat_ngram: as in generate_batch — a sequence's ban set is formed from its own row of the token buffer wherever it is
    scheduled, so the ids do not depend on the schedule.

    stop: as in generate_batch — a stopped sequence (done = 3) leaves its row at the next check like one that met its EOS, and the
    next prompt takes its KV slot.  return_state: the result gains a last element, the dict of the call's device state (tokens,
    length, done — one row per prompt — and logprobs, top_ids, top_logprobs where asked for), as generate_batch's.

    top_p, min_p: as in generate_batch — a row's kept set is a function of the row alone, so the ids do not depend on the schedule.

    repetition_penalty, frequency_penalty, presence_penalty: as in generate_batch — a sequence's adjusted values are formed from its own
    row of the token buffer wherever it is scheduled, so the ids do not depend on the schedule.

    bias: as in generate_batch — a sequence's proposals are matched against its own row of the token buffer wherever it is scheduled.

    automaton: as in generate_batch — a sequence's state is its own entry of the state buffer wherever it is scheduled, and a sequence
    that is prefilled into a row another one held begins in its own start state, with no reset launch (return_state's automaton_state
    has one entry per prompt).

    speculate, verify: refused unless 0 / "argmax", whatever the mode — a row list steps one token at a time."""
    from .schedule import StreamScheduler
    picks = _Picks.check(speculate=speculate, verify=verify, return_logprobs=return_logprobs, top_logprobs=top_logprobs, token_mask=token_mask,
                         no_repeat_ngram=no_repeat_ngram, stop=stop, top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty,
                         frequency_penalty=frequency_penalty, presence_penalty=presence_penalty, bias=bias, automaton=automaton)
    if speculate:
        raise ValueError(f"speculate={speculate}: continuous batching steps a row list one token at a time; speculative decoding runs "
                         "under generate_batch (--schedule batch) only")
    N = len(prompts)
    assert N > 0 and max_new_tokens > 0
    lens, T_max, need_pos, _ = _prompt_shape(model, prompts, max_new_tokens, prefill_batch)
    sched = StreamScheduler(N, max_new_tokens, max_rows, prefill_batch, check_every, fp8=bool(getattr(model, "fp8", False)))
    dev = model.transformer.wte.weight.device
    picks.compile(model, lens, T_max + max_new_tokens, dev, eos_id, dummy=True)
    P = _shared_prefix(model, prompts, share_prefix, dev)
    # slots 0..max_rows-1 and the spare one; a prefill packs at most the prefill_batch longest prompts (their tokens behind the prefix)
    eng = model.engine(sched.max_rows + 1, need_pos, max(P, sum(sorted(n - P for n in lens)[-prefill_batch:])), exact=True)
    eng.set_rsqrt_emulation(model.cpu_rsqrt_vec_width, whole_call=False)   # N independent batch-1 runs
    be = _StreamBackend(eng, prompts, lens, max_new_tokens, dict(temperature=temperature, top_k=top_k, eos_id=eos_id, seed=seed), picks,
                        timing, prefix=P)
    if P:       # the dummy sequence's spare slot (sched.max_rows) shares nothing: it stays at position 0
        end = be._timed("prefill_ms")
        _forward_prefix(eng, prompts[0], P, 0, range(1, sched.max_rows))
        if end:
            end.record()
    with picks.engine(eng):
        sched.run(be)
    model._cache_len = []  # slots now hold these sequences; a later cached forward must start at 0
    length_h = be.length.tolist()
    done_h = be.done.tolist()
    assert all(done_h[:N]), "generate_stream ended with an unfinished sequence"
    if timing is not None:   # the read-back above has synchronised the stream
        _add_timing(timing, **{key: sum((a.elapsed_time(b) for a, b in evs), 0.0) for key, evs in be.events.items()},
                    decode_steps=sched.decode_steps, decode_row_steps=sched.decode_row_steps, prefill_tokens=P + be.prefill_tokens)
        timing["launch_rows"] = set(timing.get("launch_rows", ())) | sched.launch_rows
        timing["shared_prefix"] = P
    rows = [_row_result(i, lens[i], length_h, done_h, max_new_tokens, be.tokens, picks.lp_buf, picks.top_buf) for i in range(N)]
    # the dummy sequence's row stays behind
    return _batch_result(rows, picks, dict(tokens=be.tokens[:N], length=be.length[:N], done=be.done[:N], **picks.state(N)) if return_state else None)


@torch.inference_mode()
def generate(model: GPT, idx: torch.Tensor, max_returned_tokens: int, *, temperature: float = 1.0,
             top_k: Optional[int] = None, eos_id: Optional[int] = None, speculate: int = 0, return_logprobs: bool = False,
             top_logprobs: int = 0, token_mask=None, no_repeat_ngram: int = 0, stop=None, top_p: Optional[float] = None,
             min_p: Optional[float] = None, repetition_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
             presence_penalty: Optional[float] = None, bias=None, automaton=None, verify: str = "argmax"):
    """Drop-in for generate/base.py:generate (one prompt of shape (T,)); speculate and verify as in generate_batch.  return_logprobs: the
    result is (ids, logprobs), logprobs as generate_batch's for the one sequence; with top_logprobs=K, (ids, logprobs, (top ids,
    top values)).  token_mask: generate_batch's — a [1, words] tensor, or a list holding the one id list.  no_repeat_ngram:
    generate_batch's.  stop: generate_batch's.  top_p, min_p: generate_batch's.  repetition_penalty, frequency_penalty,
    presence_penalty: generate_batch's.  bias: generate_batch's.  automaton: generate_batch's, a set with the one start state."""
    options = dict(speculate=speculate, return_logprobs=return_logprobs, top_logprobs=top_logprobs, token_mask=token_mask,
                   no_repeat_ngram=no_repeat_ngram, stop=stop, top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty,
                   frequency_penalty=frequency_penalty, presence_penalty=presence_penalty, bias=bias, automaton=automaton, verify=verify)
    _Picks.check(**options)
    T = idx.size(0)
    assert max_returned_tokens > T
    if model.max_seq_length < max_returned_tokens - 1:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {max_returned_tokens - 1}")
    res = generate_batch(model, [idx], max_returned_tokens - T, temperature=temperature, top_k=top_k, eos_id=eos_id, **options)
    if top_logprobs:
        return res[0][0], res[1][0], res[2][0]
    return (res[0][0], res[1][0]) if return_logprobs else res[0]


@torch.inference_mode()
def score_batch(model: GPT, prompts: Sequence[torch.Tensor], continuations: Sequence[torch.Tensor], *,
                max_tokens: Optional[int] = None, top_logprobs: int = 0):
    """Teacher-forced scoring: result[i] is a 1-D float32 tensor with the log-probability of every token of continuations[i] given
    prompts[i] and the continuation's tokens before it (both 1-D int64, len(prompt) >= 1, the continuation non-empty) — the values
    generate_batch(return_logprobs=True) reports for the tokens it produces, by the same definition (ops.token_logprobs), so a
    generated answer and given hypotheses compare on one scale.  The prompt-phase kernels compute the logits here and the decode
    kernels there: the two agree as closely as those kernel families do, not bit for bit.

    prompt + continuation[:-1] of several sequences are packed into one prompt-phase forward with the logits of every row, in groups
    of whole sequences whose token count fits max_tokens (default: what 64 MB of bf16 logits hold; a longer single sequence goes
    alone); a sequence's values do not depend on the grouping.  The head runs on the prompt rows too — a head restricted to the
    rows that predict the continuation is left for later.

    top_logprobs=K (1..8): the result is (scores, top); top[i] = (ids [len(continuation i), K] int32, lp float32 of that shape), the
    K most probable tokens at every continuation position with their log-probabilities (ops.token_top_logprobs on the rows the
    scores are read from; generate_batch's top_logprobs).  The scores are those of the call without it."""
    K = ops.check_top_logprobs(top_logprobs)
    if K:
        ops.check_top_logprobs(K, model.config.padded_vocab_size)
    N = len(prompts)
    if N == 0 or len(continuations) != N:
        raise ValueError(f"score_batch takes as many continuations as prompts, at least one ({N} prompts, {len(continuations)} continuations)")
    dev = model.transformer.wte.weight.device
    V = model.config.padded_vocab_size
    seqs, plen = [], []
    for i, (p, c) in enumerate(zip(prompts, continuations)):
        p, c = p.reshape(-1), c.reshape(-1)
        if p.dtype != torch.int64 or c.dtype != torch.int64:
            raise TypeError(f"sequence {i}: prompts and continuations are int64 tensors, got {p.dtype} and {c.dtype}")
        if p.numel() < 1 or c.numel() < 1:
            raise ValueError(f"sequence {i}: a prompt of at least one token and a non-empty continuation are needed, "
                             f"got {p.numel()} and {c.numel()} tokens")
        if p.numel() + c.numel() - 1 > model.max_seq_length:
            raise NotImplementedError(f"sequence {i}: {p.numel() + c.numel() - 1} positions, max_seq_length is {model.max_seq_length}")
        seqs.append((p.to(dev), c.to(dev)))
        plen.append(int(p.numel()))
    lo, hi = (int(v) for v in torch.aminmax(torch.cat([c for _, c in seqs])))      # one read-back for the whole call
    if lo < 0 or hi >= V:
        raise ValueError(f"continuation ids span [{lo}, {hi}], outside [0, {V})")
    rows = [int(p.numel() + c.numel() - 1) for p, c in seqs]
    if max_tokens is None:
        max_tokens = max(1, (64 << 20) // (2 * V))
    groups, cur = [], []
    for i in range(N):      # whole sequences, in order
        if cur and sum(rows[j] for j in cur) + rows[i] > max_tokens:
            groups.append(cur)
            cur = []
        cur.append(i)
    groups.append(cur)
    eng = model.engine(max(len(g) for g in groups), max(rows), max(sum(rows[j] for j in g) for g in groups))
    eng.set_rsqrt_emulation(model.cpu_rsqrt_vec_width, whole_call=False)   # N independent batch-1 runs
    out: List[Optional[torch.Tensor]] = [None] * N
    top: List[Optional[tuple]] = [None] * N
    for g in groups:
        packed = torch.cat([torch.cat([seqs[j][0], seqs[j][1][:-1]]) for j in g])
        # a group of one-token sequences alone is still a prompt forward (the engine would take it for a decode step)
        la = eng.forward_slots(packed, [rows[j] for j in g], list(range(len(g))), prompt_phase=True, want_all=True)
        start = 0
        pick, ids = [], []
        for j in g:         # row plen - 1 + k of the sequence predicts continuation token k
            pick.append(torch.arange(start + plen[j] - 1, start + rows[j], device=dev))
            ids.append(seqs[j][1])
            start += rows[j]
        picked = la[torch.cat(pick)]
        sizes = [int(seqs[j][1].numel()) for j in g]
        lp = ops.token_logprobs(picked, torch.cat(ids), check_ids=False)     # checked above
        for j, v in zip(g, lp.split(sizes)):
            out[j] = v
        if K:
            t_ids, t_lp = ops.token_top_logprobs(picked, K)
            for j, a, b in zip(g, t_ids.split(sizes), t_lp.split(sizes)):
                top[j] = (a, b)
    model._cache_len = []  # slots now hold these sequences; a later cached forward must start at 0
    return (out, top) if K else out
