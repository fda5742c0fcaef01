"""Stop conditions: the host definition of what the sampling kernels test (include/dualhyp_hip.h, "Stop conditions").

A stop specification holds a stop SET of token ids and up to 8 stop SEQUENCES of 2 .. 8 ids.  A sequence of the call ends with
done = 3 right behind the first token it GENERATES (the prompt is excluded) that is in the set or completes one of the sequences; the
token stays in the result.  The kernels run the test in their tails; compile_stop packs a specification for them, first_stop is the
host model the records and the tests use, and nothing else here touches the GPU.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple

import torch

MAX_STOP_SEQS = 8           # DH_MAX_STOP_SEQS
MAX_STOP_LEN = 8            # DH_MAX_STOP_LEN
DONE_EOS, DONE_LENGTH, DONE_STOP = 1, 2, 3      # DH_DONE_*: the values of `done`
BEAM_REFUSAL = ("stop sequences do not go with beam search: the beams' histories live on the host, so the sampling kernels cannot "
                "match a sequence against a beam's text; the stop set alone goes with it, and sequences run under generate_batch and "
                "generate_stream")
_REASONS = {DONE_EOS: "eos", DONE_LENGTH: "length", DONE_STOP: "stop"}


def _id(t, vocab: int, what: str) -> int:
    if isinstance(t, bool) or not isinstance(t, int):
        raise TypeError(f"{what} is an int token id, got {t!r}")
    if not 0 <= t < vocab:
        raise ValueError(f"{what} {t} is outside [0, {vocab})")
    return t


def normalize(ids: Iterable[int], sequences: Iterable[Sequence[int]], vocab: int) -> Tuple[Tuple[int, ...], Tuple[Tuple[int, ...], ...]]:
    """(sorted stop ids, stop sequences) of a specification, checked: ids inside [0, vocab); every sequence non-empty and of at most
    8 ids; a sequence of one id folded into the set; at most 8 sequences of two or more left, duplicates dropped, order kept."""
    if isinstance(vocab, bool) or not isinstance(vocab, int) or vocab < 1:
        raise ValueError(f"vocab is a positive int, got {vocab!r}")
    stop_ids = {_id(t, vocab, "stop id") for t in ids}
    seqs: List[Tuple[int, ...]] = []
    for s in sequences:
        s = tuple(s)
        if len(s) == 0:
            raise ValueError("an empty stop sequence would stop every sequence at once")
        if len(s) > MAX_STOP_LEN:
            raise ValueError(f"a stop sequence holds at most {MAX_STOP_LEN} tokens, got {len(s)}")
        s = tuple(_id(t, vocab, "stop sequence token") for t in s)
        if len(s) == 1:
            stop_ids.add(s[0])
        elif s not in seqs:
            seqs.append(s)
    if len(seqs) > MAX_STOP_SEQS:
        raise ValueError(f"at most {MAX_STOP_SEQS} stop sequences of two or more tokens are supported, got {len(seqs)}")
    return tuple(sorted(stop_ids)), tuple(seqs)


def split_entries(entries: Iterable) -> Tuple[List[int], List[Sequence[int]]]:
    """A list whose ints are stop ids and whose lists or tuples are stop sequences (the `stop=` of the generate functions)."""
    ids, seqs = [], []
    for e in entries:
        if isinstance(e, (list, tuple)):
            seqs.append(e)
        else:
            ids.append(e)
    return ids, seqs


class StopSpec:
    """A packed specification: `ids` and `sequences` on the host (first_stop reads them), and with a device the arrays the kernels
    read: `set_words` int32 [ceil(vocab / 32)] in the token masks' bit layout, `seq_ids` int32 [n, 8] and the host lengths."""

    def __init__(self, ids: Sequence[int], sequences: Sequence[Sequence[int]], vocab: int, device=None) -> None:
        self.ids, self.sequences = normalize(ids, sequences, vocab)
        self.vocab = vocab
        self.device = None if device is None else torch.device(device)
        self.set_words = self.seq_ids = None
        self._c = self._lens = None
        if self.device is not None:
            if self.ids:
                words = [0] * ((vocab + 31) // 32)
                for t in self.ids:
                    words[t >> 5] |= 1 << (t & 31)
                self.set_words = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).to(self.device)
            if self.sequences:
                rows = [list(s) + [-1] * (MAX_STOP_LEN - len(s)) for s in self.sequences]
                self.seq_ids = torch.tensor(rows, dtype=torch.int32).to(self.device)

    def __bool__(self) -> bool:
        return bool(self.ids or self.sequences)

    def c_struct(self):
        """dh_stop_spec of the device arrays (kept alive by this object)."""
        from . import _lib
        if self.device is None:
            raise _lib.DualHypHipError("the stop specification was compiled without a device: the HIP path has no CPU fallback")
        if self._c is None:
            n = len(self.sequences)
            self._lens = (ctypes.c_int32 * max(n, 1))(*[len(s) for s in self.sequences])
            self._c = _lib.StopSpec(set=None if self.set_words is None else self.set_words.data_ptr(),
                                    seqs=None if self.seq_ids is None else self.seq_ids.data_ptr(),
                                    h_seq_len=ctypes.cast(self._lens, ctypes.c_void_p).value if n else None, n_seqs=n)
        return self._c


def compile_stop(ids: Iterable[int] = (), sequences: Iterable[Sequence[int]] = (), vocab: int = 0, device=None) -> StopSpec:
    """The packed specification of stop ids `ids` and stop sequences `sequences` over `vocab` tokens (normalize's checks), on
    `device` for the kernels; device None: the host side only, for first_stop."""
    return StopSpec(list(ids), list(sequences), vocab, device)


def as_spec(stop, vocab: int, device) -> Optional[StopSpec]:
    """The `stop=` argument of the generate functions as a StopSpec on `device`, or None when it is off (None, or nothing in it)."""
    if stop is None:
        return None
    if isinstance(stop, StopSpec):
        if stop.vocab != vocab:
            raise ValueError(f"the stop specification was compiled for {stop.vocab} tokens, the model has {vocab}")
        if stop and (stop.device is None or stop.device != torch.device(device)):
            stop = StopSpec(stop.ids, stop.sequences, vocab, device)
    elif isinstance(stop, (list, tuple)):
        stop = StopSpec(*split_entries(stop), vocab, device)
    else:
        raise TypeError(f"stop is a compiled specification (compile_stop) or a list of ids and id lists, not {stop!r}")
    return stop if stop else None


def first_stop(generated: Sequence[int], spec) -> Optional[int]:
    """The index of the first position of `generated` (a sequence's tokens behind its prompt) at which the stop condition holds, or
    None.  spec: a StopSpec, or the pair (ids, sequences)."""
    ids, seqs = (spec.ids, spec.sequences) if isinstance(spec, StopSpec) else spec
    ids = set(int(t) for t in ids)
    seqs = [tuple(int(t) for t in s) for s in seqs]
    g = [int(t) for t in generated]
    for i, t in enumerate(g):
        if t in ids:
            return i
        for s in seqs:
            if len(s) <= i + 1 and tuple(g[i + 1 - len(s):i + 1]) == s:
                return i
    return None


def newline_ids(tokenizer, vocab: int) -> List[int]:
    """Every id below `vocab` whose decoded piece contains a newline: what --stop newline stops on."""
    out = []
    for i in range(vocab):
        try:
            piece = tokenizer.decode([i])
        except Exception:       # ids a tokenizer cannot decode (padding rows of the vocabulary) stop nothing
            continue
        if isinstance(piece, str) and "\n" in piece:
            out.append(i)
    return out


def finish_reasons(done: Iterable[int]) -> List[str]:
    """The `done` flags of a finished generate call as "eos" | "length" | "stop".  0 is "length" too: generate_batch steps its rows
    max_new_tokens - 1 times and the plain sampler flags a budget only at the end of the token buffer, which a prompt shorter than
    the call's longest never reaches — such a sequence ended on its budget with its flag still clear."""
    out = []
    for d in (done.tolist() if isinstance(done, torch.Tensor) else done):
        if int(d) != 0 and int(d) not in _REASONS:
            raise ValueError(f"done = {d} names no finish reason (0 or 2 length, 1 eos, 3 stop)")
        out.append(_REASONS.get(int(d), "length"))
    return out


def read_stop_file(path) -> Tuple[List[int], List[List[int]]]:
    """(ids, sequences) of a --stop_file: one entry per line, token ids separated by blanks; a line of one id adds to the stop set, a
    line of several is a stop sequence; blank lines and `#` comments are skipped."""
    from pathlib import Path
    ids: List[int] = []
    seqs: List[List[int]] = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        parts = line.split("#", 1)[0].split()
        if not parts:
            continue
        for part in parts:
            if not part.isdigit():
                raise ValueError(f"{path}:{n}: a token id is a non-negative integer, got {part!r}")
        if len(parts) == 1:
            ids.append(int(parts[0]))
        else:
            seqs.append([int(v) for v in parts])
    return ids, seqs
