"""Contextual biasing: the host definition of what the sampling kernels boost (include/dualhyp_hip.h, "Contextual biasing").

A bias specification holds 1 .. 256 entries, shared by all sequences of a call; an entry is 1 .. 8 token ids and one finite boost of
either sign.  At a pick, entry e proposes ids_e[k] when the sequence's last k GENERATED tokens (the prompt is excluded) are
ids_e[0 .. k); depth 0 always matches, a whole emitted phrase proposes nothing further, and nothing is taken back when a phrase is
abandoned.  An id's boost is the largest of its proposers'.  The kernels build the boosted columns themselves (csrc/sampling.hip);
compile_bias packs a specification for them, proposed and bias_hits are the host model the records and the tests use, and nothing
else here touches the GPU.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import struct
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

MAX_ENTRIES = 256           # DH_MAX_BIAS_ENTRIES
MAX_LEN = 8                 # DH_MAX_BIAS_LEN
MAX_VOCAB = 131072          # the ids the sampler's LDS row holds
MAX_HISTORY = 2048          # DH_MAX_PENALTY_HISTORY: with a penalty on, the history and the entries' ids share its tables
DEFAULT_BOOST = 4.0         # --bias_boost; its effect on a real corpus' word error rate is unmeasured
SPEC_REFUSAL = "a verify position's tail would have to include the picks of its own step, so the step would need per-position tables"
BEAM_REFUSAL = "the beams' histories live on the host, so the sampling kernels cannot match an entry against a beam's text"


def _f32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


def _boost(b, e: int) -> float:
    if isinstance(b, bool) or not isinstance(b, numbers.Real):
        raise TypeError(f"the boost of bias entry {e} is a number, not {b!r}")
    b = float(b)
    try:
        f = _f32(b)
    except OverflowError:       # beyond fp32's range
        f = math.inf
    if not math.isfinite(f):
        raise ValueError(f"the boost of bias entry {e} is {b!r}, which is not a finite fp32 value")
    return f + 0.0              # -0.0 is +0.0: the two order differently as keys and add alike


def check_bias(entries: Iterable, vocab: int) -> Tuple[Tuple[Tuple[int, ...], float], ...]:
    """The entries ((ids, boost) pairs) of a specification, checked as the C entries check them: 1 .. 256 entries of 1 .. 8 ids in
    [0, vocab), each with a finite boost, which is rounded to fp32 here; vocab at most 131072.  Duplicates are kept: the largest
    boost wins anyway."""
    if isinstance(vocab, bool) or not isinstance(vocab, int) or vocab < 1:
        raise ValueError(f"vocab is a positive int, got {vocab!r}")
    if vocab > MAX_VOCAB:
        raise ValueError(f"a bias keeps a sequence's overridden columns in an LDS row of {MAX_VOCAB} ids; a vocab of {vocab} does not fit")
    out = []
    for e, entry in enumerate(entries):
        if not isinstance(entry, (list, tuple)) or len(entry) != 2 or not isinstance(entry[0], (list, tuple)):
            raise TypeError(f"bias entry {e} is a pair (ids, boost) with ids a list of token ids, not {entry!r}")
        ids, boost = entry
        if not 1 <= len(ids) <= MAX_LEN:
            raise ValueError(f"bias entry {e} holds {len(ids)} ids, 1 .. {MAX_LEN} are supported")
        for t in ids:
            if isinstance(t, bool) or not isinstance(t, int):
                raise TypeError(f"bias entry {e} holds int token ids, got {t!r}")
            if not 0 <= t < vocab:
                raise ValueError(f"bias entry {e} holds id {t}, outside [0, {vocab})")
        out.append((tuple(ids), _boost(boost, e)))
    if not 1 <= len(out) <= MAX_ENTRIES:
        raise ValueError(f"a bias holds 1 .. {MAX_ENTRIES} entries, got {len(out)} (longer lists need a trie, which is not built)")
    return tuple(out)


def check_tables(tok_ld: int, n_ids: int) -> None:
    """With a penalty on: the token buffer and the entries' ids, refused where the shared LDS tables could not hold both."""
    if tok_ld + n_ids > MAX_HISTORY:
        raise ValueError(f"penalties and a bias keep a sequence's distinct ids in LDS tables of {MAX_HISTORY} entries; a token buffer of "
                         f"{tok_ld} places and the entries' {n_ids} ids may not fit")


class BiasSpec:
    """A packed specification: `entries` ((ids, boost) pairs) on the host, which proposed reads, and with a device the arrays the
    kernels read: `ids` int32 [n, 8] (-1 behind an entry's ids), `lens` int32 [n] and `boosts` float32 [n]."""

    def __init__(self, entries: Iterable, vocab: int, device=None) -> None:
        self.entries = check_bias(entries, vocab)
        self.vocab = vocab
        self.n_ids = sum(len(ids) for ids, _ in self.entries)
        self.device = None if device is None else torch.device(device)
        self.ids = self.lens = self.boosts = None
        self._c = self._host = None
        if self.device is not None:
            self.ids = torch.tensor(self._rows(), dtype=torch.int32).to(self.device)
            self.lens = torch.tensor([len(ids) for ids, _ in self.entries], dtype=torch.int32).to(self.device)
            self.boosts = torch.tensor([b for _, b in self.entries], dtype=torch.float32).to(self.device)

    def _rows(self) -> List[List[int]]:
        return [list(ids) + [-1] * (MAX_LEN - len(ids)) for ids, _ in self.entries]

    def __len__(self) -> int:
        return len(self.entries)

    def c_struct(self):
        """dh_bias_spec of the device arrays and their host copies (all kept alive by this object)."""
        from . import _lib
        if self.device is None:
            raise _lib.DualHypHipError("the bias specification was compiled without a device: the HIP path has no CPU fallback")
        if self._c is None:
            n = len(self.entries)
            flat = [t for row in self._rows() for t in row]
            self._host = ((ctypes.c_int32 * len(flat))(*flat), (ctypes.c_int32 * n)(*[len(ids) for ids, _ in self.entries]),
                          (ctypes.c_float * n)(*[b for _, b in self.entries]))
            addr = [ctypes.cast(a, ctypes.c_void_p).value for a in self._host]
            self._c = _lib.BiasSpec(ids=self.ids.data_ptr(), len=self.lens.data_ptr(), boost=self.boosts.data_ptr(), h_ids=addr[0],
                                    h_len=addr[1], h_boost=addr[2], n=n)
        return self._c


def compile_bias(entries: Iterable, vocab: int, device=None) -> BiasSpec:
    """The packed specification of `entries`, (ids, boost) pairs, over `vocab` tokens (check_bias's checks), on `device` for the
    kernels; device None: the host side only, for proposed and bias_hits."""
    return BiasSpec(entries, vocab, device)


def as_spec(bias, vocab: int, device) -> Optional[BiasSpec]:
    """The `bias=` argument of the generate functions and the sampling ops as a BiasSpec on `device`, or None when it is off (None, or
    an empty list)."""
    if bias is None:
        return None
    if isinstance(bias, BiasSpec):
        if bias.vocab != vocab:
            raise ValueError(f"the bias specification was compiled for {bias.vocab} tokens, the model has {vocab}")
        if bias.device is None or bias.device != torch.device(device):
            bias = BiasSpec(bias.entries, vocab, device)
        return bias
    if isinstance(bias, (list, tuple)):
        return BiasSpec(bias, vocab, device) if len(bias) else None
    raise TypeError(f"bias is a compiled specification (compile_bias) or a list of (ids, boost) pairs, not {bias!r}")


def _entries(spec) -> Sequence[Tuple[Sequence[int], float]]:
    return spec.entries if isinstance(spec, BiasSpec) else spec


def proposals(generated: Sequence[int], spec) -> Dict[int, Tuple[float, int]]:
    """{id: (boost, depth)} at the pick behind `generated`: the largest boost among the id's proposers, and the deepest depth at which
    any of them proposes it."""
    g = [int(t) for t in generated]
    m = len(g)
    out: Dict[int, Tuple[float, int]] = {}
    for ids, boost in _entries(spec):
        for k in range(len(ids)):
            if k <= m and g[m - k:] == [int(t) for t in ids[:k]]:
                t = int(ids[k])
                b, d = out.get(t, (-math.inf, 0))
                out[t] = (max(b, float(boost)), max(d, k))
    return out


def proposed(generated: Sequence[int], spec) -> Dict[int, float]:
    """{id: boost} at the pick behind `generated`, a sequence's tokens behind its prompt: the host model of the header's definition.
    spec: a BiasSpec, or its (ids, boost) pairs."""
    return {t: b for t, (b, _) in proposals(generated, spec).items()}


def bias_hits(generated: Sequence[int], spec) -> int:
    """How many tokens of `generated` were, when they were picked, proposed at a depth of 1 or more: they continued a listed phrase."""
    g = [int(t) for t in generated]
    return sum(1 for i, t in enumerate(g) if proposals(g[:i], spec).get(t, (0.0, 0))[1] >= 1)


def read_bias_file(path, default_boost: float = DEFAULT_BOOST) -> List[Tuple[object, float]]:
    """The lines of a --bias_file as (entry, boost) pairs: a line is ENTRY or BOOST<TAB>ENTRY; an entry made only of integers is a list
    of token ids (as in --stop_file), anything else is text, returned as a str for the caller's tokenizer (entries_from_lines).
    Blank lines and lines that begin with `#` are skipped."""
    from pathlib import Path
    out: List[Tuple[object, float]] = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        boost, entry = default_boost, line
        if "\t" in line:
            head, entry = line.split("\t", 1)
            try:
                boost = float(head)
            except ValueError:
                raise ValueError(f"{path}:{n}: the field in front of the tab is a boost, got {head!r}") from None
        if not math.isfinite(boost):
            raise ValueError(f"{path}:{n}: the boost {boost!r} is not finite")
        entry = entry.strip()
        if not entry:
            raise ValueError(f"{path}:{n}: a boost without an entry")
        parts = entry.split()
        out.append(([int(v) for v in parts], boost) if all(p.isdigit() for p in parts) else (entry, boost))
    return out


def _encode_plain(tokenizer, text: str) -> List[int]:
    """`text` as token ids with no BOS and no EOS: the tokenizer's encode_plain where it has one, else encode() without the BOS it
    prepends (dualhyp_amd.tokenizer)."""
    if hasattr(tokenizer, "encode_plain"):
        return [int(t) for t in tokenizer.encode_plain(text)]
    ids = [int(t) for t in tokenizer.encode(text)]
    bos, eos = getattr(tokenizer, "bos_token_id", None), getattr(tokenizer, "eos_token_id", None)
    if ids and bos is not None and ids[0] == bos:
        ids = ids[1:]
    if ids and eos is not None and ids[-1] == eos:
        ids = ids[:-1]
    return ids


def entries_from_lines(lines: Iterable[Tuple[object, float]], tokenizer=None) -> List[Tuple[List[int], float]]:
    """(ids, boost) pairs of read_bias_file's lines: id lists stay; a text is encoded by `tokenizer` with no BOS or EOS, and a second
    time with one leading space when that gives a different id sequence — both forms are entries."""
    out: List[Tuple[List[int], float]] = []
    for entry, boost in lines:
        if not isinstance(entry, str):
            out.append((list(entry), boost))
            continue
        if tokenizer is None:
            raise ValueError(f"the bias entry {entry!r} is text and needs the run's tokenizer")
        forms: List[List[int]] = []
        for text in (entry, " " + entry):
            ids = _encode_plain(tokenizer, text)
            if ids and ids not in forms:
                forms.append(ids)
        if not forms:
            raise ValueError(f"the bias entry {entry!r} encodes to no token")
        out.extend((ids, boost) for ids in forms)
    return out


def record(n_entries: int, default_boost: float) -> Dict[str, float]:
    """The `bias` field of a prediction record of a --bias_file run."""
    return {"entries": int(n_entries), "default_boost": float(default_boost)}
