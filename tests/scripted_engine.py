"""A scripted engine and model on the CPU: what the generation entry points (dualhyp_amd/generate.py) ask of gpt._Engine and GPT,
with every call recorded.  `calls` keeps the four prefill / row-list entries test_prefix_host.py reads; `trace` holds every call, in
order and JSON-able (Trace), the sampling ops included once patch_ops has replaced them.  Sequence (or row) u produces
n_gen[u % len(n_gen)] tokens, each the id 7, and then sets its done flag."""
import math

import torch

from dualhyp_amd.automaton import AutomatonSet
from dualhyp_amd.beam import BeamState
from dualhyp_amd.bias import BiasSpec
from dualhyp_amd.stop import StopSpec

VOCAB = 64
MAX_VALUES = 64         # a tensor of at most this many elements is recorded with its values


class Trace:
    """The calls of one run as [name, args, kwargs] entries.  A tensor is recorded as dtype, shape and, up to MAX_VALUES elements, its
    values at its first appearance, under a label; where the same memory, dtype, shape and strides are passed again, as the label alone.
    The tensors are kept alive here, so an address names one tensor for the whole run."""

    def __init__(self):
        self.entries, self._labels, self._alive = [], {}, []

    def add(self, name, *args, **kw):
        self.entries.append([name, [self.plain(a) for a in args], {k: self.plain(v) for k, v in kw.items()}])

    def tensor(self, t, values=True):
        key = (t.data_ptr(), t.dtype, tuple(t.shape), t.stride())
        if key in self._labels:
            return self._labels[key]
        self._alive.append(t)
        label = self._labels[key] = f"t{len(self._labels)}"
        out = dict(tensor=label, dtype=str(t.dtype), shape=list(t.shape))
        if values and t.numel() <= MAX_VALUES:
            out["values"] = self.plain(t.tolist())
        return out

    def plain(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, float):
            return v if math.isfinite(v) else repr(v)
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, (list, tuple, range, set, frozenset)):
            return [self.plain(x) for x in (sorted(v) if isinstance(v, (set, frozenset)) else v)]
        if isinstance(v, dict):
            # a returned state's automaton_state is (a view of) an AutomatonSet's uninitialised `state`, which nothing here writes
            return {str(k): self.tensor(x, values=False) if k == "automaton_state" else self.plain(x) for k, x in v.items()}
        if isinstance(v, torch.device):
            return str(v)
        if isinstance(v, StopSpec):
            return dict(stop_ids=list(v.ids), stop_sequences=[list(s) for s in v.sequences], device=str(v.device))
        if isinstance(v, BiasSpec):
            return dict(bias=[[list(ids), b] for ids, b in v.entries], device=str(v.device))
        if isinstance(v, AutomatonSet):     # `state` is uninitialised memory: its identity counts, not its values
            return dict(n_states=v.n_states, init=v.init.tolist(), device=str(v.device), state=self.tensor(v.state, values=False))
        if isinstance(v, BeamState):
            return dict(beam_state=[v.n_utt, v.W, v.max_new], fin_tok=v.fin_tok is not None, history=v.history is not None)
        raise TypeError(f"no JSON form for {type(v).__name__}")


class ScriptedEngine:
    """gpt._Engine as the generation entry points drive it."""
    vocab = VOCAB
    RECORDED = ("set_rsqrt_emulation", "fork_slots", "reserve_rows", "reserve_beams", "set_logprobs", "set_top_logprobs", "set_token_mask",
                "set_no_repeat_ngram", "set_stop", "set_beam_history", "set_nucleus", "set_penalties", "set_bias", "set_automaton",
                "set_shared_prompt")       # calls that are recorded and do nothing else

    def __init__(self, n_gen):
        self.device = torch.device("cpu")
        self.n_gen, self.calls, self.trace = n_gen, [], Trace()
        self.max_batch = None
        self._rows = None
        self.lens = None                    # the prompt length of every sequence (or row), set by the test

    def __getattr__(self, name):
        if name in ScriptedEngine.RECORDED:
            return lambda *args, **kw: self.trace.add(name, *args, **kw)
        raise AttributeError(name)

    def forward(self, ids_, seq_len, pos0, want_all, want_last, slot_base=0):
        self.calls.append(("forward", ids_.tolist(), list(seq_len), list(pos0), want_all, want_last, slot_base))
        self.trace.add("forward", ids_, seq_len, pos0, want_all=want_all, want_last=want_last, slot_base=slot_base)
        return None, torch.zeros((len(seq_len), self.vocab), dtype=torch.bfloat16) if want_last else None

    def copy_prefix(self, src_slot, dst_slots, n_pos):
        self.calls.append(("copy_prefix", src_slot, list(dst_slots), n_pos))
        self.trace.add("copy_prefix", src_slot, dst_slots, n_pos)

    def forward_slots(self, ids_, seq_len, slots, prompt_phase=False, pos0=0):
        self.calls.append(("forward_slots", ids_.tolist(), list(seq_len), list(slots), prompt_phase, pos0))
        self.trace.add("forward_slots", ids_, seq_len, slots, prompt_phase=prompt_phase, pos0=pos0)
        return torch.zeros((len(seq_len), self.vocab), dtype=torch.bfloat16)

    def row_arrays(self):
        if self._rows is None:
            self._rows = (torch.zeros(self.max_batch, dtype=torch.int32), torch.zeros(self.max_batch, dtype=torch.int32))
        return self._rows

    def _pick(self, u, tokens, length, done, made):
        tokens[u, length[u]] = 7
        length[u] += 1
        if made >= self.n_gen[u % len(self.n_gen)]:
            done[u] = 1

    def _step(self, rows, tokens, length, done, n_steps):
        for u in rows:
            for _ in range(n_steps):
                if not done[u]:
                    self._pick(u, tokens, length, done, int(length[u]) + 1 - self.lens[u])

    def decode(self, tokens, length, done, n_steps, temperature, top_k, eos_id, seed, first_step=0):
        self.trace.add("decode", tokens, length, done, n_steps, temperature, top_k, eos_id, seed, first_step=first_step)
        self._step(range(tokens.size(0)), tokens, length, done, n_steps)

    def decode_rows(self, tokens, length, done, limit, max_new, n_rows, n_steps, temperature, top_k, eos_id, seed):
        row_seq, row_slot = (t[:n_rows].tolist() for t in self._rows)
        self.calls.append(("decode_rows", row_seq, row_slot, n_steps))
        self.trace.add("decode_rows", tokens, length, done, limit, max_new, n_rows, n_steps, temperature, top_k, eos_id, seed,
                       row_seq=row_seq, row_slot=row_slot)
        self._step(row_seq, tokens, length, done, n_steps)

    def decode_spec(self, tokens, length, done, limit, max_new, n_draft, drafts, counters, n_steps, temperature, eos_id, first_step=0):
        """A verify step that confirms no draft: one token per live sequence."""
        self.trace.add("decode_spec", tokens, length, done, limit, max_new, n_draft, drafts, counters, n_steps, temperature, eos_id,
                       first_step=first_step)
        self._step(range(tokens.size(0)), tokens, length, done, n_steps)
        counters += torch.tensor([n_steps, n_steps * n_draft, 0], dtype=torch.int32)

    def read_spec(self, n_seq, n_draft):
        self.trace.add("read_spec", n_seq, n_draft)
        return torch.zeros((n_seq, n_draft), dtype=torch.int64), torch.zeros(n_seq, dtype=torch.int32)

    def decode_beam(self, state, prompt_len, n_steps, eos_id, first_step):
        """Every utterance is done behind step 3; the records stay empty."""
        self.trace.add("decode_beam", state, prompt_len, n_steps, eos_id, first_step=first_step)
        if first_step + n_steps > 3:
            state.done.fill_(1)


class ScriptedModel:
    """The attributes of GPT that the generation entry points read"""
    max_seq_length = 4096
    cpu_rsqrt_vec_width = 0
    fp8 = False
    kv_cache_dtype = "bf16"
    config = type("Config", (), dict(padded_vocab_size=VOCAB, n_head=4, n_query_groups=4, block_size=4096))()

    def __init__(self, n_gen):
        self.eng = ScriptedEngine(n_gen)
        self.transformer = type("T", (), {"wte": type("W", (), {"weight": torch.zeros(1)})()})()
        self.engine_args = None

    def engine(self, need_batch, need_pos, need_tokens, exact=False):
        self.engine_args = (need_batch, need_pos, need_tokens)
        self.eng.trace.add("engine", need_batch, need_pos, need_tokens, exact=exact)
        self.eng.max_batch = need_batch
        return self.eng


def patch_ops(monkeypatch, ops, eng):
    """ops.sample, ops.sample_rows and ops.beam_select replaced by recorders that pick as the scripted engine picks.  Every keyword
    of theirs defaults to None where it can be None, so one passed as None is recorded as one left out."""
    def given(kw):
        return {k: v for k, v in kw.items() if v is not None}

    def sample(last, tokens, length, done, **kw):
        eng.trace.add("ops.sample", last, tokens, length, done, **given(kw))
        for u in range(tokens.size(0)):
            eng._pick(u, tokens, length, done, 1)

    def sample_rows(last, tokens, length, done, limit, seqs, max_new, **kw):
        eng.trace.add("ops.sample_rows", last, tokens, length, done, limit, seqs, max_new, **given(kw))
        for u in seqs.tolist():
            eng._pick(u, tokens, length, done, 1)

    def beam_select(last, state, **kw):
        eng.trace.add("ops.beam_select", last, state, **given(kw))

    monkeypatch.setattr(ops, "sample", sample)
    monkeypatch.setattr(ops, "sample_rows", sample_rows)
    monkeypatch.setattr(ops, "beam_select", beam_select)
