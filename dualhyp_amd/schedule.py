"""Host side of continuous batching (generate.generate_stream): which prompts go in next, which KV slot each
sequence owns, the row list of a decode chunk, its row count and when the call ends.

Nothing here touches the GPU (torch only where shared_prefix_len is handed tensors): `StreamScheduler.run(backend)` drives any object with the three methods
of `ScriptedBackend`, which is also how the decisions are tested on the CPU and how the number of row-steps of a
run is predicted from the sequences' lengths."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Set, Tuple

MAX_ROW_COUNTS = 8          # the engine keeps 8 captured decode graphs (csrc/engine.hip: launch_steps)
FP8_STREAM_ROWS = 128       # fp8 decode steps stream the weights up to here and are tiled above (engine.hip: fp8_kernel)
BF16_STREAM_ROWS = 2048     # bf16 single-token steps take the streaming path up to here (engine.hip: MAX_DECODE_ROWS)
PREFIX_TILE = 32            # a shared prefix is whole KV-cache tiles (common.h: kfrag_off / vfrag_off) = whole q-tiles of the prefill attention


def shared_prefix_len(prompts: Sequence) -> int:
    """P, the number of leading tokens a call forwards once for all of its prompts (generate_batch / generate_stream,
    share_prefix): the longest common token prefix, cut so that every prompt keeps a token of its own (its last position
    must produce logits), rounded down to whole tiles of 32.  0: nothing is shared.
    prompts: 1-D integer tensors (compared on their device, one read-back) or plain sequences of ids."""
    cap = min(len(p) for p in prompts) - 1
    if cap < PREFIX_TILE:
        return 0
    first = prompts[0]
    if hasattr(first, "new_ones"):
        import torch
        m = torch.stack([p[:cap] for p in prompts])
        differs = (m != m[0]).any(dim=0)
        L = int(torch.cat([differs, differs.new_ones(1)]).int().argmax())     # the first column that differs, or cap
    else:
        L = cap
        for p in prompts[1:]:
            L = next((i for i in range(L) if p[i] != first[i]), L)
    return L // PREFIX_TILE * PREFIX_TILE


def row_buckets(max_rows: int, floor: int = 1) -> List[int]:
    """The row counts a call may launch, largest first: max_rows shrunk by 0.7 (rounded up, by at least one row) at most
    7 times, never below `floor`.  A chunk of n live rows is launched at the smallest bucket >= n, so less than a third of
    its rows are padding until the last bucket (max_rows / 12: a step over that few rows costs what a step over one row does)."""
    assert max_rows >= floor >= 1
    b = [max_rows]
    while len(b) < MAX_ROW_COUNTS and b[-1] > floor:
        b.append(max(floor, min(b[-1] - 1, (7 * b[-1] + 9) // 10)))
    return b


def class_floor(max_rows: int, fp8: bool) -> int:
    """Smallest row count of the kernel class max_rows is in.  The two fp8 decode classes sum K in different orders
    (DESIGN.md §5, §7), so a call whose max_rows is above the boundary pads up to 129 rows instead of shrinking below
    it; the bf16 boundary at 2048 rows is kept the same way."""
    edge = FP8_STREAM_ROWS if fp8 else BF16_STREAM_ROWS
    return edge + 1 if max_rows > edge else 1


class StreamScheduler:
    """Sequences 0..n_seq-1 are served in order through `max_rows` KV slots.  Slot `max_rows` is the spare one: it
    belongs to the dummy sequence `n_seq` (finished from the start), and (n_seq, max_rows) is the only padding row.

    Counters after run(): decode_steps (graph launches), decode_row_steps (rows launched summed over steps, padding
    included), launch_rows (the row counts used), prefill_calls."""

    def __init__(self, n_seq: int, max_new_tokens: int, max_rows: int = 640, prefill_batch: int = 64, check_every: int = 16,
                 fp8: bool = False) -> None:
        assert n_seq > 0 and max_new_tokens > 0 and max_rows > 0 and prefill_batch > 0 and check_every > 0
        self.n_seq, self.max_new_tokens = n_seq, max_new_tokens
        self.max_rows = min(max_rows, n_seq)             # never more rows (or a higher kernel class) than the call has sequences
        self.prefill_batch, self.check_every = prefill_batch, check_every
        self.buckets = row_buckets(self.max_rows, class_floor(self.max_rows, fp8))
        self.dummy_seq, self.spare_slot = n_seq, self.max_rows
        self.free: List[int] = list(range(self.max_rows))     # kept ascending: the lowest free slot is taken first
        self.next_seq = 0
        self.live: Dict[int, int] = {}                   # sequence -> slot, in admission order
        self.steps_done: Dict[int, int] = {}             # sequence -> decode steps it has been through
        self.retired: Set[int] = set()
        self.decode_steps = self.decode_row_steps = self.prefill_calls = 0
        self.launch_rows: Set[int] = set()

    # ---- the decisions -------------------------------------------------------------------------------------------
    @property
    def pending(self) -> int:
        return self.n_seq - self.next_seq

    def admit(self) -> Tuple[List[int], List[int]]:
        """The next prefill: up to prefill_batch of the remaining sequences, in order, each with a free slot."""
        n = min(self.prefill_batch, self.pending, len(self.free))
        seqs = list(range(self.next_seq, self.next_seq + n))
        slots, self.free = self.free[:n], self.free[n:]
        self.next_seq += n
        for u, s in zip(seqs, slots):
            self.live[u] = s
            self.steps_done[u] = 0
        return seqs, slots

    def retire(self, seqs: Sequence[int]) -> None:
        for u in seqs:
            self.free.append(self.live.pop(u))
            del self.steps_done[u]
            self.retired.add(u)
        self.free.sort()

    def rows(self) -> Tuple[List[int], List[int]]:
        """(row_seq, row_slot) of the next chunk: the live sequences, padded with the dummy row up to a bucket."""
        n = len(self.live)
        assert 0 < n <= self.max_rows
        n_rows = min(b for b in self.buckets if b >= n)
        pad = n_rows - n
        return list(self.live) + [self.dummy_seq] * pad, list(self.live.values()) + [self.spare_slot] * pad

    def chunk_steps(self) -> int:
        """Steps of the next chunk: check_every, or what the live sequence with the most budget left still needs
        (the first of a sequence's max_new_tokens comes from its prefill)."""
        left = max(self.max_new_tokens - 1 - d for d in self.steps_done.values())
        return min(self.check_every, left)

    # ---- the loop ------------------------------------------------------------------------------------------------
    def run(self, backend) -> None:
        """backend.prefill(seqs, slots): prompt forward into those slots + the first pick of each sequence;
        backend.decode(row_seq, row_slot, n_steps): n_steps decode steps over the row list;
        backend.finished(seqs) -> the subset whose done flag is set (one read-back per call)."""
        while self.pending or self.live:
            admitted: List[int] = []
            while self.pending and self.free:
                seqs, slots = self.admit()
                backend.prefill(seqs, slots)
                self.prefill_calls += 1
                admitted += seqs
            if admitted:
                first = backend.finished(admitted)       # ended on the first pick (EOS, or a budget of one token):
                if self.max_new_tokens == 1:             # these never take a decode row
                    assert len(first) == len(admitted), "a sequence with a budget of one token is not flagged as finished"
                self.retire(first)
                if first and self.pending:
                    continue
            if not self.live:
                continue
            row_seq, row_slot = self.rows()
            n_steps = self.chunk_steps()
            assert n_steps > 0, "a live sequence has no budget left: its done flag was not set"
            backend.decode(row_seq, row_slot, n_steps)
            self.decode_steps += n_steps
            self.decode_row_steps += n_steps * len(row_seq)
            self.launch_rows.add(len(row_seq))
            for u in self.steps_done:
                self.steps_done[u] += n_steps
            self.retire(backend.finished(list(self.live)))


class ScriptedBackend:
    """The engine replaced by a script: sequence u produces n_gen[u] tokens (the EOS included, at most max_new_tokens;
    1 = it ends on the pick of its prefill).  Records every call for the tests."""

    def __init__(self, n_gen: Sequence[int]) -> None:
        self.n_gen = list(n_gen)
        self.made: Dict[int, int] = {}                   # sequence -> tokens produced so far
        self.slot_of: Dict[int, int] = {}                # live sequence -> slot, as the device would see it
        self.calls: List[tuple] = []

    def _done(self, u: int) -> bool:
        return self.made[u] >= self.n_gen[u]

    def prefill(self, seqs: Sequence[int], slots: Sequence[int]) -> None:
        self.calls.append(("prefill", list(seqs), list(slots)))
        for u, s in zip(seqs, slots):
            assert u not in self.made, f"sequence {u} is prefilled twice"
            busy = {v: t for v, t in self.slot_of.items() if t == s}
            assert not busy, f"slot {s} is handed to sequence {u} while {busy} lives in it"
            self.made[u] = 1
            self.slot_of[u] = s

    def decode(self, row_seq: Sequence[int], row_slot: Sequence[int], n_steps: int) -> None:
        self.calls.append(("decode", list(row_seq), list(row_slot), n_steps))
        for u, s in zip(row_seq, row_slot):
            if u in self.slot_of:
                assert self.slot_of[u] == s, f"row of sequence {u} names slot {s}, it lives in {self.slot_of[u]}"
                self.made[u] = min(self.n_gen[u], self.made[u] + n_steps)

    def finished(self, seqs: Sequence[int]) -> List[int]:
        self.calls.append(("finished", list(seqs)))
        out = [u for u in seqs if self._done(u)]
        for u in out:
            del self.slot_of[u]                          # the scheduler retires what it is told has finished
        return out


def predict(n_gen: Sequence[int], max_new_tokens: int, max_rows: int = 640, prefill_batch: int = 64, check_every: int = 16,
            fp8: bool = False) -> StreamScheduler:
    """The scheduler after a scripted run: what generate_stream launches for sequences that produce n_gen[u] tokens."""
    sched = StreamScheduler(len(n_gen), max_new_tokens, max_rows, prefill_batch, check_every, fp8)
    sched.run(ScriptedBackend(n_gen))
    return sched
