"""The host-side decisions of continuous batching (dualhyp_amd.schedule.StreamScheduler), driven by a scripted engine on the
CPU, and the C-ABI entries the schedule needs (header, exports and ctypes table, as tests/test_capi.py checks the others)."""
import random
import re
from pathlib import Path

import pytest

from dualhyp_amd.generate import generate_stream  # noqa: F401  (the schedule's public entry point)
from dualhyp_amd.schedule import ScriptedBackend, StreamScheduler, class_floor, predict, row_buckets

REPO = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("dh_engine_forward_slots", "dh_engine_decode_rows", "dh_sample_rows_bf16")


class Watch(ScriptedBackend):
    """ScriptedBackend that checks, call by call, what the device relies on"""

    def __init__(self, n_gen, sched):
        super().__init__(n_gen)
        self.sched = sched
        self.served, self.row_counts, self.had_decode_row = [], [], set()
        self.slot_history = {}                      # slot -> sequences that held it, in order

    def prefill(self, seqs, slots):
        assert 0 < len(seqs) == len(slots) <= self.sched.prefill_batch
        assert len(set(slots)) == len(slots) and all(0 <= s < self.sched.max_rows for s in slots), "the spare slot never holds a sequence"
        for u, s in zip(seqs, slots):
            prev = self.slot_history.setdefault(s, [])
            assert not prev or prev[-1] in self.sched.retired, f"slot {s} reused before sequence {prev[-1]} retired"
            prev.append(u)
        super().prefill(seqs, slots)                # asserts: served once, slot not occupied by a live sequence
        self.served += seqs

    def decode(self, row_seq, row_slot, n_steps):
        S = self.sched
        assert 0 < n_steps <= S.check_every and len(row_seq) == len(row_slot) <= S.max_rows
        live = [(u, s) for u, s in zip(row_seq, row_slot) if u != S.dummy_seq]
        pad = [(u, s) for u, s in zip(row_seq, row_slot) if u == S.dummy_seq]
        assert all(s == S.spare_slot for _, s in pad) and all(s != S.spare_slot for _, s in live), "the dummy row is the only padding"
        assert row_seq[:len(live)] == [u for u, _ in live], "padding comes last"
        assert len({u for u, _ in live}) == len(live) == len({s for _, s in live}), "a sequence or a slot appears in two rows"
        assert all(u in self.slot_of and not self._done(u) for u, _ in live), "a finished sequence takes a row"
        assert {u for u, _ in live} == set(self.slot_of), "a live sequence is left out of the step"
        self.row_counts.append(len(row_seq))
        self.had_decode_row |= {u for u, _ in live}
        super().decode(row_seq, row_slot, n_steps)


def run(n_gen, new, **kw):
    sched = StreamScheduler(len(n_gen), new, **kw)
    be = Watch(n_gen, sched)
    sched.run(be)
    assert be.served == list(range(len(n_gen))), "every prompt exactly once, in prompt order"
    assert sched.retired == set(range(len(n_gen))) and not sched.live and not sched.pending
    assert sorted(sched.free) == list(range(sched.max_rows))
    assert all(be.made[u] == n_gen[u] for u in range(len(n_gen))), "a sequence was stepped past its end or not to it"
    assert not be.had_decode_row & {u for u, g in enumerate(n_gen) if g == 1}, "a sequence done at its first pick took a decode row"
    assert set(be.row_counts) == sched.launch_rows and len(sched.launch_rows) <= 8
    assert sched.launch_rows <= set(sched.buckets)
    return sched, be


def test_row_steps_by_hand():
    """6 sequences, budget 10, 4 rows, prefills of 2, chunks of 4 steps; tokens produced (EOS included): 3 1 10 5 2 10.
    Buckets of 4 rows: 4 3 2 1.
      prefill 0,1 -> slots 0,1; prefill 2,3 -> slots 2,3; sequence 1 ended on its first pick: slot 1 free; prefill 4 -> slot 1
      chunk 1: live 0 2 3 4  -> 4 rows x 4 steps = 16;  0 (2 steps), 3 (4 steps), 4 (1 step) finish; slots 0 1 3 free
      prefill 5 -> slot 0
      chunk 2: live 2 5      -> 2 rows x 4 steps =  8
      chunk 3: live 2 5      -> 2 rows x 4 steps =  8   (sequence 2 spends its budget in the first of them and is frozen)
      chunk 4: live 5        -> 1 row  x 1 step  =  1   (the one step of budget sequence 5 has left)
    33 row-steps in 13 steps; generate_batch would run 6 rows x 9 steps = 54."""
    sched, be = run([3, 1, 10, 5, 2, 10], 10, max_rows=4, prefill_batch=2, check_every=4)
    assert [c for c in be.calls if c[0] == "prefill"] == [("prefill", [0, 1], [0, 1]), ("prefill", [2, 3], [2, 3]), ("prefill", [4], [1]),
                                                          ("prefill", [5], [0])]
    assert [c[1:] for c in be.calls if c[0] == "decode"] == [([0, 2, 3, 4], [0, 2, 3, 1], 4), ([2, 5], [2, 0], 4), ([2, 5], [2, 0], 4),
                                                            ([5], [0], 1)]
    assert (sched.decode_row_steps, sched.decode_steps, sched.launch_rows) == (33, 13, {4, 2, 1})
    assert predict([3, 1, 10, 5, 2, 10], 10, 4, 2, 4).decode_row_steps == 33


def test_padding_rows_by_hand():
    """7 live rows of 8 are launched at the 8-row bucket (8 6 5 4 3 2 1): one dummy row, which names the spare slot"""
    sched, be = run([2, 9, 9, 9, 9, 9, 9, 9], 9, max_rows=8, prefill_batch=8, check_every=4)
    dec = [c for c in be.calls if c[0] == "decode"]
    assert dec[0][1:] == (list(range(8)), list(range(8)), 4)
    assert dec[1][1:] == ([1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8], 4)        # sequence 8 = the dummy, slot 8 = the spare one
    assert sched.decode_row_steps == 8 * 4 + 8 * 4 and sched.buckets == [8, 6, 5, 4, 3, 2, 1]


@pytest.mark.parametrize("seed", range(40))
def test_random_scripts(seed):
    rnd = random.Random(seed)
    n, new = rnd.randint(1, 400), rnd.randint(1, 30)
    n_gen = [rnd.choice((1, rnd.randint(1, new), new)) for _ in range(n)]
    kw = dict(max_rows=rnd.choice((1, 2, 4, 16, 64, 200, 640)), prefill_batch=rnd.choice((1, 8, 64)), check_every=rnd.choice((1, 3, 16)))
    sched, be = run(n_gen, new, **kw)
    # the row-steps, from the script alone: every chunk's bucket times its steps
    total = sum(len(c[1]) * c[3] for c in be.calls if c[0] == "decode")
    assert sched.decode_row_steps == total == predict(n_gen, new, **kw).decode_row_steps
    # every live sequence is in every step until it ends: at least the steps the sequences need, summed
    assert sched.decode_row_steps >= sum(g - 1 for g in n_gen)


def test_corner_cases():
    sched, _ = run([5] * 12, 24, max_rows=12, prefill_batch=64, check_every=16)        # every sequence finishes in one chunk
    assert (sched.decode_steps, sched.decode_row_steps, sched.prefill_calls) == (16, 12 * 16, 1)
    sched, be = run([3, 7, 1, 4], 8, max_rows=1, prefill_batch=4, check_every=2)        # one row: the sequences one after the other
    assert sched.buckets == [1] and sched.launch_rows == {1}
    assert sched.decode_steps == sched.decode_row_steps == 2 + 6 + 0 + 4               # 3 -> 2 steps, 7 -> 6, 1 -> none, 4 -> 3 in chunks of 2
    sched, _ = run([6, 2, 9], 9, max_rows=640, prefill_batch=64, check_every=4)         # fewer prompts than max_rows: 3 rows, 3 slots
    assert sched.max_rows == 3 and sched.spare_slot == 3 and sched.buckets == [3, 2, 1]
    assert sched.decode_row_steps == 3 * 4 + 2 * 4                                      # 2 ends in chunk 1, 6 and 9 in chunk 2
    sched, be = run([1, 1, 1], 5, max_rows=2, prefill_batch=2, check_every=4)           # all done at the first pick: no decode at all
    assert sched.decode_steps == 0 and not any(c[0] == "decode" for c in be.calls)
    sched, be = run([1] * 7, 1, max_rows=4, prefill_batch=3, check_every=4)             # a budget of one token
    assert sched.decode_steps == 0 and sched.prefill_calls >= 3


def test_row_count_rules():
    for mr in (1, 2, 3, 7, 48, 128, 129, 640, 2048, 5000):
        for fp8 in (False, True):
            b = row_buckets(mr, class_floor(mr, fp8))
            assert b[0] == mr and len(b) <= 8 and b == sorted(set(b), reverse=True)
            assert all(3 * (x - y) <= x + 2 for x, y in zip(b, b[1:])), "a bucket step pads by more than a third"
            if fp8:
                assert all(x > 128 for x in b) or all(x <= 128 for x in b), "an fp8 call crosses the 128-row kernel boundary"
            else:
                assert all(x > 2048 for x in b) or all(x <= 2048 for x in b)
    assert row_buckets(640, 129)[-1] == 129 and min(row_buckets(128)) <= 16
    # an fp8 engine with more than 128 rows: the tail of the call is padded up to 129 rows, never launched below
    n_gen = [2] * 300 + [30] * 5
    sched, be = run(n_gen, 30, max_rows=200, prefill_batch=64, check_every=4, fp8=True)
    assert min(be.row_counts) == 129
    sched, be = run(n_gen, 30, max_rows=200, prefill_batch=64, check_every=4, fp8=False)
    assert min(be.row_counts) < 129
    sched, be = run(n_gen, 30, max_rows=128, prefill_batch=64, check_every=4, fp8=True)
    assert max(be.row_counts) <= 128


def test_new_abi_entries_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "dualhyp_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text))
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/dualhyp_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is missing from the ctypes table"
    assert declared == set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6
