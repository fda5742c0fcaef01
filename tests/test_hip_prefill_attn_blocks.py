"""The prefill attention's barrier domain (csrc/attention.hip, attn_prefill_kernel<HS, PS, WPB>; dh_set_tuning 42).

Key 42 chooses how many waves (query heads of one KV group) share a block and its K / V^T stages: 0 is the whole group, 2 and 4
split it over q_per_kv / WPB blocks.  A wave computes exactly what it computes in the whole-group block, so y and lse of every arm
have to equal arm 0's bit for bit, at every head layout: also where the arm does not divide the group's heads (the launcher falls
back to the whole group) and at head size 96 (one kernel, the key is ignored)."""
import functools
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

DEV = "cuda:0"
KEY, DEFAULT, ARMS = 42, 4, (2, 4)
# (head size, query heads, KV groups): 8 heads of one group (arm 4: two blocks, arm 2: four), TinyLlama's 32 / 4, head size 128
# with four heads per group (arm 4 is the whole group as a fixed-size block), and six heads that arm 4 does not divide
LAYOUTS = ((64, 8, 1), (64, 32, 4), (128, 8, 2), (64, 6, 1))
CASES = ("packed", "continuation")


def _set(arm):
    from dualhyp_amd import _lib
    _lib.check(_lib.load().dh_set_tuning(KEY, arm))


@pytest.fixture(autouse=True)
def _default_afterwards():
    yield
    _set(DEFAULT)


def _fill(hs, n_head, n_groups, slots, s_max, tok_slot, tok_pos, gen):
    """Random q / k / v rows through ops.qkv_rope_cache: rotated q, and the two fragment-order caches filled in place."""
    from dualhyp_amd import ops
    rn = lambda *s: (torch.randn(*s, device=DEV, generator=gen) * 0.5).bfloat16()
    kc = torch.zeros(slots, n_groups, s_max, hs, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(slots, n_groups, hs, s_max, device=DEV, dtype=torch.bfloat16)
    cos, sin = rn(s_max, hs), rn(s_max, hs)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    q = ops.qkv_rope_cache(rn(len(tok_slot), (n_head + 2 * n_groups) * hs), cos, sin, i32(tok_slot), i32(tok_pos), kc, vt, n_head, n_groups)
    return q, kc, vt


@functools.lru_cache(maxsize=None)
def _inputs(hs, n_head, n_groups, case):
    gen = torch.Generator(device=DEV).manual_seed(11)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    if case == "packed":
        # one call, three sequences: a one-step block of one query, a diagonal tile that crosses the 32- and the 64-key edge, and
        # three key steps (both stage buffers used twice)
        lens = (1, 33, 130)
        tok_slot = [s for s, n in enumerate(lens) for _ in range(n)]
        tok_pos = [p for n in lens for p in range(n)]
        q, kc, vt = _fill(hs, n_head, n_groups, 3, 192, tok_slot, tok_pos, gen)
        meta = (i32([0, 1, 2]), i32([0, 1, 34]), i32(lens), i32([0, 0, 0]), 130)
    else:
        # a chunk of 50 queries behind 40 cached positions: the mask starts on an unaligned key, the cache holds both parts
        q, kc, vt = _fill(hs, n_head, n_groups, 1, 128, [0] * 90, list(range(90)), gen)
        q = q[40:].contiguous()
        meta = (i32([0]), i32([0]), i32([50]), i32([40]), 50)
    return q, kc, vt, meta


def _run(arm, hs, n_head, n_groups, case):
    from dualhyp_amd import ops
    q, kc, vt, (slot, qs, ql, p0, max_q) = _inputs(hs, n_head, n_groups, case)
    _set(arm)
    lse = torch.full((q.size(0), n_head), float("nan"), device=DEV)
    y = ops.attn_prefill(q, kc, vt, slot, qs, ql, p0, max_q, lse=lse)
    torch.cuda.synchronize()
    return y, lse


@functools.lru_cache(maxsize=None)
def _arm0(hs, n_head, n_groups, case):
    y, lse = _run(0, hs, n_head, n_groups, case)
    assert torch.isfinite(y.float()).all() and torch.isfinite(lse).all() and y.float().abs().max() > 0
    return y, lse


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("hs,n_head,n_groups", LAYOUTS)
def test_every_arm_gives_the_bits_of_the_whole_group_block(hs, n_head, n_groups, case, arm):
    y0, lse0 = _arm0(hs, n_head, n_groups, case)
    y, lse = _run(arm, hs, n_head, n_groups, case)
    assert torch.equal(y, y0), f"y of arm {arm} differs from arm 0 in {(y != y0).sum().item()} of {y.numel()} elements"
    assert torch.equal(lse, lse0), f"lse of arm {arm} differs from arm 0"


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ARMS)
def test_head_size_96_ignores_the_key(arm):
    y0, lse0 = _arm0(96, 4, 4, "packed")
    y, lse = _run(arm, 96, 4, 4, "packed")
    assert torch.equal(y, y0) and torch.equal(lse, lse0)


def test_key_42_takes_0_2_4_only():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    try:
        assert all(lib.dh_set_tuning(KEY, v) == 0 for v in (0, 2, 4))
        assert all(lib.dh_set_tuning(KEY, v) != 0 for v in (-1, 1, 3, 8))
        assert b"42" in lib.dh_last_error()
    finally:
        lib.dh_set_tuning(KEY, DEFAULT)
