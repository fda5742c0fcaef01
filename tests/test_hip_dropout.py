"""dh_dropout_bf16 bit for bit against tests/dropout_reference.py (the draw as include/dualhyp_hip.h defines it): every mask and
every output element, at one chunk, at a ragged last block and on the second trip of the kernel's 4096-block grid-stride loop;
at the edges of p, seed, call_id and the device step; on zeros, subnormals, the largest finite value, infinities and NaNs; the
separation of the call sites and steps a 22-layer model uses; and the refusals.

Comparisons are on the bf16 BIT PATTERNS (a dropped -0 must be +0), except at NaN outputs, which are compared by position: the
payload of a NaN product is the hardware's.

hi32(c), the second counter word's upper part, needs a call of 2^35 elements (64 GiB of bf16 per tensor): it is not reachable in a
test and is held by the reference's scalar form only (test_dropout_reference.test_draws_follow_the_element_layout)."""
import pytest
import torch

import dropout_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ONE, RAGGED = 8, 8 * 257
BIG = 8 * (4096 * 256 + 300)          # 8 391 008: 300 chunks are left for the grid-stride loop's second trip
SEED_LO, SEED_HI, SEED_MAX = 1337, (7 << 32) | 9, 2 ** 63 - 1
STEP_HI = 2 ** 32 + 5
P_ALL = (0.0, 1e-10, 0.05, 0.5, 0.999)
SEEDS = (SEED_LO, SEED_HI, SEED_MAX)
CALL_IDS = (0, 1, 43, 0xffffffff)          # the last wraps both the multiply and the add of the key
STEPS = (None, 0, 1, STEP_HI)

# +-0, the smallest / largest bf16 subnormals, the largest finite values, infinities, NaNs (quiet and signalling patterns), 1
SPECIAL_BITS = [0x0000, 0x8000, 0x0001, 0x007F, 0x8001, 0x807F, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81, 0x3F80, 0x0080, 0xBF80]


def _bits(v):
    return torch.tensor([b - 0x10000 if b >= 0x8000 else b for b in v], dtype=torch.int16).view(torch.bfloat16)


_X = {}


def make_x(n: int) -> torch.Tensor:
    """bf16 [n] on the CPU, made once per size: the special values repeated over the first half (every one of them is kept
    somewhere and dropped somewhere at p = 0.5 and 0.05), random normals behind them."""
    if n == ONE:
        return _bits([0x8000, 0x0000, 0x0001, 0x7F7F, 0x7F80, 0xFF80, 0x7FC0, 0x3F80])
    if n not in _X:
        x = torch.randn(n, generator=torch.Generator().manual_seed(n)).bfloat16()
        sp = _bits(SPECIAL_BITS)
        k = n // 2 // sp.numel()
        x[: k * sp.numel()] = sp.repeat(k)
        _X[n] = x
    return _X[n]


def run_hip(x, p, seed, call_id, step):
    from dualhyp_amd import ops
    st = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    y, m = ops.dropout(x.to(DEV), p, seed=seed, call_id=call_id, step=st)
    return y.cpu(), m.cpu()


def assert_same(x, p, seed, call_id, step):
    y, m = run_hip(x, p, seed, call_id, step)
    yr, mr = R.dropout(x, p, seed, call_id, step)
    what = (x.numel(), p, hex(seed), hex(call_id), step)
    assert torch.equal(m.view(torch.int16), mr.view(torch.int16)), f"mask {what}: {(m.view(torch.int16) != mr.view(torch.int16)).sum().item()} elements differ"
    nan = torch.isnan(yr)
    assert torch.equal(torch.isnan(y), nan), f"NaN positions {what}"
    bad = (y.view(torch.int16) != yr.view(torch.int16)) & ~nan
    assert not bad.any(), f"y {what}: {bad.sum().item()} elements differ, first at {bad.nonzero()[0].item()}"


def test_one_chunk_and_ragged_block_over_every_parameter():
    """The full product of p, seed, call_id and step at 8 * 257 elements (two blocks, the second ragged), and every p, seed,
    call_id and step at one chunk."""
    x = make_x(RAGGED)
    for p in P_ALL:
        for seed in SEEDS:
            for cid in CALL_IDS:
                for step in STEPS:
                    assert_same(x, p, seed, cid, step)
    x1 = make_x(ONE)
    for i in range(20):
        assert_same(x1, P_ALL[i % 5], SEEDS[i % 3], CALL_IDS[i % 4], STEPS[(i // 4) % 4])


# every value of p, seed, call_id and step at least once where the loop goes round
BIG_CASES = [(0.05, SEED_LO, 0, None), (0.0, SEED_HI, 1, 0), (1e-10, SEED_MAX, 43, 1), (0.5, SEED_LO, 0xffffffff, STEP_HI),
             (0.999, SEED_HI, 43, STEP_HI)]


@pytest.mark.parametrize("p,seed,call_id,step", BIG_CASES)
def test_second_grid_stride_trip(p, seed, call_id, step):
    assert BIG // 8 > 4096 * 256 and BIG // 8 - 4096 * 256 == 300
    assert_same(make_x(BIG), p, seed, call_id, step)


def test_threshold_is_inclusive_at_an_exact_draw():
    """Below 2^-8 every float p is a whole number of 2^-32 steps, so the threshold can be put exactly ON an element's draw: that
    element is kept at thresh = draw (>=) and dropped at thresh = draw + 1.  An off-by-one comparison shows nowhere else."""
    x = make_x(RAGGED)
    d = R.draws(RAGGED, SEED_LO, 3, 1)
    i = next(i for i in range(RAGGED) if 0 < int(d[i]) < 2 ** 24 - 1)
    t = int(d[i])
    for thresh, kept in ((t, True), (t + 1, False)):
        p = thresh / 2 ** 32
        assert R.thresh(p) == thresh and bool(R.keep_mask(RAGGED, p, SEED_LO, 3, 1)[i]) == kept
        assert_same(x, p, SEED_LO, 3, 1)
        assert bool(run_hip(x, p, SEED_LO, 3, 1)[1][i] != 0) == kept


def test_a_null_step_is_step_zero_and_shapes_do_not_matter():
    x = make_x(RAGGED)
    y0, m0 = run_hip(x, 0.05, SEED_LO, 3, None)
    y1, m1 = run_hip(x, 0.05, SEED_LO, 3, 0)
    assert torch.equal(m0, m1) and torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    y2, m2 = run_hip(x.view(257, 8), 0.05, SEED_LO, 3, 0)          # the element index is the flat one
    assert torch.equal(m2.view(-1), m0)


def test_call_sites_and_steps_draw_separate_masks():
    """The masks of call ids 0 .. 43 (22 layers x 2 sites) at steps 1 .. 4 of one seed: each IS the reference's mask for its
    (call id, step) and no two of the 176 are the same tensor — exact, not statistical."""
    from dualhyp_amd import ops
    n, p = RAGGED, 0.5
    x = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    seen = {}
    for step in (1, 2, 3, 4):
        st = torch.tensor([step], dtype=torch.int64, device=DEV)
        got = torch.stack([ops.dropout(x, p, seed=SEED_LO, call_id=cid, step=st)[1] for cid in range(44)]).cpu()
        for cid in range(44):
            keep = R.keep_mask(n, p, SEED_LO, cid, step)
            assert torch.equal(got[cid] != 0, keep), (cid, step)
            key = keep.numpy().tobytes()
            assert key not in seen, f"(call {cid}, step {step}) draws the mask of {seen.get(key)}"
            seen[key] = (cid, step)
        for a in range(44):
            for b in range(a + 1, 44):
                assert not torch.equal(got[a], got[b]), (a, b, step)
    assert len(seen) == 176


def test_refusals_write_nothing():
    """n % 8 != 0, p = 1, p < 0 and a NaN p return the error; y and mask keep the sentinel they were filled with."""
    from dualhyp_amd import _lib, ops
    lib = _lib.load()
    x = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    sentinel = _bits([0x5A5A])[0].item()
    stream = torch.cuda.current_stream().cuda_stream
    for n, p in ((12, 0.05), (60, 0.5), (64, 1.0), (64, -0.01), (64, float("nan")), (64, 1.5), (64, float("inf"))):
        y = torch.full((64,), sentinel, dtype=torch.bfloat16, device=DEV)
        m = torch.full((64,), sentinel, dtype=torch.bfloat16, device=DEV)
        rc = lib.dh_dropout_bf16(x.data_ptr(), y.data_ptr(), m.data_ptr(), n, p, SEED_LO, 3, None, stream)
        torch.cuda.synchronize()
        assert rc != 0 and b"dh_dropout_bf16" in lib.dh_last_error(), (n, p, rc)
        assert (y.view(torch.int16) == 0x5A5A).all() and (m.view(torch.int16) == 0x5A5A).all(), (n, p)
    for n, p in ((64, 1.0), (12, 0.05)):
        with pytest.raises(_lib.DualHypHipError, match="dh_dropout_bf16"):
            ops.dropout(x[:n], p, seed=1, call_id=0)
