"""Nucleus and min-p sampling on the GPU, op level (include/dualhyp_hip.h, "Nucleus and min-p").  Every comparison is torch.equal.

The yardstick is the header's equivalence: a pick under (top_k, top_p, min_p) is, bit for bit, the masked sampler's pick with top_k off
under a mask that allows exactly the kept set.  The kept set comes from the fp64 host model (tests/nucleus_reference.py), every case
of which is decided under the derived band (tests/test_nucleus_reference.py); the masked sampler is pinned by test_hip_constrain.py
and, through it, test_hip_sampling.py."""
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
import ngram_reference as NG  # noqa: E402
import nucleus_reference as NR  # noqa: E402
import sampling_reference as SR  # noqa: E402
from dualhyp_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")


def state(n_seq, tok_ld=2, length=0, done=0, fill=-1):
    i32 = dict(dtype=torch.int32, device=DEV)
    tokens = torch.full((n_seq, tok_ld), fill, dtype=torch.int64, device=DEV)
    length = torch.full((n_seq,), length, **i32) if isinstance(length, int) else torch.tensor(length, **i32)
    done = torch.full((n_seq,), done, **i32) if isinstance(done, int) else torch.tensor(done, **i32)
    return tokens, length, done


def same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def expand(row, n):
    return row.to(DEV).view(1, -1).expand(n, -1).contiguous()


def keep_mask_rows(keep, n):
    """the packed mask of one kept set, one row per sequence"""
    return CR.pack_bits(keep[None]).to(DEV).expand(n, -1).contiguous()


# the cases grouped by what they share: the logits of a launch (row, rows per launch) and the sampler's (top_k, temperature)
def _groups():
    out = OrderedDict()
    for c in NR.cases():
        out.setdefault((c.row, c.top_k, c.temperature, c.n_seq), []).append(c)
    return out


GROUPS = _groups()


def _gid(key):
    row, top_k, T, n = key
    return f"{row}.k{top_k}.T{T}"


# ---- 1. the plain entry against the masked sampler under the host model's kept set ---------------------------------------------------
@pytest.mark.parametrize("key", list(GROUPS), ids=_gid)
def test_the_pick_is_the_masked_pick_under_the_kept_set(key):
    row_key, top_k, T, n = key
    row = NR.rows()[row_key]
    lg = expand(row, n)
    eos = int(torch.argmax(row.float()))            # some sequences end on it: done is compared too
    for c in GROUPS[key]:
        keep = NR.case_keep(c)
        assert keep.any()
        mask = keep_mask_rows(keep, n)
        seen = set()
        for seed in NR.SEEDS:
            for step in NR.STEPS:
                got, want = state(n), state(n)
                ops.sample(lg, *got, temperature=T, top_k=top_k, eos_id=eos, seed=seed, step=step, top_p=c.top_p, min_p=c.min_p)
                ops.sample(lg, *want, temperature=T, top_k=None, eos_id=eos, seed=seed, step=step, mask=mask)
                assert same_state(got, want), (c.name, seed, step, int((got[0] != want[0]).sum()))
                assert got[1].tolist() == [1] * n
                if c.chunky:
                    seen |= set(got[0][:, 0].tolist())
        if c.chunky:        # every kept entry carries at least 2 % of the mass: all of them come out, and nothing else
            assert seen == set(np.flatnonzero(keep).tolist()), c.name


# ---- 2. the row-list entry ------------------------------------------------------------------------------------------------------------
ROW_CASES = [c for c in NR.cases() if c.name.startswith(("crafted.V1000", "V515")) or c.name in (
    "V32000.k50.T1.7.u3.p0.9.m0.05", "V32064.knone.T0.2.g4.p0.5.m0.0", "V128256.k200.T1.0.u3.p0.95.m0.05", "V256.k5.T0.8.u3.p0.9.m1.0")]


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c.name)
def test_the_row_list_entry(case):
    """a shuffled row_seq, padding rows (no sequence, and a finished one named twice), finished sequences, sequences at different
    places of their budgets: the draw is keyed by (seed, tokens generated so far, sequence)"""
    c = case
    n_seq, max_new, tok_ld = 40, 6, 12
    g = torch.Generator().manual_seed(len(c.name))
    order = torch.randperm(n_seq, generator=g).tolist()
    row_seq = order[:30] + [-1, n_seq, order[30], order[30], order[31]] + order[32:]
    n_rows = len(row_seq)
    prompt = [2 + u % 5 for u in range(n_seq)]
    generated = [u % max_new for u in range(n_seq)]
    length0 = [p + m for p, m in zip(prompt, generated)]
    limit = torch.tensor([p + max_new for p in prompt], dtype=torch.int32, device=DEV)
    done0 = [0] * n_seq
    for u in (order[30], order[3], order[17]):
        done0[u] = 2
    keep = NR.case_keep(c)
    mask = keep_mask_rows(keep, n_seq)
    lg = expand(NR.rows()[c.row], n_rows)
    rs = torch.tensor(row_seq, dtype=torch.int32, device=DEV)
    eos = int(torch.argmax(NR.rows()[c.row].float()))
    for seed in NR.SEEDS:
        got, want = state(n_seq, tok_ld, length0, done0), state(n_seq, tok_ld, length0, done0)
        ops.sample_rows(lg, *got, limit, rs, max_new, temperature=c.temperature, top_k=c.top_k, eos_id=eos, seed=seed,
                        top_p=c.top_p, min_p=c.min_p)
        ops.sample_rows(lg, *want, limit, rs, max_new, temperature=c.temperature, top_k=None, eos_id=eos, seed=seed, mask=mask)
        assert same_state(got, want), (c.name, seed)
        live = [u for u in range(n_seq) if not done0[u]]
        assert got[1].tolist() == [length0[u] + (0 if done0[u] else 1) for u in range(n_seq)]
        picked = got[0][torch.tensor(live), torch.tensor([length0[u] for u in live])].tolist()
        assert all(keep[t] for t in picked)
        # the same sequence at the same place in a plain launch of its own: (seed, step, seq) is all the draw knows
        u = live[0]
        one = state(n_seq)
        ops.sample(expand(NR.rows()[c.row], n_seq), *one, temperature=c.temperature, top_k=c.top_k, seed=seed, step=generated[u],
                   top_p=c.top_p, min_p=c.min_p)
        assert int(one[0][u, 0]) == int(got[0][u, length0[u]])


# ---- 3. composition with the token mask and the n-gram ban ---------------------------------------------------------------------------
def _composed(V, n):
    g = torch.Generator().manual_seed(V)
    raw = (torch.randn((n, V), generator=g, dtype=torch.float64) * 2.5).to(BF)
    allowed = torch.rand((n, V), generator=g) < 0.5
    best = torch.argsort(torch.where(allowed, raw.float(), torch.tensor(-1e9)), dim=1, descending=True)[:, :3]
    allowed[torch.arange(n), best[:, 0]] = True
    # the generated text is [a, b, a]: with no_repeat_ngram = 2 the best allowed token b is banned
    prompts = [[1, 2, 3][:1 + u % 3] for u in range(n)]
    texts = [[int(best[u, 1]), int(best[u, 0]), int(best[u, 1])] if u % 4 else [int(best[u, 1])] for u in range(n)]
    return raw, allowed.numpy(), prompts, texts


def _buffers(prompts, texts, tok_ld):
    n = len(prompts)
    tokens = torch.zeros((n, tok_ld), dtype=torch.int64)
    for u, (p, t) in enumerate(zip(prompts, texts)):
        tokens[u, :len(p) + len(t)] = torch.tensor(p + t)
    start = torch.tensor([len(p) for p in prompts], dtype=torch.int32, device=DEV)
    length = torch.tensor([len(p) + len(t) for p, t in zip(prompts, texts)], dtype=torch.int32, device=DEV)
    return tokens.to(DEV), length, torch.zeros(n, dtype=torch.int32, device=DEV), start


@pytest.mark.parametrize("V", [1000, 32000])
@pytest.mark.parametrize("top_k,top_p,min_p", [(None, 0.9, None), (50, 0.5, 0.05), (None, None, 0.2), (200, 0.95, 1.0)])
def test_mask_and_ban_reach_the_pick_as_minus_infinity(V, top_k, top_p, min_p):
    n, tok_ld, K = 48, 8, 4
    raw_cpu, allowed, prompts, texts = _composed(V, n)
    raw = raw_cpu.to(DEV)
    mask = CR.pack_bits(allowed).to(DEV)
    kw = dict(temperature=0.8, top_k=top_k, seed=SR.SEEDS[1], step=3, top_p=top_p, min_p=min_p)

    def run(lg, **more):
        tokens, length, done, start = _buffers(prompts, texts, tok_ld)
        lp = torch.full((n, tok_ld), NAN, dtype=torch.float32, device=DEV)
        top = (torch.full((n, tok_ld, K), -1, dtype=torch.int32, device=DEV), torch.full((n, tok_ld, K), NAN, dtype=torch.float32, device=DEV))
        if "no_repeat_ngram" in more:
            more["start"] = start
        ops.sample(lg, tokens, length, done, logprobs=lp, top_logprobs=top, **kw, **more)
        return tokens, length, done, lp, top

    lens = torch.tensor([len(p) + len(t) for p, t in zip(prompts, texts)], device=DEV)
    at = torch.arange(n, device=DEV)
    for rows_allowed, more in ((allowed, dict(mask=mask)), (NG.pick_rows(None, texts, 2, V), dict(no_repeat_ngram=2)),
                               (NG.pick_rows(allowed, texts, 2, V), dict(mask=mask, no_repeat_ngram=2))):
        sub = CR.substitute(raw, CR.pack_bits(rows_allowed).to(DEV))
        got, want = run(raw, **more), run(sub)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), sorted(more)
        picks = got[0][at, lens]
        assert bool(torch.from_numpy(rows_allowed).to(DEV)[at, picks].all())
        # the log-probabilities and the alternatives are the raw row's
        assert same_bits(got[3][at, lens], ops.token_logprobs(raw, picks))
        t_ids, t_lp = ops.token_top_logprobs(raw, K)
        assert torch.equal(got[4][0][at, lens], t_ids) and same_bits(got[4][1][at, lens], t_lp)
    # the ban mattered: the best allowed token of the sequences with a history differs from the banned run's pick set
    banned = NG.pick_rows(allowed, texts, 2, V)
    assert (banned != allowed).any()


# ---- 4. off is off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.grid_cases(), ids=lambda c: c.name)
def test_off_is_the_call_without_the_arguments(case):
    lg = expand(SR.case_row(case), case.n_seq)
    for seed in NR.SEEDS[:1]:
        for step in NR.STEPS:
            base = state(case.n_seq)
            ops.sample(lg, *base, temperature=case.temperature, top_k=case.top_k, seed=seed, step=step)
            for kw in (dict(top_p=1.0, min_p=0.0), dict(top_p=None, min_p=None), dict(top_p=1.0), dict(min_p=0)):
                got = state(case.n_seq)
                ops.sample(lg, *got, temperature=case.temperature, top_k=case.top_k, seed=seed, step=step, **kw)
                assert same_state(got, base), (case.name, kw)


def test_off_is_off_through_the_c_entry_and_the_row_list():
    """top_p = 1, min_p = 0 passed to the new entries themselves: each is the entry it extends"""
    from dualhyp_amd import _lib
    lib = _lib.load()
    c = SR.grid_cases()[12]
    n = 64
    lg = expand(SR.case_row(c), n)
    base, got = state(n), state(n)
    ops.sample(lg, *base, temperature=c.temperature, top_k=c.top_k, seed=7, step=2)
    _lib.check(lib.dh_sample_bf16_nucleus(lg.data_ptr(), c.vocab, got[0].data_ptr(), 2, got[1].data_ptr(), got[2].data_ptr(), n,
                                          c.temperature, c.top_k or 0, -1, 7, 2, None, None, 0, None, None, None, 0, 0, None, None, 1.0, 0.0))
    torch.cuda.synchronize()
    assert same_state(got, base)
    limit = torch.full((n,), 2, dtype=torch.int32, device=DEV)
    rs = torch.arange(n, dtype=torch.int32, device=DEV)
    base, got = state(n), state(n)
    ops.sample_rows(lg, *base, limit, rs, 2, temperature=c.temperature, top_k=c.top_k, seed=7)
    ops.sample_rows(lg, *got, limit, rs, 2, temperature=c.temperature, top_k=c.top_k, seed=7, top_p=1.0, min_p=0.0)
    assert same_state(got, base)


# ---- 5. the arg-max takes neither ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [515, 1000, 32000])
def test_top_k_1_is_the_arg_max_of_today(V):
    g = torch.Generator().manual_seed(V)
    lg = ((torch.rand((37, V), generator=g, dtype=torch.float64) * 2 - 1) * 3).to(BF).to(DEV)
    base = state(37)
    ops.sample(lg, *base, temperature=0.2, top_k=1, seed=1, step=1)
    for top_p, min_p in ((0.5, None), (None, 1.0), (0.01, 0.9), (0.95, 0.05)):
        got = state(37)
        ops.sample(lg, *got, temperature=0.2, top_k=1, seed=1, step=1, top_p=top_p, min_p=min_p)
        assert same_state(got, base)
    assert base[0][:, 0].tolist() == [SR.argmax_ref(SR.scaled(r, 0.2)) for r in lg.cpu()]


# ---- 6. determinism and placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["V32000.k50.T1.7.u3.p0.9.m0.05", "V32000.knone.T0.2.g4.p0.5.m0.0", "V32000.k200.T1.0.u3.p0.95.m0.0"])
def test_the_same_launch_twice_and_a_row_at_an_unaligned_offset(name):
    c = next(x for x in NR.cases() if x.name == name)
    row, n = NR.rows()[c.row], 96
    lg = expand(row, n)
    kw = dict(temperature=c.temperature, top_k=c.top_k, seed=NR.SEEDS[0], step=5, top_p=c.top_p, min_p=c.min_p)
    a, b = state(n), state(n)
    ops.sample(lg, *a, **kw)
    ops.sample(lg, *b, **kw)
    assert same_state(a, b)
    # V = 32000 rows one bf16 into the allocation: 2 bytes off a 16-byte boundary, the scalar loads
    V = row.numel()
    buf = torch.zeros(n * V + 1, dtype=BF, device=DEV)
    shifted = buf[1:].view(n, V)
    shifted.copy_(lg)
    assert shifted.data_ptr() % 16 == 2 and lg.data_ptr() % 16 == 0
    s = state(n)
    ops.sample(shifted, *s, **kw)
    assert same_state(a, s)
    # and fewer rows, elsewhere in the launch: the kept set is the row's alone
    few = state(5)
    ops.sample(lg[40:45].contiguous(), *few, **kw)
    ref = state(n)
    ops.sample(lg, *ref, **dict(kw, top_p=None, min_p=None, top_k=None), mask=keep_mask_rows(NR.case_keep(c), n))
    assert same_state(a, ref)
    assert all(NR.case_keep(c)[t] for t in few[0][:, 0].tolist())


# ---- 7. refusals leave the buffers alone --------------------------------------------------------------------------------------------
def test_refusals_before_any_launch_leave_the_buffers_untouched():
    from dualhyp_amd import _lib
    lib = _lib.load()
    lg = expand(SR.case_row(SR.grid_cases()[0]), 8)
    V = lg.size(1)
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=NAN), dict(min_p=-0.5), dict(min_p=2.0), dict(min_p=NAN)):
        s = state(8)
        with pytest.raises(ValueError):
            ops.sample(lg, *s, top_k=40, **kw)
        limit = torch.full((8,), 2, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError):
            ops.sample_rows(lg, *s, limit, torch.arange(8, dtype=torch.int32, device=DEV), 2, top_k=40, **kw)
        torch.cuda.synchronize()
        assert same_state(s, state(8))
    for top_p, min_p in ((0.0, 0.0), (NAN, 0.0), (0.9, 1.5), (0.9, NAN)):
        s = state(8)
        rc = lib.dh_sample_bf16_nucleus(lg.data_ptr(), V, s[0].data_ptr(), 2, s[1].data_ptr(), s[2].data_ptr(), 8, 1.0, 40, -1, 0, 0, None,
                                        None, 0, None, None, None, 0, 0, None, None, top_p, min_p)
        assert rc != 0 and (b"top_p=" in lib.dh_last_error() or b"min_p=" in lib.dh_last_error())
        torch.cuda.synchronize()
        assert same_state(s, state(8))


# ---- 8. rows outside the definition still give an id ------------------------------------------------------------------------------
def test_nan_and_all_minus_infinity_rows_give_an_id_inside_the_vocabulary():
    """NaN rows, rows of -inf and rows whose allowed logits are all -inf stay outside the definition, as they are for the sampler
    without the crop; the pick is an id in [0, vocab) and the launch ends"""
    for V in (515, 32000):
        g = torch.Generator().manual_seed(V)
        lg = (torch.randn((6, V), generator=g) * 3).to(BF)
        lg[0] = -float("inf")
        lg[1, ::3] = NAN
        lg[2] = NAN
        lg[3, 5:] = -float("inf")
        allowed = np.ones((6, V), dtype=bool)
        allowed[3, :5] = False                      # what row 3 allows is all -inf
        allowed[4, 1:] = False                      # one allowed id
        mask = CR.pack_bits(allowed).to(DEV)
        for kw in (dict(top_p=0.9), dict(min_p=0.5), dict(top_p=0.5, min_p=0.05)):
            for top_k in (None, 50):
                s = state(6)
                ops.sample(lg.to(DEV), *s, temperature=0.8, top_k=top_k, seed=3, step=1, mask=mask, **kw)
                ids = s[0][:, 0].tolist()
                assert all(0 <= t < V for t in ids) and s[1].tolist() == [1] * 6, (V, kw, ids)
                assert ids[4] == 0
