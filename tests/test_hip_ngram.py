"""No-repeat n-grams in the samplers on the GPU (include/dualhyp_hip.h, "No-repeat n-grams").  Every check is exact (torch.equal).

A pick under no_repeat_ngram — with or without a token mask — is the UNMASKED pick, which test_hip_sampling.py pins to an fp64
reference, on constrain_reference.substitute(rows, mask minus banned): 0xFF80 in every column the mask disallows or the history bans,
the ban ignored where it would leave nothing (ngram_reference.pick_rows).  The token buffers are built on the host from
ngram_reference.history, which holds every hand-written case of test_ngram_host.py, the ban's n-grams planted in the prompt part
included (`start` must be honoured).  The log-probabilities and alternatives are those of the raw rows."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import constrain_reference as CR  # noqa: E402
import ngram_reference as R  # noqa: E402
import sampling_reference as SR  # noqa: E402
import top_logprob_reference as T  # noqa: E402
from dualhyp_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
VOCABS = (8, 320, 1001, 32000)       # the smallest; the 16-byte path; the scalar path with a partial last word; production
ROW_COUNTS = (1, 3, 37)
NGRAMS = (1, 2, 3, 4)
TEMPERATURES = (1.0, 0.2)
TOK_LD = 48                          # the longest prompt (2 * 4 - 1 + ...) and history (16) of ngram_reference.history, and the pick

_ROWS = {}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def rows_for(V, n):
    """bf16 rows [n, V] on the CPU, made once: the kinds of top_logprob_reference (random rows, rows of many equal values, +-0, -inf)
    and, in the 37-row case, sampling_reference's heavily tied uniform row and its peaked Gaussian one"""
    if (V, n) not in _ROWS:
        rows = T.case(V, n, min(5, V))[0].clone()
        if n == 37:
            rows[35] = SR.case_row(SR.Case("u3", V, 5, 1.0, "u3", 1))
            rows[36] = SR.case_row(SR.Case("g4", V, None, 1.0, "g4", 1))
        _ROWS[(V, n)] = rows
    return _ROWS[(V, n)]


def hot_ids(row_cpu):
    """the three ids a sampler most likely picks from the row: its largest values, lowest index first among equals (NaN-free rows)"""
    f = row_cpu.double()
    f = torch.where(torch.isnan(f), torch.full_like(f, -float("inf")), f)
    return torch.sort(f, descending=True, stable=True)[1][:3].tolist()


def buffers(prompts, texts, tok_ld=TOK_LD):
    """(tokens, length, done, start) of sequences whose rows hold prompt + generated text, -1 behind"""
    n = len(prompts)
    tokens = torch.full((n, tok_ld), -1, dtype=torch.int64)
    for u, (p, g) in enumerate(zip(prompts, texts)):
        assert len(p) + len(g) < tok_ld
        tokens[u, :len(p) + len(g)] = torch.tensor(p + g, dtype=torch.int64)
    length = torch.tensor([len(p) + len(g) for p, g in zip(prompts, texts)], dtype=torch.int32)
    start = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    return tokens.to(DEV), length.to(DEV), torch.zeros(n, dtype=torch.int32, device=DEV), start.to(DEV)


def base_masks(kind, raw_cpu, texts, ngram):
    """bool [n, V] or None: the token mask of a case.  exactly_banned (the fallback): a row allows exactly its ban set where that is
    not empty."""
    n, V = raw_cpu.shape
    if kind == "none":
        return None
    if kind == "random_half":
        return CR.unpack_bits(CR.make_masks("random_half", raw_cpu), V)
    assert kind == "exactly_banned"
    a = np.ones((n, V), dtype=bool)
    for u, g in enumerate(texts):
        b = R.banned(g, ngram)
        if b:
            a[u] = False
            a[u, sorted(b)] = True
    return a


def pack_with_garbage(allowed):
    """the packed mask with every bit at and behind vocab set: the kernel must not count them as allowed ids"""
    m = CR.pack_bits(allowed)
    V = allowed.shape[1]
    if V % 32:
        m[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)
    return m


def defined_rows(sub):
    """rows with at least one allowed logit above -inf; the others are outside the definition"""
    return (sub.float() > -float("inf")).any(dim=1)


def bufs(shape, k):
    return (torch.full(shape, NAN, dtype=torch.float32, device=DEV), torch.full(shape + (k,), -1, dtype=torch.int32, device=DEV),
            torch.full(shape + (k,), NAN, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_is_the_unmasked_pick_on_mask_minus_banned(V, top_k):
    k_top = min(3, V)
    moved = fell = with_ban = 0
    for n in ROW_COUNTS:
        raw_cpu = rows_for(V, n)
        raw = raw_cpu.to(DEV)
        raw_top = ops.token_top_logprobs(raw, k_top)
        hots = [hot_ids(raw_cpu[u]) for u in range(n)]
        ar = torch.arange(n, device=DEV)
        for ngram in NGRAMS:
            prompts, texts = R.histories(n, ngram, lambda u: hots[u], V, offset=3 * n + ngram)
            for kind in ("none", "random_half") + (("exactly_banned",) if V == 8 else ()):
                base = base_masks(kind, raw_cpu, texts, ngram)
                rows = R.pick_rows(base, texts, ngram, V)
                sub = CR.substitute(raw, CR.pack_bits(rows).to(DEV))
                ok = defined_rows(sub)
                m = None if base is None else pack_with_garbage(base).to(DEV)
                for u, g in enumerate(texts):
                    with_ban += bool(R.banned(g, ngram))
                    fell += R.pick_row(None if base is None else base[u], g, ngram, V)[1]
                for temp in TEMPERATURES:
                    kw = dict(temperature=temp, top_k=top_k, seed=SR.SEEDS[1], step=7)
                    want = buffers(prompts, texts)
                    ops.sample(sub, *want[:3], **kw)
                    got = buffers(prompts, texts)
                    lp, t_ids, t_lp = bufs(tuple(got[0].shape), k_top)
                    ops.sample(raw, *got[:3], logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m, no_repeat_ngram=ngram, start=got[3], **kw)
                    what = f"V={V} n={n} ngram={ngram} mask={kind} T={temp} top_k={top_k}"
                    at = (got[1] - 1).long()
                    picked = got[0][ar, at]
                    assert bool(((picked >= 0) & (picked < V)).all()), what
                    for x, y, name in zip(got[:3], want[:3], ("tokens", "length", "done")):
                        assert torch.equal(x[ok], y[ok]), f"{what}: {name}\n{x[ok]}\n{y[ok]}"
                    assert bool(torch.from_numpy(rows).to(DEV)[ar, picked][ok].all()), f"{what}: a disallowed or banned id was picked"
                    # the log-probability is the raw row's, the alternatives are the raw row's
                    assert same_bits(lp[ar, at], ops.token_logprobs(raw, picked)), what
                    assert torch.equal(t_ids[ar, at], raw_top[0]) and same_bits(t_lp[ar, at], raw_top[1]), what
                    written = torch.zeros_like(got[0], dtype=torch.bool)
                    written[ar, at] = True
                    assert bool(torch.isnan(lp[~written]).all()) and bool((t_ids[~written] == -1).all()), what
                    if top_k == 1:                  # what the call without the feature picks
                        plain = buffers(prompts, texts)
                        ops.sample(raw, *plain[:3], mask=m, **kw)
                        moved += int((plain[0][ar, at] != picked)[ok].sum())
    assert with_ban > 0
    if V == 8:
        assert fell > 0                        # every id banned without a mask (n = 1), and the masks that allow exactly the ban set
    if top_k == 1:
        assert moved > 0                       # banning the arg-max moved the pick


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_rows_bans_from_the_sequences_own_history(V, top_k):
    """logits row r is picked under the mask row and the history of sequence row_seq[r]: a shuffled row list over more sequences than
    rows, a finished sequence named by two rows; start given, and left to limit - max_new_tokens"""
    k_top, max_new = min(3, V), 40
    for n in ROW_COUNTS:
        n_seq = n + 3
        g = torch.Generator().manual_seed(V * 64 + n)
        perm = torch.randperm(n_seq, generator=g)
        fin = int(perm[-1])                                    # the finished sequence, named by two padding rows when there is room
        order = perm[:n].tolist()
        if n >= 3:
            order[1] = order[-1] = fin
        row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
        raw_cpu = rows_for(V, n)
        raw = raw_cpu.to(DEV)
        raw_top = ops.token_top_logprobs(raw, k_top)
        by_seq = torch.zeros(n_seq, dtype=torch.long)          # the logits row that names sequence u (row 0 for the others)
        for r, u in enumerate(order):
            by_seq[u] = r
        hots = [hot_ids(raw_cpu[int(by_seq[u])]) for u in range(n_seq)]
        live = [r for r, u in enumerate(order) if u != fin]
        for ngram in NGRAMS:
            prompts, texts = R.histories(n_seq, ngram, lambda u: hots[u], V, offset=n + 2 * ngram)
            limit = torch.tensor([len(p) + max_new for p in prompts], dtype=torch.int32, device=DEV)

            def fresh():
                st = buffers(prompts, texts)
                st[2][fin] = 1
                return st

            for kind in ("none", "random_half") + (("exactly_banned",) if V == 8 else ()):
                base = base_masks(kind, raw_cpu[by_seq], texts, ngram)
                rows = R.pick_rows(base, texts, ngram, V)                                   # per SEQUENCE
                sub = CR.substitute(raw, CR.pack_bits(rows[np.array(order)]).to(DEV))       # per logits row
                ok = defined_rows(sub)
                m = None if base is None else pack_with_garbage(base).to(DEV)
                for temp in TEMPERATURES:
                    kw = dict(temperature=temp, top_k=top_k, seed=SR.SEEDS[0])
                    want = fresh()
                    ops.sample_rows(sub, *want[:3], limit, row_seq, max_new, **kw)
                    for given in (True, False):
                        got = fresh()
                        lp, t_ids, t_lp = bufs(tuple(got[0].shape), k_top)
                        ops.sample_rows(raw, *got[:3], limit, row_seq, max_new, logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m,
                                        no_repeat_ngram=ngram, start=got[3] if given else None, **kw)
                        what = f"V={V} n={n} ngram={ngram} mask={kind} T={temp} top_k={top_k} start={'given' if given else 'limit - max_new'}"
                        before = fresh()
                        for r in live:
                            u = order[r]
                            at = int(before[1][u])
                            pick = int(got[0][u, at])
                            assert 0 <= pick < V, what
                            if bool(ok[r]):
                                assert pick == int(want[0][u, at]) and int(got[1][u]) == int(want[1][u]) and int(got[2][u]) == int(want[2][u]), \
                                    f"{what}: row {r} sequence {u}: {pick}, want {int(want[0][u, at])}"
                                assert rows[u][pick], f"{what}: a disallowed or banned id was picked"
                            assert same_bits(lp[u, at], ops.token_logprobs(raw[r:r + 1], got[0][u, at:at + 1])[0]), what
                            assert torch.equal(t_ids[u, at], raw_top[0][r]) and same_bits(t_lp[u, at], raw_top[1][r]), what
                        assert torch.equal(got[0][fin], before[0][fin]) and int(got[1][fin]) == int(before[1][fin])
                        assert int((got[0] != before[0]).sum()) == len(live) and int((got[1] - before[1]).sum()) == len(live)


def test_a_history_longer_than_the_block():
    """more candidate positions than the block has threads (two trips of the candidate loop, the last one partial); a small alphabet
    gives hundreds of occurrences; ngram up to the largest"""
    V, n, m = 320, 3, 1500
    raw_cpu = rows_for(V, n)
    raw = raw_cpu.to(DEV)
    g = np.random.default_rng(12)
    for ngram in (1, 2, 5, 8):
        hots = [hot_ids(raw_cpu[u]) for u in range(n)]
        texts = []
        for u in range(n):
            al = hots[u] + [int(g.integers(0, V))]
            t = [int(al[int(v)]) for v in g.integers(0, 2 if ngram >= 5 else 4, m)]
            if u == 1:                                  # the one occurrence lies behind the first 1024 candidates
                t = [7] * m
                t[1100:1100 + ngram] = [9] * (ngram - 1) + [hots[u][0]]
                t[m - ngram + 1:] = [9] * (ngram - 1)
            texts.append(t)
        prompts = [[hots[u][0]] * (u + 1) for u in range(n)]
        rows = R.pick_rows(None, texts, ngram, V)
        assert all(R.banned(t, ngram) for t in texts) and hots[1][0] in R.banned(texts[1], ngram)
        sub = CR.substitute(raw, CR.pack_bits(rows).to(DEV))
        for top_k in (1, 5):
            kw = dict(temperature=1.0, top_k=top_k, seed=3, step=2)
            want = buffers(prompts, texts, tok_ld=m + 8)
            ops.sample(sub, *want[:3], **kw)
            got = buffers(prompts, texts, tok_ld=m + 8)
            ops.sample(raw, *got[:3], no_repeat_ngram=ngram, start=got[3], **kw)
            for x, y in zip(got[:3], want[:3]):
                assert torch.equal(x, y), f"ngram={ngram} top_k={top_k}"


def test_production_vocab_and_the_lds_row_limit():
    """Llama-3's 128 256 ids (4008 words of the 4096-word LDS row) through the 16-byte path; one id more than the row holds is refused"""
    V, n, ngram = 128256, 2, 2
    g = torch.Generator().manual_seed(4)
    raw_cpu = torch.randn(n, V, generator=g).to(BF)
    raw = raw_cpu.to(DEV)
    hots = [hot_ids(raw_cpu[u]) for u in range(n)]
    prompts, texts = R.histories(n, ngram, lambda u: hots[u], V, offset=2)          # several_followers, overlapping
    assert all(hots[u][0] in R.banned(texts[u], ngram) for u in range(n))
    base = np.zeros((n, V), dtype=bool)
    base[:, V - 40:] = True                                                          # the last two words
    base[np.arange(n), [h[0] for h in hots]] = True
    base[np.arange(n), [h[1] for h in hots]] = True
    for b in (None, base):
        rows = R.pick_rows(b, texts, ngram, V)
        sub = CR.substitute(raw, CR.pack_bits(rows).to(DEV))
        for top_k in (1, 5):
            kw = dict(temperature=0.7, top_k=top_k, seed=8, step=1)
            want = buffers(prompts, texts)
            ops.sample(sub, *want[:3], **kw)
            got = buffers(prompts, texts)
            ops.sample(raw, *got[:3], mask=None if b is None else CR.pack_bits(b).to(DEV), no_repeat_ngram=ngram, start=got[3], **kw)
            for x, y in zip(got[:3], want[:3]):
                assert torch.equal(x, y), f"mask={b is not None} top_k={top_k}"
    big = torch.zeros((1, 131073), dtype=BF, device=DEV)
    st = buffers([[1]], [[2, 2]])
    with pytest.raises(ValueError, match="131072"):
        ops.sample(big, *st[:3], top_k=1, no_repeat_ngram=1, start=st[3])
    assert torch.equal(st[0], buffers([[1]], [[2, 2]])[0])


def test_op_refusals_before_any_launch():
    raw = rows_for(320, 3).to(DEV)
    st = buffers([[1], [2], [3]], [[4, 4], [5], []])
    before = st[0].clone()
    with pytest.raises(ValueError, match="needs start"):
        ops.sample(raw, *st[:3], top_k=1, no_repeat_ngram=2)
    with pytest.raises(ValueError, match="0 .. 8"):
        ops.sample(raw, *st[:3], top_k=1, no_repeat_ngram=9, start=st[3])
    with pytest.raises(ValueError, match="goes with no_repeat_ngram"):
        ops.sample(raw, *st[:3], top_k=1, start=st[3])
    with pytest.raises(ValueError, match="int32"):
        ops.sample(raw, *st[:3], top_k=1, no_repeat_ngram=2, start=st[3].long())
    with pytest.raises(ValueError, match="int32"):
        ops.sample(raw, *st[:3], top_k=1, no_repeat_ngram=2, start=st[3][:2])
    with pytest.raises(_lib.DualHypHipError, match="GPU"):
        ops.sample(raw, *st[:3], top_k=1, no_repeat_ngram=2, start=st[3].cpu())
    assert torch.equal(st[0], before)
    # no_repeat_ngram = 0 is the call without the argument
    a, b = buffers([[1], [2], [3]], [[4, 4], [5], []]), buffers([[1], [2], [3]], [[4, 4], [5], []])
    ops.sample(raw, *a[:3], top_k=5, seed=3, step=1)
    ops.sample(raw, *b[:3], top_k=5, seed=3, step=1, no_repeat_ngram=0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
