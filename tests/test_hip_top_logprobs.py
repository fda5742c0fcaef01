"""Token alternatives on the GPU: ops.token_top_logprobs against the reference of tests/top_logprob_reference.py, the sampling
kernels' buffers, generate_batch / generate_stream(top_logprobs=K) under every decode schedule, the engine's graph keys and
score_batch.  Everything is exact (torch.equal): the ids are the reference's, a value is ops.token_logprobs' own bits for its id, the
flag changes no id and no log-probability, and what a call returns is the op's result on the logits row the token was picked from,
whatever schedule produced that row."""
import pytest
import torch

import top_logprob_reference as T
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, ops, quantize_model_fp8, score_batch
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NEW = 24
K = 5
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}
KW = dict(temperature=0.2, top_k=1)
NAN = float("nan")


def same_bits(a, b):
    """torch.equal, with NaN equal to NaN and -0 apart from +0"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_top(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and same_bits(x[1], y[1]) for x, y in zip(a, b))


def same_lists(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def clone_top(top):
    return [(i.clone(), v.clone()) for i, v in top]


def check_op(rows_cpu, k, what):
    """ids are the reference's; lp[:, j] is ops.token_logprobs(rows, ids[:, j]), bit for bit"""
    rows = rows_cpu.to(DEV)
    ids, lp = ops.token_top_logprobs(rows, k)
    n = rows.size(0)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32 and tuple(ids.shape) == tuple(lp.shape) == (n, k)
    want = T.top_ids(rows_cpu, k)
    bad = (ids.cpu() != want).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{what}: row {bad[0]}: got {ids[bad[0]].tolist()}, reference {want[bad[0]].tolist()}"
    for j in range(k):
        assert same_bits(lp[:, j], ops.token_logprobs(rows, ids[:, j].long())), f"{what}: rank {j}"
    return ids, lp


# ---- 1. the op against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", T.KS)
@pytest.mark.parametrize("V", T.VOCABS)
def test_op_against_the_reference(V, k):
    """1, 3 and 37 rows of every row kind; k = 8 at vocab 8 is k == vocab"""
    for n in T.ROW_COUNTS:
        rows, kinds = T.case(V, n, k)
        ids, lp = check_op(rows, k, f"V={V} k={k} rows={n}")
        for r, kind in enumerate(kinds):
            if kind in ("constant", "zeros_alternating_sign", "all_equal"):
                assert ids[r].tolist() == list(range(k)), kind
        # ranks are ordered: the values never rise along a row (-inf behind everything)
        assert bool((lp[:, 1:] <= lp[:, :-1]).all())


@pytest.mark.parametrize("k", (1, 8))
@pytest.mark.parametrize("V", (320, 1001, 128256))
def test_row_invariance_and_alignment(V, k):
    """A row alone, the same row at index 36 of 37, and the same row one bf16 into an allocation (the scalar loop: the 16-byte loads
    need an aligned row; V = 1001 takes it everywhere) give the same ids and bits."""
    rows, kinds = T.case(V, 37, k)
    rows = rows.to(DEV)
    ids, lp = ops.token_top_logprobs(rows, k)
    for r in (36, 13, 12):                      # 13: equal_maxima, 12: zeros of both signs
        a_ids, a_lp = ops.token_top_logprobs(rows[r:r + 1].contiguous(), k)
        assert torch.equal(a_ids, ids[r:r + 1]) and same_bits(a_lp, lp[r:r + 1]), (r, kinds[r])
        moved = torch.cat([rows[:36 - r], rows[r:r + 1].expand(r + 1, V)]).contiguous()     # the row again, now at index 36
        m_ids, m_lp = ops.token_top_logprobs(moved, k)
        assert torch.equal(m_ids[36], ids[r]) and same_bits(m_lp[36], lp[r]), (r, kinds[r])
    buf = torch.zeros(37 * V + 8, dtype=BF, device=DEV)
    off = buf[1:1 + 37 * V].view(37, V)
    off.copy_(rows)
    assert off.data_ptr() % 16 == 2 and off.is_contiguous()
    o_ids, o_lp = ops.token_top_logprobs(off, k)
    assert torch.equal(o_ids, ids) and same_bits(o_lp, lp)


def test_nan_rows_stay_in_bounds():
    """outside the definition, but the ids are inside [0, vocab) and nothing else is touched"""
    V = 1000
    rows = T.case(V, 3, 8)[0].to(DEV)
    rows[0, 5] = NAN
    rows[1, :] = NAN
    rows[2, ::2] = -NAN
    ids, lp = ops.token_top_logprobs(rows, 8)
    assert bool(((ids >= 0) & (ids < V)).all())
    for r in range(3):
        assert len(set(ids[r].tolist())) == 8


# ---- 2. the sampling kernels' buffers -------------------------------------------------------------------------------------------------
def _logits(V, n):
    g = torch.Generator().manual_seed(V + n)
    lg = (torch.randn((n, V), generator=g, dtype=torch.float64) * 3).to(BF)
    lg[0] = (lg[0].double() * 2).round() / 2        # a row of ties
    return lg.to(DEV)


def _top_bufs(shape, k):
    return (torch.full(shape + (k,), -1, dtype=torch.int32, device=DEV), torch.full(shape + (k,), NAN, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", (320, 32000))
def test_sample_writes_the_rows_alternatives(V, top_k):
    n_seq, tok_ld, k = 6, 5, 3
    logits = _logits(V, n_seq)
    tokens0 = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
    length0 = torch.tensor([0, 3, 4, 5, 2, 1], dtype=torch.int32, device=DEV)      # sequence 3: the buffer is full
    done0 = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.int32, device=DEV)        # sequence 4: finished
    kw = dict(temperature=0.7, top_k=top_k, seed=11, step=3)
    a = [t.clone() for t in (tokens0, length0, done0)]
    lp_a = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    ops.sample(logits, *a, logprobs=lp_a, **kw)
    b = [t.clone() for t in (tokens0, length0, done0)]
    lp_b = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    t_ids, t_lp = _top_bufs((n_seq, tok_ld), k)
    ops.sample(logits, *b, logprobs=lp_b, top_logprobs=(t_ids, t_lp), **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert same_bits(lp_a, lp_b)
    want_ids, want_lp = ops.token_top_logprobs(logits, k)
    written = torch.zeros((n_seq, tok_ld), dtype=torch.bool, device=DEV)
    for u in (0, 1, 2, 5):
        n = int(length0[u])
        written[u, n] = True
        assert torch.equal(t_ids[u, n], want_ids[u]) and same_bits(t_lp[u, n], want_lp[u]), u
    assert bool((t_ids[~written] == -1).all()) and bool(torch.isnan(t_lp[~written]).all())
    assert not bool(torch.isnan(t_lp[written]).any())


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", (320, 32000))
def test_sample_rows_writes_the_rows_alternatives(V, top_k):
    n_seq, tok_ld, max_new, k = 7, 9, 4, 8
    row_seq = torch.tensor([5, 2, 6, 0, 6, 3], dtype=torch.int32, device=DEV)      # sequence 6: finished, named by two padding rows
    logits = _logits(V, row_seq.numel())
    tokens0 = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
    plen = [3, 2, 5, 4, 1, 2, 1]
    length0 = torch.tensor([4, 2, 6, 8, 1, 3, 2], dtype=torch.int32, device=DEV)   # sequence 3: its budget 4 + 4 is spent
    limit = torch.tensor([p + max_new for p in plen], dtype=torch.int32, device=DEV)
    done0 = torch.tensor([0, 0, 0, 2, 0, 0, 1], dtype=torch.int32, device=DEV)
    kw = dict(temperature=0.7, top_k=top_k, seed=11)
    a = [t.clone() for t in (tokens0, length0, done0)]
    lp_a = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    ops.sample_rows(logits, *a, limit, row_seq, max_new, logprobs=lp_a, **kw)
    b = [t.clone() for t in (tokens0, length0, done0)]
    lp_b = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    t_ids, t_lp = _top_bufs((n_seq, tok_ld), k)
    ops.sample_rows(logits, *b, limit, row_seq, max_new, logprobs=lp_b, top_logprobs=(t_ids, t_lp), **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert same_bits(lp_a, lp_b)
    want_ids, want_lp = ops.token_top_logprobs(logits, k)
    written = torch.zeros((n_seq, tok_ld), dtype=torch.bool, device=DEV)
    for r, u in enumerate(row_seq.tolist()):
        if u in (6, 3):
            continue
        n = int(length0[u])
        written[u, n] = True
        assert torch.equal(t_ids[u, n], want_ids[r]) and same_bits(t_lp[u, n], want_lp[r]), (r, u)
    assert int(written.sum()) == 3
    assert bool((t_ids[~written] == -1).all()) and bool(torch.isnan(t_lp[~written]).all())


def test_buffer_errors_before_any_launch():
    lg = torch.zeros((2, 64), dtype=BF, device=DEV)
    tokens = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    length = torch.zeros(2, dtype=torch.int32, device=DEV)
    done = torch.zeros(2, dtype=torch.int32, device=DEV)
    lp = torch.zeros((2, 4), dtype=torch.float32, device=DEV)
    i3, f3 = _top_bufs((2, 4), 3)
    for top, lpb, exc in (((i3, f3), None, ValueError),                          # no logprobs buffer
                          ((i3.long(), f3), lp, TypeError), ((i3, f3.double()), lp, TypeError),
                          (_top_bufs((2, 5), 3), lp, ValueError), (_top_bufs((2, 4), 9), lp, ValueError),
                          ((i3, _top_bufs((2, 4), 2)[1]), lp, ValueError)):
        with pytest.raises(exc):
            ops.sample(lg, tokens, length, done, top_k=1, logprobs=lpb, top_logprobs=top)
        with pytest.raises(exc):
            ops.sample_rows(lg, tokens, length, done, torch.full((2,), 4, dtype=torch.int32, device=DEV),
                            torch.tensor([0, 1], dtype=torch.int32, device=DEV), 4, top_k=1, logprobs=lpb, top_logprobs=top)
    assert length.tolist() == [0, 0] and not bool(tokens.any())
    for bad, exc in ((0, ValueError), (9, ValueError), (True, TypeError), (2.0, TypeError)):
        with pytest.raises(exc):
            ops.token_top_logprobs(lg, bad)
    with pytest.raises(ValueError):
        ops.token_top_logprobs(lg[:, :4].contiguous(), 5)                        # k > vocab
    with pytest.raises(TypeError):
        ops.token_top_logprobs(lg.float(), 2)


# ---- 3. generation --------------------------------------------------------------------------------------------------------------------
def build(name, seed=11, **over):
    cfg = Config.from_name(name, **LORA, **over)
    assert cfg.head_size == HEAD_SIZES[name]
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=BF)
    m.load_state_dict(sd)
    m.eval()
    return cfg, m


def ragged_prompts(cfg, new=NEW, seed=70):
    """a one-token prompt; 30 .. 33 tokens around the first cache tile's end; and a prompt whose last generated token sits at the
    model's last position"""
    V = cfg.padded_vocab_size
    lens = [1, 30, 31, 32, 33, 47, 64, cfg.block_size - new + 1]
    return [synth_prompts(1, n, V, seed=seed + i)[0].to(DEV) for i, n in enumerate(lens)]


def replay_rows(m, prompt, ids):
    """the logits rows `ids` were picked from, by the model's own cached forwards, one sequence alone: the prompt's prefill (its last
    row), then one single-token forward per generated id — decode steps"""
    T_ = prompt.numel()
    m.reset_cache()
    rows = [m(prompt.view(1, -1), torch.arange(T_, device=DEV))[0, -1]]
    for s, tok in enumerate(ids[:-1].tolist()):
        rows.append(m(torch.tensor([[tok]], device=DEV), torch.tensor([T_ + s], device=DEV))[0, 0])
    m.reset_cache()
    return torch.stack(rows)


class Runs:
    """One model and, computed once and never changed: its run with return_logprobs alone, its run with top_logprobs=K, and an EOS
    taken from the run's own output."""

    def __init__(self, name):
        self.cfg, self.m = build(name)
        self.ps = ragged_prompts(self.cfg)
        out, lp, st = generate_batch(self.m, self.ps, NEW, return_state=True, return_logprobs=True, **KW)
        self.base_out, self.base_lp = [o.clone() for o in out], [v.clone() for v in lp]
        self.base_st = {k: v.clone() for k, v in st.items()}
        out, lp, top, st = generate_batch(self.m, self.ps, NEW, return_state=True, return_logprobs=True, top_logprobs=K, **KW)
        self.out, self.lp, self.top = [o.clone() for o in out], [v.clone() for v in lp], clone_top(top)
        self.st = {k: v.clone() for k, v in st.items()}
        self.eos = int(self.out[2][self.ps[2].numel() + 2])       # sequence 2's third generated token

    def with_eos(self, **kw):
        out, lp, top, st = generate_batch(self.m, self.ps, NEW, eos_id=self.eos, return_state=True, return_logprobs=True,
                                          top_logprobs=K, **KW, **kw)
        return [o.clone() for o in out], [v.clone() for v in lp], clone_top(top), {k: v.clone() for k, v in st.items()}


@pytest.fixture(scope="module", params=list(HEAD_SIZES))
def runs(request):
    return Runs(request.param)


def test_flag_changes_no_id_and_no_logprob(runs):
    r = runs
    assert same_lists(r.base_out, r.out) and same_lists(r.base_lp, r.lp)
    for k in ("tokens", "length", "done"):
        assert torch.equal(r.base_st[k], r.st[k]), k
    assert same_bits(r.base_st["logprobs"], r.st["logprobs"])
    ids, lp = r.st["top_ids"], r.st["top_logprobs"]
    shape = tuple(r.st["tokens"].shape) + (K,)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32 and tuple(ids.shape) == tuple(lp.shape) == shape
    produced = torch.zeros(shape[:2], dtype=torch.bool, device=DEV)
    for i, p in enumerate(r.ps):
        a, b = r.top[i]
        assert tuple(a.shape) == tuple(b.shape) == (NEW, K) == (r.lp[i].numel(), K)
        assert torch.equal(a, ids[i, p.numel():p.numel() + NEW]) and same_bits(b, lp[i, p.numel():p.numel() + NEW])
        produced[i, p.numel():p.numel() + NEW] = True
    assert bool((ids[~produced] == -1).all()) and bool(torch.isnan(lp[~produced]).all())
    V = r.cfg.padded_vocab_size
    assert bool(((ids[produced] >= 0) & (ids[produced] < V)).all()) and bool(torch.isfinite(lp[produced]).all())
    # generate() forwards the flag
    one = generate(r.m, r.ps[3], r.ps[3].numel() + NEW, return_logprobs=True, top_logprobs=K, **KW)
    assert torch.equal(one[0], r.out[3]) and torch.equal(one[1], r.lp[3]) and same_top([one[2]], [r.top[3]])


def test_values_are_the_ops_on_the_models_own_logits(runs):
    r = runs
    with torch.no_grad():
        for i in (3, 7):
            T_ = r.ps[i].numel()
            want = ops.token_top_logprobs(replay_rows(r.m, r.ps[i], r.out[i][T_:]), K)
            assert torch.equal(r.top[i][0], want[0]) and same_bits(r.top[i][1], want[1]), f"sequence {i}"


def test_rank_0_and_the_chosen_token(runs):
    r = runs
    # temperature 1, top_k 1: the sampler's arg-max is over the raw row, so rank 0 IS the chosen token, and its value the logprob
    out, lp, top = generate_batch(r.m, r.ps, NEW, temperature=1.0, top_k=1, return_logprobs=True, top_logprobs=2)
    for i, p in enumerate(r.ps):
        assert torch.equal(top[i][0][:, 0].long(), out[i][p.numel():]), i
        assert same_bits(top[i][1][:, 0], lp[i]), i
    # temperature 0.2: the sampler picks among bf16(l / 0.2), which can merge raw values: rank 0 is never below the chosen token,
    # and where the chosen token is among the alternatives its value is the logprob, bit for bit
    hits = 0
    for i, p in enumerate(r.ps):
        ids, val = r.top[i]
        assert bool((val[:, 0] >= r.lp[i]).all()), i
        assert bool((val[:, 1:] <= val[:, :-1]).all()), i
        at = ids.long() == r.out[i][p.numel():, None]
        assert bool((at.sum(dim=1) <= 1).all())
        hits += int(at.sum())
        assert same_bits(val[at], r.lp[i][:, None].expand(-1, K)[at]), i
    assert hits > 0                                   # the case above was met at all


def test_eos_and_lengths(runs):
    r = runs
    want = [o.clone() for o in generate_batch(r.m, r.ps, NEW, eos_id=r.eos, **KW)]
    out, lp, top, st = r.with_eos()
    assert same_lists(want, out)
    done = st["done"].tolist()
    assert done[2] == 1 and any(d != 1 for d in done)
    produced = torch.zeros(tuple(st["tokens"].shape), dtype=torch.bool, device=DEV)
    for i, p in enumerate(r.ps):
        n = out[i].numel() - p.numel() + (1 if done[i] == 1 else 0)           # the EOS token's alternatives are the last entry
        assert tuple(top[i][0].shape) == tuple(top[i][1].shape) == (n, K) and lp[i].numel() == n
        assert torch.equal(top[i][0], r.top[i][0][:n]) and same_bits(top[i][1], r.top[i][1][:n])
        produced[i, p.numel():p.numel() + n] = True
    assert bool((st["top_ids"][~produced] == -1).all()) and bool(torch.isnan(st["top_logprobs"][~produced]).all())
    assert not bool(torch.isnan(st["top_logprobs"][produced]).any())


def test_generate_stream_gives_the_same_alternatives(runs):
    r = runs
    V = r.cfg.padded_vocab_size
    ps = r.ps + [synth_prompts(1, n, V, seed=90 + n)[0].to(DEV) for n in (5, 40, 17)]
    for eos in (None, r.eos):
        want = generate_batch(r.m, ps, NEW, eos_id=eos, return_logprobs=True, top_logprobs=K, **KW)
        want = ([o.clone() for o in want[0]], [v.clone() for v in want[1]], clone_top(want[2]))
        got = generate_stream(r.m, ps, NEW, eos_id=eos, max_rows=4, check_every=3, return_logprobs=True, top_logprobs=K, **KW)
        assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])
    assert same_top(want[2][:8], r.with_eos()[2])


@pytest.mark.parametrize("D", (1, 3, 7))
def test_speculate_gives_the_same_alternatives(runs, D):
    """prompt lookup, and scripted drafts: all right, all wrong, every third wrong; then an EOS inside an accepted run"""
    r = runs
    V = r.cfg.padded_vocab_size
    right = torch.stack([r.st["tokens"][u, p.numel():p.numel() + NEW] for u, p in enumerate(r.ps)]).contiguous()
    wrong = ((right + 1) % V).contiguous()
    mixed = right.clone()
    mixed[:, 2::3] = wrong[:, 2::3]
    for kw in (dict(), dict(drafts=right), dict(drafts=wrong), dict(drafts=mixed)):
        tm = {}
        out, lp, top, st = generate_batch(r.m, r.ps, NEW, speculate=D, return_state=True, return_logprobs=True, top_logprobs=K,
                                          timing=tm, **KW, **kw)
        assert same_lists(r.out, out) and same_lists(r.lp, lp) and same_top(r.top, top)
        assert torch.equal(st["top_ids"], r.st["top_ids"]) and same_bits(st["top_logprobs"], r.st["top_logprobs"])
        if kw.get("drafts") is right:
            assert tm["spec_accepted"] > 0
        if kw.get("drafts") is wrong:
            assert tm["spec_accepted"] == 0
    want = r.with_eos()
    tm = {}
    got = r.with_eos(speculate=D, drafts=right, timing=tm)
    assert tm["spec_accepted"] > 0                     # sequence 2's EOS is its third token: inside the first accepted run for D >= 2
    assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])
    assert torch.equal(got[3]["top_ids"], want[3]["top_ids"]) and same_bits(got[3]["top_logprobs"], want[3]["top_logprobs"])


def test_share_prefix_gives_the_same_alternatives(runs):
    r = runs
    V = r.cfg.padded_vocab_size
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps = [torch.cat([head, synth_prompts(1, n, V, seed=40 + n)[0].to(DEV)]) for n in (1, 2, 31, 32, 33, 50)]
    want = generate_batch(r.m, ps, NEW, return_logprobs=True, top_logprobs=K, **KW)
    want = ([o.clone() for o in want[0]], [v.clone() for v in want[1]], clone_top(want[2]))
    tm = {}
    got = generate_batch(r.m, ps, NEW, share_prefix=True, return_logprobs=True, top_logprobs=K, timing=tm, **KW)
    assert tm["shared_prefix"] == 32
    assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])
    got = generate_stream(r.m, ps, NEW, share_prefix=True, max_rows=4, check_every=3, return_logprobs=True, top_logprobs=K, **KW)
    assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])


def test_graph_keys(runs):
    """K and the two buffers are part of the captured step's key, as the logprobs buffer is.  One engine, buffers that keep their
    addresses across calls: plain, logprobs, K = 3, K = 5 each capture one step; the K = 3 and K = 5 buffers are views of ONE
    allocation, so only K tells their keys apart; plain and K = 3 again capture nothing and give what they gave."""
    r = runs
    m, ps = r.m, r.ps[:6]
    B, lens, steps = len(ps), [int(p.numel()) for p in ps], 8
    tok_ld = max(lens) + steps + 1
    m.refresh_engine()
    eng = m.engine(B, max(lens) + steps, sum(lens), exact=True)
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    tokens0 = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(ps, batch_first=True), (0, tok_ld - max(lens))).contiguous()
    tokens, length, done = tokens0.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    lp = torch.empty((B, tok_ld), dtype=torch.float32, device=DEV)
    store_i = torch.empty(B * tok_ld * 8, dtype=torch.int32, device=DEV)
    store_f = torch.empty(B * tok_ld * 8, dtype=torch.float32, device=DEV)
    packed = torch.cat(ps)

    def run(want_lp, k):
        tokens.copy_(tokens0)
        length.copy_(torch.tensor(lens, dtype=torch.int32))
        done.zero_()
        lp.fill_(NAN)
        store_i.fill_(-1)
        store_f.fill_(NAN)
        top = (store_i[:B * tok_ld * k].view(B, tok_ld, k), store_f[:B * tok_ld * k].view(B, tok_ld, k)) if k else None
        assert top is None or (top[0].data_ptr() == store_i.data_ptr() and top[1].data_ptr() == store_f.data_ptr())
        _, last = eng.forward(packed, lens, [0] * B, want_all=False, want_last=True, slot_base=0)
        ops.sample(last, tokens, length, done, seed=3, step=0, logprobs=lp if want_lp else None, top_logprobs=top, **KW)
        eng.set_logprobs(lp if want_lp else None)
        eng.set_top_logprobs(*top) if k else eng.set_top_logprobs(None)
        try:
            eng.decode(tokens, length, done, steps, KW["temperature"], KW["top_k"], None, 3, first_step=0)
        finally:
            eng.set_logprobs(None)
            eng.set_top_logprobs(None)
        torch.cuda.synchronize()
        res = dict(tokens=tokens.clone(), lp=lp.clone(), count=eng.graph_count(0))
        if k:
            res["top"] = (top[0].clone(), top[1].clone())
        return res

    c0 = eng.graph_count(0)
    plain = run(False, 0)
    with_lp = run(True, 0)
    k3 = run(True, 3)
    k5 = run(True, 5)
    assert [x["count"] - c0 for x in (plain, with_lp, k3, k5)] == [1, 2, 3, 4]
    plain2 = run(False, 0)
    k3b = run(True, 3)
    lp2 = run(True, 0)
    assert plain2["count"] == k3b["count"] == lp2["count"] == k5["count"]      # nothing new was captured: every step was found again
    for x in (with_lp, k3, k5, plain2, k3b, lp2):
        assert torch.equal(x["tokens"], plain["tokens"])
    assert bool(torch.isnan(plain["lp"]).all()) and bool(torch.isnan(plain2["lp"]).all())
    for x in (k3, k5, k3b, lp2):
        assert same_bits(x["lp"], with_lp["lp"])
    assert torch.equal(k3["top"][0], k3b["top"][0]) and same_bits(k3["top"][1], k3b["top"][1])
    assert torch.equal(k3["top"][0], k5["top"][0][:, :, :3]) and same_bits(k3["top"][1], k5["top"][1][:, :, :3])
    n_written = int((k5["top"][0][:, :, 0] >= 0).sum())
    assert n_written == B * (steps + 1)
    m.refresh_engine()


@pytest.mark.parametrize("kv_cache", ("bf16", "fp8"))
def test_fp8_model(kv_cache):
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache=kv_cache)
    assert m.fp8 and m.kv_cache_dtype == kv_cache
    ps = ragged_prompts(cfg)
    base = generate_batch(m, ps, NEW, return_logprobs=True, **KW)
    base = ([o.clone() for o in base[0]], [v.clone() for v in base[1]])
    out, lp, top = generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=K, **KW)
    out, lp, top = [o.clone() for o in out], [v.clone() for v in lp], clone_top(top)
    assert same_lists(base[0], out) and same_lists(base[1], lp)
    with torch.no_grad():
        for i in (3, 7):
            T_ = ps[i].numel()
            want = ops.token_top_logprobs(replay_rows(m, ps[i], out[i][T_:]), K)
            assert torch.equal(top[i][0], want[0]) and same_bits(top[i][1], want[1]), f"kv_cache={kv_cache} sequence {i}"
    got = generate_stream(m, ps, NEW, max_rows=4, check_every=3, return_logprobs=True, top_logprobs=K, **KW)
    assert same_lists(out, got[0]) and same_lists(lp, got[1]) and same_top(top, got[2])


# ---- 4. score_batch -------------------------------------------------------------------------------------------------------------------
def test_score_batch(runs):
    r = runs
    cfg, m = r.cfg, r.m
    V = cfg.padded_vocab_size
    plens = [1, 30, 33, 64, 5, 47, 20, 9]
    clens = [1, 12, 1, cfg.block_size - 64 + 1, 24, 7, 3, 40]       # length 1; sequence 3 ends at the model's last position
    ps = [synth_prompts(1, n, V, seed=120 + i)[0].to(DEV) for i, n in enumerate(plens)]
    cs = [synth_prompts(1, n, V, seed=140 + i)[0].to(DEV) for i, n in enumerate(clens)]
    plain = [v.clone() for v in score_batch(m, ps, cs)]
    scores, top = score_batch(m, ps, cs, top_logprobs=K)
    assert same_lists(plain, scores)
    assert [tuple(a.shape) for a, _ in top] == [(n, K) for n in clens] and all(a.dtype == torch.int32 and b.dtype == torch.float32 for a, b in top)
    with torch.no_grad():
        for i in range(1, len(ps)):         # sequence 0 is a single row: model(idx) takes it for a decode step
            seq = torch.cat([ps[i], cs[i][:-1]])
            lg = m(seq.view(1, -1))[0]
            want = ops.token_top_logprobs(lg[plens[i] - 1:].contiguous(), K)
            assert torch.equal(top[i][0], want[0]) and same_bits(top[i][1], want[1]), i
    # a sequence's alternatives do not depend on the grouping
    s2, t2 = score_batch(m, ps, cs, top_logprobs=K, max_tokens=1)
    assert same_lists(plain, s2) and same_top(top, t2)
    assert m._cache_len == []
