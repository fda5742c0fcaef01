"""Token log-probabilities on the GPU: ops.token_logprobs against the fp64 reference of tests/logprob_reference.py, the sampling
kernels' logprobs buffer, generate_batch / generate_stream(return_logprobs=True) under every decode schedule, and score_batch.
The op is gated against fp64; everything above it is exact (torch.equal): the flag changes no id, and a returned value is the op's
own on the logits row the token was picked from, whatever schedule produced that row."""
import numpy as np
import pytest
import torch

import logprob_reference as R
from conftest import record_parity
from dualhyp_amd import GPT, Config, generate, generate_batch, generate_stream, ops, quantize_model_fp8, score_batch
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NEW = 24
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}
KW = dict(temperature=0.2, top_k=1)
NAN = float("nan")


# ---- 1. the op against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", R.VOCABS)
def test_token_logprobs_vs_fp64(V):
    """|got - ref64| <= 2e-5 + 2.4e-7 |ref64| on every row kind, for 1, 3 and 37 rows.  The measured worst cases per vocabulary size
    are in MEASUREMENTS.md ("Token log-probabilities") and go to the parity record as logprobs.op.V<vocab>."""
    worst, worst_small = 0.0, 0.0
    for n in R.ROW_COUNTS:
        rows, ids, kinds = R.case(V, n)
        ref = R.logprobs64(rows, ids)
        got = ops.token_logprobs(rows.to(DEV), ids.to(DEV))
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        got = got.cpu().numpy().astype(np.float64)
        ok = R.within_gate(got, ref)
        fin = np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin])
        worst = max(worst, float((err / R.gate(ref[fin])).max()))
        small = ref[fin] > -100.0
        if small.any():
            worst_small = max(worst_small, float(err[small].max()))
        bad = np.nonzero(~ok)[0]
        assert bad.size == 0, f"V={V} rows={n}: " + "; ".join(f"row {i} ({kinds[i]}): got {got[i]!r}, fp64 {ref[i]!r}" for i in bad[:4])
    record_parity(f"logprobs.op.V{V}", worst_abs_err_ref_above_minus_100=worst_small, worst_err_over_gate=worst)
    print(f"V={V}: worst |got - ref64| where ref > -100: {worst_small:.3g}; worst error / gate: {worst:.3g}")


@pytest.mark.parametrize("V", R.VOCABS + (1001,))
def test_row_invariance_and_alignment(V):
    """A row's bits do not depend on the row index, the row count or the row's address: alone, as row 36 of 37, and 8 bytes into an
    allocation (the scalar loop: the 16-byte loads need an aligned row; V = 1001 takes it everywhere)."""
    rows, ids, _ = R.case(V, 37)
    rows, ids = rows.to(DEV), ids.to(DEV)
    joint = ops.token_logprobs(rows, ids)
    for r in (36, 7):
        alone = ops.token_logprobs(rows[r:r + 1].contiguous(), ids[r:r + 1])
        assert torch.equal(alone, joint[r:r + 1])
    buf = torch.zeros(3 * V + 4, dtype=BF, device=DEV)
    off = buf[4:].view(3, V)
    off.copy_(rows[:3])
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    assert torch.equal(ops.token_logprobs(off, ids[:3]), joint[:3])
    ref = R.logprobs64(rows[:3], ids[:3].tolist())
    assert R.within_gate(joint[:3].cpu().numpy(), ref).all()


# ---- 2. the sampling kernels' buffer --------------------------------------------------------------------------------------------------
def _sample_inputs(V, n_seq, tok_ld):
    g = torch.Generator().manual_seed(V + n_seq)
    logits = (torch.randn((n_seq, V), generator=g, dtype=torch.float64) * 3).to(BF).to(DEV)
    tokens = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
    return logits, tokens


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", (320, 32000))
def test_sample_writes_the_picks_logprob(V, top_k):
    n_seq, tok_ld = 6, 5
    logits, tokens0 = _sample_inputs(V, n_seq, tok_ld)
    length0 = torch.tensor([0, 3, 4, 5, 2, 1], dtype=torch.int32, device=DEV)      # sequence 3: the buffer is full
    done0 = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.int32, device=DEV)        # sequence 4: finished
    kw = dict(temperature=0.7, top_k=top_k, seed=11, step=3)
    a = [t.clone() for t in (tokens0, length0, done0)]
    ops.sample(logits, *a, **kw)
    b = [t.clone() for t in (tokens0, length0, done0)]
    lp = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    ops.sample(logits, *b, logprobs=lp, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    written = torch.zeros((n_seq, tok_ld), dtype=torch.bool, device=DEV)
    for u in (0, 1, 2, 5):
        n = int(length0[u])
        written[u, n] = True
        want = ops.token_logprobs(logits[u:u + 1], b[0][u, n:n + 1])
        assert torch.equal(lp[u, n:n + 1], want), (u, lp[u, n].item(), want.item())
    assert bool(torch.isnan(lp[~written]).all()) and not bool(torch.isnan(lp[written]).any())


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", (320, 32000))
def test_sample_rows_writes_the_picks_logprob(V, top_k):
    n_seq, tok_ld, max_new = 7, 9, 4
    row_seq = torch.tensor([5, 2, 6, 0, 6, 3], dtype=torch.int32, device=DEV)      # sequence 6: finished, named by two padding rows
    logits, tokens0 = _sample_inputs(V, row_seq.numel(), tok_ld)
    tokens0 = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
    plen = [3, 2, 5, 4, 1, 2, 1]
    length0 = torch.tensor([4, 2, 6, 8, 1, 3, 2], dtype=torch.int32, device=DEV)   # sequence 3: its budget 4 + 4 is spent
    limit = torch.tensor([p + max_new for p in plen], dtype=torch.int32, device=DEV)
    done0 = torch.tensor([0, 0, 0, 2, 0, 0, 1], dtype=torch.int32, device=DEV)
    kw = dict(temperature=0.7, top_k=top_k, seed=11)
    a = [t.clone() for t in (tokens0, length0, done0)]
    ops.sample_rows(logits, *a, limit, row_seq, max_new, **kw)
    b = [t.clone() for t in (tokens0, length0, done0)]
    lp = torch.full((n_seq, tok_ld), NAN, dtype=torch.float32, device=DEV)
    ops.sample_rows(logits, *b, limit, row_seq, max_new, logprobs=lp, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    written = torch.zeros((n_seq, tok_ld), dtype=torch.bool, device=DEV)
    for r, u in enumerate(row_seq.tolist()):
        if u in (6, 3):
            continue
        n = int(length0[u])
        written[u, n] = True
        assert torch.equal(lp[u, n:n + 1], ops.token_logprobs(logits[r:r + 1], b[0][u, n:n + 1])), (r, u)
    assert int(written.sum()) == 3
    assert bool(torch.isnan(lp[~written]).all()) and not bool(torch.isnan(lp[written]).any())


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


class Runs:
    """One model and, computed once and never changed, its plain run (no flag), its flagged run and an EOS taken from the plain
    run's own output."""

    def __init__(self, name):
        self.cfg, self.m = build(name)
        self.ps = ragged_prompts(self.cfg)
        out, st = generate_batch(self.m, self.ps, NEW, return_state=True, **KW)
        self.plain = [o.clone() for o in out]
        self.plain_st = {k: v.clone() for k, v in st.items()}
        out, lp, st = generate_batch(self.m, self.ps, NEW, return_state=True, return_logprobs=True, **KW)
        self.out, self.lp = [o.clone() for o in out], [v.clone() for v in lp]
        self.st = {k: v.clone() for k, v in st.items()}
        self.eos = int(self.plain[2][self.ps[2].numel() + 2])       # sequence 2's third generated token

    def with_eos(self, **kw):
        out, lp, st = generate_batch(self.m, self.ps, NEW, eos_id=self.eos, return_state=True, return_logprobs=True, **KW, **kw)
        return [o.clone() for o in out], [v.clone() for v in lp], {k: v.clone() for k, v in st.items()}


@pytest.fixture(scope="module", params=list(HEAD_SIZES))
def runs(request):
    return Runs(request.param)


def same_lists(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_flag_changes_no_id_and_lengths_are_as_defined(runs):
    r = runs
    assert same_lists(r.plain, r.out)
    for k in ("tokens", "length", "done"):
        assert torch.equal(r.plain_st[k], r.st[k]), k
    buf = r.st["logprobs"]
    assert buf.dtype == torch.float32 and tuple(buf.shape) == tuple(r.st["tokens"].shape)
    produced = torch.zeros_like(buf, dtype=torch.bool)
    for i, p in enumerate(r.ps):
        assert r.lp[i].dtype == torch.float32 and r.lp[i].numel() == r.out[i].numel() - p.numel() == NEW
        assert torch.equal(r.lp[i], buf[i, p.numel():p.numel() + NEW])
        produced[i, p.numel():p.numel() + NEW] = True
    assert bool(torch.isnan(buf[~produced]).all()) and bool(torch.isfinite(buf[produced]).all()) and bool((buf[produced] <= 0).all())
    # with an EOS: the EOS token's entry is the last one, one more than the ids returned
    want = [o.clone() for o in generate_batch(r.m, r.ps, NEW, eos_id=r.eos, **KW)]
    out, lp, st = r.with_eos()
    assert same_lists(want, out)
    done = st["done"].tolist()
    assert done[2] == 1 and 1 in done and any(d != 1 for d in done)
    produced = torch.zeros_like(buf, dtype=torch.bool)
    for i, p in enumerate(r.ps):
        n = out[i].numel() - p.numel() + (1 if done[i] == 1 else 0)
        assert lp[i].numel() == n and n == int(st["length"][i]) - p.numel()
        if done[i] == 1:
            assert int(st["tokens"][i, p.numel() + n - 1]) == r.eos
        # the values up to the EOS are those of the EOS-free run
        assert torch.equal(lp[i], r.lp[i][:n])
        produced[i, p.numel():p.numel() + n] = True
    assert bool(torch.isnan(st["logprobs"][~produced]).all()) and not bool(torch.isnan(st["logprobs"][produced]).any())
    # generate() forwards the flag
    ids, one = generate(r.m, r.ps[3], r.ps[3].numel() + NEW, return_logprobs=True, **KW)
    assert torch.equal(ids, r.out[3]) and torch.equal(one, r.lp[3])


def replay(m, prompt, ids):
    """log-probabilities of `ids` behind `prompt` by the model's own cached forwards, one sequence alone: the prompt's prefill (its
    last row), then one single-token forward per generated id — decode steps"""
    T = prompt.numel()
    m.reset_cache()
    rows = [m(prompt.view(1, -1), torch.arange(T, device=DEV))[0, -1]]
    for s, tok in enumerate(ids[:-1].tolist()):
        rows.append(m(torch.tensor([[tok]], device=DEV), torch.tensor([T + s], device=DEV))[0, 0])
    m.reset_cache()
    return ops.token_logprobs(torch.stack(rows), ids)


def test_values_are_the_ops_on_the_models_own_logits(runs):
    r = runs
    with torch.no_grad():
        for i in (3, 7):
            T = r.ps[i].numel()
            want = replay(r.m, r.ps[i], r.out[i][T:])
            assert torch.equal(r.lp[i], want), f"sequence {i}: first difference at {int((r.lp[i] != want).nonzero()[0])}"


def test_generate_stream_gives_the_same_values(runs):
    r = runs
    V = r.cfg.padded_vocab_size
    ps = r.ps + [synth_prompts(1, n, V, seed=90 + n)[0].to(DEV) for n in (5, 40, 17)]
    for eos in (None, r.eos):
        want, want_lp = generate_batch(r.m, ps, NEW, eos_id=eos, return_logprobs=True, **KW)
        want, want_lp = [o.clone() for o in want], [v.clone() for v in want_lp]
        got, got_lp = generate_stream(r.m, ps, NEW, eos_id=eos, max_rows=4, check_every=3, return_logprobs=True, **KW)
        assert same_lists(want, got) and same_lists(want_lp, got_lp)
        assert same_lists(want, generate_stream(r.m, ps, NEW, eos_id=eos, max_rows=4, check_every=3, **KW))
    assert same_lists(want_lp[:8], r.with_eos()[1])


@pytest.mark.parametrize("D", (1, 3, 7))
def test_speculate_gives_the_same_values(runs, D):
    r = runs
    V = r.cfg.padded_vocab_size
    drafts = torch.stack([r.plain_st["tokens"][u, p.numel():p.numel() + NEW] for u, p in enumerate(r.ps)])
    drafts[:, 2::3] = (drafts[:, 2::3] + 1) % V                     # "corrupt": every third draft is wrong
    for kw in (dict(), dict(drafts=drafts.contiguous())):
        out, lp, st = generate_batch(r.m, r.ps, NEW, speculate=D, return_state=True, return_logprobs=True, **KW, **kw)
        assert same_lists(r.out, out) and same_lists(r.lp, lp)
        assert torch.equal(st["logprobs"].isnan(), r.st["logprobs"].isnan())
        assert same_lists(r.out, generate_batch(r.m, r.ps, NEW, speculate=D, **KW, **kw))
    want_out, want_lp, want_st = r.with_eos()
    out, lp, st = r.with_eos(speculate=D, drafts=drafts.contiguous())
    assert same_lists(want_out, out) and same_lists(want_lp, lp) and torch.equal(st["logprobs"].isnan(), want_st["logprobs"].isnan())


def test_share_prefix_gives_the_same_values(runs):
    r = runs
    V = r.cfg.padded_vocab_size
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps = [torch.cat([head, synth_prompts(1, n, V, seed=40 + n)[0].to(DEV)]) for n in (1, 2, 31, 32, 33, 50)]
    want, want_lp = generate_batch(r.m, ps, NEW, return_logprobs=True, **KW)
    want, want_lp = [o.clone() for o in want], [v.clone() for v in want_lp]
    tm = {}
    got, got_lp = generate_batch(r.m, ps, NEW, share_prefix=True, return_logprobs=True, timing=tm, **KW)
    assert tm["shared_prefix"] == 32
    assert same_lists(want, got) and same_lists(want_lp, got_lp)
    got, got_lp = generate_stream(r.m, ps, NEW, share_prefix=True, max_rows=4, check_every=3, return_logprobs=True, **KW)
    assert same_lists(want, got) and same_lists(want_lp, got_lp)


def test_one_engine_with_without_with(runs):
    """the buffer is part of the captured step's key: flag, no flag, flag again on one engine give what fresh engines give"""
    r = runs
    r.m.refresh_engine()
    a = generate_batch(r.m, r.ps, NEW, return_logprobs=True, **KW)
    a = ([o.clone() for o in a[0]], [v.clone() for v in a[1]])
    eng = r.m._engine
    b = [o.clone() for o in generate_batch(r.m, r.ps, NEW, **KW)]
    c = generate_batch(r.m, r.ps, NEW, return_logprobs=True, **KW)
    assert r.m._engine is eng and eng.graph_count(0) >= 2
    assert same_lists(a[0], r.out) and same_lists(a[1], r.lp)
    assert same_lists(b, r.plain)
    assert same_lists(c[0], r.out) and same_lists(c[1], r.lp)


@pytest.mark.parametrize("kv_cache", ("bf16", "fp8"))
def test_fp8_model(kv_cache):
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache=kv_cache)
    assert m.fp8 and m.kv_cache_dtype == kv_cache
    ps = ragged_prompts(cfg)
    plain = [o.clone() for o in generate_batch(m, ps, NEW, **KW)]
    out, lp = generate_batch(m, ps, NEW, return_logprobs=True, **KW)
    out, lp = [o.clone() for o in out], [v.clone() for v in lp]
    assert same_lists(plain, out)
    with torch.no_grad():
        for i in (3, 7):
            T = ps[i].numel()
            assert lp[i].numel() == NEW
            want = replay(m, ps[i], out[i][T:])
            assert torch.equal(lp[i], want), f"kv_cache={kv_cache} sequence {i}"


# ---- 4. score_batch -------------------------------------------------------------------------------------------------------------------
def test_score_batch(runs):
    r = runs
    cfg, m = r.cfg, r.m
    V = cfg.padded_vocab_size
    plens = [1, 30, 33, 64, 5, 47, 20, 9]
    clens = [1, 12, 1, cfg.block_size - 64 + 1, 24, 7, 3, 40]       # length 1; sequence 3 ends at the model's last position
    ps = [synth_prompts(1, n, V, seed=120 + i)[0].to(DEV) for i, n in enumerate(plens)]
    cs = [synth_prompts(1, n, V, seed=140 + i)[0].to(DEV) for i, n in enumerate(clens)]
    assert plens[3] + clens[3] - 1 == cfg.block_size
    joint = [v.clone() for v in score_batch(m, ps, cs)]
    assert [v.numel() for v in joint] == clens and all(v.dtype == torch.float32 for v in joint)
    with torch.no_grad():
        for i in range(1, len(ps)):         # sequence 0 is a single row: model(idx) takes it for a decode step
            seq = torch.cat([ps[i], cs[i][:-1]])
            lg = m(seq.view(1, -1))[0]
            want = ops.token_logprobs(lg[plens[i] - 1:].contiguous(), cs[i])
            assert torch.equal(joint[i], want), i
    for i in (0, 1, 3):
        assert torch.equal(score_batch(m, ps[i:i + 1], cs[i:i + 1])[0], joint[i]), i
    # max_tokens below any two sequences' rows: every sequence alone; at the largest pair's: groups of two or three
    rows = [a + b - 1 for a, b in zip(plens, clens)]
    for cap in (1, max(rows[i] + rows[i + 1] for i in range(0, 8, 2))):
        assert same_lists(joint, [v.clone() for v in score_batch(m, ps, cs, max_tokens=cap)]), cap
    assert m._cache_len == []


def test_score_batch_and_generate_batch_agree(runs):
    """The prefill kernels (score_batch) and the decode kernels (generate_batch) on the same tokens: recorded, not asserted beyond
    what two bf16 evaluations of one model can differ by at all (MEASUREMENTS.md, "Token log-probabilities")."""
    r = runs
    conts = [o[p.numel():] for o, p in zip(r.out, r.ps)]
    sc = score_batch(r.m, r.ps, conts)
    diff = max(float((a - b).abs().max()) for a, b in zip(sc, r.lp))
    record_parity(f"logprobs.score_vs_generate.{r.cfg.name}", max_abs_diff=diff)
    print(f"{r.cfg.name}: max |score_batch - generate_batch| = {diff:.4g}")
    assert all(bool(torch.isfinite(v).all()) for v in sc)


# ---- 5. error paths -------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(runs):
    r = runs
    V = r.cfg.padded_vocab_size
    lg = torch.zeros((2, 64), dtype=BF, device=DEV)
    for bad in ([0, 64], [-1, 3]):
        with pytest.raises(ValueError, match="outside"):
            ops.token_logprobs(lg, torch.tensor(bad, device=DEV))
    with pytest.raises(TypeError):
        ops.token_logprobs(lg.float(), torch.tensor([0, 1], device=DEV))
    with pytest.raises(ValueError):
        ops.token_logprobs(lg, torch.tensor([0, 1, 2], device=DEV))
    tokens = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    length = torch.zeros(2, dtype=torch.int32, device=DEV)
    done = torch.zeros(2, dtype=torch.int32, device=DEV)
    for buf, exc in ((torch.zeros((2, 4), dtype=torch.float64, device=DEV), TypeError),
                     (torch.zeros((2, 4), dtype=BF, device=DEV), TypeError),
                     (torch.zeros((2, 5), dtype=torch.float32, device=DEV), ValueError)):
        with pytest.raises(exc):
            ops.sample(lg, tokens, length, done, top_k=1, logprobs=buf)
        with pytest.raises(exc):
            ops.sample_rows(lg, tokens, length, done, torch.full((2,), 4, dtype=torch.int32, device=DEV),
                            torch.tensor([0, 1], dtype=torch.int32, device=DEV), 4, top_k=1, logprobs=buf)
    assert length.tolist() == [0, 0] and not bool(tokens.any())
    p = r.ps[1]
    with pytest.raises(ValueError, match="non-empty"):
        score_batch(r.m, [p], [torch.empty(0, dtype=torch.int64, device=DEV)])
    with pytest.raises(ValueError, match="outside"):
        score_batch(r.m, [p], [torch.tensor([1, V], device=DEV)])
    with pytest.raises(ValueError):
        score_batch(r.m, [p, p], [p])
    with pytest.raises(TypeError):
        r.m.engine().set_logprobs(torch.zeros((2, 4), dtype=torch.float64, device=DEV))
