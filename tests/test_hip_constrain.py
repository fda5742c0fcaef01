"""Constrained decoding on the GPU (include/dualhyp_hip.h, "Token masks").  Every check is exact (torch.equal).

The masked samplers are pinned to the unmasked ones, which test_hip_sampling.py pins to an fp64 reference: a masked pick on the raw rows
is the unmasked pick on constrain_reference.substitute(rows, mask) — 0xFF80 in every disallowed column — for every sampler; the
log-probabilities and alternatives are those of the raw rows (ops.token_logprobs, the unmasked call).  The engine tests hold the
captured steps to properties no row / sequence mix-up survives (disjoint masks; the first allowed id among a token's own 8
alternatives, which an independent path reports) and to schedule invariance."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_reference as BR  # noqa: E402
import constrain_reference as CR  # noqa: E402
import sampling_reference as SR  # noqa: E402
import top_logprob_reference as T  # noqa: E402
from dualhyp_amd import GPT, Config, constrain, generate, generate_batch, generate_stream, ops, quantize_model_fp8  # noqa: E402
from dualhyp_amd import _lib  # noqa: E402
from dualhyp_amd.beam import BeamState  # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
NEW = 24
KW = dict(temperature=1.0, top_k=1)
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}
VOCABS = (8, 320, 1001, 32000)       # the smallest; the 16-byte path; the scalar path with a partial last word; production
ROW_COUNTS = (1, 3, 37)
TEMPERATURES = (1.0, 0.2)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_lists(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and (same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y))
                                    for x, y in zip(a, b))


def same_top(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and same_bits(x[1], y[1]) for x, y in zip(a, b))


def clone_all(res):
    out = [[o.clone() for o in res[0]], [v.clone() for v in res[1]]]
    if len(res) > 2 and isinstance(res[2], list):
        out.append([(a.clone(), b.clone()) for a, b in res[2]])
    return out


# ---- 1. the ops, bit for bit ----------------------------------------------------------------------------------------------------------
_ROWS = {}


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


def state_for(n_seq, tok_ld=4):
    tokens = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
    length = torch.tensor([(u * 5) % (tok_ld - 1) for u in range(n_seq)], dtype=torch.int32, device=DEV)
    done = torch.zeros(n_seq, dtype=torch.int32, device=DEV)
    return tokens, length, done


def bufs(shape, k):
    return (torch.full(shape, NAN, dtype=torch.float32, device=DEV), torch.full(shape + (k,), -1, dtype=torch.int32, device=DEV),
            torch.full(shape + (k,), NAN, dtype=torch.float32, device=DEV))


def defined_rows(sub):
    """rows with at least one allowed logit above -inf; the others are outside the definition"""
    return (sub.float() > -float("inf")).any(dim=1)


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_is_the_unmasked_pick_on_substituted_rows(V, top_k):
    k_top = min(3, V)
    seen_defined = seen_forbidden = 0
    for n in ROW_COUNTS:
        raw_cpu = rows_for(V, n)
        raw = raw_cpu.to(DEV)
        raw_top = ops.token_top_logprobs(raw, k_top)
        for kind in CR.MASK_KINDS:
            m = CR.make_masks(kind, raw_cpu).to(DEV)
            sub = CR.substitute(raw, m)
            ok = defined_rows(sub)
            allowed = torch.from_numpy(CR.unpack_bits(m, V)).to(DEV)
            for temp in TEMPERATURES:
                eos = int(raw_cpu[0].float().argmax()) if kind == "all_ones" else None
                kw = dict(temperature=temp, top_k=top_k, eos_id=eos, seed=SR.SEEDS[1], step=7)
                want = state_for(n)
                ops.sample(sub, *want, **kw)
                got = state_for(n)
                lp, t_ids, t_lp = bufs(tuple(got[0].shape), k_top)
                ops.sample(raw, *got, logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m, **kw)
                what = f"V={V} n={n} {kind} T={temp} top_k={top_k}"
                ar = torch.arange(n, device=DEV)
                at = torch.tensor([(u * 5) % 3 for u in range(n)], device=DEV)
                picked = got[0][ar, at]
                assert bool(((picked >= 0) & (picked < V)).all()), what
                for x, y, name in zip(got, want, ("tokens", "length", "done")):
                    assert torch.equal(x[ok], y[ok]), f"{what}: {name}"
                assert bool(allowed[ar, picked][ok].all()), f"{what}: a disallowed id was picked"
                # the log-probability is the raw row's, the alternatives are the raw row's
                assert same_bits(lp[ar, at], ops.token_logprobs(raw, picked)), what
                assert torch.equal(t_ids[ar, at], raw_top[0]) and same_bits(t_lp[ar, at], raw_top[1]), what
                written = torch.zeros_like(got[0], dtype=torch.bool)
                written[ar, at] = True
                assert bool((got[0][~written] == -1).all()) and bool(torch.isnan(lp[~written]).all()) and bool((t_ids[~written] == -1).all())
                seen_defined += int(ok.sum())
                if kind == "argmax_forbidden":
                    plain = state_for(n)
                    ops.sample(raw, *plain, **kw)
                    seen_forbidden += int((plain[0][ar, at] != picked).sum())
    assert seen_defined > 0
    if top_k == 1:
        assert seen_forbidden > 0          # forbidding the arg-max moved the pick


@pytest.mark.parametrize("top_k", (1, 5, None))
@pytest.mark.parametrize("V", VOCABS)
def test_sample_rows_reads_the_sequences_mask_row(V, top_k):
    """logits row r is picked under mask row row_seq[r]: a shuffled row list over more sequences than rows, a finished sequence named
    by two rows"""
    k_top, max_new, tok_ld = min(3, V), 4, 9
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
        plen = [(u * 3) % 4 + 1 for u in range(n_seq)]
        limit = torch.tensor([p + max_new for p in plen], dtype=torch.int32, device=DEV)

        def fresh():
            tokens = torch.full((n_seq, tok_ld), -1, dtype=torch.int64, device=DEV)
            length = torch.tensor([p + (u % 3) for u, p in enumerate(plen)], dtype=torch.int32, device=DEV)
            done = torch.zeros(n_seq, dtype=torch.int32, device=DEV)
            done[fin] = 1
            return tokens, length, done

        live = [r for r, u in enumerate(order) if u != fin]
        for kind in CR.MASK_KINDS:
            # one mask row per SEQUENCE; sequence u's row is made from the logits row that names it (row 0's for the others)
            by_seq = torch.zeros(n_seq, dtype=torch.long)
            for r, u in enumerate(order):
                by_seq[u] = r
            m = CR.make_masks(kind, raw_cpu[by_seq]).to(DEV)
            sub = CR.substitute(raw, m[row_seq.long()])
            ok = defined_rows(sub)
            for temp in TEMPERATURES:
                kw = dict(temperature=temp, top_k=top_k, seed=SR.SEEDS[0])
                want = fresh()
                ops.sample_rows(sub, *want, limit, row_seq, max_new, **kw)
                got = fresh()
                lp, t_ids, t_lp = bufs((n_seq, tok_ld), k_top)
                ops.sample_rows(raw, *got, limit, row_seq, max_new, logprobs=lp, top_logprobs=(t_ids, t_lp), mask=m, **kw)
                what = f"V={V} n={n} {kind} T={temp} top_k={top_k}"
                start = fresh()[1]
                for r in live:
                    u = order[r]
                    at = int(start[u])
                    pick = int(got[0][u, at])
                    assert 0 <= pick < V, what
                    if bool(ok[r]):
                        assert pick == int(want[0][u, at]) and int(got[1][u]) == int(want[1][u]) and int(got[2][u]) == int(want[2][u]), \
                            f"{what}: row {r} sequence {u}"
                    assert same_bits(lp[u, at], ops.token_logprobs(raw[r:r + 1], got[0][u, at:at + 1])[0]), what
                    assert torch.equal(t_ids[u, at], raw_top[0][r]) and same_bits(t_lp[u, at], raw_top[1][r]), what
                assert bool((got[0][fin] == -1).all()) and int(got[1][fin]) == int(start[fin])
                assert int((got[0] != -1).sum()) == len(live)


# ---- 2. alignment and row invariance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (320, 128256))
def test_unaligned_logits_and_wide_mask_rows(V):
    n = 3
    g = torch.Generator().manual_seed(V)
    raw_cpu = (torch.randn((n, V), generator=g, dtype=torch.float64) * 3).to(BF)
    raw_cpu[0] = (raw_cpu[0].double() * 2).round() / 2                 # a row of ties
    raw = raw_cpu.to(DEV)
    store = torch.zeros(n * V + 8, dtype=BF, device=DEV)
    shifted = store[1:1 + n * V].view(n, V)                            # rows 2 bytes off a 16-byte boundary: the scalar loops
    shifted.copy_(raw)
    assert shifted.data_ptr() % 16 == 2 and raw.data_ptr() % 16 == 0 and shifted.is_contiguous()
    words = CR.words(V)
    for kind in ("random_half", "alternating", "argmax_forbidden", "single_last"):
        m = CR.make_masks(kind, raw_cpu).to(DEV)
        wide_store = torch.full((n, words + 3), -1, dtype=torch.int32, device=DEV)      # all-ones words between the rows
        wide_store[:, :words] = m
        wide = wide_store[:, :words]
        assert wide.stride(0) == words + 3 and not wide.is_contiguous()
        for top_k in (1, 5, None):
            kw = dict(temperature=0.7, top_k=top_k, seed=5, step=2)
            res = []
            for lg, mk in ((raw, m), (shifted, m), (raw, wide), (shifted, wide)):
                st = state_for(n)
                lp = torch.full(tuple(st[0].shape), NAN, dtype=torch.float32, device=DEV)
                ops.sample(lg, *st, logprobs=lp, mask=mk, **kw)
                res.append((st[0], lp))
            for tok, lp in res[1:]:
                assert torch.equal(tok, res[0][0]) and same_bits(lp, res[0][1]), f"V={V} {kind} top_k={top_k}"
        a = ops.token_top_logprobs(raw, 4, mask=m)
        for lg, mk in ((shifted, m), (raw, wide), (shifted, wide)):
            b = ops.token_top_logprobs(lg, 4, mask=mk)
            assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1]), f"V={V} {kind}"


# ---- 3. beam candidates ---------------------------------------------------------------------------------------------------------------
def candidate_masks(raw_cpu, W, g):
    """name -> int32 [n, words]: a random half, exactly 2 W allowed ids, and allowed ids that all lie outside the raw top 8"""
    n, V = raw_cpu.shape
    out = {"random_half": CR.make_masks("random_half", raw_cpu), "alternating": CR.make_masks("alternating", raw_cpu),
           "all_ones": CR.make_masks("all_ones", raw_cpu)}
    exact = np.zeros((n, V), dtype=bool)
    for r in range(n):
        exact[r, torch.randperm(V, generator=g)[:2 * W].numpy()] = True
    out["exactly_2W"] = CR.pack_bits(exact)
    if V > 8 + 2 * W:
        outside = np.ones((n, V), dtype=bool)
        top8 = T.top_ids(raw_cpu, 8).numpy()
        for r in range(n):
            outside[r, top8[r]] = False
        out["outside_top_8"] = CR.pack_bits(outside)
        few = np.zeros((n, V), dtype=bool)                     # ... and exactly 2 W of them
        for r in range(n):
            few[r, np.nonzero(outside[r])[0][torch.randperm(V - 8, generator=g)[:2 * W].numpy()]] = True
        out["outside_top_8_exactly_2W"] = CR.pack_bits(few)
    return out


def finite_rows(V, n, g):
    rand = (torch.randn((n, V), generator=g) * 4).to(BF)
    coarse = torch.randint(-2, 3, (n, V), generator=g).to(BF)             # many equal logits, and +0 among them
    coarse[:, 1::7] = -0.0                                                # ... and -0: equal to +0, the lower index first
    return {"random": rand, "coarse": coarse, "constant": torch.full((n, V), 1.5, dtype=BF)}


@pytest.mark.parametrize("W", (2, 4))
@pytest.mark.parametrize("V", (8, 320, 1001, 32000))
def test_candidates_are_the_first_2w_allowed_ids(V, W):
    g = torch.Generator().manual_seed(V * 8 + W)
    n, K = 5, 2 * W
    for rname, raw_cpu in finite_rows(V, n, g).items():
        raw = raw_cpu.to(DEV)
        for mname, m_cpu in candidate_masks(raw_cpu, W, g).items():
            if CR.unpack_bits(m_cpu, V).sum(axis=1).min() < K:
                continue                                        # fewer than 2 W allowed ids: the host refuses such a mask
            m = m_cpu.to(DEV)
            what = f"V={V} W={W} {rname} {mname}"
            ids, lp = ops.token_top_logprobs(raw, K, mask=m)
            want_ids = ops.token_top_logprobs(CR.substitute(raw, m), K)[0]
            assert torch.equal(ids, want_ids), what
            assert torch.equal(ids, torch.from_numpy(np.argsort(-np.where(CR.unpack_bits(m, V), raw_cpu.double().numpy(), -np.inf), axis=1,
                                                                 kind="stable")[:, :K].astype(np.int32)).to(DEV)), what
            for j in range(K):
                assert same_bits(lp[:, j], ops.token_logprobs(raw, ids[:, j].long())), f"{what} rank {j}"
            if mname == "outside_top_8":
                top8 = ops.token_top_logprobs(raw, 8)[0]
                assert not bool((ids[:, :, None] == top8[:, None, :]).any()), what
            if mname == "all_ones":
                plain = ops.token_top_logprobs(raw, K)
                assert torch.equal(ids, plain[0]) and same_bits(lp, plain[1]), what


MAXNEW = 6
KEYS_I = ("n_steps", "done", "n_fin", "fin_step", "fin_parent", "beam_tok", "beam_parent")
KEYS_F = ("cum", "fin_score", "fin_lp", "beam_lp", "beam_cum")


def select_case(logits, mask, W, rpu, n_utt, eos, step, cum, what):
    """one masked dh_beam_select_bf16_mask call against beam_reference's step fed the masked candidate rows"""
    import copy
    st = BeamState(n_utt, W, MAXNEW, DEV)
    st.n_steps.fill_(step)
    if cum is not None:
        st.cum.copy_(cum)
    before = st.host()
    ids, lp = ops.beam_select(logits, st, rows_per_utt=rpu, eos_id=eos, step=step, mask=mask)
    t_ids, t_lp = ops.token_top_logprobs(logits, 2 * W, mask=mask.repeat_interleave(rpu, dim=0).contiguous())
    assert torch.equal(ids, t_ids) and same_bits(lp, t_lp), f"{what}: the candidates are not the masked token_top_logprobs(2 W)"
    got, want = st.host(), copy.deepcopy(before)
    c_ids, c_lp = t_ids.tolist(), t_lp.tolist()
    for u in range(n_utt):
        ut = BR.Utterance(W, MAXNEW, eos)
        ut.cum = [np.float32(c) for c in before["cum"][u][:rpu]]
        ut.hist = [([], [])] * rpu
        ut.n_steps = step
        ut.step([list(zip(c_ids[u * rpu + b], c_lp[u * rpu + b])) for b in range(rpu)])
        for w, r in enumerate(ut.records[-1]):
            want["beam_tok"][u][step][w], want["beam_parent"][u][step][w] = r["tok"], r["parent"]
            want["beam_lp"][u][step][w], want["beam_cum"][u][step][w] = float(r["lp"]), float(r["cum"])
            want["cum"][u][w] = float(r["cum"])
        for k, p in enumerate(ut.pool):
            want["fin_step"][u][k], want["fin_parent"][u][k] = p["step"], p["parent"]
            want["fin_score"][u][k], want["fin_lp"][u][k] = float(p["score"]), float(p["lp"])
        want["n_fin"][u], want["n_steps"][u], want["done"][u] = len(ut.pool), ut.n_steps, ut.done
    for k in KEYS_I + KEYS_F:
        dt = torch.int32 if k in KEYS_I else torch.float32
        assert torch.equal(torch.tensor(got[k], dtype=dt), torch.tensor(want[k], dtype=dt)), f"{what}: {k} differs"
    return got, t_ids


@pytest.mark.parametrize("W", (2, 4))
@pytest.mark.parametrize("V", (320, 1001))
def test_beam_select_under_a_mask(V, W):
    g = torch.Generator().manual_seed(V * 16 + W)
    for n_utt in (1, 3):
        for rpu in (1, W):
            rows = n_utt * rpu
            step = 0 if rpu == 1 else 2
            cum = -(torch.rand((n_utt, W), generator=g) * 8).to(DEV) if rpu == W else None
            for rname, raw_cpu in finite_rows(V, rows, g).items():
                raw = raw_cpu.to(DEV)
                # one mask row per utterance, made from its first row
                for mname, m_cpu in candidate_masks(raw_cpu[::rpu].contiguous(), W, g).items():
                    if (mname.startswith("outside") and rpu > 1) or CR.unpack_bits(m_cpu, V).sum(axis=1).min() < 2 * W:
                        continue                                # "outside the top 8" is a statement about one row
                    m = m_cpu.to(DEV)
                    what = f"V={V} W={W} n={n_utt} rpu={rpu} {rname} {mname}"
                    got, cand = select_case(raw, m, W, rpu, n_utt, None, step, cum, what)
                    allowed = CR.unpack_bits(m, V)
                    for u in range(n_utt):
                        assert all(allowed[u][t] for t in got["beam_tok"][u][step]), what
                    # an allowed EOS at rank 1 of the first row of every utterance
                    eos = int(cand[0, 1])
                    if all(allowed[u][eos] for u in range(n_utt)):
                        select_case(raw, m, W, rpu, n_utt, eos, step, cum, what + " EOS")


# ---- 4. the engine --------------------------------------------------------------------------------------------------------------------
def build(name, seed=11, **over):
    cfg = Config.from_name(name, **LORA, **over)
    assert cfg.head_size == HEAD_SIZES[name]
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=BF)
    m.load_state_dict(sd)
    m.eval()
    return cfg, m


LENS = (1, 31, 32, 33, 47)


def ragged_prompts(cfg, seed=70):
    return [synth_prompts(1, n, cfg.padded_vocab_size, seed=seed + i)[0].to(DEV) for i, n in enumerate(LENS)]


@pytest.fixture(scope="module")
def tiny():
    return build("parity-tiny")


_MODELS = {}


def model_for(name, tiny):
    if name == "parity-tiny":
        return tiny
    if name not in _MODELS:
        _MODELS[name] = build(name)
    return _MODELS[name]


def produced(st, ps, u):
    """the ids sequence u produced, the EOS included"""
    return st["tokens"][u, ps[u].numel():int(st["length"][u])].tolist()


def check_disjoint(m, cfg, ps, what):
    """4a: sequence u allows the ids with id % n == u, plus the EOS"""
    V, n = cfg.padded_vocab_size, len(ps)
    free = generate_batch(m, ps, NEW, **KW)
    eos = int(free[1][ps[1].numel() + 1])
    mask = CR.disjoint_masks(n, V, eos).to(DEV)
    out, lp, st = generate_batch(m, ps, NEW, eos_id=eos, token_mask=mask, return_logprobs=True, return_state=True, **KW)
    n_tok = 0
    for u in range(n):
        ids = produced(st, ps, u)
        assert ids and all(i == eos or i % n == u for i in ids), f"{what}: sequence {u} produced {ids}"
        assert lp[u].numel() == len(ids) and bool(torch.isfinite(lp[u]).all())
        n_tok += len(ids)
    assert n_tok > n
    return eos, mask


def check_first_allowed(m, cfg, ps, what):
    """4c: every produced token is the first allowed id among its own 8 alternatives, wherever one of the 8 is allowed"""
    V, n = cfg.padded_vocab_size, len(ps)
    mask_cpu = CR.random_half_masks(n, V, seed=2024)
    allowed = CR.unpack_bits(mask_cpu, V)
    out, lp, top = generate_batch(m, ps, NEW, token_mask=mask_cpu.to(DEV), return_logprobs=True, top_logprobs=8, **KW)
    total = skipped = 0
    for u, p in enumerate(ps):
        ids = out[u][p.numel():].tolist()
        assert len(ids) == NEW and all(allowed[u][i] for i in ids), f"{what}: sequence {u}"
        for t, alts in zip(ids, top[u][0].tolist()):
            first = CR.first_allowed(alts, allowed[u])
            total += 1
            if first < 0:
                skipped += 1
                continue
            assert t == first, f"{what}: sequence {u} produced {t}, the first allowed of {alts} is {first}"
    assert total == n * NEW and skipped <= 0.05 * total, f"{what}: {skipped} of {total} tokens had none of their 8 alternatives allowed"
    return mask_cpu


@pytest.mark.parametrize("name", list(HEAD_SIZES))
def test_disjoint_masks_and_first_allowed_alternative(name, tiny):
    cfg, m = model_for(name, tiny)
    ps = ragged_prompts(cfg)
    check_disjoint(m, cfg, ps, name)
    check_first_allowed(m, cfg, ps, name)


def test_all_ones_mask_changes_nothing(tiny):
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    V = cfg.padded_vocab_size
    for kw in (KW, dict(temperature=0.7, top_k=5), dict(temperature=0.7, top_k=None)):
        want = clone_all(generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=3, seed=9, **kw))
        got = generate_batch(m, ps, NEW, return_logprobs=True, top_logprobs=3, seed=9, token_mask=constrain.all_ones(len(ps), V, DEV), **kw)
        assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2]), kw
    # a list of id lists is packed for the caller; generate() forwards the mask
    want = generate_batch(m, ps, NEW, **KW)
    assert same_lists([o.clone() for o in want], generate_batch(m, ps, NEW, token_mask=[list(range(V))] * len(ps), **KW))
    mask = CR.random_half_masks(len(ps), V, seed=2024).to(DEV)
    many = [o.clone() for o in generate_batch(m, ps, NEW, token_mask=mask, **KW)]
    one = generate(m, ps[3], ps[3].numel() + NEW, token_mask=mask[3:4].contiguous(), **KW)
    assert torch.equal(one, many[3])


def test_schedules_agree_under_a_mask(tiny):
    """4d: generate_stream, speculate and share_prefix give generate_batch's ids, logprobs and alternatives"""
    cfg, m = tiny
    V = cfg.padded_vocab_size
    head = synth_prompts(1, 32, V, seed=5)[0].to(DEV)
    ps = [torch.cat([head, synth_prompts(1, n, V, seed=40 + n)[0].to(DEV)]) for n in (1, 2, 31, 32, 33, 50)]
    mask = CR.random_half_masks(len(ps), V, seed=77).to(DEV)
    allowed = CR.unpack_bits(mask, V)
    kw = dict(return_logprobs=True, top_logprobs=8, token_mask=mask, **KW)
    free = generate_batch(m, ps, NEW, **kw)
    eos_pick = int(free[0][2][ps[2].numel() + 2])                       # sequence 2's third token: it ends there, the others may
    for eos in (None, eos_pick):
        want = clone_all(generate_batch(m, ps, NEW, eos_id=eos, **kw))
        for u, p in enumerate(ps):
            assert all(allowed[u][i] for i in want[0][u][p.numel():].tolist())
        if eos is not None:
            assert want[0][2].numel() == ps[2].numel() + 2
        runs = {"stream": generate_stream(m, ps, NEW, eos_id=eos, max_rows=4, check_every=3, **kw)}
        for D in (1, 3, 7):
            runs[f"speculate={D}"] = generate_batch(m, ps, NEW, eos_id=eos, speculate=D, **kw)
        tm = {}
        runs["share_prefix"] = generate_batch(m, ps, NEW, eos_id=eos, share_prefix=True, timing=tm, **kw)
        assert tm["shared_prefix"] == 32
        runs["share_prefix stream"] = generate_stream(m, ps, NEW, eos_id=eos, share_prefix=True, max_rows=4, check_every=3, **kw)
        for name, got in runs.items():
            assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2]), f"eos={eos} {name}"
    # scripted drafts: all right (accepted under the mask), all wrong
    want = clone_all(generate_batch(m, ps, NEW, **kw))
    right = torch.stack([o[p.numel():] for o, p in zip(want[0], ps)]).contiguous()
    for drafts, some in ((right, True), (((right + 1) % V).contiguous(), False)):
        tm = {}
        got = generate_batch(m, ps, NEW, speculate=3, drafts=drafts, timing=tm, **kw)
        assert same_lists(want[0], got[0]) and same_lists(want[1], got[1]) and same_top(want[2], got[2])
        assert (tm["spec_accepted"] > 0) == some


@pytest.mark.parametrize("kv_cache", ("bf16", "fp8"))
def test_fp8_model(kv_cache):
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache=kv_cache)
    assert m.fp8 and m.kv_cache_dtype == kv_cache
    ps = ragged_prompts(cfg)
    check_disjoint(m, cfg, ps, f"fp8 weights, {kv_cache} cache")
    check_first_allowed(m, cfg, ps, f"fp8 weights, {kv_cache} cache")


def test_graph_keys(tiny):
    """The mask pointer and its leading dimension are part of the captured step's key, as the logprobs pointer is: plain and masked
    calls capture one step each, a wider view of the same storage another; the plain call again captures nothing and gives what it
    gave; generate_batch leaves no mask on the engine."""
    cfg, m = tiny
    ps = ragged_prompts(cfg)
    V = cfg.padded_vocab_size
    B, lens, steps = len(ps), [int(p.numel()) for p in ps], 8
    tok_ld = max(lens) + steps + 1
    m.refresh_engine()
    eng = m.engine(B, max(lens) + steps, sum(lens), exact=True)
    eng.set_rsqrt_emulation(m.cpu_rsqrt_vec_width, whole_call=False)
    tokens0 = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(ps, batch_first=True), (0, tok_ld - max(lens))).contiguous()
    tokens, length, done = tokens0.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    words = CR.words(V)
    store = torch.zeros(B * 2 * words, dtype=torch.int32, device=DEV)
    half = CR.random_half_masks(B, V, seed=3)
    allowed = CR.unpack_bits(half, V)
    packed = torch.cat(ps)

    def run(ld):
        tokens.copy_(tokens0)
        length.copy_(torch.tensor(lens, dtype=torch.int32))
        done.zero_()
        mask = None
        if ld:
            mask = store[:B * ld].view(B, ld)                  # one allocation: only mask_ld tells the two masked keys apart
            mask.fill_(-1)
            mask[:, :words] = half.to(DEV)
            assert mask.data_ptr() == store.data_ptr()
        _, last = eng.forward(packed, lens, [0] * B, want_all=False, want_last=True, slot_base=0)
        ops.sample(last, tokens, length, done, seed=3, step=0, mask=mask, **KW)
        eng.set_token_mask(mask)
        try:
            eng.decode(tokens, length, done, steps, KW["temperature"], KW["top_k"], None, 3, first_step=0)
        finally:
            eng.set_token_mask(None)
        torch.cuda.synchronize()
        return dict(tokens=tokens.clone(), count=eng.graph_count(0))

    c0 = eng.graph_count(0)
    plain, masked, wide = run(0), run(words), run(2 * words)
    assert [x["count"] - c0 for x in (plain, masked, wide)] == [1, 2, 3]
    plain2, masked2 = run(0), run(words)
    assert plain2["count"] == masked2["count"] == wide["count"]          # nothing new was captured: every step was found again
    assert torch.equal(plain2["tokens"], plain["tokens"]) and torch.equal(masked2["tokens"], masked["tokens"])
    assert torch.equal(wide["tokens"], masked["tokens"]) and not torch.equal(masked["tokens"], plain["tokens"])
    for u, n in enumerate(lens):
        assert all(allowed[u][i] for i in masked["tokens"][u, n:n + steps + 1].tolist())
    m.refresh_engine()
    # the serving entry point: a masked call, then the plain call it does not disturb, and no mask left behind
    want = [o.clone() for o in generate_batch(m, ps, NEW, **KW)]
    eng = m._engine
    generate_batch(m, ps, NEW, token_mask=half.to(DEV), **KW)
    assert m._engine is eng and eng._token_mask is None
    assert same_lists(want, generate_batch(m, ps, NEW, **KW))         # (its buffers are new allocations: the step count says nothing here)
    with pytest.raises(_lib.DualHypHipError, match="mask_ld"):
        _lib.check(eng.lib.dh_engine_set_token_mask(eng.handle, half.to(DEV).data_ptr(), words - 1))
    assert eng._token_mask is None


# ---- 6. refusals before any launch ----------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(tiny):
    cfg, m = tiny
    V = cfg.padded_vocab_size
    ps = ragged_prompts(cfg)[:3]
    good = constrain.all_ones(3, V, DEV)
    empty = good.clone()
    empty[1] = 0
    for fn in (generate_batch, generate_stream):
        with pytest.raises(ValueError, match="row 1 allows 0"):
            fn(m, ps, 4, token_mask=empty, **KW)
        with pytest.raises(ValueError, match=r"\[3, 8\]"):
            fn(m, ps, 4, token_mask=constrain.all_ones(4, V, DEV), **KW)               # the wrong number of rows
        with pytest.raises(ValueError, match="lives on cpu"):
            fn(m, ps, 4, token_mask=good.cpu(), **KW)
    lg = torch.zeros((2, 65), dtype=BF, device=DEV)
    tokens, length, done = (torch.zeros((2, 4), dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                            torch.zeros(2, dtype=torch.int32, device=DEV))
    limit, row_seq = torch.full((2,), 4, dtype=torch.int32, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    ok = constrain.all_ones(2, 65, DEV)
    for bad, exc in ((ok.cpu(), _lib.DualHypHipError), (ok.long(), TypeError), (ok[:1], ValueError), (ok[:, :2], ValueError),
                     (torch.cat([ok, ok], 1)[:, ::2], ValueError)):
        with pytest.raises(exc):
            ops.sample(lg, tokens, length, done, top_k=1, mask=bad)
        with pytest.raises(exc):
            ops.sample_rows(lg, tokens, length, done, limit, row_seq, 4, top_k=1, mask=bad)
        with pytest.raises(exc):
            ops.token_top_logprobs(lg, 2, mask=bad)
    # mask_ld too small at the C entries, with real pointers
    lib = _lib.load()
    assert lib.dh_sample_bf16_mask(lg.data_ptr(), 65, tokens.data_ptr(), 4, length.data_ptr(), done.data_ptr(), 2, 1.0, 1, -1, 0, 0, None,
                                   None, 0, None, None, ok.data_ptr(), 2) != 0
    assert b"mask_ld=2 is below the 3 words" in lib.dh_last_error()
    assert lib.dh_sample_bf16_mask(lg.data_ptr(), 65, tokens.data_ptr(), 4, length.data_ptr(), done.data_ptr(), 2, 1.0, 1, -1, 0, 0, None,
                                   None, 0, None, None, None, 3) != 0
    assert b"null mask" in lib.dh_last_error()
    torch.cuda.synchronize()
    assert length.tolist() == [0, 0] and not bool(tokens.any())


# ---- the serving CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", (["--schedule", "batch", "--top_logprobs", "2"], ["--schedule", "continuous", "--logprobs"], ["--num_beams", "2"]),
                         ids=("batch", "continuous", "beams"))
def test_inference_cli_constrain_prompt(tmp_path, monkeypatch, more):
    """`python -m dualhyp_amd.inference --constrain prompt --constrain_extra FILE` end to end (in this process): the entry point gets
    each utterance's own mask — its prompt's ids, the EOS, the extras — and produces nothing outside it; every record is marked"""
    import json
    import test_harness as harness
    import importlib
    from dualhyp_amd import inference
    G = importlib.import_module("dualhyp_amd.generate")        # the package's attribute of that name is the function
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    extra = tmp_path / "extra.txt"
    extra.write_text("# allowed everywhere\n33\n63\n")
    seen = []
    name = "beam_search_batch" if "--num_beams" in more else "generate_stream" if "continuous" in more else "generate_batch"
    real = getattr(G, name)

    def spy(model, prompts, max_new, **kw):
        res = real(model, prompts, max_new, **kw)
        outs = [hyps[0]["tokens"] for hyps in res] if name == "beam_search_batch" else res[0] if isinstance(res, tuple) else res
        seen.append(([p.cpu() for p in prompts], kw.get("token_mask"), kw.get("eos_id"), [o.cpu() for o in outs]))
        return res

    monkeypatch.setattr(G, name, spy)
    inference.main(["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
                    "DualHyp", "--dual_hypotheses", "--max_new_tokens", "6", "--decode_batch", "4", "--constrain", "prompt", "--constrain_extra",
                    str(extra), "--predict_dir", str(tmp_path / "pred")] + more)
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2 and all(rec["constrained"] is True for rec in js[:-2])
    assert seen and sum(len(s[0]) for s in seen) == len(items)
    V = Config.from_name("parity-hs96").padded_vocab_size
    for prompts, mask, eos, outs in seen:
        assert mask is not None and mask.is_cuda and tuple(mask.shape) == (len(prompts), CR.words(V))
        want = np.zeros((len(prompts), V), dtype=bool)
        for u, p in enumerate(prompts):
            want[u, p.numpy()] = True
            want[u, [33, 63, eos]] = True
        assert np.array_equal(CR.unpack_bits(mask, V), want)
        for u, (p, o) in enumerate(zip(prompts, outs)):
            assert all(want[u][i] for i in o[p.numel():].tolist())
