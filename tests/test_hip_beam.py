"""Beam search on the GPU (beam_search_batch, dh_beam_select_bf16, dh_engine_decode_beam).  Every check is exact (torch.equal).

Op level: the selection kernel against tests/beam_reference.py, which is fed with ops.token_top_logprobs of the same rows (that op is
pinned by test_hip_top_logprobs.py), so every output — the fp32 scores included — has one right value.

End to end: the fused path against a plain Python beam search that uses only entry points older than beam search: at every step each
live hypothesis is recomputed from scratch in a KV slot of its own (its prompt prefilled, its tokens fed one at a time by single-token
forward calls, i.e. the decode family), the last row goes through ops.token_top_logprobs and the selection is beam_reference's.  A
decode row's bits do not depend on what it is packed with, so these are the bits the fused path must produce: tokens,
parents, log-probabilities, cumulative scores, pool, done flags, the ranked output, and the K / V^T cache of the final live beams."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_reference as R  # noqa: E402
from conftest import record_parity  # noqa: E402
from dualhyp_amd import GPT, Config, beam_search_batch, generate_batch, ops, score_batch  # noqa: E402
from dualhyp_amd.beam import BeamState  # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
HEAD_SIZES = {"parity-tiny": 64, "parity-hs96": 96, "parity-hs128": 128}
KEYS_I = ("n_steps", "done", "n_fin", "fin_step", "fin_parent", "beam_tok", "beam_parent")
KEYS_F = ("cum", "fin_score", "fin_lp", "beam_lp", "beam_cum")
MAXNEW = 6


def same_state(got, want, what=""):
    for k in KEYS_I + KEYS_F:
        dt = torch.int32 if k in KEYS_I else torch.float32
        assert torch.equal(torch.tensor(got[k], dtype=dt), torch.tensor(want[k], dtype=dt)), f"{what}: {k} differs"


# ---- op level -------------------------------------------------------------------------------------------------------------------------
def select_case(logits, W, rpu, n_utt, eos, step, cum=None, n_fin=None, done=None, what=""):
    """one dh_beam_select_bf16 call on a state prepared as asked, against the reference's step from the same state"""
    st = BeamState(n_utt, W, MAXNEW, DEV)
    st.n_steps.fill_(step)
    if cum is not None:
        st.cum.copy_(cum)
    if n_fin is not None:          # entries that are there already: marked, so that an overwritten one shows
        st.n_fin.copy_(torch.tensor(n_fin, dtype=torch.int32))
        for u, k in enumerate(n_fin):
            st.fin_step[u, :k] = 77
            st.fin_score[u, :k] = -77.0
    if done is not None:
        st.done.copy_(torch.tensor(done, dtype=torch.int32))
    before = st.host()
    ids, lp = ops.beam_select(logits, st, rows_per_utt=rpu, eos_id=eos, step=step)
    t_ids, t_lp = ops.token_top_logprobs(logits, 2 * W)
    assert torch.equal(ids, t_ids) and torch.equal(lp, t_lp), f"{what}: the candidates are not token_top_logprobs(2 W)"
    assert int(ids.min()) >= 0 and int(ids.max()) < logits.size(1)
    got = st.host()
    want = copy.deepcopy(before)
    c_ids, c_lp = t_ids.tolist(), t_lp.tolist()
    for u in range(n_utt):
        if before["done"][u]:
            continue
        ut = R.Utterance(W, MAXNEW, eos)
        ut.cum = [np.float32(c) for c in before["cum"][u][:rpu]]
        ut.hist = [([], [])] * rpu
        ut.n_steps = step
        ut.pool = [None] * before["n_fin"][u]
        ut.step([list(zip(c_ids[u * rpu + b], c_lp[u * rpu + b])) for b in range(rpu)])
        for w, r in enumerate(ut.records[-1]):
            want["beam_tok"][u][step][w], want["beam_parent"][u][step][w] = r["tok"], r["parent"]
            want["beam_lp"][u][step][w], want["beam_cum"][u][step][w] = float(r["lp"]), float(r["cum"])
            want["cum"][u][w] = float(r["cum"])
        for k in range(before["n_fin"][u], len(ut.pool)):
            p = ut.pool[k]
            want["fin_step"][u][k], want["fin_parent"][u][k] = p["step"], p["parent"]
            want["fin_score"][u][k], want["fin_lp"][u][k] = float(p["score"]), float(p["lp"])
        want["n_fin"][u], want["n_steps"][u], want["done"][u] = len(ut.pool), ut.n_steps, ut.done
    same_state(got, want, what)
    return got


@pytest.mark.parametrize("W", (1, 2, 3, 4))
@pytest.mark.parametrize("vocab", (8, 320, 1000, 1001, 32064))      # 1001: odd rows, the scalar loads
def test_beam_select_against_the_reference(vocab, W):
    g = torch.Generator().manual_seed(vocab * 8 + W)
    seen_done = set()
    for n_utt in (1, 3, 37):
        for rpu in sorted({1, W}):
            rows = n_utt * rpu
            step = 0 if rpu == 1 and W > 1 else 2
            rand = (torch.randn((rows, vocab), generator=g) * 4).to(torch.bfloat16).to(DEV)
            # coarse values: many equal logits inside a row, and the top of several rows alike
            coarse = torch.randint(-2, 3, (rows, vocab), generator=g).to(torch.bfloat16).to(DEV)
            const = torch.full((rows, vocab), 1.5, dtype=torch.bfloat16, device=DEV)
            cum = None
            if rpu == W:
                cum = -(torch.rand((n_utt, W), generator=g) * 8).to(DEV)
            eq_cum = torch.full((n_utt, W), -2.5, device=DEV)
            tag = f"V{vocab} W{W} n{n_utt} rpu{rpu}"
            select_case(rand, W, rpu, n_utt, None, step, cum, what=tag + " random")
            select_case(coarse, W, rpu, n_utt, None, step, cum, what=tag + " coarse")
            # constant rows: every lp ties; with equal cum every score ties and the order is beam, then rank
            select_case(const, W, rpu, n_utt, None, step, cum, what=tag + " constant")
            select_case(const, W, rpu, n_utt, 1, step, eq_cum if rpu == W else None, what=tag + " constant, equal cum, EOS = rank 1")
            select_case(rand, W, rpu, n_utt, None, step, eq_cum if rpu == W else None, what=tag + " equal cum")
            # EOS as rank 0 of every row
            top = rand.clone()
            top[:, 5] = 100.0
            got = select_case(top, W, rpu, n_utt, 5, step, cum, what=tag + " EOS rank 0")
            assert all(n == min(rpu, W) for n in got["n_fin"])
            # ... into a pool one short of full: one entry fits, the utterance is done
            got = select_case(top, W, rpu, n_utt, 5, step, cum, n_fin=[W - 1] * n_utt, what=tag + " pool one short")
            assert got["n_fin"] == [W] * n_utt and got["done"] == [1] * n_utt
            # EOS at walk positions W - 1 and W of utterance 0: the token found there by an EOS-free pass
            c_ids, c_lp = (t.tolist() for t in ops.token_top_logprobs(rand[:rpu], 2 * W))
            ut = R.Utterance(W, MAXNEW, None)
            ut.cum = [np.float32(c) for c in ([0.0] * rpu if cum is None else cum[0].tolist())]
            order = ut.ordered([list(zip(c_ids[b], c_lp[b])) for b in range(rpu)])
            for p in (W - 1, W):
                select_case(rand, W, rpu, n_utt, order[p]["tok"], step, cum, what=tag + f" EOS at walk position {p}")
            # the budget's last step, and utterances that are done already: their state does not change
            got = select_case(rand, W, rpu, n_utt, None, MAXNEW - 1, cum, done=[u % 3 == 1 for u in range(n_utt)], what=tag + " last step, some done")
            assert got["done"] == [1 if u % 3 == 1 else 2 for u in range(n_utt)]
            seen_done |= set(got["done"])
    assert seen_done == {1, 2}


def test_beam_select_refusals():
    st = BeamState(2, 2, 4, DEV)
    lg = torch.zeros((2, 16), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="rows_per_utt"):
        ops.beam_select(lg, st, rows_per_utt=3)
    with pytest.raises(ValueError, match="step"):
        ops.beam_select(lg, st, rows_per_utt=1, step=4)
    with pytest.raises(ValueError, match="candidates"):
        ops.beam_select(lg[:, :3].contiguous(), st, rows_per_utt=1)
    with pytest.raises(Exception, match="GPU"):
        ops.beam_select(lg.cpu(), st, rows_per_utt=1)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def build(name, seed=11, **over):
    cfg = Config.from_name(name, **LORA, **over)
    assert cfg.head_size == HEAD_SIZES[name]
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.eval()
    return cfg, m


@pytest.fixture(scope="module", params=list(HEAD_SIZES))
def model(request):
    return build(request.param)


LENS = [1, 31, 32, 33, 47]


def prompts_for(cfg, seed=90):
    return [synth_prompts(1, n, cfg.padded_vocab_size, seed=seed + i)[0].to(DEV) for i, n in enumerate(LENS)]


def k_index(pos, hs):
    """element offsets [len(pos), hs] of positions `pos` in a (slot, group) block of the K cache (common.h kfrag_off)"""
    key, d = pos.view(-1, 1), torch.arange(hs).view(1, -1)
    t, lr, ks, lh, e = key >> 5, key & 31, d >> 4, (d >> 3) & 1, d & 7
    return (((t * (hs // 16) + ks) * 2 + lh) * 32 + lr) * 8 + e


def v_index(pos, hs):
    """the same for the V^T cache (common.h vfrag_off)"""
    key, d = pos.view(-1, 1), torch.arange(hs).view(1, -1)
    t, kk = key >> 5, key & 31
    s2, r = kk >> 4, kk & 15
    j, lh, dt, lr = ((r >> 3) << 2) | (r & 3), (r >> 2) & 1, d >> 5, d & 31
    return ((((t * (hs // 32) + dt) * 2 + s2) * 2 + lh) * 32 + lr) * 8 + j


def read_kv(eng, cfg, slot, n_pos):
    """[layer][K, V]: the first n_pos positions of a slot, [G, n_pos, hs] each, in position order"""
    G, hs = cfg.n_query_groups, cfg.head_size
    pos = torch.arange(n_pos)
    out = []
    for l in range(cfg.n_layer):
        pair = []
        for what, index in ((1, k_index), (2, v_index)):
            block = eng.read(what, l, (eng.max_batch, G, eng.s_max * hs))[slot]
            pair.append(block[:, index(pos, hs).to(DEV).reshape(-1)].view(G, n_pos, hs).clone())
        out.append(pair)
    return out


def reference_search(m, cfg, ps, W, new, eos):
    """-> (the reference utterances, kv[u][b]: the cache of utterance u's live beam b of the step BEFORE its last, positions below
    prompt + tokens fed).  Every step recomputes every hypothesis from scratch: the prompts prefilled together (mixed lengths: a
    prompt-phase call, as the fused path's prefill), then the hypotheses' tokens one position per call (single-token calls: decode
    steps).  A finished utterance keeps its rows busy with its last token; nothing is read from them."""
    n = len(ps)
    lens = [int(p.numel()) for p in ps]
    eng = m.engine(n * W, max(lens) + new, sum(lens) * W, exact=True)
    eng.set_rsqrt_emulation(0, whole_call=False)
    utts = [R.Utterance(W, new, eos) for _ in ps]
    kv = [None] * n
    for t in range(new):
        if all(u.done for u in utts):
            break
        if t == 0:
            _, last = eng.forward(torch.cat(ps), lens, [0] * n, want_all=False, want_last=True)
            rows = 1
        else:
            eng.forward(torch.cat([p for p in ps for _ in range(W)]), [l for l in lens for _ in range(W)], [0] * (n * W), want_all=False,
                        want_last=False)
            hist = [utts[u].hist[b][0] for u in range(n) for b in range(W)]
            for k in range(t):
                ids = torch.tensor([h[min(k, len(h) - 1)] for h in hist], dtype=torch.int64, device=DEV)
                pos = [lens[i // W] + min(k, len(hist[i]) - 1) for i in range(n * W)]
                _, last = eng.forward(ids, [1] * (n * W), pos, want_all=False, want_last=True)
            rows = W
        c_ids, c_lp = (x.tolist() for x in ops.token_top_logprobs(last, 2 * W))
        for u, ut in enumerate(utts):
            if ut.done:
                continue
            ut.step([list(zip(c_ids[u * rows + b], c_lp[u * rows + b])) for b in range(rows)])
            if ut.done and t > 0:
                kv[u] = [read_kv(eng, cfg, u * W + b, lens[u] + t) for b in range(W)]
    m.reset_cache()
    return utts, kv


def fused_search(m, cfg, ps, W, new, eos, pen=1.0):
    out, st = beam_search_batch(m, ps, new, num_beams=W, eos_id=eos, length_penalty=pen, return_state=True)
    h = st["host"]
    eng = m._engine
    kv = [[read_kv(eng, cfg, u * W + w, int(p.numel()) + h["n_steps"][u] - 1) for w in range(W)] if h["n_steps"][u] > 1 else None
          for u, p in enumerate(ps)]
    return out, h, kv


def check_against_reference(m, cfg, ps, W, new, eos, pen=1.0):
    out, h, kv = fused_search(m, cfg, ps, W, new, eos, pen)
    utts, ref_kv = reference_search(m, cfg, ps, W, new, eos)
    same_state(h, R.host_state(utts, W, new), f"{cfg.name} W={W} new={new} eos={eos}")
    for u, (p, ut) in enumerate(zip(ps, utts)):
        want = ut.ranked(pen)
        assert len(out[u]) == len(want) <= W
        for a, b in zip(out[u], want):
            assert torch.equal(a["tokens"], torch.cat([p.cpu(), torch.tensor(b["tokens"], dtype=torch.int64)]))
            assert torch.equal(a["token_logprobs"], torch.tensor([float(v) for v in b["token_logprobs"]], dtype=torch.float32))
            assert a["sum_logprob"] == b["sum_logprob"] and a["finished"] == b["finished"]
        # the final live beams' cache: slot u * W + w holds what its parent's slot held, at every position below its length
        if kv[u] is not None:
            for w, r in enumerate(ut.records[-1]):
                for l in range(cfg.n_layer):
                    for c in (0, 1):
                        assert torch.equal(kv[u][w][l][c], ref_kv[u][r["parent"]][l][c]), \
                            f"utterance {u} beam {w} (parent {r['parent']}) layer {l} {'KV'[c]}: the re-parented cache differs"
    return out, h, utts


@pytest.mark.parametrize("W", (2, 3, 4))
def test_beams_equal_the_recomputed_search(model, W):
    cfg, m = model
    ps = prompts_for(cfg)
    out, h, utts = check_against_reference(m, cfg, ps, W, 8, None)
    moved = sum(r["parent"] != w for ut in utts for rec in ut.records[1:] for w, r in enumerate(rec))
    print(f"{cfg.name} W={W}: {moved} of {sum(W * (ut.n_steps - 1) for ut in utts)} rows continued another beam")
    assert moved > 0, "no step re-parented anything: the case does not test the copy"
    assert all(d == 2 for d in h["done"]) and all(len(o) == W and not o[0]["finished"] for o in out)
    # an EOS that the best beam of the first utterance emits around step 4: pools fill at different steps
    eos = int(out[0][0]["tokens"][LENS[0] + 4])
    out, h, utts = check_against_reference(m, cfg, ps, W, 8, eos, pen=0.5)
    print(f"{cfg.name} W={W} eos={eos}: done={h['done']} steps={h['n_steps']} pool={h['n_fin']}")
    assert sum(h["n_fin"]) > 0


def test_36_tokens_cross_two_tile_ends(model):
    """from length 31 the generated keys cross the tile ends at 32 and 64: three tiles are re-parented"""
    cfg, m = model
    check_against_reference(m, cfg, prompts_for(cfg), 3, 36, None)


def test_one_beam_is_greedy_decoding(model):
    cfg, m = model
    ps = prompts_for(cfg)
    for eos in (None, "pick"):
        if eos == "pick":
            eos = int(want[0][LENS[0] + 4])
        want, lps = generate_batch(m, ps, 8, temperature=1.0, top_k=1, eos_id=eos, return_logprobs=True)
        want, lps = [o.clone() for o in want], [x.clone() for x in lps]
        got = beam_search_batch(m, ps, 8, num_beams=1, eos_id=eos)
        for p, o, lp, hyps in zip(ps, want, lps, got):
            assert len(hyps) == 1 and torch.equal(hyps[0]["tokens"], o.cpu())
            assert torch.equal(hyps[0]["token_logprobs"], lp.cpu())
            total = np.float32(0.0)
            for v in lp.cpu().numpy():
                total = np.float32(total + v)
            assert hyps[0]["sum_logprob"] == float(total)
            assert hyps[0]["finished"] == (lp.numel() == o.numel() - p.numel() + 1)      # one log-probability more: the EOS's


def test_best_score_against_score_batch(model):
    """recorded, not asserted: score_batch runs the prefill family, the beams the decode family"""
    cfg, m = model
    ps = prompts_for(cfg)
    out = beam_search_batch(m, ps, 8, num_beams=3)
    conts = [o[0]["tokens"][n:].to(DEV) for o, n in zip(out, LENS)]
    scores = score_batch(m, ps, conts)
    diff = max(abs(float(s.double().sum()) - o[0]["sum_logprob"]) for s, o in zip(scores, out))
    record_parity(f"beam.score_vs_generate.{cfg.name}", max_abs_diff=diff)


def test_calls_do_not_disturb_each_other(model):
    """beam search, greedy decoding, beam search, greedy decoding on one model: the graph keys and the scratch keep them apart"""
    cfg, m = model
    ps = prompts_for(cfg)
    flat = lambda out: [(h["tokens"], h["token_logprobs"], h["sum_logprob"], h["finished"]) for hyps in out for h in hyps]
    b0 = flat(beam_search_batch(m, ps, 8, num_beams=3))
    g0 = [o.clone() for o in generate_batch(m, ps, 8, temperature=0.2, top_k=1)]
    b1 = flat(beam_search_batch(m, ps, 8, num_beams=3))
    g1 = [o.clone() for o in generate_batch(m, ps, 8, temperature=0.2, top_k=1)]
    b2 = flat(beam_search_batch(m, ps, 8, num_beams=2))          # another W on the same engine
    b3 = flat(beam_search_batch(m, ps, 8, num_beams=3))
    assert all(torch.equal(x, y) for x, y in zip(g0, g1))
    for a, b in ((b0, b1), (b0, b3)):
        assert len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2:] == y[2:] for x, y in zip(a, b))
    assert len(b2) == 2 * len(ps)


# ---- the serving CLI ------------------------------------------------------------------------------------------------------------------
def test_inference_cli_num_beams(tmp_path):
    """`python -m dualhyp_amd.inference --num_beams 2 --logprobs` end to end (in this process): --decode_batch // W utterances at a time,
    the prediction is the best hypothesis, every record carries the ranked beams, --logprobs reports the best beam's sums"""
    import json
    import test_harness as harness
    from dualhyp_amd import inference
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    inference.main(["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
                    "DualHyp", "--dual_hypotheses", "--max_new_tokens", "6", "--decode_batch", "4", "--num_beams", "2", "--length_penalty", "0.5",
                    "--logprobs", "--predict_dir", str(tmp_path / "pred")])
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2
    for rec in js[:-2]:
        assert set(rec) == {"inference", "ground_truth", "beams", "sum_logprob", "avg_logprob"}
        assert 1 <= len(rec["beams"]) <= 2 and all(set(b) == {"text", "sum_logprob", "avg_logprob", "finished"} for b in rec["beams"])
        assert rec["inference"] == rec["beams"][0]["text"]
        # the record's sum is the double sum of at most 7 fp32 values of one sign, the beam's their sequential fp32 sum: 7 * 2^-24 apart
        assert abs(rec["sum_logprob"] - rec["beams"][0]["sum_logprob"]) <= 1e-6 * max(1.0, abs(rec["sum_logprob"]))
        keys = [b["sum_logprob"] / round(b["sum_logprob"] / b["avg_logprob"]) ** 0.5 for b in rec["beams"]]
        assert keys == sorted(keys, reverse=True)
