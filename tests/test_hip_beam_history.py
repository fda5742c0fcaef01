"""Beam search over device histories on the GPU (include/dualhyp_hip.h, "Beam histories"): dh_beam_select_bf16_hist,
dh_engine_set_beam_history, beam_search_batch(history="device").  Every comparison is torch.equal or list equality.

Kernel level: ops.beam_select stepped from the host over the crafted cases of tests/beam_history_cases.py, against
tests/beam_history_reference.py fed with ops.token_top_logprobs under a per-row mask (the utterance's mask minus the reference's
ban) — an op pinned by its own tests, so the state, the written plane and the candidates each have one right value.

End to end: the fused path against a Python search in the style of test_hip_beam.reference_search — every hypothesis recomputed from
scratch in a slot of its own — whose candidates are built from FULL logits rows on the host (the reference's own order, filter and
fallback) and scored by ops.token_logprobs."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_history_cases as CASES  # noqa: E402
import beam_history_reference as HR  # noqa: E402
import beam_reference as R  # noqa: E402
import test_hip_beam as TB  # noqa: E402
from dualhyp_amd import _lib, beam_search_batch, generate_batch, ops  # noqa: E402
from dualhyp_amd.beam import BeamState, backtrack  # noqa: E402
from dualhyp_amd.ngram import ban_positions  # noqa: E402
from dualhyp_amd.stop import compile_stop  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = TB.DEV


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
def dev_top(logits, k, allow):
    """beam_history_cases' `top` on the device: ops.token_top_logprobs under the per-row mask"""
    mask = None if allow is None else CASES.pack_bool(allow).to(DEV)
    ids, lp = ops.token_top_logprobs(logits.to(DEV), k, mask=mask)
    return ids.tolist(), lp.tolist()


@pytest.fixture(scope="module")
def covered():
    """The reference runs of the small cases under the device's own log-probabilities, before any of them is replayed on the kernels:
    together they hold every event the replay must not miss."""
    total = {k: 0 for k in CASES.EVENTS}
    for params in CASES.small_cases():
        c = CASES.build(*params, top=dev_top)
        run = CASES.Run(c["logits"], c["W"], c["vocab"], c["ngram"], c["allow"], stop_seqs=c["stop_seqs"], top=dev_top).finish()
        for k, v in run.events().items():
            total[k] += v
    print(f"events of the crafted cases: {total}")
    assert all(total[k] > 0 for k in CASES.EVENTS), total
    return total


def replay(params, eos=None, stop_ids=()):
    """one case on the kernels, step by step beside its reference run"""
    c = CASES.build(*params, top=dev_top)
    W, vocab, N = c["W"], c["vocab"], c["ngram"]
    run = CASES.Run(c["logits"], W, vocab, N, c["allow"], stop_ids=stop_ids, stop_seqs=c["stop_seqs"], eos=eos, top=dev_top)
    st = BeamState(CASES.N_UTT, W, run.max_new, DEV)
    hist = st.history_buffer()
    mask = None if c["allow"] is None else CASES.pack_bool(c["allow"]).to(DEV)
    stop = compile_stop(stop_ids, c["stop_seqs"], vocab, DEV) if (stop_ids or c["stop_seqs"]) else None
    tag = f"W={W} vocab={vocab} N={N} mask={mask is not None} seqs={c['stop_seqs']}"
    for t, lg in enumerate(c["logits"]):
        want = run.advance()
        rpu = want["rpu"]
        ids, lp = ops.beam_select(lg.to(DEV), st, rows_per_utt=rpu, eos_id=eos, step=t, mask=mask, stop=stop, history=hist, no_repeat_ngram=N)
        h = st.host()
        TB.same_state(h, R.host_state(run.utts, W, run.max_new), f"{tag} step {t}")
        if stop is not None:
            assert h["fin_tok"] == [u.fin_tok() for u in run.utts], f"{tag} step {t}: fin_tok"
        for u, ut in enumerate(run.utts):
            n = ut.n_steps
            for w in range(W if n else 0):      # the plane the utterance's last step wrote: every live beam's backtracked text
                assert h["history"][u][w][:n] == R.backtrack_tokens(ut.records, n - 1, w) == ut.history(w), f"{tag} step {t}: H({u}, {w})"
            if want["live"][u]:                 # the rows of an utterance that took the step: the reference's candidates, bit for bit
                rows = slice(u * rpu, (u + 1) * rpu)
                assert ids[rows].tolist() == want["ids"][rows] and lp[rows].tolist() == want["lps"][rows], f"{tag} step {t}: candidates of {u}"
        assert int(ids.min()) >= 0 and int(ids.max()) < vocab
    return run


@pytest.mark.parametrize("W", (1, 2, 3, 4))
@pytest.mark.parametrize("vocab", ("2W+1", 40, 32000))      # the fallback; the scalar loads (not a multiple of 8); the 16-byte loads
def test_select_hist_against_the_reference(covered, vocab, W):
    vocab = 2 * W + 1 if vocab == "2W+1" else vocab
    for N in (1, 2, 3):
        for masked in (False, True):
            for with_seqs in (False, True):
                replay((W, vocab, N, masked, with_seqs))


@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_select_hist_on_a_full_lds_row(covered, W):
    """131 072 ids: every word of the kernel's LDS row is in use"""
    for masked in (False, True):
        for with_seqs in (False, True):
            run = replay((W, 131072, 1, masked, with_seqs))
            assert run.events()["ban_kept"] > 0


def test_select_hist_without_a_ban_and_with_an_eos_and_a_stop_set(covered):
    """N = 0 (histories and sequences only: the candidates are the plain kernels'), and an EOS and a stop id beside the sequences"""
    for W in (2, 3):
        replay((W, 40, 0, False, True))
        replay((W, 40, 0, True, False))
        c = CASES.build(W, 40, 2, False, True, top=dev_top)
        dry = CASES.Run(c["logits"], W, 40, 2, None, top=dev_top).finish()
        eos, sid = dry.utts[1].records[3][0]["tok"], dry.utts[2].records[4][W - 1]["tok"]
        run = replay((W, 40, 2, False, True), eos=eos, stop_ids=[sid])
        reasons = [p["finish_reason"] for u in run.utts for p in u.pool]
        assert "eos" in reasons and "stop" in reasons, reasons


def test_select_hist_refusals():
    st = BeamState(2, 2, 4, DEV)
    lg = torch.zeros((2, 16), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="needs history"):
        ops.beam_select(lg, st, rows_per_utt=1, no_repeat_ngram=2)
    with pytest.raises(ValueError, match="0 .. 8"):
        ops.beam_select(lg, st, rows_per_utt=1, history=st.history_buffer(), no_repeat_ngram=9)
    with pytest.raises(ValueError, match="history must be"):
        ops.beam_select(lg, st, rows_per_utt=1, history=st.history_buffer()[:1])
    with pytest.raises(ValueError, match='histories live on the host.*history="device"'):
        ops.beam_select(lg, st, rows_per_utt=1, stop=compile_stop([1], [[3, 4]], 16, DEV))
    assert st.n_steps.tolist() == [0, 0] and not bool(st.history.any())


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(TB.HEAD_SIZES))
def model(request):
    return TB.build(request.param)


@pytest.fixture(scope="module")
def tiny():
    return TB.build("parity-tiny")


def three_prompts(cfg, seed=90):
    return TB.prompts_for(cfg, seed)[1:4]            # lengths 31, 32, 33: around a tile's end


def same_output(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert torch.equal(p["tokens"], q["tokens"]) and torch.equal(p["token_logprobs"], q["token_logprobs"])
            assert p["sum_logprob"] == q["sum_logprob"] and p["finished"] == q["finished"] and p["finish_reason"] == q["finish_reason"]


def histories_are_the_backtracked_records(h, W):
    for u, n in enumerate(h["n_steps"]):
        for w in range(W if n else 0):
            path = backtrack(h["beam_parent"][u], n - 1, w)
            assert h["history"][u][w][:n] == [h["beam_tok"][u][t][b] for t, b in enumerate(path)], f"H({u}, {w})"


def test_device_history_alone_changes_nothing(model):
    cfg, m = model
    ps = three_prompts(cfg)
    plain, sp = beam_search_batch(m, ps, 36, num_beams=3, return_state=True)
    got, sg = beam_search_batch(m, ps, 36, num_beams=3, history="device", return_state=True)
    TB.same_state(sg["host"], sp["host"], cfg.name)
    same_output(got, plain)
    assert "history" not in sp["host"] and sp["beam"].history is None
    assert tuple(sg["beam"].history.shape) == (2, 3, 3, 36)
    histories_are_the_backtracked_records(sg["host"], 3)
    assert sum(p != w for u in range(3) for t in range(1, 36) for w, p in enumerate(sg["host"]["beam_parent"][u][t])) > 0


def history_reference_search(m, ps, W, new, eos=None, ngram=0, stop_ids=(), stop_seqs=()):
    """test_hip_beam.reference_search over HR.HistUtterance: every step recomputes every hypothesis from scratch in a slot of its own;
    a row's candidates are built on the host from the FULL row (HR.candidates: order, ban, fallback) and scored by ops.token_logprobs"""
    n = len(ps)
    lens = [int(p.numel()) for p in ps]
    eng = m.engine(n * W, max(lens) + new, sum(lens) * W, exact=True)
    eng.set_rsqrt_emulation(0, whole_call=False)
    utts = [HR.HistUtterance(W, new, eos, stop_ids, stop_seqs, ngram) for _ in ps]
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
        vals = last.float().cpu().tolist()
        for u, ut in enumerate(utts):           # counts the rows with a ban that held, and those that fell back
            for b in range(0 if ut.done else rows):
                ut.row_ban(b, len(vals[0]))
        c_ids =[HR.candidates(vals[u * rows + b], utts[u].history(b) if not utts[u].done else [], W, ngram)
                 for u in range(n) for b in range(rows)]
        c_lp = torch.stack([ops.token_logprobs(last, torch.tensor([c[j] for c in c_ids], dtype=torch.int64, device=DEV))
                            for j in range(2 * W)], 1).tolist()
        for u, ut in enumerate(utts):
            if not ut.done:
                ut.step([list(zip(c_ids[u * rows + b], c_lp[u * rows + b])) for b in range(rows)])
    m.reset_cache()
    return utts


def check_against(out, h, utts, ps, W, new, pen=1.0):
    TB.same_state(h, R.host_state(utts, W, new))
    for u, (p, ut) in enumerate(zip(ps, utts)):
        if "fin_tok" in h:
            assert h["fin_tok"][u] == ut.fin_tok()
        want = ut.ranked(pen)
        assert len(out[u]) == len(want) <= W
        for a, b in zip(out[u], want):
            assert torch.equal(a["tokens"], torch.cat([p.cpu(), torch.tensor(b["tokens"], dtype=torch.int64)]))
            assert torch.equal(a["token_logprobs"], torch.tensor([float(v) for v in b["token_logprobs"]], dtype=torch.float32))
            assert a["sum_logprob"] == b["sum_logprob"] and a["finished"] == b["finished"] and a["finish_reason"] == b["finish_reason"]


def generated(out, ps):
    return [[h["tokens"][p.numel():].tolist() for h in hyps] for hyps, p in zip(out, ps)]


@pytest.mark.parametrize("N", (1, 2))
def test_the_ban_against_the_recomputed_search(tiny, N):
    cfg, m = tiny
    W, NEW = 3, 10
    # the first prompts whose banned search differs from the free one (N = 1 bans from step 1 on; N = 2 needs a repeated pair)
    for seed in range(90, 96):
        ps = three_prompts(cfg, seed)
        free = beam_search_batch(m, ps, NEW, num_beams=W)
        out, st = beam_search_batch(m, ps, NEW, num_beams=W, history="device", no_repeat_ngram=N, return_state=True)
        if generated(out, ps) != generated(free, ps):
            break
    print(f"N={N}: prompts of seed {seed}")
    assert generated(out, ps) != generated(free, ps), "no prompt set was changed by the ban"
    bans = [ban_positions(g[0], N) for g in generated(out, ps)]
    assert any(bans), "no pick of a best hypothesis had a non-empty ban set"
    for g in generated(out, ps):            # no hypothesis repeats an n-gram (a fallback row would need fewer than 2 W = 6 free ids of 256)
        for toks in g:
            grams = [tuple(toks[i:i + N]) for i in range(len(toks) - N + 1)]
            assert len(grams) == len(set(grams))
    utts = history_reference_search(m, ps, W, NEW, ngram=N)
    check_against(out, st["host"], utts, ps, W, NEW)
    assert sum(u.events["ban_kept"] for u in utts) > 0
    histories_are_the_backtracked_records(st["host"], W)


def test_one_beam_under_the_ban_is_greedy_decoding(tiny):
    cfg, m = tiny
    ps = three_prompts(cfg)
    want, lps = generate_batch(m, ps, 12, temperature=1.0, top_k=1, no_repeat_ngram=2, return_logprobs=True)
    want, lps = [o.clone() for o in want], [x.clone() for x in lps]
    got = beam_search_batch(m, ps, 12, num_beams=1, history="device", no_repeat_ngram=2)
    for o, lp, hyps in zip(want, lps, got):
        assert len(hyps) == 1 and torch.equal(hyps[0]["tokens"], o.cpu()) and torch.equal(hyps[0]["token_logprobs"], lp.cpu())


@pytest.mark.parametrize("with_eos", (False, True))
def test_a_stop_sequence_against_the_recomputed_search(tiny, with_eos):
    cfg, m = tiny
    W, NEW = 3, 8
    ps = three_prompts(cfg)
    free = beam_search_batch(m, ps, NEW, num_beams=W)
    best = generated(free, ps)[0][0]
    seq = [best[2], best[3]]                  # what the best beam of the first utterance emits at steps 2 and 3
    eos = seq[1] if with_eos else None        # an EOS that also occurs: where the sequence completes, the EOS wins
    out, st = beam_search_batch(m, ps, NEW, num_beams=W, eos_id=eos, stop=[seq], history="device", length_penalty=0.5, return_state=True)
    utts = history_reference_search(m, ps, W, NEW, eos=eos, stop_seqs=[seq])
    check_against(out, st["host"], utts, ps, W, NEW, pen=0.5)
    histories_are_the_backtracked_records(st["host"], W)
    ended = [h for hyps in out for h in hyps if h["finished"]]
    assert ended, "nothing ended"
    if with_eos:
        assert sum(u.events["eos_and_seq"] for u in utts) > 0, "no candidate was the EOS and completed the sequence"
        assert all(h["finish_reason"] == "eos" for h in ended)           # every completion of the sequence is on the EOS
    else:
        assert all(h["finish_reason"] == "stop" and h["tokens"][-2:].tolist() == seq for h in ended)
        assert any(h["finish_reason"] == "stop" for h in out[0])
        # an utterance whose text never comes near the sequence is untouched
        for u in range(len(ps)):
            if not any(seq[1] in g for g in generated(free, ps)[u]) and not utts[u].pool:
                assert generated(out, ps)[u] == generated(free, ps)[u]
        assert any(not ut.pool for ut in utts), "every utterance met the sequence: none shows an untouched text"


def test_keys_and_hygiene(tiny):
    """N = 2, N = 3, histories alone, the plain call — on one engine, each equal to a fresh engine's; the engine ends unset"""
    cfg, m = tiny
    ps = three_prompts(cfg)
    kws = (dict(history="device", no_repeat_ngram=2), dict(history="device", no_repeat_ngram=3), dict(history="device"), dict())
    got = [beam_search_batch(m, ps, 10, num_beams=3, **kw) for kw in kws]
    assert getattr(m._engine, "_beam_history", None) is None and getattr(m._engine, "_stop", None) is None
    for kw, g in zip(kws, got):
        _, fresh = TB.build("parity-tiny")
        same_output(g, beam_search_batch(fresh, ps, 10, num_beams=3, **kw))
    same_output(got[2], got[3])
    # the engine itself keeps refusing what the histories do not lift
    eng = m._engine
    state = BeamState(len(ps), 3, 10, torch.device(DEV))
    plen = torch.tensor([int(p.numel()) for p in ps], dtype=torch.int32, device=DEV)
    eng.set_beam_history(state.history_buffer(), 2)
    try:
        eng.set_penalties(1.2, 0.0, 0.0, start=plen)
        with pytest.raises(_lib.DualHypHipError, match="penalties are set.*rank"):
            eng.decode_beam(state, plen, 1, None, first_step=1)
        eng.set_penalties()
        eng.set_no_repeat_ngram(2, plen)
        with pytest.raises(_lib.DualHypHipError, match="no_repeat_ngram=2 is set"):
            eng.decode_beam(state, plen, 1, None, first_step=1)
        eng.set_no_repeat_ngram(0)
        with pytest.raises(_lib.DualHypHipError, match="0 .. 8"):
            eng.set_beam_history(state.history_buffer(), 9)
    finally:
        eng.set_penalties()
        eng.set_no_repeat_ngram(0)
        eng.set_beam_history(None)
    assert not bool(state.done.any()) and not bool(state.n_steps.any())
    m._cache_len = []


def test_refusals_under_device_histories(tiny):
    cfg, m = tiny
    ps = three_prompts(cfg)[:2]
    with pytest.raises(ValueError, match="0 .. 8"):
        beam_search_batch(m, ps, 4, num_beams=2, history="device", no_repeat_ngram=9)
    with pytest.raises(ValueError, match="at most 8 tokens"):
        beam_search_batch(m, ps, 4, num_beams=2, history="device", stop=[list(range(9))])
    with pytest.raises(ValueError, match="a bias of 1 entries does not go with beam search"):
        beam_search_batch(m, ps, 4, num_beams=2, history="device", bias=[([3, 4], 2.0)])
    with pytest.raises(ValueError, match="banana"):
        beam_search_batch(m, ps, 4, num_beams=2, history="banana")
    m.fp8 = True
    try:
        with pytest.raises(ValueError, match="fp8"):
            beam_search_batch(m, ps, 4, num_beams=2, history="device", no_repeat_ngram=2)
    finally:
        del m.fp8
    with pytest.raises(ValueError, match="histories live on the host"):
        beam_search_batch(m, ps, 4, num_beams=2, no_repeat_ngram=2)


def test_inference_cli_beam_history(tmp_path):
    """`python -m dualhyp_amd.inference --num_beams 2 --beam_history device --no_repeat_ngram 2` end to end (in this process)"""
    import json
    import test_harness as harness
    from dualhyp_amd import inference
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    inference.main(["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
                    "DualHyp", "--dual_hypotheses", "--max_new_tokens", "8", "--decode_batch", "4", "--num_beams", "2", "--beam_history",
                    "device", "--no_repeat_ngram", "2", "--predict_dir", str(tmp_path / "pred")])
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2
    for rec in js[:-2]:
        assert set(rec) == {"inference", "ground_truth", "beams", "no_repeat_ngram", "ngram_bans"}
        assert rec["no_repeat_ngram"] == 2 and isinstance(rec["ngram_bans"], int) and 0 <= rec["ngram_bans"] <= 8
        assert 1 <= len(rec["beams"]) <= 2 and rec["inference"] == rec["beams"][0]["text"]
