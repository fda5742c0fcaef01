"""Beam search under a stop set, end to end (beam_search_batch(stop=...); include/dualhyp_hip.h, "Stop conditions").  Exact.

With no EOS, a stop set {s} is the existing path with eos_id = s in everything but two things: s stays in the hypothesis' tokens, and
its finish_reason is "stop".  With an EOS and a two-id set the fused path is compared with tests/stop_reference.py, the host model,
every live hypothesis recomputed from scratch as test_hip_constrain_beam.py recomputes it."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_reference as R  # noqa: E402
import stop_reference as SR  # noqa: E402
import test_hip_beam as TB  # noqa: E402
from dualhyp_amd import beam_search_batch, ops  # noqa: E402
from dualhyp_amd.stop import compile_stop  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = TB.DEV
NEW = 8


@pytest.fixture(scope="module")
def model():
    return TB.build("parity-tiny")


@pytest.mark.parametrize("W", (2, 3))
def test_a_one_id_stop_set_is_the_eos_path(model, W):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    free = beam_search_batch(m, ps, NEW, num_beams=W)
    s = int(free[0][0]["tokens"][TB.LENS[0] + 3])         # what the best beam of the first utterance emits at step 3
    want, st_w = beam_search_batch(m, ps, NEW, num_beams=W, eos_id=s, length_penalty=0.5, return_state=True)
    got, st_g = beam_search_batch(m, ps, NEW, num_beams=W, stop=[s], length_penalty=0.5, return_state=True)
    TB.same_state(st_g["host"], st_w["host"], f"W={W}")   # every token, parent, score and pool entry
    assert sum(st_g["host"]["n_fin"]) > 0
    for u in range(len(ps)):
        assert len(got[u]) == len(want[u])
        for a, b in zip(got[u], want[u]):                 # the same rank order
            assert torch.equal(a["token_logprobs"], b["token_logprobs"]) and a["sum_logprob"] == b["sum_logprob"]
            assert a["finished"] == b["finished"]
            if b["finished"]:
                assert a["finish_reason"] == "stop" and b["finish_reason"] == "eos"
                assert torch.equal(a["tokens"], torch.cat([b["tokens"], torch.tensor([s])]))        # s stays in the tokens
                assert a["tokens"].numel() - ps[u].numel() == a["token_logprobs"].numel()             # and counts in n
            else:
                assert a["finish_reason"] == b["finish_reason"] == "length" and torch.equal(a["tokens"], b["tokens"])
        k = st_g["host"]["n_fin"][u]
        assert st_g["host"]["fin_tok"][u][:k] == [s] * k and st_g["host"]["fin_tok"][u][k:] == [-1] * (W - k)
    # the list form, a compiled specification and the plain call behind them
    again = beam_search_batch(m, ps, NEW, num_beams=W, stop=compile_stop([s], [], cfg.padded_vocab_size, DEV), length_penalty=0.5)
    assert all(torch.equal(a["tokens"], b["tokens"]) for x, y in zip(got, again) for a, b in zip(x, y))
    plain = beam_search_batch(m, ps, NEW, num_beams=W)
    assert all(torch.equal(a["tokens"], b["tokens"]) and a["finish_reason"] == "length" for x, y in zip(free, plain) for a, b in zip(x, y))
    assert getattr(m._engine, "_stop", None) is None


def stop_reference_search(m, ps, W, new, eos, stop_ids):
    """test_hip_constrain_beam.masked_reference_search without a mask, over SR.StopUtterance"""
    n = len(ps)
    lens = [int(p.numel()) for p in ps]
    eng = m.engine(n * W, max(lens) + new, sum(lens) * W, exact=True)
    eng.set_rsqrt_emulation(0, whole_call=False)
    utts = [SR.StopUtterance(W, new, eos, stop_ids) for _ in ps]
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
            if not ut.done:
                ut.step([list(zip(c_ids[u * rows + b], c_lp[u * rows + b])) for b in range(rows)])
    m.reset_cache()
    return utts


@pytest.mark.parametrize("W", (2, 3))
def test_eos_and_a_two_id_set_against_the_host_model(model, W):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    free = beam_search_batch(m, ps, NEW, num_beams=W)
    eos = int(free[0][0]["tokens"][TB.LENS[0] + 3])
    others = [int(t) for hyps in free[1:] for h in hyps for t in h["tokens"][-NEW + 1:-NEW + 5].tolist() if int(t) != eos]
    s1 = others[0]
    s2 = next(t for t in others if t != s1)
    out, st = beam_search_batch(m, ps, NEW, num_beams=W, eos_id=eos, stop=[s1, s2, eos], length_penalty=0.5, return_state=True)
    h = st["host"]
    utts = stop_reference_search(m, ps, W, NEW, eos, [s1, s2, eos])
    TB.same_state(h, R.host_state(utts, W, NEW), f"W={W}")
    reasons = set()
    for u, (p, ut) in enumerate(zip(ps, utts)):
        assert h["fin_tok"][u] == ut.fin_tok()
        want = ut.ranked(0.5)
        assert len(out[u]) == len(want) <= W
        for a, b in zip(out[u], want):
            assert torch.equal(a["tokens"], torch.cat([p.cpu(), torch.tensor(b["tokens"], dtype=torch.int64)]))
            assert torch.equal(a["token_logprobs"], torch.tensor([float(v) for v in b["token_logprobs"]], dtype=torch.float32))
            assert a["sum_logprob"] == b["sum_logprob"] and a["finished"] == b["finished"] and a["finish_reason"] == b["finish_reason"]
            reasons.add(a["finish_reason"])
    assert "stop" in reasons, "the inputs let no hypothesis end on a stop id"
    assert sum(h["n_fin"]) > 0


def test_stop_sequences_are_refused(model):
    cfg, m = model
    ps = TB.prompts_for(cfg)[:2]
    with pytest.raises(ValueError, match="histories live on the host"):
        beam_search_batch(m, ps, 4, num_beams=2, stop=[[3, 4]])
    from dualhyp_amd.beam import BeamState
    st = BeamState(2, 2, 4, DEV)
    lg = torch.zeros((2, cfg.padded_vocab_size), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="histories live on the host"):
        ops.beam_select(lg, st, rows_per_utt=1, stop=compile_stop([1], [[3, 4]], cfg.padded_vocab_size, DEV))
    assert st.n_steps.tolist() == [0, 0]
