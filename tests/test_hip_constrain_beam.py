"""Beam search under a token mask, end to end (beam_search_batch(token_mask=...); include/dualhyp_hip.h, "Token masks").  Exact.

The fused path against test_hip_beam.py's plain Python beam search — every live hypothesis recomputed from scratch in a slot of its
own, the selection by tests/beam_reference.py — with one change: a row's candidates are the first 2 W ids its utterance's mask allows
(ops.token_top_logprobs(mask=...), pinned by test_hip_constrain.py)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_reference as R  # noqa: E402
import constrain_reference as CR  # noqa: E402
import test_hip_beam as TB  # noqa: E402
from dualhyp_amd import beam_search_batch, constrain, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = TB.DEV
NEW = 8


@pytest.fixture(scope="module")
def model():
    return TB.build("parity-tiny")


def masked_reference_search(m, ps, W, new, eos, mask):
    """TB.reference_search with the candidates taken under the utterance's mask row"""
    n = len(ps)
    lens = [int(p.numel()) for p in ps]
    eng = m.engine(n * W, max(lens) + new, sum(lens) * W, exact=True)
    eng.set_rsqrt_emulation(0, whole_call=False)
    utts = [R.Utterance(W, new, eos) for _ in ps]
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
        c_ids, c_lp = (x.tolist() for x in ops.token_top_logprobs(last, 2 * W, mask=mask.repeat_interleave(rows, dim=0).contiguous()))
        for u, ut in enumerate(utts):
            if not ut.done:
                ut.step([list(zip(c_ids[u * rows + b], c_lp[u * rows + b])) for b in range(rows)])
    m.reset_cache()
    return utts


def flat(out):
    return [(h["tokens"], h["token_logprobs"], h["sum_logprob"], h["finished"]) for hyps in out for h in hyps]


def same_hyps(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2:] == y[2:] for x, y in zip(a, b))


@pytest.mark.parametrize("eos_in_mask", (True, False))
@pytest.mark.parametrize("W", (2, 4))
def test_masked_beams_equal_the_recomputed_search(model, W, eos_in_mask):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    V, n = cfg.padded_vocab_size, len(ps)
    half = CR.unpack_bits(CR.random_half_masks(n, V, seed=31 + W), V)
    # the EOS: what the best masked beam of the first utterance emits around step 3 — allowed everywhere, or nowhere
    first = beam_search_batch(m, ps, NEW, num_beams=W, token_mask=CR.pack_bits(half).to(DEV))
    eos = int(first[0][0]["tokens"][TB.LENS[0] + 3])
    half[:, eos] = eos_in_mask
    mask = CR.pack_bits(half).to(DEV)
    out, st = beam_search_batch(m, ps, NEW, num_beams=W, eos_id=eos, length_penalty=0.5, token_mask=mask, return_state=True)
    h = st["host"]
    utts = masked_reference_search(m, ps, W, NEW, eos, mask)
    TB.same_state(h, R.host_state(utts, W, NEW), f"W={W} eos {'in' if eos_in_mask else 'outside'} the mask")
    for u, (p, ut) in enumerate(zip(ps, utts)):
        want = ut.ranked(0.5)
        assert len(out[u]) == len(want) <= W
        for a, b in zip(out[u], want):
            assert torch.equal(a["tokens"], torch.cat([p.cpu(), torch.tensor(b["tokens"], dtype=torch.int64)]))
            assert torch.equal(a["token_logprobs"], torch.tensor([float(v) for v in b["token_logprobs"]], dtype=torch.float32))
            assert a["sum_logprob"] == b["sum_logprob"] and a["finished"] == b["finished"]
            assert all(half[u][i] for i in a["tokens"][p.numel():].tolist()), f"utterance {u}: a hypothesis holds a disallowed id"
    if eos_in_mask:
        assert sum(h["n_fin"]) > 0
    else:
        assert sum(h["n_fin"]) == 0 and not any(hyp["finished"] for hyps in out for hyp in hyps)
    assert getattr(m._engine, "_token_mask", None) is None


@pytest.mark.parametrize("W", (2, 4))
def test_all_ones_mask_is_the_unmasked_search(model, W):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    V = cfg.padded_vocab_size
    free = flat(beam_search_batch(m, ps, NEW, num_beams=W))
    eos = int(free[0][0][TB.LENS[0] + 3])
    for e in (None, eos):
        want = flat(beam_search_batch(m, ps, NEW, num_beams=W, eos_id=e))
        got = flat(beam_search_batch(m, ps, NEW, num_beams=W, eos_id=e, token_mask=constrain.all_ones(len(ps), V, DEV)))
        assert same_hyps(want, got), f"W={W} eos={e}"
        assert same_hyps(want, flat(beam_search_batch(m, ps, NEW, num_beams=W, eos_id=e))), "the plain call after a masked one"


def test_refusals_before_any_launch(model):
    cfg, m = model
    ps = TB.prompts_for(cfg)[:2]
    V = cfg.padded_vocab_size
    with pytest.raises(ValueError, match="row 1 allows 7 ids below vocab=256, at least 8"):
        beam_search_batch(m, ps, 4, num_beams=4, token_mask=[list(range(8)), list(range(7))])
    with pytest.raises(ValueError, match="lives on cpu"):
        beam_search_batch(m, ps, 4, num_beams=2, token_mask=constrain.all_ones(2, V))
    with pytest.raises(ValueError, match=r"\[2, 8\]"):
        beam_search_batch(m, ps, 4, num_beams=2, token_mask=constrain.all_ones(3, V, DEV))
