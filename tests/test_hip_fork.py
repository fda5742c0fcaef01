"""dh_engine_fork_slots on the GPU, at byte level: every utterance's prompt tiles go from slot u * N into the N - 1 slots behind, by
one launch that reads the lengths on the device, and nothing else in the cache changes.  Every check is exact (torch.equal on whole
cache images, test_hip_prefix.py's `caches` reading; an fp8 cache is read as stored, bytes and exponents).  Lengths 1, 31, 32, 33, 64
and 100: one token, either side of a tile edge, an exact multiple, and ragged."""
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import quantize_model_fp8
from dualhyp_amd._lib import DualHypHipError
from dualhyp_amd.synth import synth_prompts

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_hip_prefix import DEV, build, caches  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = [1, 31, 32, 33, 64, 100]
S = 128
FILL = 100          # every slot holds a sequence of its own, 4 tiles long, before the sources are prefilled


def images(eng, cfg, B, fp8):
    """The cache as a list of (name, [slots, groups, tiles, bytes or elements per tile]) images, every layer"""
    out = []
    if fp8:
        for l in range(cfg.n_layer):
            for what, name in ((9, "K bytes"), (10, "V^T bytes"), (11, "K exponents"), (12, "V exponents")):
                t = eng.read_kv8(what, l)
                out.append((f"layer {l} {name}", t.reshape(t.size(0), t.size(1), S // 32, -1).clone()))
    else:
        for l, (k, v) in enumerate(caches(eng, cfg, B, S)):
            for t, name in ((k, "K"), (v, "V^T")):
                out.append((f"layer {l} {name}", t.reshape(B, t.size(1), S // 32, -1)))
    return out


def forked(before, lens, N):
    """What the fork must leave: the source's tiles 0 .. ceil(len / 32) - 1 in the N - 1 slots behind it, everything else as it was"""
    want = before.clone()
    for u, n in enumerate(lens):
        t = -(-n // 32)
        want[u * N + 1:(u + 1) * N, :, :t] = before[u * N, :, :t]
    return want


@pytest.mark.parametrize("N", [2, 8])
@pytest.mark.parametrize("name,fp8", [("parity-tiny", False), ("parity-hs96", False), ("parity-hs128", False), ("parity-hs128", True)])
def test_fork_slots_kernel(name, fp8, N):
    cfg, m = build(name, n_layer=3)             # a first, a middle and the last layer
    if fp8:
        quantize_model_fp8(m, kv_cache="fp8")
    V = cfg.padded_vocab_size
    n_utt = len(LENS)
    B = n_utt * N + 2                           # two slots behind the last utterance's: never touched
    m.refresh_engine()
    eng = m.engine(B, S, B * FILL, exact=True)
    assert (eng.max_batch, eng.s_max, eng.kv_cache_dtype) == (B, S, "fp8" if fp8 else "bf16")
    fill = [synth_prompts(1, FILL, V, seed=500 + i)[0].to(DEV) for i in range(B)]
    eng.forward(torch.cat(fill), [FILL] * B, [0] * B, want_all=False, want_last=True)
    fresh = [synth_prompts(1, n, V, seed=900 + u)[0].to(DEV) for u, n in enumerate(LENS)]
    eng.forward_slots(torch.cat(fresh), LENS, [u * N for u in range(n_utt)], prompt_phase=True)
    before = images(eng, cfg, B, fp8)
    plen = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    eng.fork_slots(plen, N, max(LENS))
    after = images(eng, cfg, B, fp8)
    exp_tiles = [0, 0]      # exponent tiles that differed from their source before the fork, and all of them
    for (what, b), (_, a) in zip(before, after):
        want = forked(b, LENS, N)
        # the check proves something: every destination held other values than its source in every tile that is copied (a tile of
        # exponents is 32 small integers per group, which two sequences may share: those are counted over the whole cache)
        for u, n in enumerate(LENS):
            differs = [not torch.equal(b[u * N + 1, :, t], b[u * N, :, t]) for t in range(-(-n // 32))]
            if "exponents" in what:
                exp_tiles[0] += sum(differs)
                exp_tiles[1] += len(differs)
            else:
                assert all(differs), f"{what}: utterance {u} equals its source before the fork: {differs}"
        bad = (a != want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{what}: slots {bad} are not what the fork leaves (sources, tiles behind a prompt and slots {B - 2}, {B - 1} unchanged)"
        assert torch.equal(a[::N][:n_utt], b[::N][:n_utt]), f"{what}: a source slot was written"
    if fp8:
        print(f"exponent tiles that differed from their source before the fork: {exp_tiles[0]} of {exp_tiles[1]}")
        assert 2 * exp_tiles[0] > exp_tiles[1], "the exponent images would prove little"

    # a second call with one utterance, a new prompt in its source: nothing but that utterance's N - 1 slots changes
    again = synth_prompts(1, 50, V, seed=77)[0].to(DEV)
    eng.forward_slots(again, [50], [0], prompt_phase=True)
    before = images(eng, cfg, B, fp8)
    eng.fork_slots(torch.tensor([50], dtype=torch.int32, device=DEV), N, 50)
    for (what, b), (_, a) in zip(before, images(eng, cfg, B, fp8)):
        assert "exponents" in what or not torch.equal(b[1, :, :2], b[0, :, :2])
        assert torch.equal(a, forked(b, [50], N)), f"{what}: the one-utterance fork wrote outside slots 1 .. {N - 1}, tiles 0 and 1"

    # max_len sizes the grid only: with lengths shorter than it the same tiles move; a length of 0 moves nothing
    short = torch.tensor([33, 0], dtype=torch.int32, device=DEV)
    eng.forward_slots(fresh[5], [100], [0], prompt_phase=True)
    before = images(eng, cfg, B, fp8)
    eng.fork_slots(short, N, S)
    for (what, b), (_, a) in zip(before, images(eng, cfg, B, fp8)):
        assert torch.equal(a, forked(b, [33], N)), f"{what}: lengths [33, 0] under max_len {S}"

    # refused before anything is launched, each with a reason
    for bad, why in (((plen, 1, 100), "n_copies=1"), ((plen, 9, 100), "n_copies=9"), ((plen, N, 0), "max_len=0"),
                     ((plen, N, S + 1), "exceeds s_max"), ((torch.full((B // N + 1,), 5, dtype=torch.int32, device=DEV), N, 100), "exceed the engine's")):
        with pytest.raises(DualHypHipError, match=why):
            eng.fork_slots(*bad)
    with pytest.raises(TypeError):
        eng.fork_slots(plen.to(torch.int64), N, 100)
    for (what, b), (_, a) in zip(before, images(eng, cfg, B, fp8)):
        assert torch.equal(a, forked(b, [33], N)), f"{what}: a refused call wrote"
