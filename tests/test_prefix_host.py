"""Host side of prefix sharing (generate_batch / generate_stream, share_prefix): the shared length, the order of engine calls of
generate_stream against a scripted engine on the CPU, the two refusals, and the C-ABI entry (header, exports, ctypes table)."""
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd.schedule import shared_prefix_len

sys.path.insert(0, str(Path(__file__).resolve().parent))
from scripted_engine import ScriptedModel  # noqa: E402

REPO = Path(__file__).resolve().parent.parent
G = importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function


def ids(*parts):
    return torch.tensor([t for p in parts for t in p], dtype=torch.int64)


@pytest.mark.parametrize("as_lists", [False, True])
def test_shared_prefix_len(as_lists):
    conv = (lambda ps: [p.tolist() for p in ps]) if as_lists else (lambda ps: ps)
    common = list(range(3, 103))
    # identical for 100 tokens, then different
    assert shared_prefix_len(conv([ids(common, [200, 5, 6]), ids(common, [201]), ids(common, [202, 9])])) == 96
    # a common prefix of 31 tokens
    assert shared_prefix_len(conv([ids(common[:31], [200] * 40), ids(common[:31], [201] * 50)])) == 0
    # one prompt entirely a prefix of the others, 64 long: capped at 63, rounded down
    assert shared_prefix_len(conv([ids(common[:64], [200, 1]), ids(common[:64]), ids(common[:64], [201])])) == 32
    # a single prompt of 65 tokens
    assert shared_prefix_len(conv([ids(common[:65])])) == 64
    # no common token
    assert shared_prefix_len(conv([ids([5] * 70), ids([6] * 70)])) == 0
    # the difference that ends the prefix may sit in any prompt of the call, not in the second one only
    assert shared_prefix_len(conv([ids(common), ids(common), ids(common[:70], [250] * 30)])) == 64
    assert shared_prefix_len(conv([ids(common[:33]), ids(common[:33])])) == 32 and shared_prefix_len(conv([ids(common[:32])] * 2)) == 0


# ---- generate_stream against a scripted engine -------------------------------------------------------------------------------
def stream(prompts, n_gen, share, monkeypatch, **kw):
    model = ScriptedModel(n_gen)
    eng = model.eng
    eng.lens = [p.numel() for p in prompts]

    def sample_rows(last, tokens, length, done, limit, seqs, max_new, **_):
        for u in seqs.tolist():
            eng._pick(u, tokens, length, done, 1)
    monkeypatch.setattr(G.ops, "sample_rows", sample_rows)
    out = G.generate_stream(model, prompts, 12, top_k=1, eos_id=99, share_prefix=share, **kw)
    return model, out


def corpus(n=20, shared=80):
    g = torch.Generator().manual_seed(3)
    head = torch.randint(3, 200, (shared,), generator=g)
    ps = [torch.cat([head, torch.tensor([200 + i]), torch.randint(3, 200, (i % 7,), generator=g)]) for i in range(n)]
    n_gen = [1 + (5 * i) % 12 for i in range(n)]          # 1 = ends on the pick of its prefill, 12 = runs to its budget
    return ps, n_gen


def test_generate_stream_forwards_the_prefix_once_and_prefills_the_rest(monkeypatch):
    ps, n_gen = corpus()
    lens = [p.numel() for p in ps]
    kw = dict(max_rows=4, prefill_batch=3, check_every=4)
    plain, out_plain = stream(ps, n_gen, False, monkeypatch, **kw)
    shared, out_shared = stream(ps, n_gen, True, monkeypatch, **kw)
    P = 64
    calls = shared.eng.calls
    # exactly one prefix forward (no logits) and one copy, in front of everything else
    assert calls[0] == ("forward", ps[0][:P].tolist(), [P], [0], False, False, 0)
    assert calls[1] == ("copy_prefix", 0, [1, 2, 3], P)
    rest = calls[2:]
    assert not any(c[0] in ("forward", "copy_prefix") for c in rest)
    assert not any(c[0] in ("forward", "copy_prefix") for c in plain.eng.calls)
    # every slot a prefill or a decode row names later holds the prefix; the spare slot (4) is not among the copy's destinations
    used = {s for c in rest if c[0] == "forward_slots" for s in c[3]}
    assert used <= {0, 1, 2, 3} and len(used) > 1
    # every prefill: the tokens behind the prefix, at position P
    pre_s = [c for c in rest if c[0] == "forward_slots"]
    pre_p = [c for c in plain.eng.calls if c[0] == "forward_slots"]
    assert len(pre_s) == len(pre_p) > 5, "the corpus must refill slots several times"
    served = 0
    for cs, cp in zip(pre_s, pre_p):
        n = len(cs[2])
        seqs = list(range(served, served + n))
        served += n
        assert cs[5] == P and cp[5] == 0
        assert cs[2] == [lens[u] - P for u in seqs] and cp[2] == [lens[u] for u in seqs]
        assert cs[1] == [t for u in seqs for t in ps[u][P:].tolist()]
        assert cs[3] == cp[3] and cs[4] is True and cp[4] is True          # the same slots, prompt phase in both
    assert served == len(ps)
    # the refill, row and slot decisions are those of the unshared run
    strip = lambda cc: [(c[0],) + tuple(c[3:5]) if c[0] == "forward_slots" else c for c in cc if c[0] in ("forward_slots", "decode_rows")]
    assert strip(rest) == strip(plain.eng.calls)
    assert all(torch.equal(a, b) for a, b in zip(out_plain, out_shared))
    # workspace: the larger of the prefix and the largest pack of remainders
    assert plain.engine_args == (5, max(lens) + 11, sum(sorted(lens)[-3:]))
    assert shared.engine_args == (5, max(lens) + 11, max(P, sum(sorted(n - P for n in lens)[-3:])))


def test_refusals(monkeypatch):
    ps, n_gen = corpus(5)
    model = ScriptedModel(n_gen)
    model.cpu_rsqrt_vec_width = 32
    model.eng.lens = [p.numel() for p in ps]
    monkeypatch.setattr(G.ops, "sample_rows", lambda last, tokens, length, done, limit, seqs, max_new, **_:
                        [model.eng._pick(u, tokens, length, done, 1) for u in seqs.tolist()])
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.generate_stream(model, ps, 12, top_k=1, share_prefix=True)
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.generate_batch(model, ps, 12, top_k=1, share_prefix=True)
    assert not model.eng.calls
    G.generate_stream(model, ps, 12, top_k=1, eos_id=99, share_prefix="auto", max_rows=2, prefill_batch=2)
    assert model.eng.calls and not any(c[0] in ("forward", "copy_prefix") for c in model.eng.calls)
    assert all(c[5] == 0 for c in model.eng.calls if c[0] == "forward_slots")
    with pytest.raises(ValueError, match="share_prefix"):
        G.generate_stream(model, ps, 12, top_k=1, share_prefix="on")
    # the RelPrompt decoder is refused the same way, whatever its other settings
    from dualhyp_amd.relprompt import GPT as RelGPT
    rel = object.__new__(RelGPT)
    object.__setattr__(rel, "cpu_rsqrt_vec_width", 0)
    with pytest.raises(ValueError, match="RelPrompt"):
        G._shared_prefix(rel, ps, True, "cpu")
    assert G._shared_prefix(rel, ps, "auto", "cpu") == 0
    model.cpu_rsqrt_vec_width = 0
    assert G._shared_prefix(model, ps, "auto", "cpu") == G._shared_prefix(model, ps, True, "cpu") == 64
    assert G._shared_prefix(model, ps, False, "cpu") == 0


def test_copy_prefix_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from dualhyp_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "dualhyp_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text))
    n = "dh_engine_copy_prefix"
    assert n in declared, f"{n} is not declared in include/dualhyp_hip.h"
    assert hasattr(lib, n), f"{n} is not exported"
    assert n in _lib.SIGNATURES, f"{n} is missing from the ctypes table"
    assert declared == set(_lib.SIGNATURES)
    assert lib.dh_abi_version() == 6
    # refused before anything is read through the handle: a null engine, and a handle dh_engine_create never returned
    import ctypes as C
    assert lib.dh_engine_copy_prefix(None, 0, (C.c_int32 * 1)(1), 1, 32, None) != 0
    assert b"null engine" in lib.dh_last_error()
    foreign = C.create_string_buffer(4096)
    assert lib.dh_engine_copy_prefix(C.cast(foreign, C.c_void_p), 0, (C.c_int32 * 1)(1), 1, 32, None) != 0
    assert b"not an engine" in lib.dh_last_error()
