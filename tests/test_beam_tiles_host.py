"""The beam KV tile table on the host (include/dualhyp_hip.h, "Beam KV tile table"): the plain-Python model of the table update
(tests/beam_tiles_reference.py) on a toy cache, the re-parenting copy and the table scheme side by side; the package's host helpers
against the model; the refusals that need no GPU; the header and the ABI."""
import importlib
import itertools
import random
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_tiles_reference as R  # noqa: E402

G = importlib.import_module("dualhyp_amd.generate")
B = importlib.import_module("dualhyp_amd.beam")
PROMPTS = (1, 31, 32, 33, 47)
STEPS = 70
NEW_ENTRIES = ("dh_attn_decode_shared_tab_bf16", "dh_beam_retile", "dh_engine_set_beam_tiles", "dh_engine_reserve_beam_tiles")


def _checker(W, P, NT):
    """behind every step: the text through the new plane is the copy scheme's slot, and the open tile's entry is the row itself"""
    def check(t, cc, tc, planes, n_steps):
        new = planes[t & 1]
        n = P + n_steps - 1                       # positions written so far in every live row's hypothesis
        for w in range(W):
            assert R.text(tc, new, w, P, n, W) == R.text(cc, None, w, P, n, W), f"W {W} P {P} step {t} row {w}"
            assert new[w][((P + n_steps - 1) >> 5) - (P >> 5)] == w, f"W {W} P {P} step {t}: row {w}'s open tile is not its own"
            assert all(0 <= e < W for e in new[w])
    return check


def _run(W, P, seq):
    NT = R.n_tiles(STEPS + 1, 4096)
    return R.simulate(W, P, seq, NT, _checker(W, P, NT))


@pytest.mark.parametrize("W", (2, 3))
def test_every_parent_map_at_every_step(W):
    """all W ** W maps for W = 2 and 3: map m at the steps t = m (mod W ** W), offset by the prompt, so each meets an open tile and a
    tile end behind every prompt length"""
    maps = list(itertools.product(range(W), repeat=W))
    for P in PROMPTS:
        for off in range(len(maps)):
            seq = [maps[(t + off) % len(maps)] for t in range(STEPS)]
            st = _run(W, P, seq)
            assert st["open_copies"] > 0 and st["closed_reads"] > 0


def test_sampled_maps_for_four_beams():
    rng = random.Random(4)
    for P in PROMPTS:
        for _ in range(12):
            seq = [tuple(rng.randrange(4) for _ in range(4)) for _ in range(STEPS)]
            st = _run(4, P, seq)
            assert st["open_copies"] > 0 and st["closed_reads"] > 0


def test_a_finished_utterance_leaves_both_planes_equal():
    rng = random.Random(7)
    for W in (2, 3, 4):
        for P in PROMPTS:
            for stop_at in (1, 2, 31, 32, 33, 40):      # the step from which the utterance takes no step
                seq = [tuple(rng.randrange(W) for _ in range(W)) if t < stop_at else None for t in range(1, STEPS + 1)]
                NT = R.n_tiles(STEPS + 1, 4096)
                seen = []
                inner = _checker(W, P, NT)

                def check(t, cc, tc, planes, n_steps):
                    inner(t, cc, tc, planes, n_steps)
                    if t > stop_at:
                        assert planes[0] == planes[1], f"W {W} P {P} stop {stop_at} step {t}"
                        seen.append(t)
                st = R.simulate(W, P, seq, NT, check)
                assert seen and st["frozen_steps"] == STEPS - stop_at + 1


def test_identity_and_update_rules():
    planes = R.identity(2, 3, 4)
    assert planes[0] == planes[1] == [[0] * 4, [1] * 4, [2] * 4] * 2
    # P = 31: tile0 = 0; step 1 writes position 31 and closes tile 0 — nothing is copied, the entry names the parent
    assert R.update(planes, 1, 1, 3, 31, (2, 2, 0)) == []
    assert planes[1][3:] == [[2, 0, 0, 0], [2, 1, 1, 1], [0, 2, 2, 2]] and planes[1][:3] == planes[0][:3]
    # step 2 writes position 32 into tile 1, which stays open: the parents' tile 1 is copied, tile 0 is inherited
    assert R.update(planes, 2, 1, 3, 31, (1, 0, 1)) == [(3, 4, 1), (4, 3, 1), (5, 4, 1)]
    assert planes[0][3:] == [[2, 0, 0, 0], [2, 1, 1, 1], [2, 2, 2, 2]]
    # utterance 0 took neither step: its rows move over unchanged
    R.update(planes, 2, 0, 3, 5, None)
    assert planes[0][:3] == planes[1][:3]
    assert R.n_tiles(8, 640) == 2 and R.n_tiles(64, 640) == 3 and R.n_tiles(256, 640) == 9 and R.n_tiles(70, 128) == 4
    assert B.beam_tiles(70, 128) == 4 and all(B.beam_tiles(n, s) == R.n_tiles(n, s) for n in (1, 2, 33, 34, 66, 256) for s in (64, 192, 640))


def test_package_helpers_against_the_model():
    rng = random.Random(1)
    for W in (2, 3, 4):
        for P in PROMPTS:
            planes = R.identity(1, W, 4)
            for t in range(1, 80):
                R.update(planes, t, 0, W, P, tuple(rng.randrange(W) for _ in range(W)))
                pl = planes[t & 1]
                for w in range(W):
                    for pos in (0, P - 1, P, P + t - 1, P + t, 32 * ((P >> 5) + 4)):
                        assert B.resolve_slot(pl, w, pos, P, W) == R.resolve(pl, w, pos, P, W)
                    assert B.resolve_slot(torch.tensor(pl), w, P + t - 1, P, W) == R.resolve(pl, w, P + t - 1, P, W)
    st = B.BeamState(2, 3, 8, "cpu")
    tab = st.tile_table(2)
    assert tab.dtype == torch.int32 and tab.is_contiguous() and tab.tolist() == [[[[w] * 2 for w in range(3)]] * 2] * 2
    assert st.tile_table(2) is tab and st.host()["tiles"] == [[[0, 0], [1, 1], [2, 2]]] * 2
    assert B.MAX_BEAM_TILES == 64 and B.KV_MODES == ("copy", "table")


def _cpu_model(name="parity-tiny"):
    from dualhyp_amd import GPT, Config
    return GPT(Config.from_name(name))


def test_refusals_before_the_gpu():
    m = _cpu_model()
    ps = [torch.arange(3, 20), torch.arange(3, 9)]
    with pytest.raises(ValueError, match='"copy" or "table"'):
        G.beam_search_batch(m, ps, 8, num_beams=2, shared_prompt=True, kv="tiles")
    with pytest.raises(ValueError, match="shared_prompt=True"):
        G.beam_search_batch(m, ps, 8, num_beams=2, kv="table")
    with pytest.raises(ValueError, match="num_beams >= 2"):
        G.beam_search_batch(m, ps, 8, num_beams=1, kv="table")
    m.fp8 = True
    with pytest.raises(ValueError, match="fp8"):
        G.beam_search_batch(m, ps, 8, num_beams=2, shared_prompt=True, kv="table")
    del m.fp8
    m.kv_cache_dtype = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        G.beam_search_batch(m, ps, 8, num_beams=2, shared_prompt=True, kv="table")
    m.kv_cache_dtype = "bf16"
    m.cpu_rsqrt_vec_width = 32
    with pytest.raises(ValueError, match="cpu_rsqrt_vec_width"):
        G.beam_search_batch(m, ps, 8, num_beams=2, shared_prompt=True, kv="table")
    m.cpu_rsqrt_vec_width = 0
    with pytest.raises(ValueError, match="2048"):
        G.beam_search_batch(m, [ps[0]] * 600, 8, num_beams=4, shared_prompt=True, kv="table")
    from dualhyp_amd.relprompt import GPT as RelGPT
    rel = object.__new__(RelGPT)
    object.__setattr__(rel, "cpu_rsqrt_vec_width", 0)
    object.__setattr__(rel, "config", m.config)
    with pytest.raises(ValueError, match="RelPrompt"):
        G.beam_search_batch(rel, ps, 8, num_beams=2, shared_prompt=True, kv="table")
    assert B.check_kv("copy", 1, False) == "copy" and B.check_kv("table", 2, True) == "table"
    # what is left is a model on the CPU: the engine says that there is no CPU path
    with pytest.raises(Exception, match="GPU"):
        G.beam_search_batch(m, ps, 8, num_beams=2, shared_prompt=True, kv="table")


def test_cli_flags_and_refusals(capsys):
    from dualhyp_amd import inference
    base = ["--test_path", "/nonexistent/none.json", "--random_init", "--tokenizer", "byte"]
    assert inference.parse_args(base).beam_kv == "copy"
    assert inference.parse_args(base + ["--num_beams", "3", "--share_prompt_kv"]).beam_kv == "copy"
    a = inference.parse_args(base + ["--num_beams", "3", "--share_prompt_kv", "--beam_kv", "table"])
    assert a.beam_kv == "table" and a.share_prompt_kv and a.num_beams == 3
    for extra, word in ((["--beam_kv", "table"], "--num_beams W > 1"),
                        (["--beam_kv", "table", "--num_beams", "2"], "--share_prompt_kv"),
                        (["--beam_kv", "table", "--num_samples", "2", "--top_k", "4", "--share_prompt_kv"], "--num_beams W > 1"),
                        (["--beam_kv", "table", "--num_beams", "2", "--share_prompt_kv", "--quantize", "fp8"], "--quantize fp8"),
                        (["--beam_kv", "tiles", "--num_beams", "2", "--share_prompt_kv"], "invalid choice")):
        with pytest.raises(SystemExit) as ex:
            inference.main(base + extra)          # ends at the parser: nothing has been loaded
        assert ex.value.code == 2 and word in capsys.readouterr().err, extra


def test_records_gain_beam_kv():
    from dualhyp_amd.inference import run_inference
    decode = lambda t: "".join(chr(int(c)) for c in t)
    enc = lambda s: torch.tensor([ord(c) for c in s], dtype=torch.int64)
    examples = [dict(input_ids_no_response=enc("ab:"), ground_truth="hello")]

    def gen(prompts):
        return {"beams": [[dict(tokens=torch.cat([p, enc("hello")]), token_logprobs=torch.full((5,), -0.5), sum_logprob=-2.5, finished=True)]
                          for p in prompts], "logprobs": False}
    assert "beam_kv" not in run_inference(gen, examples, decode, batch_size=1)["predictions"][0]
    gen.beam_kv = "copy"
    assert "beam_kv" not in run_inference(gen, examples, decode, batch_size=1)["predictions"][0]
    gen.beam_kv = "table"
    assert run_inference(gen, examples, decode, batch_size=1)["predictions"][0]["beam_kv"] == "table"


def test_entries_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    import ctypes as C
    from dualhyp_amd import _lib
    lib = _lib.load()
    raw = (REPO / "include" / "dualhyp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in NEW_ENTRIES:
        assert re.search(r"\b" + n + r"\s*\(", text), f"{n} is not declared in include/dualhyp_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is missing from the ctypes table"
        assert n in raw.split("#define DH_ABI_VERSION 6")[0], f"{n} is missing from the list of what ABI 6 gained"
        decl = text[text.index(f"int {n}("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_lib.SIGNATURES[n][1])
    assert lib.dh_abi_version() == 6 and "#define DH_ABI_VERSION 6" in raw and "#define DH_MAX_BEAM_TILES 64" in raw
    assert "Beam KV tile table" in raw
    # the table entry is the shared entry plus the table, its row stride and the step counter
    assert _lib.SIGNATURES["dh_attn_decode_shared_tab_bf16"][1][:-4] == _lib.SIGNATURES["dh_attn_decode_shared_bf16"][1][:-1]
    # refused before anything is read through a pointer
    assert lib.dh_beam_retile(None, None, None, None, 2, None, None, None, 1, 2, 8, 1, None, 1, 64, 128, None) != 0
    assert b"dh_beam_retile: null argument" in lib.dh_last_error()
    assert lib.dh_engine_set_beam_tiles(None, None, 0) != 0 and b"null engine" in lib.dh_last_error()
    assert lib.dh_engine_reserve_beam_tiles(None, 2, 8) != 0 and b"null engine" in lib.dh_last_error()
    args = [None] * 27
    for i, t in enumerate(_lib.SIGNATURES["dh_attn_decode_shared_tab_bf16"][1]):
        if t is C.c_int:
            args[i] = 0
        elif t is C.c_float:
            args[i] = 0.0
    assert lib.dh_attn_decode_shared_tab_bf16(*args) != 0 and b"dh_attn_decode_shared_tab_bf16" in lib.dh_last_error()
