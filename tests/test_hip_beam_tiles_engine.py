"""beam_search_batch(kv="table", shared_prompt=True) end to end (include/dualhyp_hip.h, "Beam KV tile table"): the call records what
the default call records — every output and every array of the host state, bit for bit — and the K / V of every final live beam,
gathered position by position through the final plane, are the default call's slot caches.  The default path is pinned to the
recomputed search by tests/test_hip_beam.py, whose models, prompts and cache readers these tests use.

What keeps the comparisons from passing vacuously is computed on the host from the DEFAULT call's beam_parent records: the rows that
re-parent while their tile is open (the one-tile copy) and the closed tiles that a later step's attention reads from a sibling's slot
(the table).  Both are asserted to be above zero for every case."""
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beam_tiles_reference as R  # noqa: E402
import test_hip_beam as TB  # noqa: E402
from dualhyp_amd import _lib, beam_search_batch  # noqa: E402
from dualhyp_amd import beam as B  # noqa: E402
from dualhyp_amd.stop import compile_stop  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = TB.DEV
KEYS = TB.KEYS_I + TB.KEYS_F


@pytest.fixture(scope="module", params=list(TB.HEAD_SIZES))
def model(request):
    return TB.build(request.param)


@pytest.fixture(scope="module")
def tiny():
    return TB.build("parity-tiny")


def flat(out):
    return [(h["tokens"], h["token_logprobs"], h["sum_logprob"], h["finished"], h["finish_reason"]) for hyps in out for h in hyps]


def same_call(tag, got, want):
    (o1, s1), (o0, s0) = got, want
    a, b = flat(o1), flat(o0)
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2:] == y[2:], f"{tag}: hypothesis {i} differs from the default call's"
    for k in KEYS + tuple(k for k in ("fin_tok", "history") if k in s0["host"]):
        assert s1["host"][k] == s0["host"][k], f"{tag}: the host state's {k} differs from the default call's"


def vacuity_counts(h, lens, W, NT):
    """from the default call's records: (rows that re-parent while their tile is open, closed tiles read from a sibling's slot)"""
    open_copies = sibling_reads = 0
    for u, P in enumerate(lens):
        planes = R.identity(1, W, NT)
        tile0 = P >> 5
        for t in range(1, h["n_steps"][u]):
            rd, last = planes[(t - 1) & 1], ((P + t - 1) >> 5) - tile0
            # the open tile holds a visible key unless the position has just entered it
            sibling_reads += sum(rd[w][j] != w for w in range(W) for j in range(last))
            open_copies += len(R.update(planes, t, 0, W, P, h["beam_parent"][u][t]))
    return open_copies, sibling_reads


def run(m, ps, W, new, table, **kw):
    timing = {}
    extra = dict(shared_prompt=True, kv="table") if table else {}
    out, st = beam_search_batch(m, ps, new, num_beams=W, return_state=True, timing=timing, **extra, **kw)
    st["timing"] = timing
    return out, st


def gathered_kv_equals(tag, m, cfg, ps, W, new, **kw):
    """the table call's K / V of every live beam, position by position through the final plane, against the default call's slots"""
    want = run(m, ps, W, new, False, **kw)
    h0 = want[1]["host"]
    eng = m._engine
    n_pos = [int(p.numel()) + h0["n_steps"][u] - 1 for u, p in enumerate(ps)]
    kv0 = [[TB.read_kv(eng, cfg, u * W + w, n_pos[u]) for w in range(W)] for u in range(len(ps))]
    got = run(m, ps, W, new, True, **kw)
    same_call(tag, got, want)
    h1 = got[1]["host"]
    eng = m._engine
    for u, p in enumerate(ps):
        P = int(p.numel())
        slots = [TB.read_kv(eng, cfg, u * W + w, n_pos[u]) for w in range(W)]
        for w in range(W):
            src = torch.tensor([B.resolve_slot(h1["tiles"][u], w, i, P, W) for i in range(n_pos[u])])
            assert bool((src[:(P >> 5) << 5] == 0).all()) and all(0 <= int(s) < W for s in src)
            for l in range(cfg.n_layer):
                for c in (0, 1):
                    rows = torch.stack([slots[int(s)][l][c][:, i] for i, s in enumerate(src)], dim=1)
                    assert torch.equal(rows, kv0[u][w][l][c]), f"{tag}: utterance {u} beam {w} layer {l} {'KV'[c]} through the table differs"
    return got, want


def check_counts(tag, st0, ps, W, new, eng):
    lens = [int(p.numel()) for p in ps]
    NT = B.beam_tiles(new, eng.s_max)
    oc, sr = vacuity_counts(st0["host"], lens, W, NT)
    print(f"{tag}: {oc} rows re-parented into an open tile, {sr} closed tiles read from a sibling's slot")
    assert oc > 0, f"{tag}: no row re-parented while its tile was open: the case does not test the one-tile copy"
    assert sr > 0, f"{tag}: no closed tile was read from a sibling's slot: the case does not test the table"
    return oc, sr


@pytest.mark.parametrize("W", (2, 3, 4))
def test_table_call_equals_the_default_call(model, W):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    want = run(m, ps, W, 8, False)
    got = run(m, ps, W, 8, True)
    tag = f"{cfg.name} W={W} new=8"
    same_call(tag, got, want)
    oc, _ = check_counts(tag, want[1], ps, W, 8, m._engine)
    t1, t0 = got[1]["timing"], want[1]["timing"]
    assert t1["beam_kv"] == "table" and t0["beam_kv"] == "copy" and t1["shared_prompt"] is True
    assert t1["beam_copied_tiles"] == oc and t0["beam_copied_tiles"] >= t0["beam_copied_rows"] == t1["beam_copied_rows"] >= oc
    assert got[1]["beam"].tiles is not None and want[1]["beam"].tiles is None and "tiles" not in want[1]["host"]
    # an EOS that the best beam of the first utterance emits around step 4: pools fill at different steps
    eos = int(want[0][0][0]["tokens"][TB.LENS[0] + 4])
    want = run(m, ps, W, 8, False, eos_id=eos, length_penalty=0.5)
    got = run(m, ps, W, 8, True, eos_id=eos, length_penalty=0.5)
    same_call(tag + f" eos={eos}", got, want)
    assert sum(want[1]["host"]["n_fin"]) > 0


def test_36_tokens_cross_two_tile_ends(model):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    tag = f"{cfg.name} W=3 new=36"
    got, want = gathered_kv_equals(tag, m, cfg, ps, 3, 36)
    check_counts(tag, want[1], ps, 3, 36, m._engine)


def test_70_tokens_cross_three_tile_ends(tiny):
    cfg, m = tiny
    ps = TB.prompts_for(cfg)
    tag = f"{cfg.name} W=4 new=70"
    got, want = gathered_kv_equals(tag, m, cfg, ps, 4, 70)
    check_counts(tag, want[1], ps, 4, 70, m._engine)
    assert max(len(set(row)) for u in got[1]["host"]["tiles"] for row in u) > 1, "no final row names a sibling's tile"


def test_device_histories_ban_stop_sequence_and_mask(model):
    cfg, m = model
    ps = TB.prompts_for(cfg)
    V = cfg.padded_vocab_size
    base = run(m, ps, 3, 12, False, history="device", no_repeat_ngram=3)
    text = base[0][1][0]["tokens"][TB.LENS[1]:].tolist()
    stop = compile_stop([], [text[4:6]], vocab=V)                   # two tokens the second utterance's best beam emits
    mask = [[i for i in range(V) if i != text[2]]] * len(ps)       # and a token nobody may emit
    kw = dict(history="device", no_repeat_ngram=3, stop=stop, token_mask=mask)
    want = run(m, ps, 3, 12, False, **kw)
    got = run(m, ps, 3, 12, True, **kw)
    same_call(f"{cfg.name} device histories", got, want)
    assert "history" in want[1]["host"] and "fin_tok" in want[1]["host"]


def test_calls_do_not_disturb_each_other(model):
    """default, table, default, table on one engine: the graph keys and the two scratches keep them apart"""
    cfg, m = model
    ps = TB.prompts_for(cfg)
    calls = [run(m, ps, 3, 8, table) for table in (False, True, False, True)]
    for i in (1, 2, 3):
        same_call(f"{cfg.name} call {i}", calls[i], calls[0])
    assert calls[1][1]["host"]["tiles"] == calls[3][1]["host"]["tiles"]


def test_refusals_and_the_one_tile_scratch():
    cfg, m = TB.build("parity-tiny", seed=12)
    ps = TB.prompts_for(cfg)
    for kw, word in ((dict(kv="table"), "shared_prompt=True"), (dict(kv="tiles", shared_prompt=True), '"copy" or "table"')):
        with pytest.raises(ValueError, match=word):
            beam_search_batch(m, ps, 8, num_beams=2, **kw)
    with pytest.raises(ValueError, match="num_beams >= 2"):
        beam_search_batch(m, ps, 8, num_beams=1, kv="table")
    W, new, n_utt = 2, 8, len(ps)
    rows = n_utt * W
    eng = m.engine(rows, max(TB.LENS) + new, rows)
    eng.set_rsqrt_emulation(0, whole_call=False)
    lib, hd = eng.lib, eng.handle
    eng.reserve_beams(W, new)
    state = B.BeamState(n_utt, W, new, DEV)
    state.n_steps.fill_(1)
    plen = torch.tensor(TB.LENS, dtype=torch.int32, device=DEV)
    NT = B.beam_tiles(new, eng.s_max)
    tab = state.tile_table(NT)

    def refused(word):
        with pytest.raises(_lib.DualHypHipError, match=word):
            eng.decode_beam(state, plen, 1, None, first_step=1)

    try:
        eng.set_beam_tiles(tab)
        refused("group_rows = W = 2")                               # no shared-prompt attention
        eng.set_shared_prompt(W, plen)
        refused("dh_engine_reserve_beam_tiles")                     # the re-parenting scratch is not the one-tile scratch
        before = lib.dh_engine_device_bytes(hd)
        eng.reserve_beam_tiles(W, new)
        added = lib.dh_engine_device_bytes(hd) - before
        assert added == eng.max_batch * 2 * cfg.n_layer * cfg.n_query_groups * cfg.head_size * 32 * 2, "one tile per (row, 2 L, G), in bf16"
        eng.reserve_beam_tiles(W, 70)                               # whatever the length: nothing more
        assert lib.dh_engine_device_bytes(hd) - before == added
        eng.set_beam_tiles(torch.zeros((2, n_utt, W, NT + 1), dtype=torch.int32, device=DEV))
        refused("tiles per row")
        with pytest.raises(_lib.DualHypHipError, match="n_tiles=65"):
            eng.set_beam_tiles(torch.zeros((2, n_utt, W, 65), dtype=torch.int32, device=DEV))
        for bad in (tab[0], tab.long(), tab.cpu(), tab.transpose(2, 3)):
            with pytest.raises(TypeError, match="set_beam_tiles"):
                eng.set_beam_tiles(bad)
    finally:
        eng.set_beam_tiles(None)
        eng.set_shared_prompt()
    # dh_set_tuning key 10 moves steps to the tiled kernels by row count: the whole call refuses, with the reason, and leaves nothing set
    _lib.check(lib.dh_set_tuning(10, 4))
    try:
        with pytest.raises(_lib.DualHypHipError, match="key 10"):
            beam_search_batch(m, ps, new, num_beams=W, shared_prompt=True, kv="table")
    finally:
        _lib.check(lib.dh_set_tuning(10, 0))
    # with the table off the call is the default call again
    a = flat(beam_search_batch(m, ps, new, num_beams=W))
    b = flat(beam_search_batch(m, ps, new, num_beams=W, shared_prompt=True, kv="table"))
    assert len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2:] == y[2:] for x, y in zip(a, b))


def test_inference_cli_beam_kv(tmp_path):
    """`python -m dualhyp_amd.inference --num_beams 2 --share_prompt_kv --beam_kv table` end to end (in this process): the predictions
    of the run without the flag, and every record gains beam_kv"""
    import test_harness as harness
    from dualhyp_amd import inference
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    base = ["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
            "DualHyp", "--dual_hypotheses", "--max_new_tokens", "6", "--decode_batch", "4", "--num_beams", "2", "--share_prompt_kv"]
    inference.main(base + ["--predict_dir", str(tmp_path / "copy")])
    inference.main(base + ["--beam_kv", "table", "--predict_dir", str(tmp_path / "table")])
    js0 = json.loads((tmp_path / "copy" / "random_init.json").read_text())
    js1 = json.loads((tmp_path / "table" / "random_init.json").read_text())
    assert len(js1) == len(js0) == len(items) + 2
    for a, b in zip(js0[:-2], js1[:-2]):
        assert "beam_kv" not in a and b["beam_kv"] == "table" and b["shared_prompt"] is True
        assert {k: v for k, v in b.items() if k != "beam_kv"} == a
