"""`python -m dualhyp_amd.inference --constrain chain` end to end on the GPU (in this process), on the harness fixture with the byte
tokenizer: the entry points get a chain automaton built from the call's own prompts, every prediction's ids are a text that automaton
accepts, and the records carry the order.  A run without the flag hands the entry point no automaton and writes the records it always
wrote."""
import importlib
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import automaton_reference as AR  # noqa: E402
import test_harness as harness  # noqa: E402
from dualhyp_amd import automaton as A  # noqa: E402
from dualhyp_amd import inference  # noqa: E402

pytestmark = pytest.mark.gpu


def run(tmp_path, monkeypatch, name, more):
    G = importlib.import_module("dualhyp_amd.generate")        # the package's attribute of that name is the function
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    seen = []
    real = getattr(G, name)

    def spy(model, prompts, max_new, **kw):
        res = real(model, prompts, max_new, **kw)
        outs = res[0] if isinstance(res, tuple) else res
        seen.append(([p.cpu() for p in prompts], kw.get("automaton"), kw.get("eos_id"), [o.cpu() for o in outs], max_new))
        return res

    monkeypatch.setattr(G, name, spy)
    pred = tmp_path / ("pred_" + "_".join(m.strip("-") for m in more))
    inference.main(["--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init", "--tokenizer", "byte", "--prompts_format",
                    "DualHyp", "--dual_hypotheses", "--max_new_tokens", "12", "--decode_batch", "4", "--predict_dir", str(pred)] + more)
    js = json.loads((pred / "random_init.json").read_text())
    assert len(js) == len(items) + 2 and seen and sum(len(s[0]) for s in seen) == len(items)
    return js[:-2], seen


@pytest.mark.parametrize("schedule", ("batch", "continuous"))
def test_inference_cli_constrain_chain(tmp_path, monkeypatch, schedule):
    name = "generate_stream" if schedule == "continuous" else "generate_batch"
    recs, seen = run(tmp_path, monkeypatch, name, ["--schedule", schedule, "--constrain", "chain", "--constrain_order", "2"])
    assert all(rec["constrained"] is True and rec["constrain_order"] == 2 for rec in recs)
    moved = 0
    for prompts, aset, eos, outs, max_new in seen:
        assert isinstance(aset, A.AutomatonSet) and aset.n_seq == len(prompts) and eos is not None
        off, tok, dst, init = aset.edge_off.tolist(), aset.edge_tok.tolist(), aset.edge_dst.tolist(), aset.init.tolist()
        for u, (p, o) in enumerate(zip(prompts, outs)):
            g = o[p.numel():].tolist()
            whole = len(g) < max_new                                     # cut before an EOS; a full budget may have been cut short
            assert A.accepts(aset, u, g, eos, complete=whole) and AR.accepts(off, tok, dst, init[u], g, eos, complete=whole), (u, g)
            assert AR.window_accepts(p.tolist(), g, 2), (u, g)          # every bigram of the answer is a bigram of its prompt
            moved += len(g)
    assert moved > 0


def test_inference_cli_without_the_flag(tmp_path, monkeypatch):
    recs, seen = run(tmp_path, monkeypatch, "generate_batch", ["--schedule", "batch"])
    assert all("constrained" not in rec and "constrain_order" not in rec for rec in recs)
    assert all(aset is None for _, aset, _, _, _ in seen)
    # the same run under the chain constraint answers otherwise: the flag is what moves the predictions
    chained, _ = run(tmp_path, monkeypatch, "generate_batch", ["--schedule", "batch", "--constrain", "chain"])
    assert [r["inference"] for r in chained] != [r["inference"] for r in recs]
    assert [r["ground_truth"] for r in chained] == [r["ground_truth"] for r in recs]
