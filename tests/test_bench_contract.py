"""bench.py's one-line JSON contract (driver + judge read it): run a short bench as a child process on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_has_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--in-flight", "2", "--full",
                          "--no-cpu-baseline", "--no-overlap-probe"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 32 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.05 < r["frac"] < 1.0 and d["value"] > 50
    assert d["roofline_decode"]["bound"] == "hbm" and 32 <= d["phases"]["decode_rows_per_launch"] <= 64   # groups of 2 and 1 batches
    assert d["config"]["prefill_tokens_per_launch"] == 2 * 32 * 512
    # round 4: the line says what it was measured on and how far its repeats were apart
    dev = d["device"]
    assert dev["arch"].startswith("gfx950") and dev["compute_units"] == 256 and dev["hbm_bytes"] > 200e9 and dev["name"]
    rep = d["repeats"]
    assert rep["timed_regions"] == 3 and len(rep["ms_per_step_all"]) == 3 and rep["reported"] == "median by wall time"
    assert sorted(rep["ms_per_step_all"])[1] == pytest.approx(d["ms_per_step"]) and rep["spread_pct"] >= 0
    assert r["traffic"] is not None and "profiles/" in r["traffic_source"]


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: ONE timed region of exactly --steps steps, the headline fields and none of the --full figures;
    --dump-outputs writes the ids the last timed step returned, whose prompts are the seeded corpus's."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--in-flight", "2",
                          "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["repeats"]["timed_regions"] == 1 and d["unit"] == "utterances/s"
    assert abs(d["value"] - 32 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6 and d["value"] > 50
    assert not {"roofline", "roofline_decode", "phases", "cpu_baseline", "parity", "one_batch_in_flight", "overlap_probe"} & set(d)
    assert sorted(os.listdir(tmp_path / "dump")) == ["token_ids.npy"]
    ids = np.load(tmp_path / "dump" / "token_ids.npy")
    assert ids.dtype == np.float32 and ids.shape == (32, 512 + 64)
    from dualhyp_amd import Config
    from dualhyp_amd.synth import synth_prompts
    vocab = Config.from_name("tiny-llama-1.1b-chat").padded_vocab_size
    want = torch.stack(synth_prompts(32 * 4, 512, vocab, seed=1337)[32 * 3:])       # batches: 1 warm-up + 3 timed, the last one
    assert torch.equal(torch.from_numpy(ids[:, :512]).long(), want)
    assert ids.min() >= 0 and ids.max() < vocab and ids.max() == np.floor(ids.max())
