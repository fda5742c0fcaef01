"""The engine and sampling calls of the generation entry points, call by call, against a recorded trace: which calls are made, in which
order, with which arguments, and which buffer goes where (a tensor passed twice is named by its first appearance, so "the buffer
given to ops.sample is the one given to set_logprobs" is part of the trace).  Everything runs on the CPU against the scripted engine
of tests/scripted_engine.py; neither the library nor a GPU is needed.

Each entry point runs with no option and with every option it accepts at once (no compile step had to be left out: all of them run
on CPU tensors), and generate_batch once more under speculate.  tests/golden/generate_trace.json holds the expected traces.  They are
the traces of dualhyp_amd/generate.py as it stood before the per-call options object, recorded by this file with

    git show 26788e8:dualhyp_amd/generate.py > /tmp/generate_before.py && \
        GENERATE_TRACE_SUBJECT=/tmp/generate_before.py GENERATE_TRACE_RECORD=1 python -m pytest tests/test_generate_trace_host.py

GENERATE_TRACE_SUBJECT alone runs the comparison against that file instead of the package's module."""
import importlib
import importlib.util
import json
import os
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from scripted_engine import ScriptedModel, patch_ops  # noqa: E402

from dualhyp_amd import automaton as A  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "generate_trace.json"
EOS = 1


def subject():
    """dualhyp_amd.generate, or the file GENERATE_TRACE_SUBJECT names, loaded as a module of the package."""
    path = os.environ.get("GENERATE_TRACE_SUBJECT")
    if not path:
        return importlib.import_module("dualhyp_amd.generate")        # the package's `generate` attribute is the function
    spec = importlib.util.spec_from_file_location("dualhyp_amd._generate_trace_subject", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = subject()


def prompts():
    """70, 71 and 66 tokens; the first 64 are shared, token 64 differs."""
    g = torch.Generator().manual_seed(11)
    head = torch.randint(8, 60, (64,), generator=g)
    return [torch.cat([head, torch.tensor([2 + i]), torch.randint(8, 60, (n - 65,), generator=g)]) for i, n in enumerate((70, 71, 66))]


def options(*names):
    """The keyword arguments that switch the named options on."""
    every = dict(
        logprobs=dict(return_logprobs=True), top=dict(top_logprobs=2),
        mask=dict(token_mask=[[EOS, 5, 6, 7, 9], [EOS, 7, 8, 9, 10, 11], [EOS, 3, 7, 12]]), ngram=dict(no_repeat_ngram=2),
        stop_set=dict(stop=[5]), stop=dict(stop=[5, [6, 7]]), nucleus=dict(top_p=0.9, min_p=0.05),
        penalties=dict(repetition_penalty=1.25, frequency_penalty=0.5, presence_penalty=-0.25), bias=dict(bias=[([3, 4], 2.0), ([9], -1.5)]),
        automaton=dict(automaton=A.from_sequences([[[7, 7, 7]], [[7, 7, 7, 7], [7, 9]], [[7]]], EOS)), prefix=dict(share_prefix=True),
        shared_prompt=dict(shared_prompt=True), state=dict(return_state=True))
    out = {}
    for n in names:
        out.update(every[n])
    return out


SAMPLED = dict(temperature=0.75, top_k=5, seed=7)
ALL = ("mask", "ngram", "stop", "nucleus", "penalties", "bias", "automaton", "prefix", "state")
CASES = {
    "generate_batch.plain": ("generate_batch", 1, dict(SAMPLED)),
    "generate_batch.all": ("generate_batch", 1, dict(SAMPLED, **options("logprobs", "top", *ALL))),
    "generate_batch.speculate": ("generate_batch", 1, dict(top_k=1, speculate=2, **options("logprobs", "mask", "ngram", "stop", "state"))),
    "sample_batch.plain": ("sample_batch", 2, dict(SAMPLED, num_samples=2)),
    "sample_batch.all": ("sample_batch", 2, dict(SAMPLED, num_samples=2, **options("top", *ALL, "shared_prompt"))),
    "generate_stream.plain": ("generate_stream", 1, dict(SAMPLED, max_rows=2, check_every=2)),
    "generate_stream.all": ("generate_stream", 1, dict(SAMPLED, max_rows=2, check_every=2, **options("logprobs", "top", *ALL))),
    "beam_host.plain": ("beam_search_batch", 2, dict(num_beams=2, history="host")),
    "beam_host.all": ("beam_search_batch", 2, dict(num_beams=2, history="host", length_penalty=0.5,
                                                   **options("mask", "stop_set", "shared_prompt", "state"))),
    "beam_device.plain": ("beam_search_batch", 2, dict(num_beams=2, history="device")),
    "beam_device.all": ("beam_search_batch", 2, dict(num_beams=2, history="device", length_penalty=0.5,
                                                     **options("mask", "ngram", "stop", "shared_prompt", "state"))),
}
N_GEN = [2, 4, 3]       # tokens per sequence: all have finished behind 4 of the 6, so the loops that check for it end early


def run(name, monkeypatch):
    fn, rows_per_prompt, kw = CASES[name]
    ps = prompts()
    model = ScriptedModel([n for n in N_GEN for _ in range(rows_per_prompt)])
    model.eng.lens = [p.numel() for p in ps for _ in range(rows_per_prompt)]
    patch_ops(monkeypatch, G.ops, model.eng)
    monkeypatch.setattr(G, "EOS_CHECK_EVERY", 2)        # several chunks within the 6 tokens
    result = getattr(G, fn)(model, ps, 6, eos_id=EOS, prefill_batch=2, **kw)
    model.eng.trace.add("return", result)
    return json.loads(json.dumps(model.eng.trace.entries))


def test_a_stream_without_options_asks_nothing_of_the_models_config(monkeypatch):
    ps = prompts()
    model = ScriptedModel(N_GEN)
    model.config = None
    model.eng.lens = [p.numel() for p in ps]
    patch_ops(monkeypatch, G.ops, model.eng)
    out = G.generate_stream(model, ps, 6, top_k=1, eos_id=EOS, max_rows=2, prefill_batch=2, share_prefix=True)
    assert [o.numel() - p.numel() for o, p in zip(out, ps)] == [n - 1 for n in N_GEN]       # the EOS is cut


@pytest.mark.parametrize("name", list(CASES))
def test_trace(name, monkeypatch):
    got = run(name, monkeypatch)
    if os.environ.get("GENERATE_TRACE_RECORD"):
        golden = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
        golden[name] = got
        GOLDEN.write_text(json.dumps(golden, indent=0, sort_keys=True) + "\n")
        return
    want = json.loads(GOLDEN.read_text())[name]
    assert [e[0] for e in got] == [e[0] for e in want], "the calls, in order"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i} ({w[0]})"
