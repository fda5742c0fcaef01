#!/usr/bin/env python3
"""What stop conditions save and cost (GPU box): python tools/bench_stop.py [--parent_lib OTHER.so] [--out profiles/stop.json]

Measurements, each in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

"corpus": --rows synthetic prompts of --prompt_len tokens on the TinyLlama shape (hash weights + LoRA r16, vocab 32 000), greedy,
--max_new_tokens new tokens, an EOS that never comes (the harness's worst case: every row runs to its budget).  The stop set is taken
from the unstopped run's own ids: ids are added, the one that ends the most still-unstopped sequences within their first --within
tokens first, until every sequence stops there — a synthetic stand-in for "the first newline", which a hash-weight model does not
emit.  Reported with the feature off and on, under generate_batch and under generate_stream (--stream_rows rows): the decode steps
until the last sequence had ended, the decode row-steps, utterances/s over the call's prefill and decode time (median of --repeats
after a warm-up), and that the stopped ids are the unstopped ids cut behind stop.first_stop.  This says how the machinery behaves,
not what it does to a word error rate.

--parent_lib: the feature-off 640-row decode step (generate_batch's decode time over its steps, no EOS, 64 new tokens) in children
of their own, this build and the other library (DUALHYP_HIP_LIB; a build of the parent commit has none of the feature's entries, so
the child drops them from the symbol table it binds — the feature-off path never calls them) in alternation, --rounds times each,
with a hash of the generated ids: the two must be equal.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=640)
ap.add_argument("--stream_rows", type=int, default=160)
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=150)
ap.add_argument("--within", type=int, default=40, help="every sequence stops within this many tokens")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3, help="children per library of the --parent_lib comparison")
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the feature-off step with")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the measurement of this run")
a = ap.parse_args()

NEW_ENTRIES = ("dh_sample_bf16_stop", "dh_sample_rows_bf16_stop", "dh_beam_select_bf16_stop", "dh_engine_set_stop")


def model_and_corpus():
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    corpus = [p.to(dev) for p in synth_prompts(a.rows, a.prompt_len, cfg.padded_vocab_size, seed=7)]
    return cfg, m, corpus


def cover(texts, within):
    """ids, added greedily, until every text holds one among its first `within` tokens"""
    left, ids = set(range(len(texts))), []
    while left:
        count = {}
        for u in left:
            for t in set(texts[u][:within]):
                count[t] = count.get(t, 0) + 1
        best = max(sorted(count), key=lambda t: count[t])
        ids.append(best)
        left = {u for u in left if best not in texts[u][:within]}
    return ids


def corpus_worker() -> dict:
    from dualhyp_amd import generate_batch, generate_stream
    from dualhyp_amd.stop import compile_stop, first_stop
    cfg, m, corpus = model_and_corpus()
    V = cfg.padded_vocab_size
    kw = dict(temperature=0.2, top_k=1)
    free = generate_batch(m, corpus, a.max_new_tokens, prefill_batch=32, **kw)
    texts = [o[a.prompt_len:].tolist() for o in free]
    eos = next(t for t in range(V) if all(t not in g for g in texts))          # an EOS that never comes
    ids = cover(texts, a.within)
    spec = compile_stop(ids, [], V, "cuda:0")
    stops = [first_stop(g, spec) for g in texts]
    res = dict(rows=a.rows, stream_rows=a.stream_rows, max_new_tokens=a.max_new_tokens, eos=eos, stop_ids=len(ids),
               first_stop=dict(min=min(stops), median=statistics.median(stops), max=max(stops)))

    def call(schedule, stop):
        tm = {}
        more = dict(stop=stop) if stop is not None else {}
        if schedule == "batch":
            out = generate_batch(m, corpus, a.max_new_tokens, eos_id=eos, prefill_batch=32, timing=tm, **more, **kw)
        else:
            out = generate_stream(m, corpus, a.max_new_tokens, eos_id=eos, max_rows=a.stream_rows, prefill_batch=32, timing=tm, **more, **kw)
        return [o.tolist() for o in out], tm

    for schedule in ("batch", "continuous"):
        for arm, stop in (("off", None), ("on", spec)):
            out, tm = call(schedule, stop)                     # warm-up: allocation, graph capture; and the ids
            for o, g, s in zip(out, texts, stops):
                assert o[a.prompt_len:] == (g if stop is None else g[:s + 1]), "the stopped ids are not the unstopped ids, cut"
            rate = []
            for _ in range(a.repeats):
                _, tm = call(schedule, stop)
                rate.append(a.rows / ((tm["prefill_ms"] + tm["decode_ms"]) * 1e-3))
            res[f"{schedule}_{arm}"] = dict(decode_steps=tm["decode_steps"], decode_row_steps=tm["decode_row_steps"],
                                            utterances_per_s=[round(x, 1) for x in rate], median_utterances_per_s=round(statistics.median(rate), 1))
    return res


def step_worker() -> dict:
    import torch
    from dualhyp_amd import generate_batch
    cfg, m, corpus = model_and_corpus()
    ms = []
    for i in range(a.repeats + 1):                             # the first call is the warm-up
        tm = {}
        out = generate_batch(m, corpus, 64, temperature=0.2, top_k=1, prefill_batch=32, timing=tm)
        if i:
            ms.append(tm["decode_ms"] / tm["decode_steps"])
    sha = hashlib.sha256(torch.stack([o[a.prompt_len:] for o in out]).cpu().numpy().tobytes()).hexdigest()[:16]
    return dict(rows=a.rows, ms_per_step=[round(x, 4) for x in ms], ids_sha256=sha)


def child(what: str, lib: str = "") -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", what, "--rows", str(a.rows), "--stream_rows", str(a.stream_rows),
           "--prompt_len", str(a.prompt_len), "--max_new_tokens", str(a.max_new_tokens), "--within", str(a.within), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    if lib:
        env["DUALHYP_HIP_LIB"] = lib
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout, env=env)      # a step that fails ends the tool
    if r.returncode != 0:
        sys.exit(f"{what} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("{"):
            return json.loads(l)
    sys.exit(f"{what}: the child printed no result")


def main() -> None:
    if a.worker == "step_off":
        from dualhyp_amd import _lib
        if os.environ.get("DUALHYP_HIP_LIB"):                 # a build without the feature: bind what it has
            for name in NEW_ENTRIES:
                _lib.SIGNATURES.pop(name, None)
        print(json.dumps(step_worker()), flush=True)
        return
    if a.worker:
        print(json.dumps(corpus_worker()), flush=True)
        return
    res = dict(tool="bench_stop", prompt_len=a.prompt_len, repeats=a.repeats, corpus=child("corpus"))
    if a.parent_lib:
        lib = str(Path(a.parent_lib).resolve())
        runs = {"parent": [], "this": []}
        for _ in range(a.rounds):
            runs["parent"].append(child("step_off", lib))
            runs["this"].append(child("step_off"))
        med = {k: statistics.median(x for r in v for x in r["ms_per_step"]) for k, v in runs.items()}
        child_med = {k: [statistics.median(r["ms_per_step"]) for r in v] for k, v in runs.items()}
        hashes = {k: sorted({r["ids_sha256"] for r in v}) for k, v in runs.items()}
        res["feature_off_vs_parent"] = dict(ms_per_step={k: [r["ms_per_step"] for r in v] for k, v in runs.items()},
                                            median_ms={k: round(x, 4) for k, x in med.items()},
                                            parent_spread_percent=round((max(child_med["parent"]) / min(child_med["parent"]) - 1) * 100, 2),
                                            this_over_parent_percent=round((med["this"] / med["parent"] - 1) * 100, 2),
                                            ids_sha256=hashes, ids_equal=hashes["this"] == hashes["parent"] and len(hashes["this"]) == 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
