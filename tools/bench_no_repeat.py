#!/usr/bin/env python3
"""What no_repeat_ngram costs and does (GPU box): python tools/bench_no_repeat.py [--parent_lib OTHER.so] [--out profiles/no_repeat.json]

Measurements, each in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

"step": a 640-row decode step of the TinyLlama shape (hash weights + LoRA r16, vocab 32 000) through generate_batch, greedy, no EOS,
--prompt_len-token prompts, --max_new_tokens new tokens: the call's own HIP-event decode time divided by its decode steps, with
no_repeat_ngram = --ngram and without, in alternation in ONE process after a warm-up of both arms; median over --repeats.  The
feature-on ids are checked on the host: no generated n-gram occurs twice.

"corpus": the same model and prompts with an EOS (--eos; default: the id the feature-off run produces most often, so that sequences
do end), feature off and on: the share of sequences that end on their budget (done == 2), the decode steps until the last sequence
had finished, and the share of sequences with at least one non-empty ban set.  The prompts are synthetic: this says how the
machinery behaves, not what it does to a word error rate.

--parent_lib: the feature-off step time once more in children of their own, this build and the other library (DUALHYP_HIP_LIB; a
build of the parent commit has none of the feature's entries, so the child drops them from the symbol table it binds — the
feature-off path never calls them) in alternation, --rounds times each, with a hash of the generated ids: the two must be equal.
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
ap.add_argument("--what", nargs="+", default=["step", "corpus"], choices=["step", "corpus"])
ap.add_argument("--step_rows", type=int, default=640)
ap.add_argument("--ngram", type=int, default=4)
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--eos", type=int, default=-1, help="the corpus measurement's EOS id (-1: the feature-off run's most frequent id)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2, help="children per library of the --parent_lib comparison")
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the feature-off step with")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the measurement of this run")
a = ap.parse_args()

NEW_ENTRIES = ("dh_sample_bf16_ngram", "dh_sample_rows_bf16_ngram", "dh_engine_set_no_repeat_ngram")


def model_and_corpus():
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    corpus = [p.to(dev) for p in synth_prompts(a.step_rows, a.prompt_len, cfg.padded_vocab_size, seed=7)]
    return m, corpus


def ids_hash(out) -> str:
    import torch
    return hashlib.sha256(torch.stack([o[a.prompt_len:] for o in out]).cpu().numpy().tobytes()).hexdigest()[:16]


def step_worker(arms=("off", "on")) -> dict:
    from dualhyp_amd import generate_batch, ngram
    m, corpus = model_and_corpus()
    kw = dict(temperature=0.2, top_k=1, prefill_batch=32)

    def call(arm):
        tm = {}
        more = dict(no_repeat_ngram=a.ngram) if arm == "on" else {}
        out = generate_batch(m, corpus, a.max_new_tokens, timing=tm, **more, **kw)
        return out, tm["decode_ms"] / tm["decode_steps"]

    res = dict(rows=a.step_rows, ngram=a.ngram)
    for arm in arms:                                          # warm-up of the arms: allocation, graph capture
        out, _ = call(arm)
        res[f"ids_sha256_{arm}"] = ids_hash(out)
        if arm == "on":
            texts = [o[a.prompt_len:].tolist() for o in out]
            for g in texts:
                grams = [tuple(g[i:i + a.ngram]) for i in range(len(g) - a.ngram + 1)]
                assert len(set(grams)) == len(grams), "the feature-on call repeated an n-gram"
            res["sequences_with_a_ban"] = sum(bool(ngram.ban_positions(g, a.ngram)) for g in texts)
    ms = {arm: [] for arm in arms}
    for _ in range(a.repeats):
        for arm in arms:
            ms[arm].append(call(arm)[1])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    res.update(ms_per_step={arm: [round(x, 4) for x in v] for arm, v in ms.items()}, median_ms={arm: round(x, 4) for arm, x in med.items()})
    if len(arms) == 2:
        res.update(added_us_per_step=round((med["on"] - med["off"]) * 1e3, 1), added_percent=round((med["on"] / med["off"] - 1) * 100, 2))
    return res


def corpus_worker() -> dict:
    import torch
    from dualhyp_amd import generate_batch, ngram
    m, corpus = model_and_corpus()
    kw = dict(temperature=0.2, top_k=1, prefill_batch=32)
    eos = a.eos
    if eos < 0:
        free = generate_batch(m, corpus, a.max_new_tokens, **kw)
        eos = int(torch.bincount(torch.stack([o[a.prompt_len:] for o in free]).reshape(-1)).argmax())
    res = dict(rows=a.step_rows, ngram=a.ngram, eos=eos, max_new_tokens=a.max_new_tokens)
    for arm, more in (("off", {}), ("on", dict(no_repeat_ngram=a.ngram))):
        tm = {}
        out, st = generate_batch(m, corpus, a.max_new_tokens, eos_id=eos, return_state=True, timing=tm, **more, **kw)
        done = st["done"].tolist()
        made = (st["length"] - a.prompt_len).tolist()
        texts = [o[a.prompt_len:].tolist() for o in out]
        res[arm] = dict(ended_on_budget_share=round(sum(d == 2 for d in done) / len(done), 4),
                        ended_on_eos_share=round(sum(d == 1 for d in done) / len(done), 4),
                        steps_until_last_finished=max(made) - 1,              # the first token is the prefill's
                        decode_steps_launched=tm["decode_steps"],
                        mean_new_tokens=round(sum(made) / len(made), 2),
                        sequences_with_a_repeated_ngram=sum(len({tuple(g[i:i + a.ngram]) for i in range(len(g) - a.ngram + 1)})
                                                            < max(len(g) - a.ngram + 1, 0) for g in texts),
                        sequences_with_a_ban=sum(bool(ngram.ban_positions(g, a.ngram)) for g in texts))
    return res


def child(what: str, lib: str = "") -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", what, "--step_rows", str(a.step_rows), "--ngram", str(a.ngram),
           "--prompt_len", str(a.prompt_len), "--max_new_tokens", str(a.max_new_tokens), "--repeats", str(a.repeats), "--eos", str(a.eos)]
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
        print(json.dumps(step_worker(("off",))), flush=True)
        return
    if a.worker:
        print(json.dumps(step_worker() if a.worker == "step" else corpus_worker()), flush=True)
        return
    res = dict(tool="bench_no_repeat", ngram=a.ngram, prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats)
    for what in a.what:
        res[what] = child(what)
    if a.parent_lib:
        lib = str(Path(a.parent_lib).resolve())
        runs = {"this": [], "parent": []}
        for _ in range(a.rounds):
            runs["this"].append(child("step_off"))
            runs["parent"].append(child("step_off", lib))
        med = {k: statistics.median(x for r in v for x in r["ms_per_step"]["off"]) for k, v in runs.items()}
        hashes = {k: sorted({r["ids_sha256_off"] for r in v}) for k, v in runs.items()}
        res["feature_off_vs_parent"] = dict(ms_per_step={k: [r["ms_per_step"]["off"] for r in v] for k, v in runs.items()},
                                            median_ms={k: round(x, 4) for k, x in med.items()},
                                            this_over_parent_percent=round((med["this"] / med["parent"] - 1) * 100, 2),
                                            ids_sha256=hashes, ids_equal=hashes["this"] == hashes["parent"] and len(hashes["this"]) == 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
