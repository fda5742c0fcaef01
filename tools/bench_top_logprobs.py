#!/usr/bin/env python3
"""What top_logprobs costs a decode step (GPU box): python tools/bench_top_logprobs.py [--out profiles/top_logprobs.json]
                                                                                      [--baseline_lib other/libdualhyp_hip.so]

generate_batch with return_logprobs alone ("lp"), with top_logprobs=1 ("k1") and with top_logprobs=8 ("k8"), in one process per
shape: TinyLlama (hash weights + LoRA r16, vocab 32 000) at 32 and 640 rows, and the same decoder with a 128 256-entry vocabulary
(Llama-3's) at 32 rows — the shapes of tools/bench_logprobs.py.  Prompts of --prompt_len tokens, --max_new_tokens new tokens, greedy,
no EOS.  After a warm-up call of each arm (allocation, graph capture), --repeats rounds of the arms in alternation; the figure is the
call's own HIP-event decode time divided by its decode steps (ms per token and row set), median over the repeats, and the
differences to the "lp" arm.  The ids and the log-probabilities of the arms must be equal (digests).

--baseline_lib: another build of the library with the same entry points (a build of the commit before the feature, whose new entries
are stubs): a second child per shape, right after the first, times the "lp" arm alone under it (DUALHYP_HIP_LIB), so the baseline
the differences are also given against does not come from the build under test.  Every child runs under its own time limit; the
parent never touches the GPU and prints ONE JSON line.
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

SHAPES = {"tinyllama_32": (32, None), "tinyllama_640": (640, None), "vocab128256_32": (32, 128256)}
ARMS = {"lp": 0, "k1": 1, "k8": 8}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--baseline_lib", type=str, default="", help="a library of the parent commit: its 'lp' arm is timed too")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the shape of this run")
ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS), help="(child) the arms of this run")
a = ap.parse_args()


def digest(tensors) -> str:
    h = hashlib.sha256()
    for o in tensors:
        h.update(o.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def worker(shape: str) -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, generate_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    rows, vocab = SHAPES[shape]
    dev = "cuda:0"
    over = {} if vocab is None else dict(vocab_size=vocab, padded_vocab_size=vocab)
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0}, **over)
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    corpus = [p.to(dev) for p in synth_prompts(rows, a.prompt_len, cfg.padded_vocab_size, seed=7)]
    kw = dict(temperature=0.2, top_k=1, prefill_batch=32)

    def call(arm):
        tm = {}
        extra = dict(top_logprobs=ARMS[arm]) if ARMS[arm] else {}       # the "lp" arm passes nothing a build without the feature lacks
        res = generate_batch(m, corpus, a.max_new_tokens, timing=tm, return_logprobs=True, **extra, **kw)
        return digest(res[0]) + digest(res[1]), tm["decode_ms"] / tm["decode_steps"], res

    ident = {arm: call(arm)[0] for arm in a.arms}                      # warm-up of every arm
    ms = {arm: [] for arm in a.arms}
    for _ in range(a.repeats):
        for arm in a.arms:
            d, t, res = call(arm)
            assert d == ident[arm]
            ms[arm].append(t)
    out = dict(rows=rows, vocab=cfg.padded_vocab_size, ids_and_logprobs_equal=len(set(ident.values())) == 1,
               ms_per_step={arm: [round(x, 4) for x in v] for arm, v in ms.items()},
               median={arm: round(statistics.median(v), 4) for arm, v in ms.items()})
    if len(res) > 2:    # the last arm's alternatives: how often rank 0 is the token the sampler chose
        hit = sum(int((t[0][:, 0].long() == o[-t[0].size(0):]).sum()) for t, o in zip(res[2], res[0]))
        out["rank0_is_the_chosen_token"] = round(hit / sum(t[0].size(0) for t in res[2]), 4)
    print(json.dumps({shape: out}), flush=True)


def child(shape: str, arms, lib: str) -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", shape, "--prompt_len", str(a.prompt_len),
           "--max_new_tokens", str(a.max_new_tokens), "--repeats", str(a.repeats), "--arms", *arms]
    env = dict(os.environ, DUALHYP_HIP_LIB=str(Path(lib).resolve())) if lib else None
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout, env=env)      # a step that fails ends the tool
    if r.returncode != 0:
        sys.exit(f"shape {shape} ({'baseline library' if lib else 'this library'}) failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("{"):
            return json.loads(l)[shape]
    sys.exit(f"shape {shape}: the child printed no result")


def main() -> None:
    if a.worker:
        worker(a.worker)
        return
    res = dict(tool="bench_top_logprobs", prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats,
               baseline_lib=bool(a.baseline_lib), shapes={})
    for shape in a.shapes:
        s = child(shape, list(ARMS), "")
        base = s["median"]["lp"]
        if a.baseline_lib:
            b = child(shape, ["lp"], a.baseline_lib)
            s["baseline_lib_ms_per_step_lp"] = b["ms_per_step"]["lp"]
            s["baseline_lib_median_lp"] = base = b["median"]["lp"]
        for arm in ("k1", "k8"):
            s[f"added_us_per_step_{arm}"] = round((s["median"][arm] - base) * 1e3, 1)
            s[f"added_percent_{arm}"] = round((s["median"][arm] / base - 1) * 100, 2)
        res["shapes"][shape] = s
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
