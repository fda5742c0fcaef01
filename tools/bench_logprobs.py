#!/usr/bin/env python3
"""What return_logprobs costs a decode step (GPU box): python tools/bench_logprobs.py [--out profiles/logprobs.json]

generate_batch with and without return_logprobs in one process per shape: TinyLlama (hash weights + LoRA r16, vocab 32 000) at 32 and
640 rows, and the same decoder with a 128 256-entry vocabulary (Llama-3's) at 32 rows — the head and the sampling tail are what the
vocabulary changes.  Prompts of --prompt_len tokens, --max_new_tokens new tokens, greedy, no EOS.  After a warm-up call of each arm
(allocation, graph capture), --repeats alternating timed calls; the figure is the call's own HIP-event decode time divided by its
decode steps (ms per token and row set), median over the repeats, and the difference of the arms.  The ids of the two arms must be
equal (digest).  Every shape is a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.
"""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"tinyllama_32": (32, None), "tinyllama_640": (640, None), "vocab128256_32": (32, 128256)}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the shape of this run")
a = ap.parse_args()


def digest(outs) -> str:
    h = hashlib.sha256()
    for o in outs:
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

    def call(flag):
        tm = {}
        res = generate_batch(m, corpus, a.max_new_tokens, timing=tm, return_logprobs=flag, **kw)
        outs = res[0] if flag else res
        return digest(outs), tm["decode_ms"] / tm["decode_steps"], (res[1] if flag else None)

    ident = {flag: call(flag)[0] for flag in (False, True)}          # warm-up of both arms
    ms = {False: [], True: []}
    for _ in range(a.repeats):
        for flag in (False, True):
            d, t, lp = call(flag)
            assert d == ident[flag]
            ms[flag].append(t)
    mean_lp = float(torch.cat(lp).double().mean())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps({shape: dict(rows=rows, vocab=cfg.padded_vocab_size, ids_equal=ident[False] == ident[True],
                                  ms_per_step_off=[round(x, 4) for x in ms[False]], ms_per_step_on=[round(x, 4) for x in ms[True]],
                                  median_off=round(off, 4), median_on=round(on, 4), added_us_per_step=round((on - off) * 1e3, 1),
                                  added_percent=round((on / off - 1) * 100, 2), mean_logprob=round(mean_lp, 4))}), flush=True)


def main() -> None:
    if a.worker:
        worker(a.worker)
        return
    res = dict(tool="bench_logprobs", prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats, shapes={})
    for shape in a.shapes:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", shape, "--prompt_len", str(a.prompt_len),
               "--max_new_tokens", str(a.max_new_tokens), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a step that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"shape {shape} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                res["shapes"].update(json.loads(l))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
