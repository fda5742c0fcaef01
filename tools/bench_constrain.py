#!/usr/bin/env python3
"""What a token mask costs (GPU box): python tools/bench_constrain.py [--out profiles/constrain.json]

Two measurements, each in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

"sampler": the sampling launch alone (dh_sample_bf16 / dh_sample_bf16_mask) at 32 and 640 rows of vocabulary 32 000, for top_k = 1
(the serving path's arg-max) and top_k = 50.  --launches launches are captured into one graph (so the figure is the kernels', not
the Python wrapper's), the graph is replayed once to warm up and --repeats times under HIP events, with and without a mask in
alternation; the figure is microseconds per launch, median over the repeats.  The mask is a random half of the vocabulary per row;
the logits are Gaussian rows.

"step": a 640-row decode step of the TinyLlama shape (hash weights + LoRA r16, vocab 32 000) through generate_batch, greedy, no EOS,
--prompt_len-token prompts, --max_new_tokens new tokens: the call's own HIP-event decode time divided by its decode steps, with
token_mask (each utterance's own prompt ids, constrain.allowed_from_prompts, the serving path's --constrain prompt) and without,
in alternation after a warm-up of both arms; median over --repeats.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--what", nargs="+", default=["sampler", "step"], choices=["sampler", "step"])
ap.add_argument("--rows", nargs="+", type=int, default=[32, 640], help="row counts of the sampler measurement")
ap.add_argument("--step_rows", type=int, default=640)
ap.add_argument("--vocab", type=int, default=32000)
ap.add_argument("--launches", type=int, default=50, help="sampling launches per captured graph")
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the measurement of this run")
a = ap.parse_args()


def sampler_worker() -> dict:
    import torch
    from dualhyp_amd import constrain, ops
    dev = "cuda:0"
    V = a.vocab
    out = {}
    for rows in a.rows:
        g = torch.Generator().manual_seed(rows)
        logits = (torch.randn((rows, V), generator=g) * 4).to(torch.bfloat16).to(dev)
        half = torch.rand((rows, V), generator=g) < 0.5
        mask = constrain.pack_mask([torch.nonzero(r).reshape(-1) for r in half], V, dev)
        tok_ld = a.launches * (a.repeats + 1) + 1
        for top_k in (1, 50):
            arms = {}
            for arm, mk in (("plain", None), ("mask", mask)):
                tokens = torch.zeros((rows, tok_ld), dtype=torch.int64, device=dev)
                length = torch.zeros(rows, dtype=torch.int32, device=dev)
                done = torch.zeros(rows, dtype=torch.int32, device=dev)
                ops.sample(logits, tokens, length, done, temperature=0.8, top_k=top_k, seed=1, step=0, mask=mk)     # loads the kernel
                length.zero_()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for s in range(a.launches):
                        ops.sample(logits, tokens, length, done, temperature=0.8, top_k=top_k, seed=1, step=s, mask=mk)
                length.zero_()
                arms[arm] = (graph, tokens, length, done)
            us = {arm: [] for arm in arms}
            for rep in range(a.repeats + 1):
                for arm, (graph, tokens, length, done) in arms.items():
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    graph.replay()
                    ev[1].record()
                    torch.cuda.synchronize()
                    if rep:                                   # the first replay warms up
                        us[arm].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.launches)
            for arm, (graph, tokens, length, done) in arms.items():
                assert int(length.min()) == int(length.max()) == a.launches * (a.repeats + 1) and not bool(done.any())
            allowed = half.to(dev)
            picked = arms["mask"][1][:, :a.launches]
            assert bool(allowed.gather(1, picked).all()), "a masked launch picked a disallowed id"
            med = {arm: statistics.median(v) for arm, v in us.items()}
            out[f"rows{rows}_topk{top_k}"] = dict(us_per_launch={arm: [round(x, 2) for x in v] for arm, v in us.items()},
                                                  median_us={arm: round(x, 2) for arm, x in med.items()},
                                                  added_us=round(med["mask"] - med["plain"], 2),
                                                  added_percent=round((med["mask"] / med["plain"] - 1) * 100, 1))
    return out


def step_worker() -> dict:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, constrain, generate_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    rows = a.step_rows
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    V = cfg.padded_vocab_size
    corpus = [p.to(dev) for p in synth_prompts(rows, a.prompt_len, V, seed=7)]
    mask = constrain.pack_mask(constrain.allowed_from_prompts([p.cpu() for p in corpus], None), V, dev)
    allowed = constrain.unpack_mask(mask, V)
    kw = dict(temperature=0.2, top_k=1, prefill_batch=32)

    def call(arm):
        tm = {}
        out = generate_batch(m, corpus, a.max_new_tokens, timing=tm, token_mask=mask if arm == "mask" else None, **kw)
        return out, tm["decode_ms"] / tm["decode_steps"]

    for arm in ("plain", "mask"):                             # warm-up of both arms: allocation, graph capture
        out, _ = call(arm)
    gen = torch.stack([o[a.prompt_len:] for o in out])
    assert bool(allowed.gather(1, gen).all()), "the masked call produced a disallowed id"
    ms = {"plain": [], "mask": []}
    for _ in range(a.repeats):
        for arm in ms:
            ms[arm].append(call(arm)[1])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    return dict(rows=rows, vocab=V, allowed_ids_per_row_mean=round(float(allowed.sum(1).float().mean()), 1),
                ms_per_step={arm: [round(x, 4) for x in v] for arm, v in ms.items()},
                median_ms={arm: round(x, 4) for arm, x in med.items()},
                added_us_per_step=round((med["mask"] - med["plain"]) * 1e3, 1),
                added_percent=round((med["mask"] / med["plain"] - 1) * 100, 2))


def child(what: str) -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", what, "--rows", *map(str, a.rows), "--step_rows", str(a.step_rows),
           "--vocab", str(a.vocab), "--launches", str(a.launches), "--prompt_len", str(a.prompt_len), "--max_new_tokens",
           str(a.max_new_tokens), "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a step that fails ends the tool
    if r.returncode != 0:
        sys.exit(f"{what} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("{"):
            return json.loads(l)
    sys.exit(f"{what}: the child printed no result")


def main() -> None:
    if a.worker:
        print(json.dumps(sampler_worker() if a.worker == "sampler" else step_worker()), flush=True)
        return
    res = dict(tool="bench_constrain", vocab=a.vocab, launches=a.launches, prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens,
               repeats=a.repeats)
    for what in a.what:
        res[what] = child(what)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
