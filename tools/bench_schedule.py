#!/usr/bin/env python3
"""The two schedules of the inference harness on one synthetic corpus, one GPU: `batch` (generate_batch, --decode_batch
utterances at a time, each batch stepped until its last sequence has finished) against `continuous` (generate_stream: finished
rows retire, their KV slots are refilled).  TinyLlama shape, hash weights + LoRA r16, ragged prompts, greedy, up to 150 new tokens.

The weights tie the head to the embedding through a successor permutation (dualhyp_amd.synth, head_tie), so a greedy
continuation walks a chain of tokens.  The EOS id and the lengths come from an EOS-free run of one utterance: the EOS is the
last token of its chain, and a prompt that ends on the chain's token k places before it produces k tokens.  80 % of the
utterances get a correction of 20-40 tokens, 10 % anything up to the budget, 10 % never meet the EOS and run to the budget
(each step reports the lengths it has actually seen).  Prints one JSON line per schedule: utterances
per second (second, warm run of the corpus), decode_row_steps, and a digest of the returned ids, which must be equal.

Every GPU step is a child process of its own under a time limit; the parent never touches the GPU.

    python tools/bench_schedule.py [--utterances 1280] [--decode_batch 640] [--max_new_tokens 150]
"""
import argparse
import hashlib
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=1280)
ap.add_argument("--decode_batch", type=int, default=640)
ap.add_argument("--prefill_batch", type=int, default=64)
ap.add_argument("--max_new_tokens", type=int, default=150)
ap.add_argument("--lo", type=int, default=200, help="shortest prompt")
ap.add_argument("--hi", type=int, default=600, help="longest prompt")
ap.add_argument("--chain", type=str, default="", help="(workers) JSON file with the probe's token chain")
ap.add_argument("--step_timeout", type=int, default=240, help="seconds each GPU step may take")
ap.add_argument("--worker", choices=("probe", "batch", "continuous"), default=None)
ap.add_argument("--eos", type=int, default=-1)
a = ap.parse_args()


def worker() -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, generate_batch, generate_stream
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    V, new = cfg.padded_vocab_size, a.max_new_tokens
    corpus = [p.to(dev) for p in synth_prompts(a.utterances, 0, V, seed=7, ragged=True, lo=a.lo, hi=a.hi)]
    kw = dict(temperature=0.2, top_k=1)
    if a.worker == "probe":
        free = generate_batch(m, corpus[:1], new, **kw)[0]
        chain = free[corpus[0].numel() - 1:].tolist()          # the prompt's last token and the `new` tokens behind it
        print(json.dumps(dict(step="probe", eos=chain[-1], chain=chain, distinct=len(set(chain)))), flush=True)
        return
    chain = json.loads(Path(a.chain).read_text())
    assert chain[-1] == a.eos and len(chain) == new + 1
    import random
    rnd = random.Random(11)
    for p in corpus:
        r = rnd.random()
        want = rnd.randint(20, 40) if r < 0.8 else (rnd.randint(1, new) if r < 0.9 else 0)     # 0: left as drawn
        if want:
            p[-1] = chain[new - min(want, new)]

    def run(timing):
        if a.worker == "batch":        # what the harness does: --decode_batch utterances per generate_batch call
            out = []
            for b in range(0, len(corpus), a.decode_batch):
                out += [o.clone() for o in generate_batch(m, corpus[b:b + a.decode_batch], new, eos_id=a.eos,
                                                          prefill_batch=min(a.prefill_batch, a.decode_batch), timing=timing, **kw)]
            return out
        return generate_stream(m, corpus, new, eos_id=a.eos, max_rows=a.decode_batch,
                               prefill_batch=min(a.prefill_batch, a.decode_batch), timing=timing, **kw)

    run(None)                          # allocation + graph capture
    torch.cuda.synchronize()
    tm = {}
    t0 = time.perf_counter()
    out = run(tm)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    h = hashlib.sha256()
    for o in out:
        h.update(o.cpu().numpy().tobytes())
    made = sorted(o.numel() - p.numel() for o, p in zip(out, corpus))
    n_new = sum(made)
    print(json.dumps(dict(schedule=a.worker, utterances=len(corpus), decode_batch=a.decode_batch, max_new_tokens=new, eos=a.eos,
                          wall_s=round(dt, 3), utt_per_s=round(len(corpus) / dt, 1), prefill_ms=round(tm["prefill_ms"], 1),
                          decode_ms=round(tm["decode_ms"], 1), decode_steps=tm["decode_steps"], decode_row_steps=tm["decode_row_steps"],
                          launch_rows=sorted(tm.get("launch_rows", {a.decode_batch})), mean_new_tokens=round(n_new / len(corpus), 1),
                          new_tokens_p10_p50_p90_max=[made[len(made) // 10], made[len(made) // 2], made[9 * len(made) // 10], made[-1]],
                          ids_sha256=h.hexdigest()[:16])), flush=True)


def step(name: str, eos: int, chain: str = "") -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", name, "--eos", str(eos), "--chain", chain]
    for k in ("utterances", "decode_batch", "prefill_batch", "max_new_tokens", "lo", "hi"):
        cmd += [f"--{k}", str(getattr(a, k))]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a step that fails ends the tool
    if r.returncode != 0:
        sys.exit(f"step {name} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    print(json.dumps({k: v for k, v in out.items() if k != "chain"}), flush=True)
    return out


if a.worker:
    worker()
else:
    import tempfile
    probe = step("probe", -1)
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "chain.json").write_text(json.dumps(probe["chain"]))
        res = [step(s, probe["eos"], str(Path(tmp) / "chain.json")) for s in ("batch", "continuous")]
    assert res[0]["ids_sha256"] == res[1]["ids_sha256"], "the two schedules returned different ids"
    print(json.dumps(dict(continuous_over_batch_utt_per_s=round(res[1]["utt_per_s"] / res[0]["utt_per_s"], 3),
                          row_steps_ratio=round(res[1]["decode_row_steps"] / res[0]["decode_row_steps"], 3))))
