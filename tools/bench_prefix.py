#!/usr/bin/env python3
"""Prefix sharing (share_prefix of generate_batch / generate_stream) against the unshared call, one GPU: TinyLlama shape, hash
weights + LoRA r16, 640 prompts of 512 tokens whose first --shared tokens are the same (default: a run with 64, then one with
256), 64 new tokens, greedy, no EOS.

Per run and schedule, in ONE process on one box: a warm-up call of each variant (allocation, graph capture), then three timed
regions of each, alternating off / on; the line gives every region and the median.  A region is one whole call between two device
synchronisations (host clock); prefill_ms is the call's own HIP-event figure.  The ids of the two variants must be equal (digest).
The prefix forward + copy and the copy alone are timed with HIP events in front of that, five launches each after a warm-up; the
copy's bytes are what the algorithm moves (the source read once, every destination written once) against 8 TB/s.

Every GPU run is a child process of its own under a time limit; the parent never touches the GPU.

    python tools/bench_prefix.py [--shared 64 256] [--utterances 640] [--out profiles/prefix.json]
"""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--shared", type=int, nargs="+", default=[64, 256], help="leading tokens the prompts have in common, one run each")
ap.add_argument("--utterances", type=int, default=640)
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--prefill_batch", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=420, help="seconds each GPU run may take")
ap.add_argument("--out", type=str, default="", help="write the lines as one JSON file")
ap.add_argument("--worker", type=int, default=None, help="(child) the shared length of this run")
a = ap.parse_args()
HBM_BYTES_PER_S = 8e12


def digest(outs) -> str:
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def worker(shared: int) -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, generate_batch, generate_stream
    from dualhyp_amd.generate import _forward_prefix
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    N, T, new = a.utterances, a.prompt_len, a.max_new_tokens
    corpus = [p.to(dev) for p in synth_prompts(N, T, cfg.padded_vocab_size, seed=7)]
    for p in corpus[1:]:
        p[:shared] = corpus[0][:shared]
    kw = dict(temperature=0.2, top_k=1)
    calls = {"generate_batch": lambda share, tm: generate_batch(m, corpus, new, prefill_batch=a.prefill_batch, share_prefix=share, timing=tm, **kw),
             "generate_stream": lambda share, tm: generate_stream(m, corpus, new, max_rows=N, prefill_batch=a.prefill_batch,
                                                                 share_prefix=share, timing=tm, **kw)}
    for name, call in calls.items():
        ids = {}
        for share in (False, True):                       # warm-up: allocation, graph capture, code objects of both variants
            ids[share] = digest(call(share, None))
        torch.cuda.synchronize()
        assert ids[False] == ids[True], f"{name}: the ids with a shared prefix differ"
        if name == "generate_batch":                      # the engine of the call above: the prefix forward and the copy by themselves
            eng, P = m._engine, shared // 32 * 32
            L, G, hs = cfg.n_layer, cfg.n_query_groups, cfg.head_size

            def events(fn, n=5):
                fn()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                for e0, e1 in ev:
                    e0.record()
                    fn()
                    e1.record()
                torch.cuda.synchronize()
                return sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            both = events(lambda: _forward_prefix(eng, corpus[0], P, 0, range(1, N)))
            copy = events(lambda: eng.copy_prefix(0, list(range(1, N)), P))
            moved = 2 * L * G * P * hs * 2 * N            # K and V^T, bf16: one read of the source + N - 1 writes
            rate = moved / (statistics.median(copy) * 1e-3)
            print(json.dumps(dict(step="prefix_forward_and_copy", shared=shared, P=P, destinations=N - 1, forward_plus_copy_ms=[round(x, 4) for x in both],
                                  copy_ms=[round(x, 4) for x in copy], copy_bytes=moved, copy_TB_per_s=round(rate / 1e12, 3),
                                  copy_share_of_8TBps=round(rate / HBM_BYTES_PER_S, 3))), flush=True)
        runs = {False: [], True: []}
        for _ in range(a.repeats):
            for share in (False, True):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(share, tm)
                torch.cuda.synchronize()
                runs[share].append((time.perf_counter() - t0, tm))
        line = dict(step=name, shared=shared, utterances=N, prompt_len=T, max_new_tokens=new, ids_sha256=ids[True])
        for share, tag in ((False, "off"), (True, "on")):
            walls = [w for w, _ in runs[share]]
            tm = runs[share][walls.index(statistics.median(walls))][1]
            line[tag] = dict(utt_per_s=round(N / statistics.median(walls), 1), utt_per_s_regions=[round(N / w, 1) for w in walls],
                             prefill_ms=round(tm["prefill_ms"], 2), prefill_ms_regions=[round(t["prefill_ms"], 2) for _, t in runs[share]],
                             decode_ms=round(tm["decode_ms"], 2), prefill_tokens=tm["prefill_tokens"], shared_prefix=tm["shared_prefix"])
        line["on_over_off_utt_per_s"] = round(line["on"]["utt_per_s"] / line["off"]["utt_per_s"], 4)
        line["on_over_off_prefill_ms"] = round(line["on"]["prefill_ms"] / line["off"]["prefill_ms"], 4)
        print(json.dumps(line), flush=True)


if a.worker is not None:
    worker(a.worker)
else:
    lines = []
    for shared in a.shared:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(shared)]
        for k in ("utterances", "prompt_len", "max_new_tokens", "prefill_batch", "repeats"):
            cmd += [f"--{k}", str(getattr(a, k))]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a run that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"run --shared {shared} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                print(l, flush=True)
                lines.append(json.loads(l))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(lines, indent=1) + "\n")
