#!/usr/bin/env python3
"""Beam search (beam_search_batch) against greedy generate_batch at the SAME decode row count, one GPU: TinyLlama shape, hash weights +
LoRA r16, prompts of 512 tokens, 64 new tokens, no EOS.

Per W in --beams and per utterance count (32, and 640 // W), in one child process each: a warm-up call of either kind (allocation,
graph capture), then --repeats alternating pairs of calls — beam search over n utterances x W beams, greedy decoding of n * W
prompts — and the median of each kind's own HIP-event decode time, in ms per step.  The difference is what a beam step adds to a
greedy step over the same rows: the selection (2 W alternatives per row instead of an arg-max, plus the merge) and the KV
re-parenting.  The selection is also timed alone (ops.beam_select on the step's rows x vocab of random logits, beside ops.sample with
top_k = 1 on the same rows); "reparent_prep_us_remainder" is difference - (selection - greedy
sampler): a subtraction remainder that holds the prep kernel and the two copy launches, not an event time of them.  Also reported: the
share of step rows that continued their own beam and skipped the copy, and the bytes dh_engine_reserve_beams added to the engine.

The parent never touches the GPU and prints ONE JSON line.

    python tools/bench_beam.py [--beams 1 2 4] [--out profiles/beam_search.json]
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
ap.add_argument("--beams", type=int, nargs="+", default=[1, 2, 4])
ap.add_argument("--utterances", type=int, default=32, help="the small arm; the large one is --rows // W")
ap.add_argument("--rows", type=int, default=640)
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--prefill_batch", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=420, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=int, nargs=2, default=None, metavar=("W", "N"), help="(child) beams and utterances of this run")
a = ap.parse_args()


def event_us(fn, n=20):
    import torch
    fn()
    evs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return statistics.median(x.elapsed_time(y) for x, y in evs) * 1e3


def worker(W: int, n: int) -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, beam_search_batch, generate_batch, ops
    from dualhyp_amd.beam import BeamState
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    rows, new, V = n * W, a.max_new_tokens, cfg.padded_vocab_size
    corpus = [p.to(dev) for p in synth_prompts(rows, a.prompt_len, V, seed=7)]
    beam = lambda tm=None: beam_search_batch(m, corpus[:n], new, num_beams=W, prefill_batch=a.prefill_batch, timing=tm)
    greedy = lambda tm=None: generate_batch(m, corpus, new, temperature=0.2, top_k=1, prefill_batch=a.prefill_batch, timing=tm)
    # the engine is sized by the first call and kept: the beam call needs one position more, so it goes first
    beam()
    bytes_with = m._engine.lib.dh_engine_device_bytes(m._engine.handle)
    greedy()
    tb, tg = [], []
    for _ in range(a.repeats):
        tm = {}
        beam(tm)
        tb.append(tm)
        tm = {}
        greedy(tm)
        tg.append(tm)
    steps = new - 1
    b_ms = statistics.median(t["decode_ms"] for t in tb) / steps
    g_ms = statistics.median(t["decode_ms"] for t in tg) / steps
    # the selection and the greedy sampler alone, on the step's rows
    logits = (torch.randn((rows, V), device=dev) * 4).to(torch.bfloat16)
    st = BeamState(n, W, new, dev)

    def select():
        st.done.zero_()
        ops.beam_select(logits, st, rows_per_utt=W, step=1)

    tokens = torch.zeros((rows, 8), dtype=torch.int64, device=dev)
    length = torch.ones(rows, dtype=torch.int32, device=dev)
    done = torch.zeros(rows, dtype=torch.int32, device=dev)

    def sample():
        length.fill_(1)
        done.zero_()
        ops.sample(logits, tokens, length, done, temperature=0.2, top_k=1)

    fill_us = event_us(lambda: (length.fill_(1), done.zero_()))
    sel_us = event_us(select) - event_us(lambda: st.done.zero_())
    smp_us = event_us(sample) - fill_us
    added_us = (b_ms - g_ms) * 1e3
    m.refresh_engine()
    torch.cuda.synchronize()
    eng = m.engine(rows, a.prompt_len + new, max(rows, a.prefill_batch * a.prompt_len), exact=True)
    bytes_without = eng.lib.dh_engine_device_bytes(eng.handle)
    eng.reserve_beams(W, new)
    scratch = eng.lib.dh_engine_device_bytes(eng.handle) - bytes_without
    t = tb[-1]
    print(json.dumps(dict(W=W, utterances=n, rows=rows, steps=steps, beam_ms_per_step=round(b_ms, 4), greedy_ms_per_step=round(g_ms, 4),
                          beam_decode_ms=[round(x["decode_ms"], 3) for x in tb], greedy_decode_ms=[round(x["decode_ms"], 3) for x in tg],
                          added_us_per_step=round(added_us, 1), select_us=round(sel_us, 1), greedy_sampler_us=round(smp_us, 1),
                          reparent_prep_us_remainder=round(added_us - (sel_us - smp_us), 1),
                          rows_skipping_copy_share=round(1 - t["beam_copied_rows"] / max(t["beam_step_rows"], 1), 4),
                          reserve_beams_bytes=int(scratch), engine_bytes=int(bytes_with))), flush=True)


if a.worker is not None:
    worker(*a.worker)
else:
    line = dict(tool="bench_beam", prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats, runs=[])
    for W in a.beams:
        for n in sorted({a.utterances, max(1, a.rows // W)}):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(W), str(n)]
            for k in ("prompt_len", "max_new_tokens", "prefill_batch", "repeats"):
                cmd += [f"--{k}", str(getattr(a, k))]
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a run that fails ends the tool
            if r.returncode != 0:
                sys.exit(f"run W={W} utterances={n} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            line["runs"] += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print(json.dumps(line), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + "\n")
