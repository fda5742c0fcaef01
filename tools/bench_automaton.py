#!/usr/bin/env python3
"""What an automaton constraint costs in the sampling kernel (GPU box):
python tools/bench_automaton.py [--parent_lib OTHER.so] [--out profiles/automaton.json]

One measurement in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

The sampling kernel alone (ops.sample on [640, vocab] bf16 logits, Gaussian rows of sigma 4, temperature 0.8) on the TinyLlama
vocabulary (32 000) and the Llama-3 vocabulary (128 256), for the arg-max (top_k 1) and for top_k 40, in arms run in alternation in one
process: the order-2 chain automaton of 512-token random prompts (every sequence has generated 16 tokens and sits in the state of a
prompt token, so its row holds that token's followers and the EOS), a token mask alone (the ids of the prompt), no_repeat_ngram = 2
alone and the penalties alone (1.2, 0.5, 0.5) over the same 16 generated tokens.  With --parent_lib the other library's
dh_sample_bf16_mask, dh_sample_bf16_ngram and dh_sample_bf16_penalty are arms of the same alternation (bound beside this build's in the
same process): the parent commit's launches, whose spread over the rounds is the same-box noise band, and against which this build's
history-family launches are re-timed.  Microseconds per launch, the median and the minimum over --rounds rounds of --launches launches
between two events, and the automaton launch as a share of a 640-row decode step of --step_ms milliseconds.  Nothing is gated.

An arm's --launches launches are captured once into a graph and a round replays it, as the engine's decode steps replay theirs: the
events then bracket device time alone.  The exported entry checks the whole set's host copies on every call (a million edges here), which
a captured step pays once, when the set is set; --eager times the calls as they are issued instead, that host work included.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=50, help="kernel launches between two events")
ap.add_argument("--rounds", type=int, default=7, help="rounds per arm")
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the existing launches with")
ap.add_argument("--step_ms", type=float, default=4.5, help="a 640-row TinyLlama decode step, for the share (README: 4.45-4.52 ms)")
ap.add_argument("--eager", action="store_true", help="issue every launch from the host inside the timed region (host checks included)")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds the child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", action="store_true", help="(child) the measurement")
a = ap.parse_args()

SAMPLERS = {"argmax": dict(temperature=0.8, top_k=1), "top40": dict(temperature=0.8, top_k=40)}
VOCABS = (32000, 128256)
ROWS = 640
PROMPT = 512
PEN = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5)
GENERATED = 16
ORDER = 2


def summary(v):
    return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
            "rounds": [round(x, 3) for x in v]}


def worker() -> dict:
    import ctypes as C
    import torch
    from dualhyp_amd import _lib, ops
    from dualhyp_amd.automaton import from_prompts, walk
    from dualhyp_amd.constrain import pack_mask
    dev = "cuda:0"
    other = None
    if a.parent_lib:
        other = C.CDLL(a.parent_lib)
        for name in ("dh_sample_bf16_mask", "dh_sample_bf16_ngram", "dh_sample_bf16_penalty"):
            getattr(other, name).restype, getattr(other, name).argtypes = _lib.SIGNATURES[name]
    pen_args = _lib.PenaltyArgs(PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"])
    res = {}
    tok_ld, at = 128, 100
    for vocab in VOCABS:
        g = torch.Generator().manual_seed(vocab)
        lg = (torch.randn((ROWS, vocab), generator=g) * 4.0).to(torch.bfloat16).to(dev)
        eos = vocab - 1
        prompts = torch.randint(0, vocab - 1, (ROWS, PROMPT), generator=g).tolist()
        tokens = torch.randint(0, vocab - 1, (ROWS, tok_ld), generator=g, dtype=torch.int64)
        aset = from_prompts(prompts, order=ORDER, eos_id=eos)
        for r in range(ROWS):                               # the generated text is a run of the prompt: the state is a prompt token's
            tokens[r, at - GENERATED:at] = torch.tensor(prompts[r][7:7 + GENERATED])
        states = [walk(aset, r, prompts[r][7:7 + GENERATED])[-1] for r in range(ROWS)]
        aset = aset.to(dev)
        first_state = torch.tensor(states, dtype=torch.int32, device=dev)
        mask = pack_mask([sorted(set(p)) + [eos] for p in prompts], vocab, dev)
        tokens = tokens.to(dev)
        length = torch.empty(ROWS, dtype=torch.int32, device=dev)
        done = torch.zeros(ROWS, dtype=torch.int32, device=dev)
        start = torch.full((ROWS,), at - GENERATED, dtype=torch.int32, device=dev)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        for sname, skw in SAMPLERS.items():
            def this_build(kw, reset_state=False):
                def launch(step):
                    length.fill_(at)
                    if reset_state:
                        aset.state.copy_(first_state)      # rides in the automaton arm only: a 2.5 KB device copy
                    ops.sample(lg, tokens, length, done, seed=11, step=step, eos_id=eos, **skw, **kw)
                    done.zero_()
                return launch

            def parent(entry, *tail):
                def launch(step):
                    length.fill_(at)
                    rc = getattr(other, entry)(lg.data_ptr(), vocab, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(), ROWS,
                                               skw["temperature"], skw["top_k"], eos, 11, step, stream(), None, 0, None, None, *tail)
                    assert rc == 0
                    done.zero_()
                return launch

            arms = [("automaton", this_build(dict(automaton=aset, start=start), reset_state=True)),
                    ("mask", this_build(dict(mask=mask))),
                    ("ngram", this_build(dict(no_repeat_ngram=2, start=start))),
                    ("penalties", this_build(dict(PEN, start=start)))]
            if other:
                arms += [("parent_mask", parent("dh_sample_bf16_mask", mask.data_ptr(), mask.size(1))),
                         ("parent_ngram", parent("dh_sample_bf16_ngram", None, 0, 2, start.data_ptr())),
                         ("parent_penalties", parent("dh_sample_bf16_penalty", None, 0, 0, start.data_ptr(), None, 1.0, 0.0,
                                                     C.byref(pen_args)))]
            picks = {}
            for name, launch in arms:                      # warm-up, and the picks of step 0
                launch(0)
                torch.cuda.synchronize()
                picks[name] = tokens[:, at].clone()
            times = {name: [] for name, _ in arms}
            graphs = {}
            if not a.eager:
                for name, launch in arms:                  # the launches of a round, captured once (one stream: no parallel branch)
                    graphs[name] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[name]):
                        for i in range(a.launches):
                            launch(i)
                torch.cuda.synchronize()
            for _ in range(a.rounds):
                for name, launch in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if a.eager:
                        for i in range(a.launches):
                            launch(i)
                    else:
                        graphs[name].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
            # the fills of `length` and `done` ride in every arm alike
            entry = {name: summary(us) for name, us in times.items()}
            aut = entry["automaton"]["median_us"]
            entry["automaton_share_of_step_percent"] = round(aut / (a.step_ms * 1e3) * 100, 2)
            entry["automaton_over_percent"] = {name: round((aut / entry[name]["median_us"] - 1) * 100, 2) for name in ("mask", "ngram")}
            entry["mean_allowed_ids"] = round(sum(len(aset.edges(q)) for q in states[:64]) / 64, 2)
            if other:
                for name in ("mask", "ngram", "penalties"):
                    p = entry["parent_" + name]
                    entry[name + "_equals_parent_picks"] = bool(torch.equal(picks[name], picks["parent_" + name]))
                    entry[name + "_over_parent_percent"] = round((entry[name]["median_us"] / p["median_us"] - 1) * 100, 2)
                    entry["parent_" + name + "_spread_percent"] = round((p["max_us"] / p["min_us"] - 1) * 100, 2)
                entry["automaton_over_parent_percent"] = {name: round((aut / entry["parent_" + name]["median_us"] - 1) * 100, 2)
                                                          for name in ("mask", "ngram")}
            res[f"vocab{vocab}_rows{ROWS}_{sname}"] = entry
    return res


def child() -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--launches", str(a.launches), "--rounds", str(a.rounds),
           "--step_ms", str(a.step_ms)] + (["--eager"] if a.eager else [])
    if a.parent_lib:
        cmd += ["--parent_lib", str(Path(a.parent_lib).resolve())]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout, env=dict(os.environ))
    if r.returncode != 0:
        sys.exit(f"the measurement failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("{"):
            return json.loads(l)
    sys.exit("the child printed no result")


def main() -> None:
    if a.worker:
        print(json.dumps(worker()), flush=True)
        return
    res = dict(tool="bench_automaton", samplers=SAMPLERS, vocabs=VOCABS, rows=ROWS, prompt=PROMPT, order=ORDER, generated=GENERATED,
               step_ms=a.step_ms, launches=a.launches, rounds=a.rounds, timed="eager calls" if a.eager else "graph replays", kernel=child())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
