#!/usr/bin/env python3
"""What contextual biasing costs in the sampling kernel (GPU box):
python tools/bench_bias.py [--parent_lib OTHER.so] [--out profiles/bias.json]

One measurement in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

The sampling kernel alone (ops.sample on [rows, vocab] bf16 logits, Gaussian rows of sigma 4, temperature 0.8) on the TinyLlama
vocabulary (32 000) at 640 rows and the Llama-3 vocabulary (128 256) at 128 rows, for the arg-max (top_k 1) and for top_k 40 with
top_p 0.9, in arms run in alternation in one process: bias off, 16 entries of 3 ids, and 256 entries of 8 ids (random ids,
boost 4; every sequence has generated 16 tokens, the last two of which begin one of the entries, so proposals at depth 0, 1 and 2 are
made).  Microseconds per launch, the median and the minimum over --rounds rounds of --launches launches between two events.  With
--parent_lib the other library's dh_sample_bf16_nucleus is a fourth arm of the same alternation (bound beside this build's in the
same process): the bias-off launch of the parent commit, the same-box noise band of "off".  The builder of the overridden columns
is shared with the penalties, so the penalties alone (1.2, 0.5, 0.5 over the same 16 generated tokens) are an arm too, and with
--parent_lib the parent's dh_sample_bf16_penalty beside it.  Nothing is gated.
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
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the bias-off path with")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds the child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", action="store_true", help="(child) the measurement")
a = ap.parse_args()

SAMPLERS = {"argmax": dict(temperature=0.8, top_k=1), "top40_p0.9": dict(temperature=0.8, top_k=40, top_p=0.9)}
SHAPES = ((32000, 640), (128256, 128))          # (vocab, rows)
TABLES = {"on_16x3": (16, 3), "on_256x8": (256, 8)}
PEN = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5)
BOOST = 4.0
GENERATED = 16


def summary(v):
    return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "rounds": [round(x, 3) for x in v]}


def worker() -> dict:
    import ctypes as C
    import torch
    from dualhyp_amd import _lib, ops
    from dualhyp_amd.bias import compile_bias
    dev = "cuda:0"
    other = None
    if a.parent_lib:
        other = C.CDLL(a.parent_lib)
        other.dh_sample_bf16_nucleus.restype, other.dh_sample_bf16_nucleus.argtypes = _lib.SIGNATURES["dh_sample_bf16_nucleus"]
        other.dh_sample_bf16_penalty.restype, other.dh_sample_bf16_penalty.argtypes = _lib.SIGNATURES["dh_sample_bf16_penalty"]
    pen_args = _lib.PenaltyArgs(PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"])
    res = {}
    tok_ld, at = 128, 100
    for vocab, rows in SHAPES:
        g = torch.Generator().manual_seed(vocab)
        lg = (torch.randn((rows, vocab), generator=g) * 4.0).to(torch.bfloat16).to(dev)
        tokens = torch.randint(0, vocab, (rows, tok_ld), generator=g, dtype=torch.int64)
        specs = {}
        for name, (n, L) in TABLES.items():
            ids = torch.randint(0, vocab, (n, L), generator=g)
            specs[name] = compile_bias([(row.tolist(), BOOST) for row in ids], vocab, dev)
        first = specs["on_256x8"].entries
        for r in range(rows):                               # every sequence ends on the first two ids of an entry of the large table
            tokens[r, at - 2:at] = torch.tensor(first[r % len(first)][0][:2])
        tokens = tokens.to(dev)
        length = torch.empty(rows, dtype=torch.int32, device=dev)
        done = torch.zeros(rows, dtype=torch.int32, device=dev)
        start = torch.full((rows,), at - GENERATED, dtype=torch.int32, device=dev)
        for sname, skw in SAMPLERS.items():
            def this_build(kw):
                def launch(step):
                    length.fill_(at)
                    ops.sample(lg, tokens, length, done, seed=11, step=step, **skw, **kw)
                return launch

            def parent_build(step):
                length.fill_(at)
                rc = other.dh_sample_bf16_nucleus(lg.data_ptr(), vocab, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(), rows,
                                                  skw["temperature"], skw["top_k"], -1, 11, step, torch.cuda.current_stream().cuda_stream,
                                                  None, 0, None, None, None, 0, 0, None, None, skw.get("top_p", 1.0), 0.0)
                assert rc == 0

            def parent_pen(step):
                length.fill_(at)
                rc = other.dh_sample_bf16_penalty(lg.data_ptr(), vocab, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(), rows,
                                                  skw["temperature"], skw["top_k"], -1, 11, step, torch.cuda.current_stream().cuda_stream,
                                                  None, 0, None, None, None, 0, 0, start.data_ptr(), None, skw.get("top_p", 1.0), 0.0,
                                                  C.byref(pen_args))
                assert rc == 0

            arms = [("off", this_build({}))] + [(name, this_build(dict(bias=spec, start=start))) for name, spec in specs.items()]
            arms.append(("penalties", this_build(dict(PEN, start=start))))
            if other:
                arms += [("parent_off", parent_build), ("parent_penalties", parent_pen)]
            picks = {}
            for name, launch in arms:                      # warm-up, and the picks of step 0
                launch(0)
                torch.cuda.synchronize()
                picks[name] = tokens[:, at].clone()
            times = {name: [] for name, _ in arms}
            for _ in range(a.rounds):
                for name, launch in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.launches):
                        launch(i)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
            # the fill of `length` rides in every arm alike
            entry = {name: summary(us) for name, us in times.items()}
            off = entry["off"]["median_us"]
            entry["on_over_off_percent"] = {name: round((entry[name]["median_us"] / off - 1) * 100, 2) for name in TABLES}
            entry["picks_that_differ_from_off"] = {name: int((picks["off"] != picks[name]).sum()) for name in TABLES}
            if other:
                entry["off_equals_parent_picks"] = bool(torch.equal(picks["off"], picks["parent_off"]))
                entry["off_over_parent_percent"] = round((off / entry["parent_off"]["median_us"] - 1) * 100, 2)
                entry["penalties_equal_parent_picks"] = bool(torch.equal(picks["penalties"], picks["parent_penalties"]))
                entry["penalties_over_parent_percent"] = round(
                    (entry["penalties"]["median_us"] / entry["parent_penalties"]["median_us"] - 1) * 100, 2)
            res[f"vocab{vocab}_rows{rows}_{sname}"] = entry
    return res


def child() -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--launches", str(a.launches), "--rounds", str(a.rounds)]
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
    res = dict(tool="bench_bias", samplers=SAMPLERS, shapes=SHAPES, tables=TABLES, boost=BOOST, generated=GENERATED, launches=a.launches,
               rounds=a.rounds, kernel=child())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
