#!/usr/bin/env python3
"""What the repetition / frequency / presence penalties cost (GPU box):
python tools/bench_penalties.py [--parent_lib OTHER.so] [--out profiles/penalties.json]

Measurements, each in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

"kernel": the sampling kernel alone (ops.sample on [640, vocab] bf16 logits, Gaussian rows of sigma 4, temperature 0.8) on the
TinyLlama vocabulary (32 000) and the Llama-3 vocabulary (128 256), for the arg-max (top_k 1) and for top_k 40 with top_p 0.9, in
four arms run in alternation in one process: penalties off, and on (repetition 1.2, frequency 0.5, presence 0.5) with histories of 0,
16 and 64 generated tokens per sequence (random ids; `start` is set that far before the sequence's length).  Microseconds per launch,
the median and the minimum over --rounds rounds of --launches launches between two events.  With --parent_lib the other library's
dh_sample_bf16_nucleus is a fifth arm of the same alternation (bound beside this build's in the same process): the penalties-off
launch of the parent commit.

"step": a decode step of the TinyLlama shape (hash weights + LoRA r16) through the engine at 640 rows of --prompt_len tokens: the
prompts are prefilled once, then calls of --steps captured steps are timed between two events, the same samplers and arms in
alternation; a history of h tokens is the last h places before each sequence's length (it grows by one per step of a call, and
every call starts from the same state).  With --parent_lib the penalties-off step in children of their own, this build and the other
library in alternation (DUALHYP_HIP_LIB; a build of the parent commit has none of the feature's entries, so the child drops them from
the symbol table it binds), with a hash of the generated ids: the two must be equal.
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
ap.add_argument("--prompt_len", type=int, default=128)
ap.add_argument("--steps", type=int, default=8, help="captured decode steps per timed call")
ap.add_argument("--launches", type=int, default=50, help="kernel launches between two events")
ap.add_argument("--rounds", type=int, default=7, help="rounds per arm (kernel), calls per arm (step), children per library / 3 (step vs parent)")
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the penalties-off path with")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the measurement of this run")
a = ap.parse_args()

NEW_ENTRIES = ("dh_sample_bf16_penalty", "dh_sample_rows_bf16_penalty", "dh_engine_set_penalties")
ROWS = 640
SAMPLERS = {"argmax": dict(temperature=0.8, top_k=1), "top40_p0.9": dict(temperature=0.8, top_k=40, top_p=0.9)}
PEN = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5)
HISTORIES = (0, 16, 64)
VOCABS = (32000, 128256)


def summary(v, unit="us"):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), "rounds": [round(x, 3) for x in v]}


def growth(entry, unit):
    """on over off, percent, per history"""
    off = entry["off"][f"median_{unit}"]
    return {f"h{h}": round((entry[f"on_h{h}"][f"median_{unit}"] / off - 1) * 100, 2) for h in HISTORIES}


def kernel_worker() -> dict:
    import ctypes as C
    import torch
    from dualhyp_amd import _lib, ops
    dev = "cuda:0"
    other = None
    if a.parent_lib:
        other = C.CDLL(a.parent_lib)
        other.dh_sample_bf16_nucleus.restype, other.dh_sample_bf16_nucleus.argtypes = _lib.SIGNATURES["dh_sample_bf16_nucleus"]
    res = {}
    tok_ld, at = 128, 100
    for vocab in VOCABS:
        g = torch.Generator().manual_seed(vocab)
        lg = (torch.randn((ROWS, vocab), generator=g) * 4.0).to(torch.bfloat16).to(dev)
        tokens = torch.randint(0, vocab, (ROWS, tok_ld), generator=g, dtype=torch.int64).to(dev)
        length = torch.empty(ROWS, dtype=torch.int32, device=dev)
        done = torch.zeros(ROWS, dtype=torch.int32, device=dev)
        starts = {h: torch.full((ROWS,), at - h, dtype=torch.int32, device=dev) for h in HISTORIES}
        for sname, skw in SAMPLERS.items():
            def this_build(kw):
                def launch(step):
                    length.fill_(at)
                    ops.sample(lg, tokens, length, done, seed=11, step=step, **skw, **kw)
                return launch

            def parent_build(step):
                length.fill_(at)
                rc = other.dh_sample_bf16_nucleus(lg.data_ptr(), vocab, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(), ROWS,
                                                  skw["temperature"], skw["top_k"], -1, 11, step, torch.cuda.current_stream().cuda_stream,
                                                  None, 0, None, None, None, 0, 0, None, None, skw.get("top_p", 1.0), 0.0)
                assert rc == 0

            arms = [("off", this_build({}))] + [(f"on_h{h}", this_build(dict(PEN, start=starts[h]))) for h in HISTORIES]
            if other:
                arms.append(("parent_off", parent_build))
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
            entry["on_over_off_percent"] = growth(entry, "us")
            entry["h0_equals_off_picks"] = bool(torch.equal(picks["off"], picks["on_h0"]))
            entry["h64_differs_from_off_picks"] = int((picks["off"] != picks["on_h64"]).sum())
            if other:
                entry["off_equals_parent_picks"] = bool(torch.equal(picks["off"], picks["parent_off"]))
                entry["off_over_parent_percent"] = round((entry["off"]["median_us"] / entry["parent_off"]["median_us"] - 1) * 100, 2)
            res[f"vocab{vocab}_{sname}"] = entry
    return res


def model_and_corpus():
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    return m, [p.to(dev) for p in synth_prompts(ROWS, a.prompt_len, cfg.padded_vocab_size, seed=7)]


def step_worker(with_penalties: bool) -> dict:
    """calls of a.steps captured steps from one prefilled state; -> ms per step per (sampler, arm)"""
    import torch
    m, corpus = model_and_corpus()
    dev, T = "cuda:0", a.prompt_len
    tok_ld = T + a.steps + 1
    eng = m.engine(ROWS, tok_ld, 32 * T, exact=True)
    eng.set_rsqrt_emulation(0, whole_call=False)
    for c in range(0, ROWS, 32):
        eng.forward(torch.cat(corpus[c:c + 32]), [T] * 32, [0] * 32, want_all=False, want_last=False, slot_base=c)
    base = torch.nn.functional.pad(torch.stack(corpus), (0, tok_ld - T)).contiguous()
    tokens = base.clone()
    length = torch.empty(ROWS, dtype=torch.int32, device=dev)
    done = torch.zeros(ROWS, dtype=torch.int32, device=dev)
    starts = {h: torch.full((ROWS,), T - h, dtype=torch.int32, device=dev) for h in HISTORIES}
    res, sha = {}, {}
    for sname, skw in SAMPLERS.items():
        arms = [("off", None)] + ([(f"on_h{h}", h) for h in HISTORIES] if with_penalties else [])
        ms = {name: [] for name, _ in arms}
        eng.set_nucleus(skw.get("top_p"), None)
        for i in range(a.rounds + 1):                          # the first round is the warm-up and the capture
            for name, h in arms:
                if h is not None:
                    eng.set_penalties(PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"], start=starts[h])
                tokens.copy_(base)
                length.fill_(T)
                done.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.decode(tokens, length, done, a.steps, skw["temperature"], skw["top_k"], None, 11, first_step=0)
                e1.record()
                torch.cuda.synchronize()
                if h is not None:
                    eng.set_penalties()
                if i:
                    ms[name].append(e0.elapsed_time(e1) / a.steps)
                sha[f"{sname}_{name}"] = hashlib.sha256(tokens[:, T:].cpu().numpy().tobytes()).hexdigest()[:16]
        eng.set_nucleus(None, None)
        entry = {name: summary(v, "ms") for name, v in ms.items()}
        if with_penalties:
            entry["on_over_off_percent"] = growth(entry, "ms")
        res[sname] = entry
    return dict(rows=ROWS, steps_per_call=a.steps, ms_per_step=res, ids_sha256=sha)


def child(what: str, lib: str = "") -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", what, "--prompt_len", str(a.prompt_len), "--steps", str(a.steps),
           "--launches", str(a.launches), "--rounds", str(a.rounds)]
    if what == "kernel" and a.parent_lib:
        cmd += ["--parent_lib", str(Path(a.parent_lib).resolve())]
    env = dict(os.environ)
    if lib:
        env["DUALHYP_HIP_LIB"] = lib
    print(f"[bench_penalties] {what} lib={lib or 'this build'}", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout, env=env)      # a step that fails ends the tool
    if r.returncode != 0:
        sys.exit(f"{what} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    for l in r.stdout.splitlines():
        if l.startswith("{"):
            return json.loads(l)
    sys.exit(f"{what}: the child printed no result")


def main() -> None:
    if a.worker == "kernel":
        print(json.dumps(kernel_worker()), flush=True)
        return
    if a.worker == "step":
        print(json.dumps(step_worker(True)), flush=True)
        return
    if a.worker == "step_off":
        from dualhyp_amd import _lib
        if os.environ.get("DUALHYP_HIP_LIB"):                 # a build without the feature: bind what it has
            for name in NEW_ENTRIES:
                _lib.SIGNATURES.pop(name, None)
        print(json.dumps(step_worker(False)), flush=True)
        return
    res = dict(tool="bench_penalties", rows=ROWS, samplers=SAMPLERS, penalties=PEN, histories=HISTORIES, prompt_len=a.prompt_len,
               steps=a.steps, launches=a.launches, rounds=a.rounds, kernel=child("kernel"), step=child("step"))
    if a.parent_lib:
        lib = str(Path(a.parent_lib).resolve())
        runs = {"parent": [], "this": []}
        for _ in range(max(2, a.rounds // 3)):
            runs["parent"].append(child("step_off", lib))
            runs["this"].append(child("step_off"))
        res["step_off_vs_parent"] = {}
        for sname in SAMPLERS:
            child_med = {k: [r["ms_per_step"][sname]["off"]["median_ms"] for r in v] for k, v in runs.items()}
            med = {k: statistics.median(x for r in v for x in r["ms_per_step"][sname]["off"]["rounds"]) for k, v in runs.items()}
            hashes = {k: sorted({r["ids_sha256"][f"{sname}_off"] for r in v}) for k, v in runs.items()}
            res["step_off_vs_parent"][sname] = dict(
                child_median_ms=child_med, median_ms={k: round(x, 4) for k, x in med.items()},
                parent_spread_percent=round((max(child_med["parent"]) / min(child_med["parent"]) - 1) * 100, 2),
                this_over_parent_percent=round((med["this"] / med["parent"] - 1) * 100, 2),
                ids_equal=hashes["this"] == hashes["parent"] and len(hashes["this"]) == 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
