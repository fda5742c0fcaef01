#!/usr/bin/env python3
"""What nucleus and min-p sampling cost (GPU box): python tools/bench_nucleus.py [--parent_lib OTHER.so] [--out profiles/nucleus.json]

Measurements, each in a child process under its own time limit; the parent never touches the GPU and prints ONE JSON line.

"kernel": the sampling kernel alone (ops.sample on [rows, vocab] bf16 logits, Gaussian rows of sigma 4, temperature 0.8, top_k 50),
at 32 and 640 rows on the TinyLlama vocabulary (32 000) and the Llama-3 vocabulary (128 256), in three arms run in alternation in one
process: the feature off, top_p = 0.9, and top_p = 0.9 with min_p = 0.05.  Microseconds per launch, the median and the minimum over
--rounds rounds of --launches launches between two events.  With --parent_lib the other library's dh_sample_bf16_top is a fourth arm
of the same alternation (bound beside this build's in the same process): the feature-off launch of the parent commit.

"step": a sampled decode step of the TinyLlama shape (hash weights + LoRA r16) through the engine, generate_batch's decode time over
its steps at 32 and 640 rows of --prompt_len tokens, the same three arms in alternation.  With --parent_lib the feature-off step in
children of their own, this build and the other library in alternation (DUALHYP_HIP_LIB; a build of the parent commit has none of
the feature's entries, so the child drops them from the symbol table it binds), with a hash of the generated ids: the two must be
equal.  The Llama-3 shape is not stepped here: its vocabulary is measured at the kernel.
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
ap.add_argument("--new_tokens", type=int, default=48)
ap.add_argument("--launches", type=int, default=50, help="kernel launches between two events")
ap.add_argument("--rounds", type=int, default=7, help="rounds per arm (kernel), calls per arm (step), children per library (step vs parent)")
ap.add_argument("--parent_lib", type=str, default="", help="another build of libdualhyp_hip.so to time the feature-off path with")
ap.add_argument("--step_timeout", type=int, default=300, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=str, default=None, help="(child) the measurement of this run")
ap.add_argument("--rows", type=int, default=640, help="(child) rows of the step worker")
a = ap.parse_args()

NEW_ENTRIES = ("dh_sample_bf16_nucleus", "dh_sample_rows_bf16_nucleus", "dh_engine_set_nucleus")
SAMPLER = dict(temperature=0.8, top_k=50)
ARMS = (("off", {}), ("top_p_0.9", dict(top_p=0.9)), ("top_p_0.9_min_p_0.05", dict(top_p=0.9, min_p=0.05)))
SHAPES = ((32, 32000), (640, 32000), (32, 128256), (640, 128256))


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), rounds=[round(x, 2) for x in us])


def kernel_worker() -> dict:
    import ctypes as C
    import torch
    from dualhyp_amd import _lib, ops
    dev = "cuda:0"
    other = None
    if a.parent_lib:
        other = C.CDLL(a.parent_lib)
        other.dh_sample_bf16_top.restype, other.dh_sample_bf16_top.argtypes = _lib.SIGNATURES["dh_sample_bf16_top"]
    res = {}
    for rows, vocab in SHAPES:
        g = torch.Generator().manual_seed(vocab + rows)
        lg = (torch.randn((rows, vocab), generator=g) * 4.0).to(torch.bfloat16).to(dev)
        tokens = torch.zeros((rows, 2), dtype=torch.int64, device=dev)
        length = torch.zeros(rows, dtype=torch.int32, device=dev)
        done = torch.zeros(rows, dtype=torch.int32, device=dev)

        def this_build(kw):
            def launch(step):
                length.zero_()
                ops.sample(lg, tokens, length, done, seed=11, step=step, **SAMPLER, **kw)
            return launch

        def parent_build(step):
            length.zero_()
            rc = other.dh_sample_bf16_top(lg.data_ptr(), vocab, tokens.data_ptr(), 2, length.data_ptr(), done.data_ptr(), rows,
                                          SAMPLER["temperature"], SAMPLER["top_k"], -1, 11, step, torch.cuda.current_stream().cuda_stream,
                                          None, 0, None, None)
            assert rc == 0

        arms = [(name, this_build(kw)) for name, kw in ARMS] + ([("parent_off", parent_build)] if other else [])
        picks = {}
        for name, launch in arms:                      # warm-up, and the picks of step 0
            launch(0)
            torch.cuda.synchronize()
            picks[name] = tokens[:, 0].clone()
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
        # the zeroing of `length` rides in every arm alike
        entry = {name: summary(us) for name, us in times.items()}
        if other:
            entry["off_equals_parent_picks"] = bool(torch.equal(picks["off"], picks["parent_off"]))
            entry["off_over_parent_percent"] = round((entry["off"]["median_us"] / entry["parent_off"]["median_us"] - 1) * 100, 2)
        res[f"rows{rows}_vocab{vocab}"] = entry
    return res


def model_and_corpus(rows):
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    return m, [p.to(dev) for p in synth_prompts(rows, a.prompt_len, cfg.padded_vocab_size, seed=7)]


def step_worker(arms) -> dict:
    import torch
    from dualhyp_amd import generate_batch
    m, corpus = model_and_corpus(a.rows)
    ms = {name: [] for name, _ in arms}
    sha = {}
    for i in range(a.rounds + 1):                              # the first round is the warm-up
        for name, kw in arms:
            tm = {}
            out = generate_batch(m, corpus, a.new_tokens, prefill_batch=32, timing=tm, seed=11, **SAMPLER, **kw)
            if i:
                ms[name].append(tm["decode_ms"] / tm["decode_steps"])
            sha[name] = hashlib.sha256(torch.stack([o[a.prompt_len:] for o in out]).cpu().numpy().tobytes()).hexdigest()[:16]
    return dict(rows=a.rows, ms_per_step={k: [round(x, 4) for x in v] for k, v in ms.items()},
                median_ms={k: round(statistics.median(v), 4) for k, v in ms.items()}, ids_sha256=sha)


def child(what: str, rows: int = 640, lib: str = "") -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", what, "--rows", str(rows), "--prompt_len", str(a.prompt_len),
           "--new_tokens", str(a.new_tokens), "--launches", str(a.launches), "--rounds", str(a.rounds)]
    if what == "kernel" and a.parent_lib:
        cmd += ["--parent_lib", str(Path(a.parent_lib).resolve())]
    env = dict(os.environ)
    if lib:
        env["DUALHYP_HIP_LIB"] = lib
    print(f"[bench_nucleus] {what} rows={rows} lib={lib or 'this build'}", file=sys.stderr, flush=True)
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
        print(json.dumps(step_worker(ARMS)), flush=True)
        return
    if a.worker == "step_off":
        from dualhyp_amd import _lib
        if os.environ.get("DUALHYP_HIP_LIB"):                 # a build without the feature: bind what it has
            for name in NEW_ENTRIES:
                _lib.SIGNATURES.pop(name, None)
        print(json.dumps(step_worker(ARMS[:1])), flush=True)
        return
    res = dict(tool="bench_nucleus", sampler=SAMPLER, prompt_len=a.prompt_len, new_tokens=a.new_tokens, launches=a.launches,
               rounds=a.rounds, kernel=child("kernel"), step={f"rows{rows}": child("step", rows) for rows in (32, 640)})
    if a.parent_lib:
        lib = str(Path(a.parent_lib).resolve())
        res["step_off_vs_parent"] = {}
        for rows in (32, 640):
            runs = {"parent": [], "this": []}
            for _ in range(max(2, a.rounds // 3)):
                runs["parent"].append(child("step_off", rows, lib))
                runs["this"].append(child("step_off", rows))
            med = {k: statistics.median(x for r in v for x in r["ms_per_step"]["off"]) for k, v in runs.items()}
            child_med = {k: [r["median_ms"]["off"] for r in v] for k, v in runs.items()}
            hashes = {k: sorted({r["ids_sha256"]["off"] for r in v}) for k, v in runs.items()}
            res["step_off_vs_parent"][f"rows{rows}"] = dict(
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
