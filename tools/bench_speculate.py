#!/usr/bin/env python3
"""Speculative decoding (generate_batch(..., speculate=D)) against speculate=0, one GPU: TinyLlama shape, hash weights + LoRA
r16, --rows prompts of 512 tokens, 64 new tokens, no EOS; greedy, or with --verify draw the sampled call of --top_k / --temperature
(/ --top_p / the three penalties), whose verify steps confirm drafts against the seeded draw.

Per row count (default 32 and 640), in ONE process on one box: the plain call (warm-up, then --repeats timed calls), then for
D = 1, 2, 3 and the target acceptance rates 0, 0.5 and 1.0 a scripted proposer — `drafts` = the plain run's own continuation with
every token replaced independently with the probability that makes the expected share of accepted drafts the target — warm-up and
--repeats timed calls each.  Figures are the call's own HIP-event decode time (median call): ms per issued step, decode tokens per second,
the measured acceptance, and per D the break-even acceptance (ms per verify step / ms per plain step - 1) / D.  The ids of every
speculative call must equal the plain call's (digest).  A combination the engine refuses (rows x (D + 1) > 2048) is recorded as such.

--verify draw adds, per D, `argmax_verify`: the arg-max verify step (top_k = 1, the same D, every draft wrong) timed in the same process,
and the draw step's time over it.  --lookup adds, per D, a call drafted by prompt lookup (drafts=None) and its accepted share.

    python tools/bench_speculate.py --rows 32 --verify draw --top_k 40 --temperature 0.8 [--top_p 0.9 --repetition_penalty 1.3] [--lookup]

Every row count is a child process of its own under a time limit; the parent never touches the GPU and prints ONE JSON line.

    python tools/bench_speculate.py [--rows 32 640] [--out profiles/speculate.json]

--trace plain|spec is the workload of the launch count: one process, the first --rows and (spec) the first --drafts, random drafts,
a warm-up call and one counted call of that kind alone; it prints the steps the two calls issued, to divide the kernel calls by.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/bench_speculate.py --rows 32 --drafts 3 --trace spec
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

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[32, 640])
ap.add_argument("--drafts", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--rates", type=float, nargs="+", default=[0.0, 0.5, 1.0])
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--prefill_batch", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=420, help="seconds each child may take")
ap.add_argument("--out", type=str, default="", help="write the line as a JSON file too")
ap.add_argument("--worker", type=int, default=None, help="(child) the row count of this run")
ap.add_argument("--verify", choices=("argmax", "draw"), default="argmax", help="draw: the sampled call, verified against the seeded draw")
ap.add_argument("--top_k", type=int, default=1, help="with --verify draw: 0 (no crop) or K")
ap.add_argument("--temperature", type=float, default=0.2)
ap.add_argument("--top_p", type=float, default=None)
ap.add_argument("--repetition_penalty", type=float, default=None)
ap.add_argument("--frequency_penalty", type=float, default=None)
ap.add_argument("--presence_penalty", type=float, default=None)
ap.add_argument("--seed", type=int, default=1337)
ap.add_argument("--lookup", action="store_true", help="per D, a call drafted by prompt lookup as well")
ap.add_argument("--trace", choices=("plain", "spec"), default=None, help="two calls of one kind in this process, for a kernel trace")
a = ap.parse_args()
if a.verify == "argmax" and (a.top_k != 1 or any(v is not None for v in (a.top_p, a.repetition_penalty, a.frequency_penalty, a.presence_penalty))):
    ap.error("--top_k other than 1, --top_p and the penalties go with --verify draw: the arg-max verifies a greedy call")
SAMPLER = {k: getattr(a, k) for k in ("top_p", "repetition_penalty", "frequency_penalty", "presence_penalty") if getattr(a, k) is not None}


def digest(outs) -> str:
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def corruption(rate: float, D: int) -> float:
    """p with mean_j (1 - p)^j = rate over j = 1 .. D: a draft is accepted when it and every draft before it in the step are right"""
    if rate >= 1.0:
        return 0.0
    if rate <= 0.0:
        return 1.0
    lo, hi = 0.0, 1.0
    for _ in range(60):
        p = (lo + hi) / 2
        if sum((1 - p) ** j for j in range(1, D + 1)) / D > rate:
            lo = p
        else:
            hi = p
    return (lo + hi) / 2


def setup(rows: int):
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    corpus = [p.to(dev) for p in synth_prompts(rows, a.prompt_len, cfg.padded_vocab_size, seed=7)]
    kw = dict(temperature=a.temperature, top_k=a.top_k or None, prefill_batch=a.prefill_batch)
    if a.verify == "draw":
        kw.update(seed=a.seed, **SAMPLER)
    return m, corpus, cfg.padded_vocab_size, kw


def trace(kind: str) -> None:
    import torch
    from dualhyp_amd import generate_batch
    rows, D, new = a.rows[0], a.drafts[0], a.max_new_tokens
    m, corpus, V, kw = setup(rows)
    extra = {}
    if kind == "spec":        # random drafts: next to none is accepted, so a call issues as many steps as the plain call does
        extra = dict(speculate=D, drafts=torch.randint(0, V, (rows, new), generator=torch.Generator().manual_seed(11)).to("cuda:0"))
    steps = 0
    for _ in range(2):
        tm = {}
        generate_batch(m, corpus, new, timing=tm, **kw, **extra)
        steps += tm["decode_steps"]
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="bench_speculate", trace=kind, rows=rows, D=D if kind == "spec" else 0, calls=2, steps_issued=steps,
                          n_layer=m.config.n_layer)), flush=True)


def worker(rows: int) -> None:
    import torch
    from dualhyp_amd import generate_batch
    dev = "cuda:0"
    m, corpus, V, kw = setup(rows)
    T, new = a.prompt_len, a.max_new_tokens

    def timed(**extra):
        outs = generate_batch(m, corpus, new, **kw, **extra)             # warm-up: allocation, graph capture
        ident = digest(outs)
        tms = []
        for _ in range(a.repeats):
            tm = {}
            generate_batch(m, corpus, new, timing=tm, **kw, **extra)
            tms.append(tm)
        tm = sorted(tms, key=lambda t: t["decode_ms"])[len(tms) // 2]
        return outs, ident, tm, [round(t["decode_ms"], 3) for t in tms]

    outs, ident, tm, regions = timed()
    truth = torch.stack([o[T:T + new] for o in outs]).contiguous()
    steps = new - 1
    plain_ms = tm["decode_ms"] / steps
    vkw = dict(verify="draw") if a.verify == "draw" else {}
    res = dict(rows=rows, ids_sha256=ident, verify=a.verify, sampler=dict(temperature=a.temperature, top_k=a.top_k, **SAMPLER),
               plain=dict(decode_ms=round(tm["decode_ms"], 3), decode_ms_regions=regions, steps=steps, ms_per_step=round(plain_ms, 4),
                          tokens_per_s=round(rows * steps / tm["decode_ms"] * 1e3, 1)), speculate={})
    g = torch.Generator().manual_seed(11)
    for D in a.drafts:
        cell = {}
        for rate in a.rates:
            p = corruption(rate, D)
            wrong = (torch.rand((rows, new), generator=g) < p).to(dev)
            drafts = torch.where(wrong, (truth + 1) % V, truth).contiguous()
            try:
                o2, id2, t2, reg2 = timed(speculate=D, drafts=drafts, **vkw)
            except ValueError as e:
                cell[str(rate)] = dict(refused=str(e))
                continue
            assert id2 == ident, f"rows {rows} D {D} rate {rate}: the ids differ from the plain run's"
            ms = t2["decode_ms"] / t2["decode_steps"]          # steps issued: 16 per read-back, the last ones may find every sequence finished
            cell[str(rate)] = dict(corruption=round(p, 4), accepted_share=round(t2["spec_accepted"] / max(t2["spec_drafted"], 1), 4),
                                   decode_ms=round(t2["decode_ms"], 3), decode_ms_regions=reg2, steps=t2["spec_steps"],
                                   steps_issued=t2["decode_steps"], ms_per_step=round(ms, 4),
                                   ms_per_step_over_plain=round(ms / plain_ms, 4),
                                   tokens_per_s=round(rows * steps / t2["decode_ms"] * 1e3, 1),
                                   tokens_per_s_over_plain=round(tm["decode_ms"] / t2["decode_ms"], 4))
        done = [c for c in cell.values() if "ms_per_step" in c]
        if done:   # tokens per step = 1 + share * D: equal tokens/s where share = (verify / plain - 1) / D
            ratio = statistics.median(c["ms_per_step_over_plain"] for c in done)
            cell["break_even_accepted_share"] = round((ratio - 1) / D, 4)
        if done and a.lookup:       # prompt lookup on the rows' own text: what share of its drafts this call's picks confirm
            o3, id3, t3, _ = timed(speculate=D, **vkw)
            assert id3 == ident, f"rows {rows} D {D} lookup: the ids differ from the plain run's"
            cell["lookup"] = dict(accepted_share=round(t3["spec_accepted"] / max(t3["spec_drafted"], 1), 4), steps=t3["spec_steps"],
                                  decode_ms=round(t3["decode_ms"], 3), tokens_per_s_over_plain=round(tm["decode_ms"] / t3["decode_ms"], 4))
        if done and a.verify == "draw":     # the arg-max verify step of the same D in the same process (greedy call, every draft wrong)
            greedy = dict(kw, temperature=0.2, top_k=1)
            for k in ("seed", *SAMPLER):
                greedy.pop(k, None)
            wrong = torch.randint(0, V, (rows, new), generator=g).to(dev)
            tms = []
            for i in range(a.repeats + 1):      # the first call is the warm-up
                t4 = {}
                generate_batch(m, corpus, new, timing=t4, speculate=D, drafts=wrong, **greedy)
                tms.append(t4["decode_ms"] / t4["decode_steps"])
            am = statistics.median(tms[1:])
            dm = statistics.median(c["ms_per_step"] for c in done)
            cell["argmax_verify"] = dict(ms_per_step=round(am, 4), draw_ms_per_step=round(dm, 4), draw_over_argmax=round(dm / am, 4),
                                         draw_minus_argmax_us=round((dm - am) * 1e3, 1))
        res["speculate"][str(D)] = cell
    print(json.dumps(res), flush=True)


if a.trace is not None:
    trace(a.trace)
elif a.worker is not None:
    worker(a.worker)
else:
    line = dict(tool="bench_speculate", verify=a.verify, prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats, runs=[])
    for rows in a.rows:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(rows), "--drafts", *map(str, a.drafts), "--rates", *map(str, a.rates)]
        for k in ("prompt_len", "max_new_tokens", "prefill_batch", "repeats", "verify", "top_k", "temperature", "seed"):
            cmd += [f"--{k}", str(getattr(a, k))]
        for k, v in SAMPLER.items():
            cmd += [f"--{k}", str(v)]
        cmd += ["--lookup"] * a.lookup
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a run that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"run --rows {rows} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        line["runs"] += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print(json.dumps(line), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + "\n")
