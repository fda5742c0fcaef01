#!/usr/bin/env python3
"""Sampled candidates (sample_batch: one prefill per utterance, one fork launch, N decode rows each) against generate_batch over the
prompt list with every prompt repeated N times, one GPU: TinyLlama shape, hash weights + LoRA r16, 512-token prompts, 64 new tokens,
temperature 0.8, top_k 5, no EOS, for N in 2, 4, 8.  Both variants step --rows decode rows (default 640), i.e. rows // N utterances,
so the decode halves are the same work and the difference is the prefill: B prompts and a fork against B * N prompts.

Per N, in ONE process on one box: a warm-up call of each variant (allocation, graph capture), then three timed regions of each,
alternating; the line gives every region and the median.  A region is one whole call between two device synchronisations (host
clock); prefill_ms and fork_ms are the call's own HIP-event figures.  The ids of the two variants must be equal (digest).  Then, on
the engine of those calls, the fork by itself: dh_engine_fork_slots (one launch over all utterances) against the loop it replaces,
one dh_engine_copy_prefix call per utterance — five times each after a warm-up, host clock between two synchronisations, since the
loop's cost is its host synchronisations; the fork's HIP-event time and the bytes it moves (every source tile read once, written
N - 1 times) against 8 TB/s are given too.

--shared_prompt: the arm for shared-prompt attention instead (include/dualhyp_hip.h; sample_batch(shared_prompt=True)).  Same shape,
same regions, same alternation, per N in one process: sample_batch without and with the flag — equal ids (digest), decode_ms of every
region and the median of each — and then the attention launch by itself at that shape: ops.attn_decode_fused against
ops.attn_decode_shared on one layer's caches (rows decode rows, 8 pair-summed partials + LoRA, every row half-way through its budget),
HIP events around 20 launches each, alternating, three times.

Every GPU run is a child process of its own under a time limit; the parent never touches the GPU.

    python tools/bench_samples.py [--num_samples 2 4 8] [--rows 640] [--out profiles/samples.json]
    python tools/bench_samples.py --shared_prompt --out profiles/shared_prompt.json
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
ap.add_argument("--num_samples", type=int, nargs="+", default=[2, 4, 8], help="candidates per utterance, one run each")
ap.add_argument("--rows", type=int, default=640, help="decode rows of both variants: rows // N utterances")
ap.add_argument("--prompt_len", type=int, default=512)
ap.add_argument("--max_new_tokens", type=int, default=64)
ap.add_argument("--prefill_batch", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--step_timeout", type=int, default=420, help="seconds each GPU run may take")
ap.add_argument("--out", type=str, default="", help="write the lines as one JSON file")
ap.add_argument("--shared_prompt", action="store_true", help="the shared-prompt attention arm: sample_batch without and with shared_prompt")
ap.add_argument("--worker", type=int, default=None, help="(child) the N of this run")
a = ap.parse_args()
HBM_BYTES_PER_S = 8e12


def worker(N: int) -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, generate_batch, sample_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    B, T, new = a.rows // N, a.prompt_len, a.max_new_tokens
    corpus = [p.to(dev) for p in synth_prompts(B, T, cfg.padded_vocab_size, seed=7)]
    folded = [p for p in corpus for _ in range(N)]
    kw = dict(temperature=0.8, top_k=5, seed=1337, prefill_batch=a.prefill_batch)

    def digest(rows) -> str:
        h = hashlib.sha256()
        for r in rows:
            h.update(r.cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    calls = {"generate_batch": lambda tm: digest(o[T:] for o in generate_batch(m, folded, new, timing=tm, **kw)),
             "sample_batch": lambda tm: digest(s["tokens"] for ss in sample_batch(m, corpus, new, num_samples=N, timing=tm, **kw) for s in ss)}
    ids = {name: call(None) for name, call in calls.items()}      # warm-up: allocation, graph capture, code objects of both variants
    torch.cuda.synchronize()
    assert ids["generate_batch"] == ids["sample_batch"], "the sampled candidates differ from the N-fold call's rows"
    runs = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, call in calls.items():
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(tm)
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0, tm))
    line = dict(step="sample_batch_vs_n_fold_generate_batch", num_samples=N, utterances=B, rows=B * N, prompt_len=T, max_new_tokens=new,
                ids_sha256=ids["sample_batch"])
    for name in calls:
        walls = [w for w, _ in runs[name]]
        tm = runs[name][walls.index(statistics.median(walls))][1]
        line[name] = dict(utt_per_s=round(B / statistics.median(walls), 1), utt_per_s_regions=[round(B / w, 1) for w in walls],
                          prefill_ms=round(tm["prefill_ms"], 2), prefill_ms_regions=[round(t["prefill_ms"], 2) for _, t in runs[name]],
                          decode_ms=round(tm["decode_ms"], 2), prefill_tokens=tm["prefill_tokens"])
        if "fork_ms" in tm:
            line[name]["fork_ms"] = round(tm["fork_ms"], 4)
            line[name]["fork_ms_regions"] = [round(t["fork_ms"], 4) for _, t in runs[name]]
    line["sample_over_fold_utt_per_s"] = round(line["sample_batch"]["utt_per_s"] / line["generate_batch"]["utt_per_s"], 4)
    line["sample_over_fold_prefill_ms"] = round(line["sample_batch"]["prefill_ms"] / line["generate_batch"]["prefill_ms"], 4)
    print(json.dumps(line), flush=True)

    # the fork by itself, on the engine of the calls above (its slots hold the last call's sequences: any bytes do)
    eng = m._engine
    L, G, hs = cfg.n_layer, cfg.n_query_groups, cfg.head_size
    plen = torch.full((B,), T, dtype=torch.int32, device=dev)
    tiles = -(-T // 32) * 32

    def fork():
        eng.fork_slots(plen, N, T)

    def loop():
        for u in range(B):
            eng.copy_prefix(u * N, list(range(u * N + 1, (u + 1) * N)), tiles)

    def walls(fn, n=5):
        fn()
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return sorted(out)

    def events(fn, n=5):
        fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sorted(e0.elapsed_time(e1) for e0, e1 in ev)

    fork_wall, loop_wall, fork_ev = walls(fork), walls(loop), events(fork)
    moved = 2 * L * G * tiles * hs * 2 * N * B            # K and V^T, bf16: one read of every source + N - 1 writes
    rate = moved / (statistics.median(fork_ev) * 1e-3)
    print(json.dumps(dict(step="fork_slots_vs_copy_prefix_loop", num_samples=N, utterances=B, prompt_len=T,
                          fork_wall_ms=[round(x, 4) for x in fork_wall], copy_prefix_loop_wall_ms=[round(x, 4) for x in loop_wall],
                          loop_over_fork_wall=round(statistics.median(loop_wall) / statistics.median(fork_wall), 2),
                          fork_event_ms=[round(x, 4) for x in fork_ev], fork_bytes=moved, fork_TB_per_s=round(rate / 1e12, 3),
                          fork_share_of_8TBps=round(rate / HBM_BYTES_PER_S, 3))), flush=True)


def shared_worker(N: int) -> None:
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, ops, sample_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0), strict=True)
    m.eval()
    B, T, new = a.rows // N, a.prompt_len, a.max_new_tokens
    corpus = [p.to(dev) for p in synth_prompts(B, T, cfg.padded_vocab_size, seed=7)]
    kw = dict(temperature=0.8, top_k=5, seed=1337, prefill_batch=a.prefill_batch)

    def digest(rows) -> str:
        h = hashlib.sha256()
        for r in rows:
            h.update(r.cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def call(shared):
        return lambda tm: digest(s["tokens"] for ss in sample_batch(m, corpus, new, num_samples=N, timing=tm, shared_prompt=shared, **kw) for s in ss)

    calls = {"unshared": call(False), "shared": call(True)}
    ids = {name: c(None) for name, c in calls.items()}            # warm-up: allocation, graph capture of both steps
    torch.cuda.synchronize()
    assert ids["unshared"] == ids["shared"], "shared_prompt changed the sampled ids"
    runs = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, c in calls.items():
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c(tm)
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0, tm))
    line = dict(step="sample_batch_shared_prompt_vs_unshared", num_samples=N, utterances=B, rows=B * N, prompt_len=T, max_new_tokens=new,
                ids_sha256=ids["shared"])
    for name in calls:
        dec = [t["decode_ms"] for _, t in runs[name]]
        walls = [w for w, _ in runs[name]]
        steps = runs[name][0][1]["decode_steps"]
        line[name] = dict(decode_ms=round(statistics.median(dec), 2), decode_ms_regions=[round(x, 2) for x in dec], decode_steps=steps,
                          step_ms=round(statistics.median(dec) / steps, 4), utt_per_s=round(B / statistics.median(walls), 1),
                          utt_per_s_regions=[round(B / w, 1) for w in walls])
    line["shared_over_unshared_decode_ms"] = round(line["shared"]["decode_ms"] / line["unshared"]["decode_ms"], 4)
    print(json.dumps(line), flush=True)
    del m
    torch.cuda.empty_cache()

    # the attention launch by itself: one layer's caches at the same shape, every row half-way through its budget
    H, G, hs, R = cfg.n_head, cfg.n_query_groups, cfg.head_size, B * N
    s_max = -(-(T + new) // 64) * 64
    qkv_dim = (H + 2 * G) * hs
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *sh: torch.randn(*sh, device=dev, generator=g).bfloat16()
    kc, vt = r(R, G, s_max, hs), r(R, G, hs, s_max)
    # the fork: every row's slot holds its utterance's whole prompt tiles (hs * 32 elements each, back to back in a (slot, group) block)
    n_pre = (T // 32) * 32 * hs
    for c in (kc, vt):
        v = c.view(B, N, G, -1)
        v[:, 1:, :, :n_pre] = v[:, :1, :, :n_pre]
    cos, sin = r(s_max, hs), r(s_max, hs)
    q32 = torch.randn(4, R, qkv_dim + 48, device=dev, generator=g) * 0.3       # d = 2048: 8 K-slices, handed over as 4 pair sums
    bq = (torch.randn(qkv_dim, 16, device=dev, generator=g) * 0.05).bfloat16()
    slot = torch.arange(R, dtype=torch.int32, device=dev)
    kv_len = torch.full((R,), T + new // 2 + 1, dtype=torch.int32, device=dev)
    plen = torch.full((B,), T, dtype=torch.int32, device=dev)
    args = (q32, qkv_dim, bq, 2.0, (H * hs, (H + G) * hs), cos, sin, slot, kv_len, kc, vt, H)
    ops_ = {"unshared": lambda: ops.attn_decode_fused(*args, pairs=False),
            "shared": lambda: ops.attn_decode_shared(*args, N, plen, pairs=False)}
    y = {name: fn() for name, fn in ops_.items()}
    torch.cuda.synchronize()
    assert torch.equal(y["unshared"], y["shared"]), "the shared launch differs from the unshared one"
    us = {name: [] for name in ops_}
    n_launch = 20
    for _ in range(a.repeats):
        for name, fn in ops_.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_launch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / n_launch)
    q_per_kv = H // G
    Gs = 32 // q_per_kv
    line = dict(step="attention_launch_shared_vs_unshared", num_samples=N, rows=R, kv_len=int(kv_len[0]), prompt_len=T, n_head=H, n_groups=G,
                head_size=hs, blocks_unshared=R * G, blocks_shared=B * -(-N // Gs) * G, rows_per_block=min(N, Gs),
                unshared_us=round(statistics.median(us["unshared"]), 2), unshared_us_regions=[round(x, 2) for x in us["unshared"]],
                shared_us=round(statistics.median(us["shared"]), 2), shared_us_regions=[round(x, 2) for x in us["shared"]])
    line["shared_over_unshared_us"] = round(line["shared_us"] / line["unshared_us"], 4)
    print(json.dumps(line), flush=True)


if a.worker is not None:
    (shared_worker if a.shared_prompt else worker)(a.worker)
else:
    lines = []
    for N in a.num_samples:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(N)] + (["--shared_prompt"] if a.shared_prompt else [])
        for k in ("rows", "prompt_len", "max_new_tokens", "prefill_batch", "repeats"):
            cmd += [f"--{k}", str(getattr(a, k))]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a run that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"run --num_samples {N} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                print(l, flush=True)
                lines.append(json.loads(l))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(lines, indent=1) + "\n")
