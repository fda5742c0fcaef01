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

--history adds the device-history arms to every run (beam_search_batch(history="device"): histories alone, no_repeat_ngram = 3, and
that with two stop sequences), each timed in alternation with the plain call, and the selection's kernels alone with and without
histories (history_arms below says which figures are subtraction remainders).  Without the flag the tool runs what it always ran, so
the same command line times the plain beam step on another build of the library (DUALHYP_HIP_LIB) or another checkout.

--kv table runs the tile-table arms INSTEAD (beam_search_batch(shared_prompt=True, kv="table"); include/dualhyp_hip.h, "Beam KV tile
table"): per W, utterance count and --max_new_tokens, three arms in alternation — "table"; "copy", this build's
beam_search_batch(shared_prompt=True); and, with --parent_lib, "parent", the same call on a second model whose engine is bound to
another build of the library (a build of the parent commit) — and, apart, this build's default call beside the parent's.  Reported:
ms per step of every arm (median and min .. max of --repeats), the (row, tile) pairs either scheme copied, the two scratches' bytes,
and the event time of the table's two copy launches alone (ops.beam_retile over one K / V^T pair with n_groups = layers x groups, the
engine's grid and bytes, at the call's middle step and its recorded parents).

The parent never touches the GPU and prints ONE JSON line.

    python tools/bench_beam.py [--beams 1 2 4] [--history] [--out profiles/beam_search.json]
    python tools/bench_beam.py --kv table --beams 2 4 --max_new_tokens 64 [--parent_lib OTHER.so] [--out profiles/beam_kv_table.json]
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
ap.add_argument("--history", action="store_true",
                help="also time the device-history arms (beam_search_batch(history='device')): histories alone, no_repeat_ngram = 3, and "
                     "that with two stop sequences, each beside the plain call; and the selection's two kernels with and without histories")
ap.add_argument("--kv", choices=("copy", "table"), default="copy", help="table: the tile-table arms instead of the greedy comparison")
ap.add_argument("--parent_lib", type=str, default="", help="--kv table: another build of libdualhyp_hip.so for the baseline arm")
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
    hist_fields = history_arms(m, corpus[:n], W, n, new, V, logits, beam) if a.history else {}
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
                          reserve_beams_bytes=int(scratch), engine_bytes=int(bytes_with), **hist_fields)), flush=True)


def kv_worker(W: int, n: int) -> None:
    """--kv table: the arms of one (W, utterances, max_new_tokens) in alternation"""
    import ctypes as C
    import torch
    from dualhyp_amd import GPT, Config, GER_LORA, _lib, beam_search_batch, ops
    from dualhyp_amd.beam import beam_tiles
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = "cuda:0"
    cfg = Config.from_name("tiny-llama-1.1b-chat", **{**GER_LORA, "dropout": 0.0})
    sd = synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0)

    def model():
        m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
        m.load_state_dict(sd, strict=True)
        m.eval()
        return m

    rows, new, V = n * W, a.max_new_tokens, cfg.padded_vocab_size
    corpus = [p.to(dev) for p in synth_prompts(n, a.prompt_len, V, seed=7)]
    need = (rows, a.prompt_len + new, max(rows, a.prefill_batch * a.prompt_len))
    m = model()
    call = lambda mm, tm, **kw: beam_search_batch(mm, corpus, new, num_beams=W, prefill_batch=a.prefill_batch, timing=tm, **kw)
    arms = dict(table=lambda tm=None: call(m, tm, shared_prompt=True, kv="table"), copy=lambda tm=None: call(m, tm, shared_prompt=True),
                default=lambda tm=None: call(m, tm))
    if a.parent_lib:      # a second model whose engine is created, and so bound, while the other build stands in for this one's
        other = C.CDLL(a.parent_lib)
        for name, sig in _lib.SIGNATURES.items():
            if hasattr(other, name):
                getattr(other, name).restype, getattr(other, name).argtypes = sig
        m0 = model()
        _lib.load()
        mine, _lib._lib = _lib._lib, other
        try:
            m0.engine(*need, exact=rows > a.prefill_batch)
        finally:
            _lib._lib = mine
        assert m0._engine.lib is other
        arms["parent"] = lambda tm=None: call(m0, tm, shared_prompt=True)
        arms["parent_default"] = lambda tm=None: call(m0, tm)
    for f in arms.values():
        f()                                                   # allocation, graph capture
    steps = new - 1
    times = {k: [] for k in arms}
    last = {}
    for _ in range(a.repeats):
        for k, f in arms.items():
            tm = {}
            f(tm)
            times[k].append(tm["decode_ms"] / steps)
            last[k] = tm
    stat = lambda xs: dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))
    eng = m._engine
    L, G, hs = cfg.n_layer, cfg.n_query_groups, cfg.head_size
    NT = beam_tiles(new, eng.s_max)
    # the table's two copy launches alone: one K / V^T pair with n_groups = L * G is the engine's grid and the engine's bytes
    _, st = beam_search_batch(m, corpus, new, num_beams=W, prefill_batch=a.prefill_batch, shared_prompt=True, kv="table", return_state=True)
    S = -(-(a.prompt_len + new + 1) // 32) * 32
    kc = torch.zeros((rows, L * G, S, hs), dtype=torch.bfloat16, device=dev)
    vt = torch.zeros((rows, L * G, hs, S), dtype=torch.bfloat16, device=dev)
    scratch = torch.empty(rows * 2 * L * G * hs * 32, dtype=torch.bfloat16, device=dev)
    tab = st["beam"].tile_table(NT).view(2, rows, NT).clone()
    t_mid = next(t for t in range(new // 2, new) if (a.prompt_len + t) >> 5 == (a.prompt_len + t - 1) >> 5)      # a step whose tile stays open
    n_steps = torch.full((n,), t_mid + 1, dtype=torch.int32, device=dev)
    retile_us = event_us(lambda: ops.beam_retile(kc, vt, tab, st["beam"].beam_parent, n_steps, st["prompt_len"], t_mid, scratch=scratch))
    moved_mid = sum(p != w for u in range(n) for w, p in enumerate(st["host"]["beam_parent"][u][t_mid]))
    print(json.dumps(dict(W=W, utterances=n, rows=rows, steps=steps, max_new_tokens=new, n_tiles=NT,
                          ms_per_step={k: stat(v) for k, v in times.items()},
                          copied_rows=last["table"]["beam_copied_rows"], step_rows=last["table"]["beam_step_rows"],
                          copied_tiles_table=last["table"]["beam_copied_tiles"], copied_tiles_copy=last["copy"]["beam_copied_tiles"],
                          retile_two_launches_us=round(retile_us, 1), retile_step=t_mid, retile_rows_moved=moved_mid,
                          scratch_bytes_table=rows * 2 * L * G * hs * 32 * 2, scratch_bytes_copy=rows * 2 * L * G * hs * 32 * 2 * NT)), flush=True)


def history_arms(m, prompts, W, n, new, V, logits, plain):
    """--history: the whole step under device histories (the plain call repeated beside each arm, alternating), and the selection's
    kernels alone on the step's rows at step new // 2.  merge_us is beam_select minus token_top_logprobs at K = 2 W, and
    candidates_ban_us is beam_select under N = 3 minus the merge with histories: subtraction remainders of event times, not kernel
    times of their own."""
    import torch
    from dualhyp_amd import beam_search_batch, ops
    from dualhyp_amd.beam import BeamState
    from dualhyp_amd.stop import compile_stop
    dev = logits.device
    seqs = [[V - 2, V - 3], [V - 4, V - 5, V - 6]]          # ids the hash weights rarely pick: the test runs, nothing ends
    arms = dict(history_only=dict(history="device"), ngram3=dict(history="device", no_repeat_ngram=3),
                ngram3_stop2=dict(history="device", no_repeat_ngram=3, stop=seqs))
    out = {}
    steps = new - 1
    for name, kw in arms.items():
        run = lambda tm=None: beam_search_batch(m, prompts, new, num_beams=W, prefill_batch=a.prefill_batch, timing=tm, **kw)
        run()
        t_arm, t_off = [], []
        for _ in range(a.repeats):
            tm = {}
            plain(tm)
            t_off.append(tm["decode_ms"] / steps)
            tm = {}
            run(tm)
            t_arm.append(tm["decode_ms"] / steps)
        out[name + "_ms_per_step"] = [round(x, 4) for x in t_arm]
        out[name + "_off_ms_per_step"] = [round(x, 4) for x in t_off]
    # the kernels alone: a state in the middle of a call, histories of random ids from a small pool (bans happen)
    step = new // 2
    st = BeamState(n, W, new, dev)
    st.n_steps.fill_(step)
    hist = st.history_buffer()
    hist.copy_(torch.randint(0, 64, tuple(hist.shape), device=dev))
    stop = compile_stop([], seqs, V, dev)
    keep = (st.n_steps.clone(), st.cum.clone())

    def reset():
        st.done.zero_()
        st.n_fin.zero_()
        st.n_steps.copy_(keep[0])
        st.cum.copy_(keep[1])

    def select(**kw):
        reset()
        ops.beam_select(logits, st, rows_per_utt=W, step=step, **kw)

    reset_us = event_us(reset)
    top_us = event_us(lambda: ops.token_top_logprobs(logits, 2 * W))
    plain_us = event_us(select) - reset_us
    hist_us = event_us(lambda: select(history=hist)) - reset_us
    ban_us = event_us(lambda: select(history=hist, no_repeat_ngram=3)) - reset_us
    ban_stop_us = event_us(lambda: select(history=hist, no_repeat_ngram=3, stop=stop)) - reset_us
    out.update(kernel_step=step, token_top_logprobs_us=round(top_us, 1), select_us_plain=round(plain_us, 1),
               select_us_history=round(hist_us, 1), select_us_ngram3=round(ban_us, 1), select_us_ngram3_stop2=round(ban_stop_us, 1),
               merge_us_plain=round(plain_us - top_us, 1), merge_us_history=round(hist_us - top_us, 1),
               merge_us_history_stop2=round(ban_stop_us - ban_us + hist_us - top_us, 1),
               candidates_ban_us=round(ban_us - (hist_us - top_us), 1))
    return out


if a.worker is not None:
    (kv_worker if a.kv == "table" else worker)(*a.worker)
else:
    line = dict(tool="bench_beam", prompt_len=a.prompt_len, max_new_tokens=a.max_new_tokens, repeats=a.repeats, runs=[])
    if a.kv != "copy":
        line.update(kv=a.kv, parent_lib=bool(a.parent_lib))
    for W in a.beams:
        for n in sorted({a.utterances, max(1, a.rows // W)}):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(W), str(n)]
            for k in ("prompt_len", "max_new_tokens", "prefill_batch", "repeats"):
                cmd += [f"--{k}", str(getattr(a, k))]
            cmd += ["--history"] if a.history else []
            cmd += ["--kv", a.kv] if a.kv != "copy" else []
            cmd += ["--parent_lib", str(Path(a.parent_lib).resolve())] if a.parent_lib else []
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a run that fails ends the tool
            if r.returncode != 0:
                sys.exit(f"run W={W} utterances={n} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
            line["runs"] += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print(json.dumps(line), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + "\n")
