#!/usr/bin/env python3
"""MXFP4 weights against e4m3 weights on the fp8 serving path (GPU box): python tools/bench_mxfp4.py [--out profiles/mxfp4.json]

Kernel level, at the Llama-3-8B linears (N x K = 6144 x 4096 qkv, 4096 x 4096 proj, 2 x 14336 x 4096 SwiGLU, 4096 x 14336 mlp
proj): the streaming kernels at M = 32 and 128 and the tiled kernels at the prefill M of the llama3-8b-fp8 bench line (--prefill_m),
dh_linear_fp8_ex against dh_linear_mxfp4_ex on the same activations.  HIP events over a hipGraph of back-to-back calls
(tools/tune_decode_common.bench), --repeats alternating repeats per arm; the record holds every repeat, the median, the spread
(max - min over the median) and, for the streaming kernels, the achieved fraction of the HBM peak over the weight bytes each
arm has to read (e4m3: N K + 4 N; MXFP4: N K / 2 + N K / 32).

Step level (--step): Llama-3-8B with synthetic weights, 128 decode rows, fp8 against mxfp4 with the bf16 and with the fp8 KV
cache: milliseconds per decode step (HIP events of generate_batch's decode phase) and dh_engine_device_bytes plus the bytes of
the quantised block weights.

--activations mxfp6: the MXFP6-activation arm (csrc/mxfp6.hip) against the e4m3-activation MXFP4 kernels as the baseline, by the same
method.  Kernel level: dh_linear_mxfp4_ex against dh_linear_mxfp4a6_ex, each on its own quantisation of the same bf16 rows.  Quantiser
level: dh_quant_rows_fp8 / dh_rmsnorm_quant_fp8 against dh_quant_rows_mxfp6 / dh_rmsnorm_quant_mxfp6 at the same row counts and
K = 4096 / 14336 (the rmsnorm forms at 4096).  Step level (--step): mxfp4 with fp8 and with mxfp6 activations over the bf16 KV cache,
prefill milliseconds of the 128 x 512-token prompts as well as milliseconds per decode step.

Each part is a child process under its own time limit (--step_timeout); a part that fails ends the tool, what the parts before
it measured is in --out already."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

ROOT = Path(__file__).resolve().parent.parent
HBM_PEAK = 8.0e12          # bytes/s, MI355X
LINEARS = {"qkv": (6144, 4096, False), "proj": (4096, 4096, False), "swiglu": (14336, 4096, True), "mlp_proj": (4096, 14336, False)}


def _summary(us):
    med = statistics.median(us)
    return dict(us=[round(x, 2) for x in us], median_us=round(med, 2), spread=round((max(us) - min(us)) / med, 4))


def kernel_level(name, M, repeats, activations="fp8"):
    from dualhyp_amd import ops
    from dualhyp_amd.quant import quantize_rows_fp8, quantize_blocks_mxfp4, pack_mxfp4
    from tools.tune_decode_common import bench, D
    N, K, swiglu = LINEARS[name]
    g = torch.Generator(device=D).manual_seed(7)
    x = (torch.rand((M, K), device=D, generator=g) * 3 - 1.5).bfloat16()
    ws = [(torch.rand((N, K), device=D, generator=g) * 0.1 - 0.05).bfloat16() for _ in range(2 if swiglu else 1)]
    xq, xs = ops.quant_rows_fp8(x)
    f8 = [quantize_rows_fp8(w) for w in ws]
    m4 = [pack_mxfp4(*quantize_blocks_mxfp4(w)) for w in ws]
    del ws
    kernel = 2 if M <= 128 else 1
    kw8 = dict(kernel=kernel, **(dict(epilogue=ops.EPI_SWIGLU, w2q=f8[1][0], w2_scale=f8[1][1]) if swiglu else {}))
    kw4 = dict(kernel=kernel, **(dict(epilogue=ops.EPI_SWIGLU, w2q=m4[1][0], w2_scale=m4[1][1]) if swiglu else {}))
    arms = {"fp8": lambda i: ops.linear_fp8(xq, xs, f8[0][0], f8[0][1], **kw8),
            "mxfp4": lambda i: ops.linear_mxfp4(xq, xs, m4[0][0], m4[0][1], **kw4)}
    if activations == "mxfp6":      # the baseline arm is the e4m3-activation MXFP4 kernel
        x6, s6 = ops.quant_rows_mxfp6(x)
        arms = {"mxfp4": arms["mxfp4"], "mxfp4a6": lambda i: ops.linear_mxfp4a6(x6, s6, M, m4[0][0], m4[0][1], **kw4)}
    base = next(iter(arms))
    us = {k: [] for k in arms}
    reps = 20 if M <= 128 else 3
    for _ in range(repeats):
        for arm, fn in arms.items():
            us[arm].append(bench(fn, reps=reps))
    n_w = 2 if swiglu else 1
    w_bytes = {"fp8": n_w * (N * K + 4 * N), "mxfp4": n_w * (N * K // 2 + N * K // 32), "mxfp4a6": n_w * (N * K // 2 + N * K // 32)}
    out = {}
    for arm, t in us.items():
        out[arm] = _summary(t)
        out[arm]["weight_bytes"] = w_bytes[arm]
        if M <= 128:
            out[arm]["hbm_fraction"] = round(w_bytes[arm] / (out[arm]["median_us"] * 1e-6) / HBM_PEAK, 4)
        else:
            out[arm]["pflops"] = round(2.0 * n_w * M * N * K / (out[arm]["median_us"] * 1e-6) / 1e15, 4)
    other = [a for a in arms if a != base][0]
    out[f"{other}_over_{base}_time"] = round(out[other]["median_us"] / out[base]["median_us"], 4)
    print(json.dumps({"kernel": {f"{name}.M{M}": out}}), flush=True)


def quant_level(K, M, repeats):
    """The two fp8 quantisers against the two MXFP6 ones on the same bf16 rows; bytes moved: 2 K read and K + 4 (e4m3) or 3 K / 4 + K / 32
    (MXFP6) written per row."""
    from dualhyp_amd import ops
    from tools.tune_decode_common import bench, D
    g = torch.Generator(device=D).manual_seed(7)
    x = (torch.rand((M, K), device=D, generator=g) * 3 - 1.5).bfloat16()
    w = (1 + torch.rand((K,), device=D, generator=g) * 0.2).bfloat16()
    arms = {"quant_fp8": lambda i: ops.quant_rows_fp8(x), "quant_mxfp6": lambda i: ops.quant_rows_mxfp6(x, fill=None)}
    if K <= 8192:
        arms.update({"rmsnorm_quant_fp8": lambda i: ops.rmsnorm_quant_fp8(x, w, 1e-5),
                     "rmsnorm_quant_mxfp6": lambda i: ops.rmsnorm_quant_mxfp6(x, w, 1e-5, fill=None)})
    us = {k: [] for k in arms}
    reps = 20 if M <= 128 else 3
    for _ in range(repeats):
        for arm, fn in arms.items():
            us[arm].append(bench(fn, reps=reps))
    out = {arm: _summary(t) for arm, t in us.items()}
    for kind in ("quant", "rmsnorm_quant"):
        if kind + "_fp8" in out:
            out[f"{kind}_mxfp6_over_fp8_time"] = round(out[kind + "_mxfp6"]["median_us"] / out[kind + "_fp8"]["median_us"], 4)
    print(json.dumps({"quant": {f"K{K}.M{M}": out}}), flush=True)


def step_level(fmt, kv_cache, rows, prompt, new_tokens, repeats, activations="fp8"):
    from dualhyp_amd import GPT, Config, GER_LORA, quantize_model_fp8, quantize_model_mxfp4
    from dualhyp_amd.generate import generate_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    dev = torch.device("cuda", 0)
    cfg = Config.from_name("Llama-3-8B", **{**GER_LORA, "dropout": 0.0})
    cfg.block_size = 4096
    sd = synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0)
    model = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
    model.load_state_dict(sd, strict=True)
    del sd
    model.eval()
    if fmt == "mxfp4":
        quantize_model_mxfp4(model, kv_cache=kv_cache, activations=activations)
    else:
        quantize_model_fp8(model, kv_cache=kv_cache)
    torch.cuda.empty_cache()
    weight_bytes = sum(b.numel() * b.element_size() for n, b in model.named_buffers() if "weight_" in n)
    prompts = [p.to(dev) for p in synth_prompts(rows, prompt, cfg.padded_vocab_size, seed=1337)]
    model.set_capacity(rows, prompt + new_tokens, 32 * prompt)
    kw = dict(temperature=0.2, top_k=1, eos_id=None, prefill_batch=32)
    generate_batch(model, prompts, new_tokens, **kw)                      # warm-up: code objects, the decode graph
    ms, pre = [], []
    for _ in range(repeats):
        t = {}
        generate_batch(model, prompts, new_tokens, timing=t, **kw)
        ms.append(t["decode_ms"] / t["decode_steps"])
        pre.append(t["prefill_ms"])
    eng = model._engine
    med = statistics.median(ms)
    out = dict(ms_per_step=[round(v, 4) for v in ms], median_ms_per_step=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4),
               prefill_ms=[round(v, 3) for v in pre], median_prefill_ms=round(statistics.median(pre), 3),
               prefill_spread=round((max(pre) - min(pre)) / statistics.median(pre), 4), prefill_tokens=rows * prompt,
               rows=rows, engine_device_bytes=int(eng.lib.dh_engine_device_bytes(eng.handle)), quantised_weight_bytes=int(weight_bytes),
               torch_allocated_bytes=int(torch.cuda.memory_allocated()))
    print(json.dumps({"step": {f"{fmt}.kv_{kv_cache}" + ("" if activations == "fp8" else f".act_{activations}"): out}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default="profiles/mxfp4.json")
    ap.add_argument("--prefill_m", type=int, default=49152, help="rows of the tiled comparison: 32 prompts of 1536 tokens (llama3-8b-fp8)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also the step-level comparison (loads Llama-3-8B four times)")
    ap.add_argument("--no_kernel", action="store_true", help="skip the kernel-level comparison")
    ap.add_argument("--step_timeout", type=int, default=600, help="seconds each child may take")
    ap.add_argument("--activations", choices=("fp8", "mxfp6"), default="fp8",
                    help="mxfp6: the MXFP6-activation arm against the e4m3-activation MXFP4 kernels, the quantisers, and (with --step) the two engines")
    ap.add_argument("--worker", type=str, default=None, help="internal: one child's part")
    a = ap.parse_args()
    if a.worker:
        part = a.worker.split(":")
        if part[0] == "kernel":
            kernel_level(part[1], int(part[2]), a.repeats, a.activations)
        elif part[0] == "quant":
            quant_level(int(part[1]), int(part[2]), a.repeats)
        else:
            step_level(part[1], part[2], 128, 512, 33, a.repeats, part[3] if len(part) > 3 else "fp8")
        return
    assert torch.cuda.is_available(), "bench_mxfp4.py needs an MI355X"
    parts = [] if a.no_kernel else [f"kernel:{n}:{m}" for m in (32, 128, a.prefill_m) for n in LINEARS]
    if a.activations == "mxfp6" and not a.no_kernel:
        parts += [f"quant:{k}:{m}" for m in (32, 128, a.prefill_m) for k in (4096, 14336)]
    if a.step:
        parts += ([f"step:mxfp4:bf16:{act}" for act in ("fp8", "mxfp6")] if a.activations == "mxfp6"
                  else [f"step:{f}:{kv}" for kv in ("bf16", "fp8") for f in ("fp8", "mxfp4")])
    res = {"prefill_m": a.prefill_m, "repeats": a.repeats, "hbm_peak_bytes_per_s": HBM_PEAK, "activations": a.activations, "kernel": {}, "quant": {}, "step": {}}
    for part in parts:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", part, "--repeats", str(a.repeats), "--activations", a.activations]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.step_timeout)      # a part that fails ends the tool
        if r.returncode != 0:
            sys.exit(f"part {part} failed with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                print(l, flush=True)
                for k, v in json.loads(l).items():
                    res[k].update(v)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
