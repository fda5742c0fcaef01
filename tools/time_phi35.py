#!/usr/bin/env python3
"""Phi-3.5-mini-instruct shape (32 layers, 32 heads of 96, multi-head attention, d 3072, I 8192, V 32064), hash weights +
LoRA r16 on q/k/v/proj: DualHyp-length prompts (560 tokens) -> 64 tokens, greedy.  One batch of 32 and a decode batch of
4 x 32 decoded jointly (chunked prefill of 32); utt/s, prefill / decode ms and the prefill-attention us per launch.
Prints one JSON line per setting (profiles/ keeps the record).

    python tools/time_phi35.py [--decode_batches 4]
"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from dualhyp_amd import GPT, Config, GER_LORA, generate_batch          # noqa: E402
from dualhyp_amd.synth import synth_state_dict, synth_prompts           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--decode_batches", type=int, default=4, help="batches of 32 decoded jointly in the second setting")
ap.add_argument("--prompt", type=int, default=560)
ap.add_argument("--new", type=int, default=64)
a = ap.parse_args()

dev = "cuda:0"
cfg = Config.from_name("Phi-3.5-mini-instruct", **{**GER_LORA, "dropout": 0.0})
t0 = time.time()
sd = synth_state_dict(cfg, seed=1337, device=dev, embed_scale=50.0, head_tie=1.0)
m = GPT(cfg).to(device=dev, dtype=torch.bfloat16)
m.load_state_dict(sd, strict=True)
del sd
m.eval()
print(f"model built in {time.time() - t0:.1f}s, {sum(p.numel() for p in m.parameters()) / 1e9:.2f} B params", flush=True)
B, T, G = 32, a.prompt, a.new
V = cfg.padded_vocab_size
kv_mib = cfg.n_layer * 2 * cfg.n_query_groups * cfg.head_size * 2 * (T + G) / 2**20


def run(n_batches: int, seed: int) -> dict:
    corpus = [p.to(dev) for p in synth_prompts(B * n_batches, T, V, seed=seed)]
    generate_batch(m, corpus, G, temperature=0.2, top_k=1, prefill_batch=B)           # allocation + decode-graph capture
    eng = m.engine()
    eng.set_timing(True)
    phase = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = generate_batch(m, corpus, G, temperature=0.2, top_k=1, prefill_batch=B, timing=phase)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    attn_ms, attn_n = eng.get_timing(2)
    gemm_ms, gemm_n = eng.get_timing(0)
    eng.set_timing(False)
    assert all(x.numel() == T + G for x in o)
    return dict(model="Phi-3.5-mini-instruct", weights="hash + LoRA r16 (q,k,v,proj)", prompt=T, new_tokens=G, sequences=B * n_batches,
                prefill_batch=B, kv_cache_mib_per_sequence=round(kv_mib, 1), wall_ms=round(dt * 1e3, 1),
                utt_per_s=round(B * n_batches / dt, 2), prefill_ms=round(phase.get("prefill_ms", 0.0), 1),
                decode_ms=round(phase.get("decode_ms", 0.0), 1), decode_steps=phase.get("decode_steps", 0),
                prefill_attention_us_per_launch=round(1e3 * attn_ms / max(attn_n, 1), 1), prefill_attention_launches=attn_n,
                prefill_gemm_ms=round(gemm_ms, 1), ids_head=o[0][T:T + 8].tolist())


for nb, seed in ((1, 1), (a.decode_batches, 2)):
    print(json.dumps(run(nb, seed)), flush=True)
