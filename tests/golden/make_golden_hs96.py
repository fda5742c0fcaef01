#!/usr/bin/env python3
"""Golden vectors of head size 96 (Phi-3.5-mini-instruct's attention shape), by RUNNING THE REFERENCE ITSELF.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_hs96.py [--only NAME]

Uses the helpers of make_golden.py (reference import under stubs, `save`, `gen_tiny`).  Writes
  tiny_hs96_r16 / tiny_hs96_gqa_r16   gen_tiny on parity-hs96 (multi-head) / parity-hs96-gqa (4 heads, 2 groups)
  convert_hf_phi3                      a tiny Phi-3-named HF dict through the reference's copy_weights_phi
  phi35_config.json                    the fields of the reference's Config.from_name("Phi-3.5-mini-instruct")
  phi35_shape                          Phi-3.5's layer shape, 2 layers, a DualHyp-length prompt + 16 decode steps (bf16 + fp32 yardstick)
  train_phi35_shape                    one LoRA micro-step at that shape (fp32, bf16-true, bf16-mixed)
"""
from __future__ import annotations

import argparse
import json
import math

import torch

from make_golden import HERE, import_reference, save, gen_tiny, ref_model, cfg_kwargs_of, _margins_teacher_forced, _train_micro


def gen_convert_phi3(rlora) -> None:
    """HF Phi-3 checkpoint -> lit state dict by the reference's copy_weights_phi (scripts/convert_hf_checkpoint.py:204-291),
    fed in two shards (layer 1's gate_up_proj, o_proj and the final norm in the second).  Distinct integers pin the exact
    placement: qkv_proj is copied as it stands ([Q; K; V]) and gate_up_proj is chunked into fc_1 / fc_2."""
    import scripts.convert_hf_checkpoint as rconv
    kw = dict(name="Phi-3.5-mini-instruct", block_size=32, vocab_size=60, padding_multiple=4, n_layer=2, n_head=4, n_embd=64,
              rotary_percentage=1.0, parallel_residual=False, bias=False, _norm_class="RMSNorm", norm_eps=1e-5,
              _mlp_class="LLaMAMLP", intermediate_size=96)
    cfg = rlora.Config(**kw)
    hs, G, d, I, V = cfg.head_size, cfg.n_query_groups, cfg.n_embd, cfg.intermediate_size, cfg.padded_vocab_size
    counter = [0]

    def t(*shape):
        n = math.prod(shape)
        out = (torch.arange(n, dtype=torch.float32) + counter[0]).reshape(shape)
        counter[0] += n
        return out

    hf = {"model.embed_tokens.weight": t(V, d), "model.norm.weight": t(d), "lm_head.weight": t(V, d)}
    for l in range(cfg.n_layer):
        p = f"model.layers.{l}."
        hf.update({p + "input_layernorm.weight": t(d), p + "post_attention_layernorm.weight": t(d),
                   p + "self_attn.qkv_proj.weight": t((cfg.n_head + 2 * G) * hs, d), p + "self_attn.o_proj.weight": t(d, d),
                   p + "mlp.gate_up_proj.weight": t(2 * I, d), p + "mlp.down_proj.weight": t(d, I)})
    late = {k for k in hf if k.startswith("model.layers.1.mlp.gate_up") or k.startswith("model.layers.1.self_attn.o_proj")
            or k in ("model.norm.weight",)}
    shard1 = {k: v for k, v in hf.items() if k not in late}
    shard2 = {k: v for k, v in hf.items() if k in late}
    out, qkv = {}, {}
    rconv.copy_weights_phi(cfg, qkv, out, shard1)
    rconv.copy_weights_phi(cfg, qkv, out, shard2)
    tensors = {f"hf.{k}": v for k, v in hf.items()}
    tensors.update({f"lit.{k}": v for k, v in out.items()})
    try:
        rconv.copy_weights_phi(cfg, {}, {}, {"transformer.h.0.attn.attn.weight": t(4, 4)})
        outdated = "accepted"
    except ValueError as e:
        outdated = str(e)
    save("convert_hf_phi3", tensors, {"config": kw, "shard2_keys": sorted(late), "outdated_error": outdated,
                                      "leftover_qkv": {str(k): sorted(v) for k, v in qkv.items()}})


def gen_phi35_config(rlora) -> None:
    import ger.config as rcfg
    c = rcfg.Config.from_name("Phi-3.5-mini-instruct")
    fields = {k: v for k, v in vars(c).items() if isinstance(v, (int, float, str, bool, dict, type(None)))}
    (HERE / "phi35_config.json").write_text(json.dumps(fields, indent=1, sort_keys=True))
    print("wrote phi35_config.json")


def gen_phi35_shape(rlora, rgenerate, name: str, seed: int, T: int, G: int, n_layer: int) -> None:
    """Phi-3.5-mini-instruct's layer shape (d 3072, 32 heads of 96, multi-head, I 8192, V 32064 untied) with `n_layer` layers and
    LoRA r16 on q/k/v/proj, as gen_llama3_shape: prefill logits (last 4 positions: first 4096 and last 256 vocabulary entries),
    greedy ids of the reference's generate() with teacher-forced top-2 margins, bf16 + fp32 yardstick."""
    from dualhyp_amd.config import Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    cfg = Config.from_name("Phi-3.5-mini-instruct", **{**GER_LORA, "dropout": 0.0, "n_layer": n_layer})
    sd = synth_state_dict(cfg, seed=seed, embed_scale=50.0, head_tie=1.0)
    idx = synth_prompts(1, T, cfg.padded_vocab_size, seed=seed)[0]
    out = {"idx": idx}
    m = ref_model(rlora, cfg_kwargs_of(cfg), sd, torch.bfloat16)
    torch.manual_seed(seed)
    g = rgenerate(m, idx, T + G, temperature=0.2, top_k=1, eos_id=None)
    m.reset_cache()
    out["generate_ids"] = g
    with torch.no_grad():
        lg = m(idx.view(1, -1), torch.arange(T))[0]
        out["prefill_logits_last4_v4096"] = lg[-4:, :4096].clone()
        out["prefill_logits_last4_tail256"] = lg[-4:, -256:].clone()
        m.reset_cache()
    mg, first, tv, ti = _margins_teacher_forced(m, idx, g, T, G)
    out.update({"generate_margins_ulps": mg, "step_logits_v4096": first, "step_top8_values": tv, "step_top8_indices": ti})
    del m
    m32 = ref_model(rlora, cfg_kwargs_of(cfg), sd, torch.float32)
    with torch.no_grad():
        lg = m32(idx.view(1, -1), torch.arange(T))[0]
        out["prefill_logits_last4_v4096_fp32"] = lg[-4:, :4096].clone()
        out["prefill_logits_last4_tail256_fp32"] = lg[-4:, -256:].clone()
        m32.reset_cache()
    _, f32, _, _ = _margins_teacher_forced(m32, idx, g, T, G)
    out["step_logits_fp32_v4096"] = f32
    print(name, "margins", [round(float(x), 1) for x in mg], flush=True)
    save(name, out, {"config": cfg_kwargs_of(cfg), "seed": seed, "T": T, "G": G, "embed_scale": 50.0, "head_tie": 1.0})


def gen_train_phi35_shape(rlora, rutils, name: str, seed: int, T: int, n_layer: int, stride: int = 4) -> None:
    """gen_train_shape at Phi-3.5's layer shape: one micro-batch of T tokens (T - 48 prompt positions masked with -1), loss and
    LoRA gradients of finetune/ger.py:278-285 in fp32, bf16-true and bf16-mixed.  To stay within a committed file's size the
    gradients are kept on a fixed sample: every `stride`-th row of lora_B, every `stride`-th column of lora_A (fp32 run in
    full precision; the bf16 / mixed runs as their max error against it on that sample), plus (max |g|, ||g||) of the whole fp32
    gradient."""
    from dualhyp_amd.config import Config, GER_LORA
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    cfg = Config.from_name("Phi-3.5-mini-instruct", **{**GER_LORA, "dropout": 0.0, "n_layer": n_layer})
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25)
    ids = synth_prompts(1, T, cfg.padded_vocab_size, seed=seed)[0].view(1, -1)
    labels = ids.clone()
    labels[:, :T - 48] = -1
    out = {"input_ids": ids, "labels": labels}
    sample = lambda n, g: g[::stride] if "lora_B" in n else g[:, ::stride]
    for tag, dt, ac in (("fp32", torch.float32, False), ("bf16", torch.bfloat16, False), ("mixed", torch.float32, True)):
        m = ref_model(rlora, cfg_kwargs_of(cfg), sd, dt)
        m.train()
        rlora.mark_only_lora_as_trainable(m)
        out[f"{tag}.train_loss"] = _train_micro(rlora, rutils, m, ids, labels, 128, 32, ac)
        for n, p in m.named_parameters():
            if not p.requires_grad:
                continue
            g = sample(n, p.grad.float())
            if tag == "fp32":
                out[f"fp32.grad.{n}"] = g.contiguous()
                out[f"fp32.gradstat.{n}"] = torch.stack([p.grad.float().abs().max(), p.grad.float().norm()])
            else:
                g32 = out[f"fp32.grad.{n}"]
                out[f"{tag}.graderr.{n}"] = ((g - g32).abs().max() / g32.abs().max()).reshape(1)
        print(tag, "loss", float(out[f"{tag}.train_loss"]), flush=True)
        del m
    save(name, out, {"config": cfg_kwargs_of(cfg), "seed": seed, "T": T, "norm_jitter": 0.25, "grad_accum": 32, "stride": stride})


CHAT_TEMPLATE = ("{% for message in messages %}{{ '<|' + message['role'] + '|>\\n' + message['content'] + '<|end|>\\n' }}{% endfor %}"
                 "{% if add_generation_prompt %}{{ '<|assistant|>\\n' }}{% endif %}")


def gen_chat_packing() -> None:
    """Prompt packing with --apply_chat_template (Phi-3.5) by the reference's own get_prompt (data/av_dataset.py:205-256, 371-430)
    on a tiny byte-level BPE tokenizer built here with `tokenizers` (Phi-3-style special tokens, eos "<|end|>", a short chat
    template of its own), after the reference's Phi EOS override (eos -> "<|endoftext|>", inference/ger.py:196-198).  The
    reference targeted transformers 4.x, whose apply_chat_template(tokenize=True) returns the id list: the stand-in below gives it
    that list.  Writes the tokenizer to phi_chat_tokenizer/ and the ids / labels to phi_chat_packing.json."""
    import sys
    import types
    from tokenizers import Tokenizer, models, trainers, pre_tokenizers, decoders
    from transformers import PreTrainedTokenizerFast
    sys.path.insert(0, str(HERE.parent))
    import test_harness as harness
    import data.prompts as rprompts
    items = harness.merged_items(n=3)
    for name in ("h5py", "scipy", "scipy.io", "data.whisper", "data.visual_corruption"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["scipy.io"].wavfile = None
    sys.modules["data.utils"] = types.SimpleNamespace(get_preprocessing_pipelines=None, load_mouthroi=None, pad_mouth=None,
                                                      random_sample_sequence=None, word_emb_diff=None, sent_emb_diff=None)
    import data.av_dataset as rav
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    special = ["<s>", "</s>", "<|endoftext|>", "<|system|>", "<|user|>", "<|assistant|>", "<|end|>"]
    corpus = [rprompts.get_prompts_format(f)[k] for f in ("GER", "DualHyp") for k in ("prompt_1", "prompt_2", "prompt_3")]
    corpus += [it["Caption"] for it in items] + ["You are a helpful AI assistant."]
    tok.train_from_iterator(corpus, trainer=trainers.BpeTrainer(vocab_size=420, special_tokens=special,
                                                                initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    hf = PreTrainedTokenizerFast(tokenizer_object=tok, bos_token="<s>", eos_token="<|end|>")
    hf.chat_template = CHAT_TEMPLATE
    out_dir = HERE / "phi_chat_tokenizer"
    hf.save_pretrained(str(out_dir))
    hf.eos_token = "<|endoftext|>"                                   # the reference's override for phi- configs

    class V4:                                                        # transformers 4.x: apply_chat_template(tokenize=True) -> ids
        def __init__(self, t):
            self.t = t

        def __getattr__(self, k):
            return getattr(self.t, k)

        def __call__(self, *a, **k):
            return self.t(*a, **k)

        def apply_chat_template(self, *a, **k):
            return list(self.t.apply_chat_template(*a, **k)["input_ids"])

    rec = {"eos_token": hf.eos_token, "eos_token_id": hf.eos_token_id, "system": "You are a helpful AI assistant.", "items": items,
           "GER": [], "DualHyp": []}
    for fmt, cls in (("GER", rav.AVDataset), ("DualHyp", rav.DualHypothesesAVDataset)):
        ds = object.__new__(cls)
        pf = rprompts.get_prompts_format(fmt)
        ds.prompt_1, ds.prompt_2, ds.prompt_3 = pf["prompt_1"], pf["prompt_2"], pf["prompt_3"]
        ds.tokenizer, ds.apply_chat_template, ds.max_nhyps, ds.random_sample_nhyps = V4(hf), True, None, False
        ds.nhyps_key, ds.nhyps_key_asr, ds.nhyps_key_vsr = "nhyps_asr", "nhyps_asr", "nhyps_vsr"
        for it in items:
            r = ds.get_prompt(it) if fmt == "GER" else ds.get_prompt(it, it)
            rec[fmt].append({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items()})
    (HERE / "phi_chat_packing.json").write_text(json.dumps(rec, indent=0))
    print("wrote phi_chat_tokenizer/, phi_chat_packing.json")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    torch.set_num_threads(8)
    rlora, rmodel, rutils, rgenerate, rprompts = import_reference()
    want = lambda k: (not a.only) or a.only == k
    if want("tiny"):
        gen_tiny(rlora, rutils, rgenerate, "tiny_hs96_r16", "parity-hs96", r=16, seed=9696)
        gen_tiny(rlora, rutils, rgenerate, "tiny_hs96_gqa_r16", "parity-hs96-gqa", r=16, seed=9697)
    if want("convert"):
        gen_convert_phi3(rlora)
    if want("config"):
        gen_phi35_config(rlora)
    if want("chat"):
        gen_chat_packing()
    if want("phi35_shape"):
        gen_phi35_shape(rlora, rgenerate, "phi35_shape", seed=1337, T=560, G=16, n_layer=2)
    if want("train_phi35_shape"):
        gen_train_phi35_shape(rlora, rutils, "train_phi35_shape", seed=1337, T=560, n_layer=2)


if __name__ == "__main__":
    main()
