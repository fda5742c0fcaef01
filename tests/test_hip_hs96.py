"""Head size 96 (Phi-3.5-mini-instruct's attention: 32 heads of 96, multi-head) on the GPU: the assertions the suite makes at
head sizes 64 and 128, restated for hs 96 in the multi-head (q_per_kv = 1) and grouped shapes.

The bodies are the existing tests' own (imported as modules and called with the hs-96 parameters), so the gates are the same
ones: kernels against the oracle's SDPA and fp64 rope / attention backward, the tiny end-to-end models against tensors the
reference produced (tests/golden/make_golden_hs96.py), the LoRA micro-step against the reference's gradients.
"""
import pytest
import torch

import test_hip_model as model_tests
import test_hip_ops as ops_tests
import test_hip_train as train_tests
import test_hip_train_bwd as bwd_tests

pytestmark = pytest.mark.gpu

TINY96 = ["tiny_hs96_r16", "tiny_hs96_gqa_r16"]
# (n_head, n_groups): multi-head as Phi-3.5 (small and at its 32 heads), grouped
MHA_GQA = [(4, 4), (32, 32), (4, 2), (8, 2)]


@pytest.fixture
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_head,n_groups,case", [(4, 4, "short"), (4, 2, "short"), (8, 2, "short"), (8, 2, "long"), (4, 4, "long"), (32, 32, "long")])
def test_qkv_rope_cache_and_prefill_attention_hs96(dev, n_head, n_groups, case):
    ops_tests.test_qkv_rope_cache_and_prefill_attention(dev, 96, n_head, n_groups, case)


@pytest.mark.parametrize("n_head,n_groups,case", [(4, 4, "short"), (32, 32, "short"), (8, 2, "short"), (4, 4, "long"), (8, 2, "long")])
def test_chunked_prefill_and_decode_attention_hs96(dev, n_head, n_groups, case):
    ops_tests.test_chunked_prefill_and_decode_attention(dev, 96, n_head, n_groups, case)


@pytest.mark.parametrize("n_head,n_groups,r,case", [(4, 4, 16, "short"), (32, 32, 16, "short"), (8, 2, 16, "short"), (4, 4, 16, "long"),
                                                    (8, 2, 4, "long")])
def test_fused_decode_kernels_hs96(dev, n_head, n_groups, r, case):
    ops_tests.test_fused_decode_kernels(dev, 96, n_head, n_groups, r, case)


@pytest.mark.parametrize("n_head,n_groups", MHA_GQA)
def test_qkv_rope_bwd_against_fp64_hs96(n_head, n_groups):
    bwd_tests.test_qkv_rope_bwd_against_fp64(96, n_head, n_groups)


@pytest.mark.parametrize("n_head,n_groups", MHA_GQA)
def test_attention_bwd_per_row_against_fp64_hs96(n_head, n_groups):
    bwd_tests.test_attention_bwd_per_row_against_fp64(96, n_head, n_groups)


@pytest.mark.parametrize("n_head,n_groups,n", [(32, 32, 1025), (4, 2, 300)])
def test_attention_bwd_single_sequence_hs96(n_head, n_groups, n):
    bwd_tests.test_attention_bwd_single_sequence(96, n_head, n_groups, n)


@pytest.mark.parametrize("n_head,n_groups", [(4, 4), (8, 2)])
def test_rope_and_attention_bwd_hs96(n_head, n_groups):
    train_tests.test_rope_and_attention_bwd(96, n_head, n_groups)


@pytest.mark.parametrize("heads", [3, 32])
def test_fragment_order_transpose_from_the_inverse_map_hs96(heads):
    train_tests.test_fragment_order_transpose_from_the_inverse_map(96, heads)


def test_fused_qkv_epilogue_refuses_hs96(dev):
    """The QKV GEMM's rope + cache epilogue is built for 64 and 128: head size 96 is refused, pointing at the two-step path the
    engine takes instead, and never runs on another size's code."""
    from dualhyp_amd import ops, _lib
    from oracle import ger_oracle as O
    H, G, hs, M, K = 4, 4, 96, 512, 384
    x = torch.zeros((M, K), dtype=torch.bfloat16, device=dev)
    w = torch.zeros(((H + 2 * G) * hs, K), dtype=torch.bfloat16, device=dev)
    cos, sin = O.build_rope_cache(64, hs)
    kc = torch.zeros((1, G, 64, hs), dtype=torch.bfloat16, device=dev)
    vt = torch.zeros((1, G, hs, 64), dtype=torch.bfloat16, device=dev)
    i32 = torch.int32
    with pytest.raises(_lib.DualHypHipError, match=r"head_size 96 unsupported \(64 or 128; use dh_linear_bf16 \+ dh_qkv_rope_cache_bf16\)"):
        ops.linear_qkv_rope_cache(x, w, cos.to(dev), sin.to(dev), torch.zeros(M, dtype=i32, device=dev),
                                  torch.zeros(M, dtype=i32, device=dev), kc, vt, H, G)


# ---- tiny models end to end against the reference -------------------------------------------------------------------
@pytest.mark.parametrize("name", TINY96)
def test_forward_nocache_and_cache_hs96(golden, name):
    model_tests.test_forward_nocache_and_cache(golden, name)


@pytest.mark.parametrize("name", TINY96)
def test_generate_ids_hs96(golden, name):
    model_tests.test_generate_ids(golden, name)


@pytest.mark.parametrize("name", TINY96)
def test_merged_lora_matches_unmerged_hs96(golden, name):
    model_tests.test_merged_lora_matches_unmerged(golden, name)


@pytest.mark.parametrize("name", TINY96)
def test_joint_decode_is_batch_invariant_hs96(golden, name):
    model_tests.test_joint_decode_is_batch_invariant(golden, name)


@pytest.mark.parametrize("name", TINY96)
def test_train_micro_step_matches_reference_hs96(golden, name):
    train_tests.test_train_micro_step_matches_reference(golden, name)


# ---- Phi-3.5's own layer shape against the reference ------------------------------------------------------------------
def test_phi35_shape_vs_reference(golden):
    """Phi-3.5-mini-instruct's layer shape (d 3072, 32 heads of 96, multi-head, I 8192, V 32 064 untied, LoRA r 16), 2 layers, a
    DualHyp-length prompt (T = 560) + 16 decode steps, bf16, against the reference (tests/golden/phi35_shape), with the gates of
    test_llama3_8b_shape_vs_reference.  At this shape a single-token step splits the QKV / projection GEMMs into 12 K-slices and the
    MLP down-projection into 16 (the fused decode attention's n_part > 8 forms), and the head's last 256-column tile is ragged
    (32 064 = 250 x 128 + 64): prefill logits, decode logits and the sampled ids all cross it.  A joint decode of three prompts
    keeps the first one's ids (batched decode at these widths)."""
    from dualhyp_amd import generate, generate_batch
    t, meta = golden("phi35_shape")
    cfg, m = model_tests.build(meta)
    assert (cfg.n_embd, cfg.head_size, cfg.n_head, cfg.n_query_groups, cfg.intermediate_size, cfg.padded_vocab_size) == \
        (3072, 96, 32, 32, 8192, 32064)
    T, G = meta["T"], meta["G"]
    ids, margins = t["generate_ids"], t["generate_margins_ulps"]
    DEV = model_tests.DEV
    with torch.no_grad():
        lg = m(t["idx"].view(1, -1).to(DEV), torch.arange(T, device=DEV))[0].float().cpu()
    m.reset_cache()
    model_tests.gate(lg[-4:, :4096], t["prefill_logits_last4_v4096"], t["prefill_logits_last4_v4096_fp32"], "phi35_shape prefill logits")
    model_tests.gate(lg[-4:, -256:], t["prefill_logits_last4_tail256"], t["prefill_logits_last4_tail256_fp32"], "phi35_shape prefill vocab tail")
    got = model_tests._teacher_forced(m, t["idx"], ids, T, G)
    model_tests.gate(got[:, :4096], t["step_logits_v4096"], t["step_logits_fp32_v4096"], "phi35_shape step logits")
    decided = margins >= model_tests.SAFE_MARGIN_ULPS
    assert bool(decided.all()), "fixture must be tie-free on every step"
    assert bool((got.argmax(-1) == ids[T:T + G]).all()), "arg-max differs from the reference on a decided step"
    free = generate(m, t["idx"].to(DEV), T + G, temperature=0.2, top_k=1).cpu()
    model_tests.record_parity("phi35_shape.generate_ids", generated=G, min_margin_ulps=float(margins.min()),
                              ids_equal_prefix=model_tests._equal_prefix(free[T:], ids[T:]))
    assert torch.equal(free, ids)
    idx = t["idx"].to(DEV)
    joint = generate_batch(m, [idx, idx[:301], idx[:517]], G, temperature=0.2, top_k=1)
    assert torch.equal(joint[0].cpu(), ids), "joint decode changed the first prompt's ids"


def test_train_micro_step_phi35_shape(golden):
    """One LoRA micro-step at Phi-3.5's layer shape (2 layers, T = 560, the last 48 positions are the answer) against the
    reference's autograd in fp32, bf16-true and bf16-mixed (tests/golden/train_phi35_shape), with the gates of
    test_train_micro_step_tinyllama_shape: loss within 1.3x the reference's own bf16 / mixed distance to fp32, every LoRA
    gradient within 1.3x their distance (or 0.02 of its scale).  The fixture keeps the gradients on a fixed sample (every
    `stride`-th row of lora_B, column of lora_A) and the whole fp32 gradient's (max |g|, ||g||)."""
    from dualhyp_amd import GPT, Config, chunked_cross_entropy
    from dualhyp_amd.synth import synth_state_dict
    from dualhyp_amd.train import prepare_for_training
    DEV = model_tests.DEV
    t, meta = golden("train_phi35_shape")
    cfg = Config(**meta["config"])
    stride = meta["stride"]
    sd = synth_state_dict(cfg, seed=meta["seed"], norm_jitter=meta["norm_jitter"], device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.cpu_rsqrt_vec_width = 32
    m.train()
    prepare_for_training(m)
    ids, labels = t["input_ids"].to(DEV), t["labels"].to(DEV)
    logits = m(ids, lm_head_chunk_size=128)
    logits[-1] = logits[-1][..., :-1, :]
    loss = chunked_cross_entropy(logits, labels[..., 1:], chunk_size=128)
    (loss / meta["grad_accum"]).backward()
    l32, lbf, lmx = (t[f"{k}.train_loss"].float().item() for k in ("fp32", "bf16", "mixed"))
    assert abs(loss.item() - l32) <= max(1.3 * abs(lbf - l32), 1.3 * abs(lmx - l32), 1e-3), (loss.item(), l32, lbf, lmx)
    worst = {"hip": 0.0, "bf16": 0.0, "mixed": 0.0}
    n_lora = 0
    for n, p in m.named_parameters():
        if "lora_" not in n:
            continue
        n_lora += 1
        full = p.grad.float().cpu()
        g = full[::stride] if "lora_B" in n else full[:, ::stride]
        g32 = t[f"fp32.grad.{n}"].float()
        assert g.shape == g32.shape, n
        scale = g32.abs().max().item()
        e = {"hip": (g - g32).abs().max().item() / scale, "bf16": t[f"bf16.graderr.{n}"].item(), "mixed": t[f"mixed.graderr.{n}"].item()}
        for k in worst:
            worst[k] = max(worst[k], e[k])
        assert e["hip"] <= max(1.3 * max(e["bf16"], e["mixed"]), 0.02), f"{n}: {e}"
        gmax, gnorm = t[f"fp32.gradstat.{n}"].tolist()
        assert abs(full.abs().max().item() - gmax) <= max(1.3 * max(e["bf16"], e["mixed"]), 0.02) * gmax, f"{n}: max |g|"
        assert abs(full.norm().item() - gnorm) <= 0.05 * gnorm, f"{n}: ||g||"
    assert n_lora == 4 * cfg.n_layer
    assert worst["hip"] <= 1.3 * max(worst["bf16"], worst["mixed"]), worst
    model_tests.record_parity("train_phi35_shape.lora_grads", loss_hip=loss.item(), loss_fp32=l32, loss_bf16=lbf, loss_mixed=lmx,
                              worst_hip=worst["hip"], worst_ref_bf16=worst["bf16"], worst_ref_mixed=worst["mixed"])


# ---- the serving CLI ------------------------------------------------------------------------------------------------
def test_inference_cli_hs96_random_init(tmp_path):
    """`python -m dualhyp_amd.inference --config_name parity-hs96 --random_init` (multi-head, head size 96) end to end: DualHyp prompts
    of ~700 byte tokens through prefill and joint decode, predictions written in the reference's format."""
    import json
    import subprocess
    import sys
    import test_harness as harness
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    cmd = [sys.executable, "-m", "dualhyp_amd.inference", "--test_path", str(test_json), "--config_name", "parity-hs96", "--random_init",
           "--tokenizer", "byte", "--prompts_format", "DualHyp", "--dual_hypotheses", "--max_new_tokens", "12", "--decode_batch", "4",
           "--predict_dir", str(tmp_path / "pred")]
    out = subprocess.run(cmd, cwd=tmp_path, env=harness._env(), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2 and set(js[0]) == {"inference", "ground_truth"} and set(js[-2]) == {"wer", "gtms"}


def test_inference_cli_chat_template(tmp_path):
    """`--apply_chat_template` end to end with a Hugging Face tokenizer that carries a chat template (tests/golden/phi_chat_tokenizer):
    the harness packs every prompt through the template, as the reference does for Phi-3.5, and decodes it."""
    import json
    import shutil
    import subprocess
    import sys
    import test_harness as harness
    from conftest import GOLDEN
    items = harness.merged_items()
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    ckpt = tmp_path / "parity-hs96"
    shutil.copytree(GOLDEN / "phi_chat_tokenizer", ckpt)
    cmd = [sys.executable, "-m", "dualhyp_amd.inference", "--test_path", str(test_json), "--llm_checkpoint", str(ckpt), "--random_init",
           "--tokenizer", "hf", "--apply_chat_template", "--prompts_format", "DualHyp", "--dual_hypotheses", "--max_new_tokens", "12",
           "--decode_batch", "4", "--predict_dir", str(tmp_path / "pred")]
    out = subprocess.run(cmd, cwd=tmp_path, env=harness._env(), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    js = json.loads((tmp_path / "pred" / "random_init.json").read_text())
    assert len(js) == len(items) + 2 and set(js[0]) == {"inference", "ground_truth"}
