"""Sharded GER / DualHyp inference + WER — the MI355X counterpart of inference/ger.py:30-124.

The reference decodes the test set one utterance at a time on every rank (no sharding, quirk Q4).
Here each rank takes a strided shard of the utterances, decodes them in batches through
`generate_batch` (one packed prefill + hipGraph decode per batch) and the ranks all-reduce four
integers (edit errors, reference words, exact matches, count) for the corpus WER; predictions are
gathered to rank 0.  No collective runs inside the decode loop."""
from __future__ import annotations

import math
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Sequence

import torch

from .wer import post_normalize, wer_counts


def shard_indices(n: int, rank: int, world: int) -> List[int]:
    """Strided shard: rank r takes r, r+world, ... (balanced to within one utterance)."""
    return list(range(rank, n, world))


def extract_answer(decoded_full: str, decoded_prompt: str) -> str:
    """inference/ger.py:84-86: strip the prompt text, keep the first line."""
    return decoded_full[len(decoded_prompt):].split("\n")[0].strip()


def _reduce_counts(c: Dict[str, int], device) -> Dict[str, int]:
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return c
    keys = sorted(c)
    if dist.get_backend() == "gloo":
        device = "cpu"
    t = torch.tensor([c[k] for k in keys], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return dict(zip(keys, t.tolist()))


def _gather(obj: Any) -> List[Any]:
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [obj]
    out: List[Any] = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def _finite_or_none(v: float) -> Optional[float]:
    """JSON has no NaN or infinity: they are written as null."""
    v = float(v)
    return v if math.isfinite(v) else None


def run_inference(generate_fn: Callable[[List[torch.Tensor]], List[torch.Tensor]], examples: Sequence[Dict[str, Any]],
                  decode: Callable[[torch.Tensor], str], *, batch_size: int = 32, rank: int = 0, world: int = 1,
                  device="cpu", eos_id: Optional[int] = None) -> Dict[str, Any]:
    """examples[i] needs 'input_ids_no_response' (1-D ids) and 'ground_truth'.  `generate_fn` maps a
    list of prompts to a list of prompt+continuation id tensors (dualhyp_amd.generate_batch bound to a
    model; a stub in the CPU tests), or to the pair (that list, a list of 1-D float tensors with the log-probability of every
    generated token, the EOS included: generate_batch(return_logprobs=True)); with the pair every prediction record gains
    'sum_logprob' and 'avg_logprob' (the mean over those tokens); or to the triple (those two, a list of (ids [n, K], values [n, K])
    with the K alternatives of every generated token: generate_batch(top_logprobs=K)), with which a record also gains, one entry per
    generated token, 'token_ids' (the EOS, which the id tensors leave out, is `eos_id`), 'token_logprobs' and 'top_logprobs' (K
    [id, log-probability] pairs); values that are not finite are written as null.  Or to a dict {'beams': per prompt the ranked
    hypotheses of dualhyp_amd.beam_search_batch, 'logprobs': bool}: the prediction is the best hypothesis, every record gains
    'beams', one {'text', 'sum_logprob', 'avg_logprob', 'finished'} per hypothesis in rank order, and with 'logprobs' the best
    one's 'sum_logprob' and 'avg_logprob' as above.  A generate_fn with a true attribute `constrained` (--constrain: it decodes under
    per-utterance token masks or automata) marks every record with 'constrained': true, and one with an attribute `constrain_order` = K > 0
    (--constrain chain) gives every record 'constrain_order': K as well.  A generate_fn with an attribute `no_repeat_ngram` = N > 0
    (--no_repeat_ngram) gives every record 'no_repeat_ngram': N and 'ngram_bans': the generated positions (of the ids it returned)
    whose pick had a non-empty ban set, counted on the host from those ids (dualhyp_amd.ngram.ban_positions).  A generate_fn with a
    true attribute `stop` (--stop / --stop_file: it decodes under a stop specification) gives every record 'finish_reason', "eos",
    "length" or "stop": it leaves them, one per prompt of the call it has just answered, in its attribute `finish_reasons` (from
    the call's `done` flags, dualhyp_amd.stop.finish_reasons); with beams the best hypothesis' own 'finish_reason' is taken and every
    entry of 'beams' carries its own.  A generate_fn with an attribute `sampling` (--temperature / --top_k / --top_p / --min_p: a dict
    {temperature, top_k, top_p, min_p, seed}, set when any of them is not the default) gives every record 'sampling', a copy of it.
    A generate_fn with an attribute `penalties` (--repetition_penalty / --frequency_penalty / --presence_penalty: a dict {repetition,
    frequency, presence}, set when any of them is not the default) gives every record 'penalties', a copy of it.
    A generate_fn with an attribute `bias` (--bias_file: a dict {entries, default_boost}) and `bias_entries` (its (ids, boost) pairs)
    gives every record 'bias', a copy of the dict, and 'bias_hits', the generated tokens that continued a listed phrase when they were
    picked (dualhyp_amd.bias.bias_hits).
    Or to a dict {'samples': per prompt the N sampled candidates of dualhyp_amd.sample_batch, 'select': 'avg_logprob' | 'sum_logprob' |
    'mbr', 'logprobs': bool}: the prediction is the text of the candidate dualhyp_amd.select.select chooses among the candidates'
    answers, every record gains 'samples', one {'text', 'sum_logprob', 'avg_logprob', 'finish_reason', 'key'} per candidate in sample
    order ('key' is its selection key: the score, or the mbr risk), and 'selected', the chosen index; 'logprobs', 'finish_reason' and
    the alternatives, where asked for, are the chosen candidate's.
    A generate_fn with a true attribute `shared_prompt` (--share_prompt_kv: its decode steps read an utterance's prompt tiles once for
    its candidates or beams) gives every record 'shared_prompt': true; one with an attribute `beam_kv` of "table" (--beam_kv table:
    the beams' closed KV tiles are read where they were written) gives every record 'beam_kv': "table".
    Returns corpus metrics on every rank and predictions on
    rank 0."""
    mine = shard_indices(len(examples), rank, world)
    preds: Dict[int, Dict[str, str]] = {}
    for b in range(0, len(mine), batch_size):
        idxs = mine[b:b + batch_size]
        prompts = [examples[i]["input_ids_no_response"] for i in idxs]
        outs = generate_fn(prompts)
        stopping = bool(getattr(generate_fn, "stop", False))
        reasons = list(getattr(generate_fn, "finish_reasons", None) or ()) if stopping else []
        lps = tops = beams = sampled = None
        if isinstance(outs, dict) and "samples" in outs:
            from .select import select
            sampled = []                # per prompt: (candidates, their answers, the chosen index, the selection keys)
            for p, cands in zip(prompts, outs["samples"]):
                text = decode(p)
                texts = [extract_answer(decode(torch.cat([p.reshape(-1).cpu(), c["tokens"].reshape(-1).cpu()])), text) for c in cands]
                sampled.append((cands, texts) + select(cands, texts, outs.get("select", "avg_logprob")))
            chosen = [cands[best] for cands, _, best, _ in sampled]
            lps = [c["token_logprobs"] for c in chosen] if outs.get("logprobs") else None
            tops = [c["top_logprobs"] for c in chosen] if lps is not None and all("top_logprobs" in c for c in chosen) else None
            if stopping:
                reasons = [c.get("finish_reason") for c in chosen]
            outs = [torch.cat([p.reshape(-1).cpu(), c["tokens"].reshape(-1).cpu()]) for p, c in zip(prompts, chosen)]
        elif isinstance(outs, dict):
            beams = outs["beams"]
            lps = [hyps[0]["token_logprobs"] for hyps in beams] if outs.get("logprobs") else None
            if stopping:
                reasons = [hyps[0].get("finish_reason") for hyps in beams]
            outs = [hyps[0]["tokens"] for hyps in beams]
        elif isinstance(outs, tuple):
            if len(outs) == 3:
                outs, lps, tops = outs
            else:
                outs, lps = outs
        if stopping and len(reasons) != len(prompts):
            raise ValueError(f"generate_fn.stop is set, but generate_fn.finish_reasons holds {len(reasons)} reasons for {len(prompts)} prompts")
        for k, (i, p, o) in enumerate(zip(idxs, prompts, outs)):
            preds[i] = {"inference": extract_answer(decode(o), decode(p)),
                        "ground_truth": examples[i]["ground_truth"].strip()}
            if getattr(generate_fn, "constrained", False):
                preds[i]["constrained"] = True
            if getattr(generate_fn, "constrain_order", 0):
                preds[i]["constrain_order"] = int(generate_fn.constrain_order)
            if getattr(generate_fn, "no_repeat_ngram", 0):
                from .ngram import ban_positions
                preds[i]["no_repeat_ngram"] = int(generate_fn.no_repeat_ngram)
                preds[i]["ngram_bans"] = len(ban_positions(o.reshape(-1)[p.numel():].tolist(), int(generate_fn.no_repeat_ngram)))
            if stopping:
                preds[i]["finish_reason"] = reasons[k]
            if getattr(generate_fn, "sampling", None):
                preds[i]["sampling"] = dict(generate_fn.sampling)
            if getattr(generate_fn, "speculate_verify", "argmax") != "argmax":
                preds[i]["speculate_verify"] = str(generate_fn.speculate_verify)
            if getattr(generate_fn, "penalties", None):
                preds[i]["penalties"] = dict(generate_fn.penalties)
            if getattr(generate_fn, "activations", "fp8") != "fp8":
                preds[i]["activations"] = str(generate_fn.activations)
            if getattr(generate_fn, "shared_prompt", False):
                preds[i]["shared_prompt"] = True
            if getattr(generate_fn, "beam_kv", "copy") == "table":
                preds[i]["beam_kv"] = "table"
            if getattr(generate_fn, "bias", None):
                from .bias import bias_hits
                preds[i]["bias"] = dict(generate_fn.bias)
                preds[i]["bias_hits"] = bias_hits(o.reshape(-1)[p.numel():].tolist(), generate_fn.bias_entries)
            if beams is not None:
                text = decode(p)
                preds[i]["beams"] = [{"text": extract_answer(decode(hyp["tokens"]), text), "sum_logprob": _finite_or_none(hyp["sum_logprob"]),
                                      "avg_logprob": _finite_or_none(hyp["sum_logprob"] / max(int(hyp["token_logprobs"].numel()), 1)),
                                      "finished": bool(hyp["finished"]),
                                      **({"finish_reason": hyp.get("finish_reason")} if stopping else {})} for hyp in beams[k]]
            if sampled is not None:
                cands, texts, best, keys = sampled[k]
                preds[i]["samples"] = [{"text": t, "sum_logprob": _finite_or_none(c["sum_logprob"]), "avg_logprob": _finite_or_none(c["avg_logprob"]),
                                        "finish_reason": c.get("finish_reason"), "key": None if key is None else _finite_or_none(key)}
                                       for c, t, key in zip(cands, texts, keys)]
                preds[i]["selected"] = int(best)
            if lps is not None:
                total = float(lps[k].double().sum())
                preds[i]["sum_logprob"] = total
                preds[i]["avg_logprob"] = total / max(int(lps[k].numel()), 1)
            if tops is not None:
                ids = o.reshape(-1)[p.numel():].tolist()
                ids += [eos_id] * (int(lps[k].numel()) - len(ids))       # behind an EOS the log-probabilities have one entry more
                t_ids, t_lp = (t.tolist() for t in tops[k])
                preds[i]["token_ids"] = ids
                preds[i]["token_logprobs"] = [_finite_or_none(v) for v in lps[k].tolist()]
                preds[i]["top_logprobs"] = [[[int(a), _finite_or_none(b)] for a, b in zip(ra, rb)] for ra, rb in zip(t_ids, t_lp)]
    order = sorted(preds)
    pr = [preds[i]["inference"] for i in order]
    gt = [preds[i]["ground_truth"] for i in order]
    raw = _reduce_counts(wer_counts(pr, gt), device)
    post = _reduce_counts(wer_counts([post_normalize(p) for p in pr], [post_normalize(g) for g in gt]), device)
    gathered = _gather(preds)
    merged: Dict[int, Dict[str, str]] = {}
    for g in gathered:
        merged.update(g)
    n = max(raw["n"], 1)
    return {"WER": raw["errors"] / max(raw["ref_words"], 1), "gtms": raw["exact"] / n,
            "post_ST_wer": post["errors"] / max(post["ref_words"], 1), "post_gtms": post["exact"] / n,
            "n": raw["n"], "predictions": [merged[i] for i in sorted(merged)] if rank == 0 else None}


# ------------------------------------------------------------------------------------------ harness
def read_token_ids(path) -> List[int]:
    """The token ids of a --constrain_extra file: one non-negative integer per line; blank lines and `#` comments are skipped."""
    ids = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if not line.isdigit():
            raise ValueError(f"{path}:{n}: a token id is a non-negative integer, got {line!r}")
        ids.append(int(line))
    return ids


def stop_from_args(args, tokenizer, vocab: int, device=None):
    """The stop specification of --stop and --stop_file (dualhyp_amd.stop.compile_stop), or None when both are off."""
    from .stop import compile_stop, newline_ids, read_stop_file
    ids, seqs = [], []
    if getattr(args, "stop", "off") == "newline":
        ids += newline_ids(tokenizer, vocab)
    if getattr(args, "stop_file", None):
        f_ids, f_seqs = read_stop_file(args.stop_file)
        ids += f_ids
        seqs += f_seqs
    spec = compile_stop(ids, seqs, vocab, device) if ids or seqs else None
    return spec if spec else None


def bias_from_args(args, tokenizer, vocab: int):
    """((ids, boost) pairs, the records' `bias` field) of --bias_file and --bias_boost, checked against `vocab`, or (None, None) when
    the flag is off."""
    if not getattr(args, "bias_file", None):
        return None, None
    from .bias import DEFAULT_BOOST, check_bias, entries_from_lines, read_bias_file, record
    default = float(getattr(args, "bias_boost", DEFAULT_BOOST))
    entries = check_bias(entries_from_lines(read_bias_file(args.bias_file, default), tokenizer), vocab)
    return [(list(ids), b) for ids, b in entries], record(len(entries), default)


SAMPLING_DEFAULTS = dict(temperature=0.2, top_k=1, top_p=1.0, min_p=0.0)      # inference/ger.py:71-72 decodes greedily at 0.2


def sampling_from_args(args) -> Optional[Dict[str, Any]]:
    """{temperature, top_k, top_p, min_p, seed} of --temperature / --top_k / --top_p / --min_p when any of them is not the default,
    None for the default run (whose calls and records are the ones they always were)."""
    got = {k: getattr(args, k, v) for k, v in SAMPLING_DEFAULTS.items()}
    got = dict(temperature=float(got["temperature"]), top_k=int(got["top_k"]), top_p=float(got["top_p"]), min_p=float(got["min_p"]))
    if got == SAMPLING_DEFAULTS:
        return None
    got["seed"] = int(getattr(args, "seed", 1337))
    return got


def add_lora_arguments(parser) -> None:
    """The LoRA flags shared by both reference harnesses (inference/ger.py:145-153, finetune/ger.py:386-394).
    `type=bool` is the reference's: any non-empty string is True, so the flags are effectively constants."""
    parser.add_argument("--lora_r", type=int, default=16)
    parser.add_argument("--lora_alpha", type=int, default=16)
    parser.add_argument("--lora_dropout", type=float, default=0.05)
    parser.add_argument("--lora_query", type=bool, default=True)
    parser.add_argument("--lora_key", type=bool, default=True)
    parser.add_argument("--lora_value", type=bool, default=True)
    parser.add_argument("--lora_projection", type=bool, default=True)
    parser.add_argument("--lora_mlp", type=bool, default=False)
    parser.add_argument("--lora_head", type=bool, default=False)


def config_from_args(args):
    """Config.from_name(checkpoint_dir.name, r=..., ...) as inference/ger.py:177-190 / finetune/ger.py:101-112."""
    from pathlib import Path
    from .config import Config
    name = getattr(args, "config_name", None) or Path(args.llm_checkpoint).name
    cfg = Config.from_name(name, r=args.lora_r, alpha=args.lora_alpha, dropout=args.lora_dropout, to_query=args.lora_query,
                           to_key=args.lora_key, to_value=args.lora_value, to_projection=args.lora_projection,
                           to_mlp=args.lora_mlp, to_head=args.lora_head)
    if "llama-3" in cfg.name.lower():
        cfg.block_size = 4096                      # inference/ger.py:189-190
    return cfg


def init_distributed(n_devices: int):
    """One process per GPU (the reference's Fabric launch): -> (rank, world, device).  Under torchrun the env is read;
    `--d N` without a launcher re-runs this module under torch.distributed.run BEFORE anything touches the GPU."""
    import os
    import sys
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and n_devices > 1:
        import subprocess
        # --standalone lets the launcher pick (and hold) its own rendezvous port on 127.0.0.1: no bind/close race.  The
        # target is this run's entry point: `-m package.module` when started that way, else the script path
        # (__main__.__spec__ is None for `python dualhyp_amd/finetune.py` or when called from another entry point)
        spec = getattr(sys.modules.get("__main__"), "__spec__", None)
        target = ["-m", spec.name] if spec is not None and spec.name else [os.path.abspath(sys.argv[0])]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               f"--nproc-per-node={n_devices}", *target, *sys.argv[1:]]
        sys.exit(subprocess.run(cmd).returncode)
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    rehearsal = os.environ.get("DUALHYP_DP_REHEARSAL") == "1"    # every rank on cuda:0, gloo (one-GPU boxes, tests)
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)      # RCCL over xGMI
    return rank, world, dev


def result(adapter_path: str, model, tokenizer, args, rank: int = 0, world: int = 1) -> Dict[str, Any]:
    """inference/ger.py:30-124: load the fine-tuned state dict, decode the test JSON, WER, predictions file."""
    import json
    import os
    from pathlib import Path
    from .checkpoint import load_checkpoint
    from .data import HypothesesDataset, prompt_ids
    from .constrain import allowed_from_prompts, pack_mask
    from .generate import beam_search_batch, generate_batch, generate_stream, sample_batch
    if adapter_path:
        sd = load_checkpoint(adapter_path)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        if rank == 0:
            print("Missing:", missing)
            print("Unexpected:", unexpected)
    if getattr(args, "quantize", "none") == "fp8":     # after the checkpoint: a quantised model has no bf16 weights to load into
        from .quant import quantize_model_fp8
        quantize_model_fp8(model, kv_cache=getattr(args, "kv_cache", "bf16"))
    elif getattr(args, "quantize", "none") == "mxfp4":
        from .quant import quantize_model_mxfp4
        quantize_model_mxfp4(model, kv_cache=getattr(args, "kv_cache", "bf16"), activations=getattr(args, "activations", "fp8"))
    fmt = args.prompts_format
    if args.dual_hypotheses and "Dual" not in fmt and fmt != "RelPrompt":
        print("Warning: dual hypotheses is enabled, but prompts format is not Dual.")
    # RelPrompt with encoder features at hand: the prompt's mask tokens are PREDICTED by the reliability classifiers
    # (inference/relprompt.py:113-153); without features the ground-truth chunk labels of the corruption records are used
    feats_dir = getattr(args, "enc_features_dir", None) if fmt == "RelPrompt" else None
    enc_features = None
    _variants: dict = {}          # Uid -> its items (filled from the dataset below; read when a feature file is looked up)
    if feats_dir:
        def enc_features(s1, s2, _d=Path(feats_dir)):
            # <dir>/<Uid>.pt = {'audio', 'visual'} when the Uid has one variant; with several, the audio features of s1's corruption
            # and the visual features of s2's come from <Uid>.<hash of that corruption record>.pt (data.feature_key)
            from .data import feature_key
            n_var = len(_variants.get(s1["Uid"], (s1,)))
            fa = torch.load(_d / f"{feature_key(s1, 'Audio_Corruption', n_var)}.pt", map_location="cpu")
            fv = fa if n_var <= 1 else torch.load(_d / f"{feature_key(s2, 'Visual_Corruption', n_var)}.pt", map_location="cpu")
            return fa["audio"].float(), fv["visual"].float()
    ds = HypothesesDataset(args.test_path, tokenizer, prompts_format=fmt if (args.dual_hypotheses or fmt == "RelPrompt") else "GER",
                           nhyps_key=args.nhyps_key, max_nhyps=args.max_nhyps, language=args.language, seed=args.seed,
                           mask_threshold=getattr(args, "mask_threshold", None), time_window=getattr(args, "time_window", 0.4),
                           enc_features=enc_features, leave_masks=bool(feats_dir), apply_chat_template=args.apply_chat_template)
    _variants.update(ds.uid2sample)
    examples = [ds[i] for i in range(len(ds))]
    mask_stats = None
    if feats_dir:
        from .relprompt import predicted_mask_prompt
        hit = {"audio": [0, 0], "visual": [0, 0]}
        for ex in examples:
            prompt, a, v = predicted_mask_prompt(model, ex["input_no_response"], ex["audio_enc_features"], ex["visual_enc_features"])
            ex["input_no_response"] = prompt
            ex["input_ids_no_response"] = torch.tensor(prompt_ids(tokenizer, prompt, args.apply_chat_template),   # re-encoded with the
                                                       dtype=torch.int64)                                        # predicted masks
            for name, pred, tgt in (("audio", a, ex["audio_mask_targets"]), ("visual", v, ex["visual_mask_targets"])):
                n = min(pred.numel(), tgt.numel())                                                   # trimmed to the shorter, as the reference
                hit[name][0] += int((pred[:n] == tgt[:n]).sum())
                hit[name][1] += n
        mask_stats = {f"{k}_mask_accuracy": h[0] / max(h[1], 1) for k, h in hit.items()}
    eos = tokenizer.eos_token_id

    # --decode_batch is a throughput knob tuned on TinyLlama (2 x 22.5 KB of KV per position); the KV cache is allocated for
    # decode_batch x (longest prompt + max_new_tokens) positions (--schedule continuous: its decode rows, plus one spare slot), so
    # bound it by what the device has free (Llama-3-8B: 131 KB per position — 640 x 1700 positions would be 140 GB)
    if torch.cuda.is_available() and model.transformer.wte.weight.is_cuda:
        c_ = model.config
        kv_per_pos = c_.n_layer * 2 * c_.n_query_groups * c_.head_size * 2
        if getattr(model, "kv_cache_dtype", "bf16") == "fp8":      # a byte per element, an exponent per vector, one layer of bf16 scratch
            kv_per_pos = c_.n_layer * 2 * c_.n_query_groups * (c_.head_size + 1) + 2 * c_.n_query_groups * c_.head_size * 2
        longest = max((int(e["input_ids_no_response"].numel()) for e in examples), default=1) + args.max_new_tokens
        free, _total = torch.cuda.mem_get_info(model.transformer.wte.weight.device)
        fit = int(0.8 * free // max(kv_per_pos * longest, 1))
        if getattr(args, "schedule", "batch") == "continuous" and fit > 1:
            fit -= 1                                   # the spare slot of the padding rows
        if fit < 1:
            raise RuntimeError(f"not enough device memory for one sequence of {longest} positions ({kv_per_pos * longest / 2**30:.1f} GiB of KV cache)")
        if fit < args.decode_batch:
            print(f"[dualhyp_amd] --decode_batch {args.decode_batch} -> {fit}: {kv_per_pos * longest / 2**20:.0f} MiB of KV cache per sequence, "
                  f"{free / 2**30:.0f} GiB free")
            args.decode_batch = fit

    continuous = getattr(args, "schedule", "batch") == "continuous"
    share = "auto" if getattr(args, "share_prefix", "off") == "auto" else False
    spec = int(getattr(args, "speculate", 0) or 0)
    # --speculate_verify draw: the verify steps draw; the default run passes no keyword at all
    draw = bool(spec) and getattr(args, "speculate_verify", "argmax") == "draw"
    vkw = dict(verify="draw") if draw else {}
    top_n = int(getattr(args, "top_logprobs", 0) or 0)
    want_lp = bool(getattr(args, "logprobs", False)) or top_n > 0
    beams = int(getattr(args, "num_beams", 1) or 1)
    n_samples = int(getattr(args, "num_samples", 1) or 1)
    how = getattr(args, "select", None) or "avg_logprob"
    constrain = getattr(args, "constrain", "off") == "prompt"
    extra = read_token_ids(args.constrain_extra) if constrain and getattr(args, "constrain_extra", None) else ()
    # --constrain chain: every run of K generated tokens is a run of the utterance's own prompt; the default run passes no keyword at all
    chain = int(getattr(args, "constrain_order", 2) or 2) if getattr(args, "constrain", "off") == "chain" else 0
    ngram = int(getattr(args, "no_repeat_ngram", 0) or 0)
    # --beam_history device: the beams' histories on the device; the default run passes no keyword at all
    hkw = dict(history="device") if getattr(args, "beam_history", "host") == "device" else {}
    # --share_prompt_kv: likewise
    shared_kv = bool(getattr(args, "share_prompt_kv", False))
    shkw = dict(shared_prompt=True) if shared_kv else {}
    # --beam_kv table: likewise
    beam_kv = getattr(args, "beam_kv", "copy") or "copy"
    bkw = dict(kv="table") if beam_kv == "table" else {}
    stop = stop_from_args(args, tokenizer, model.config.padded_vocab_size, model.transformer.wte.weight.device)
    skw = dict(stop=stop, return_state=True) if stop is not None else {}       # the reasons are read from the state's done flags
    from .penalty import record as penalty_record
    penalties = penalty_record(getattr(args, "repetition_penalty", 1.0), getattr(args, "frequency_penalty", 0.0),
                               getattr(args, "presence_penalty", 0.0))
    # the default run passes no penalty keyword at all
    pkw = {} if penalties is None else dict(repetition_penalty=penalties["repetition"], frequency_penalty=penalties["frequency"],
                                            presence_penalty=penalties["presence"])
    bias_entries, bias_rec = bias_from_args(args, tokenizer, model.config.padded_vocab_size)
    if bias_entries is not None:      # the default run passes no bias keyword at all; compiled once for the run
        from .bias import compile_bias
        pkw["bias"] = compile_bias(bias_entries, model.config.padded_vocab_size, model.transformer.wte.weight.device)
    sampling = sampling_from_args(args)
    # the default run passes what it always passed: temperature 0.2, top_k 1 and the functions' own seed
    samp = dict(temperature=0.2, top_k=1) if sampling is None else dict(
        temperature=sampling["temperature"], top_k=sampling["top_k"] or None, top_p=sampling["top_p"], min_p=sampling["min_p"],
        seed=sampling["seed"])

    def gen(prompts):
        dev = model.transformer.wte.weight.device
        # --constrain prompt: an utterance may emit the ids of its own prompt (its hypotheses and the template), the EOS and the extras
        mask = pack_mask(allowed_from_prompts(prompts, eos, extra), model.config.padded_vocab_size, dev) if constrain else None
        akw = {}
        if chain:          # built from the call's prompts: an automaton per utterance
            from .automaton import from_prompts
            akw["automaton"] = from_prompts([p.reshape(-1).tolist() for p in prompts], order=chain, eos_id=eos)
        if beams > 1:      # --decode_batch counts decode rows: W per utterance
            hyps = beam_search_batch(model, [p.to(dev) for p in prompts], args.max_new_tokens, num_beams=beams, eos_id=eos,
                                     length_penalty=float(getattr(args, "length_penalty", 1.0)),
                                     prefill_batch=max(1, min(args.prefill_batch, args.decode_batch)), token_mask=mask,
                                     no_repeat_ngram=ngram, stop=stop, **hkw, **shkw, **bkw)
            return {"beams": hyps, "logprobs": want_lp}
        if n_samples > 1:  # --decode_batch counts decode rows: N per utterance
            cands = sample_batch(model, [p.to(dev) for p in prompts], args.max_new_tokens, num_samples=n_samples, eos_id=eos,
                                 prefill_batch=max(1, min(args.prefill_batch, args.decode_batch)), share_prefix=share, token_mask=mask,
                                 no_repeat_ngram=ngram, stop=stop, top_logprobs=top_n, **samp, **pkw, **akw, **shkw,
                                 **(dict(speculate=spec, **vkw) if draw else {}))
            return {"samples": cands, "select": how, "logprobs": want_lp}
        if continuous:     # the rank's whole shard in one call: finished rows hand their KV slots to the next utterances
            outs = generate_stream(model, [p.to(dev) for p in prompts], args.max_new_tokens, eos_id=eos,
                                   max_rows=args.decode_batch, prefill_batch=max(1, min(args.prefill_batch, args.decode_batch)),
                                   share_prefix=share, speculate=spec, return_logprobs=want_lp, top_logprobs=top_n, token_mask=mask,
                                   no_repeat_ngram=ngram, **samp, **skw, **pkw, **akw)
        else:
            outs = generate_batch(model, [p.to(dev) for p in prompts], args.max_new_tokens, eos_id=eos,
                                  prefill_batch=max(1, min(args.prefill_batch, args.decode_batch)), share_prefix=share, speculate=spec,
                                  return_logprobs=want_lp, top_logprobs=top_n, token_mask=mask, no_repeat_ngram=ngram,
                                  **samp, **skw, **pkw, **akw, **vkw)
        if stop is not None:
            from .stop import finish_reasons
            gen.finish_reasons = finish_reasons(outs[-1]["done"])
            outs = outs[:-1] if len(outs) > 2 else outs[0]
        if top_n:
            return [o.cpu() for o in outs[0]], [lp.cpu() for lp in outs[1]], [(a.cpu(), b.cpu()) for a, b in outs[2]]
        if want_lp:
            return [o.cpu() for o in outs[0]], [lp.cpu() for lp in outs[1]]
        return [o.cpu() for o in outs]

    gen.constrained = constrain or bool(chain)
    gen.constrain_order = chain
    gen.no_repeat_ngram = ngram
    gen.stop = stop is not None
    gen.sampling = sampling
    gen.speculate_verify = "draw" if draw else "argmax"
    gen.penalties = penalties
    gen.activations = getattr(model, "activation_format", "fp8")
    gen.bias, gen.bias_entries = bias_rec, bias_entries
    gen.shared_prompt = shared_kv
    gen.beam_kv = beam_kv
    out = run_inference(gen, examples, tokenizer.decode, batch_size=max(len(examples), 1) if continuous else max(1, args.decode_batch // beams // n_samples), rank=rank, world=world, eos_id=eos,
                        device="cpu" if os.environ.get("DUALHYP_DP_REHEARSAL") == "1" or world == 1 else model.transformer.wte.weight.device)
    out["adapter_path"] = adapter_path
    if mask_stats:
        out.update(mask_stats)
        if rank == 0:
            print("reliability masks predicted by the classifiers:", mask_stats)
    if rank == 0:
        n = out["n"]
        to_json = list(out["predictions"])
        to_json.append({"wer": out["WER"], "gtms": f"{round(out['gtms'] * n)}/{n}"})
        to_json.append({"post_wer": out["post_ST_wer"], "post_gtms": out["post_gtms"]})
        os.makedirs(args.predict_dir, exist_ok=True)
        stem = Path(adapter_path).name.replace(".pth", "") if adapter_path else "random_init"
        path = Path(args.predict_dir) / f"{stem}.json"
        path.write_text(json.dumps(to_json, indent=4, ensure_ascii=False))
        out["predictions_file"] = str(path)
        print(f"\nFor {adapter_path}\nWER is {out['WER']}\nGround truth matches is {round(out['gtms'] * n)}/{n}")
        print(f"the post string normalization wer is\nWER {out['post_ST_wer']}\nResults in {path}")
    return out


def build_parser():
    """The harness's flags: those of inference/ger.py:129-153 and this build's additions."""
    import argparse
    p = argparse.ArgumentParser(prog="python -m dualhyp_amd.inference")
    p.add_argument("--test_path", type=str, required=True)
    p.add_argument("--model_path", type=str, default="", help="fine-tuned checkpoint ({'model': state_dict}); empty with --random_init")
    p.add_argument("--llm_checkpoint", type=str, default="checkpoints/TinyLlama/TinyLlama-1.1B-Chat-v1.0")
    p.add_argument("--nhyps_key", type=str, default="nhyps_asr")
    p.add_argument("--dual_hypotheses", action="store_true")
    p.add_argument("--max_nhyps", type=int, default=None)
    p.add_argument("--d", type=int, default=1, help="number of GPUs")
    p.add_argument("--audio_corruption_disabled", action="store_true", help="accepted for compatibility: the LLM path never reads the media")
    p.add_argument("--visual_corruption_disabled", action="store_true", help="accepted for compatibility")
    p.add_argument("--seed", type=int, default=1337)
    p.add_argument("--prompts_format", type=str, default="GER")
    p.add_argument("--apply_chat_template", action="store_true", help="prompts through the tokenizer's chat template (phi-3.5)")
    p.add_argument("--language", type=str, default=None)
    add_lora_arguments(p)
    # additions of this build
    p.add_argument("--tokenizer", choices=("auto", "hf", "byte"), default="auto")
    p.add_argument("--config_name", type=str, default=None, help="Config.from_name key (default: the checkpoint directory's name)")
    p.add_argument("--random_init", action="store_true", help="synthetic weights from the counter hash instead of --model_path")
    p.add_argument("--decode_batch", type=int, default=640,
                   help="utterances decoded jointly (one weight stream per step for all of them; bench.py: 260 utt/s at 32, 770 at 640); "
                        "a sequence's tokens do not depend on it")
    p.add_argument("--schedule", choices=("batch", "continuous"), default="batch",
                   help="batch: --decode_batch utterances at a time, each batch stepped until its last sequence has finished; continuous: "
                        "--decode_batch decode rows over the whole shard, finished rows are retired and refilled (generate_stream); "
                        "the predictions do not depend on it")
    p.add_argument("--share_prefix", choices=("off", "auto"), default="off",
                   help="auto: the tokens every prompt of a call opens with (the template's instruction and header, the chat preamble; "
                        "whole 32-token tiles) are prefilled once and their KV cache is copied to the other utterances, which forward "
                        "the rest of their prompts only; the predictions do not depend on it")
    p.add_argument("--speculate", type=int, default=0, metavar="D",
                   help="D in 1..7: a decode step verifies D tokens drafted by prompt lookup (the correction mostly copies spans of its "
                        "prompt) next to each sequence's last one and keeps those the greedy arg-max confirms; --schedule batch only; "
                        "the predictions do not depend on it.  Default 0: off (acceptance on real corpora is unmeasured)")
    p.add_argument("--speculate_verify", choices=("argmax", "draw"), default="argmax",
                   help="with --speculate D: how a verify step confirms a draft.  argmax (the default): against the greedy arg-max, so "
                        "--top_k 1 only.  draw: against the seeded draw the plain step would have made at that place, so --speculate goes "
                        "with any --top_k, --top_p, --min_p, the penalties, --bias_file, --constrain chain and --num_samples (not with "
                        "--share_prompt_kv); the predictions are those of the run without --speculate; every record gains "
                        "speculate_verify: draw")
    p.add_argument("--quantize", choices=("none", "fp8", "mxfp4"), default="none",
                   help="fp8: after the checkpoint is loaded, LoRA is merged and every dense weight becomes e4m3 rows with channel scales "
                        "(quantize_model_fp8); activations are quantised per token and every product runs on the fp8 MFMA.  mxfp4: the "
                        "same path with the five dense matrices of every block stored as OCP MXFP4 (blocks of 32 four-bit elements with "
                        "one power-of-two scale byte, 4.25 bits per weight; quantize_model_mxfp4), lm_head stays e4m3; what does not go "
                        "with fp8 does not go with it (its effect on a real corpus's WER is unmeasured)")
    p.add_argument("--kv_cache", choices=("bf16", "fp8"), default="bf16",
                   help="fp8 (with --quantize fp8 or mxfp4): cached K and V vectors are stored as e4m3 bytes with one power-of-two exponent each, "
                        "half the cache bytes per token; the predictions are those of attention over the rounded cache")
    p.add_argument("--activations", choices=("fp8", "mxfp6"), default="fp8",
                   help="mxfp6 (with --quantize mxfp4 only): the activations of every block are quantised to OCP MXFP6 (blocks of 32 e2m3 "
                        "elements with one power-of-two scale byte, no per-token scale) instead of e4m3 rows, the operand pair the MFMA runs at "
                        "twice the fp8 rate; the final norm and lm_head stay e4m3; every record gains activations: \"mxfp6\".  Default fp8: "
                        "the path it always was")
    p.add_argument("--logprobs", action="store_true",
                   help="every record of the predictions file gains sum_logprob and avg_logprob: the model's log-probability of the tokens "
                        "it generated (the EOS included; temperature 1, no top-k crop), computed inside the decode steps; the predictions "
                        "do not depend on it.  Default off: the file is what it always was")
    p.add_argument("--top_logprobs", type=int, default=0, metavar="K",
                   help="K in 1..8 (implies --logprobs): every record also gains token_ids, token_logprobs and top_logprobs — per generated "
                        "token the K most probable tokens of the model's distribution as [id, log-probability] pairs, by value descending, "
                        "then by id ascending — computed inside the decode steps; the predictions do not depend on it.  Default 0: off")
    p.add_argument("--num_beams", type=int, default=1, metavar="W",
                   help="W in 2..4: beam search over W hypotheses per utterance (beam_search_batch), --decode_batch // W utterances at a "
                        "time; the prediction is the best hypothesis and every record gains beams, the ranked hypotheses with text, "
                        "sum_logprob, avg_logprob and finished.  Default 1: greedy decoding, the path it always was")
    p.add_argument("--beam_history", choices=("host", "device"), default="host",
                   help="with --num_beams W > 1: device keeps every live beam's generated tokens in two planes on the device, "
                        "re-parented by the selection kernel, which lets --no_repeat_ngram (the ban on a beam's own text; the records gain "
                        "no_repeat_ngram and ngram_bans of the best hypothesis) and the stop sequences of --stop_file run under beam "
                        "search; penalties and --bias_file stay refused there: they would change what a candidate's rank means.  Default "
                        "host: the steps, and the refusals, it always had")
    p.add_argument("--beam_kv", choices=("copy", "table"), default="copy",
                   help="with --num_beams W > 1 and --share_prompt_kv: table keeps, per beam and 32-key tile, the sibling KV slot that "
                        "holds the tile; a beam step's attention reads every closed tile where it was written and the re-parenting copies "
                        "one open tile instead of every tile with a generated key (the same keys, so the same predictions); every "
                        "record gains beam_kv: table.  Default copy: the launches it always made")
    p.add_argument("--num_samples", type=int, default=1, metavar="N",
                   help="N in 2..8 (with --top_k other than 1): N sampled candidates per utterance from one prefill of its prompt "
                        "(sample_batch: the prompt's KV cache is forked into N decode slots by one launch), --decode_batch // N "
                        "utterances at a time; the prediction is the candidate --select chooses and every record gains samples (text, "
                        "sum_logprob, avg_logprob, finish_reason and the selection key of every candidate) and selected, the chosen "
                        "index; --schedule batch only, not with --num_beams or --speculate.  Default 1: the path it always was (the "
                        "effect on a real corpus's WER is unmeasured)")
    p.add_argument("--share_prompt_kv", action="store_true",
                   help="with --num_samples N > 1 or --num_beams W > 1: the decode steps' attention reads an utterance's whole 32-key "
                        "prompt tiles once per block of its N (or W) rows instead of once per row (shared-prompt attention; the same "
                        "bits, so the same predictions); every record gains shared_prompt: true; not with --quantize fp8 or mxfp4.  "
                        "Default off: the launches it always made")
    p.add_argument("--select", choices=("avg_logprob", "sum_logprob", "mbr"), default=None,
                   help="with --num_samples N > 1: the candidate kept — the highest avg_logprob (the default) or sum_logprob, or mbr: "
                        "the candidate with the lowest word edit distance to the other N - 1, each standing in as a reference (minimum "
                        "Bayes risk; ties go to the higher avg_logprob)")
    p.add_argument("--constrain", choices=("off", "prompt", "chain"), default="off",
                   help="prompt: constrained decoding — an utterance may emit only token ids that occur in its own prompt (its n-best "
                        "hypotheses and the template), the EOS and the ids of --constrain_extra; the mask is applied inside the sampling "
                        "kernels, under both schedules and with --num_beams; every record gains constrained: true.  chain: every run of "
                        "--constrain_order K generated tokens is a run of the utterance's own prompt — a per-utterance automaton built from "
                        "the call's prompts and walked inside the sampling kernels, under both schedules and with --num_samples; every "
                        "record gains constrained: true and constrain_order: K; not with --constrain_extra, --speculate or --num_beams.  "
                        "Default off: the path it always was")
    p.add_argument("--constrain_order", type=int, default=2, metavar="K",
                   help="with --constrain chain: the window length K, 2 .. 4 (default 2)")
    p.add_argument("--constrain_extra", type=str, default=None, metavar="FILE",
                   help="with --constrain prompt: a file of token ids, one per line, allowed for every utterance")
    p.add_argument("--no_repeat_ngram", type=int, default=0, metavar="N",
                   help="N in 1..8: an utterance never emits a token that would complete an N-gram its generated text already holds "
                        "(the prompt's N-grams stay free), which ends the loops a greedy corrector can fall into; the ban set is built "
                        "inside the sampling kernels, under both schedules, with --constrain and --speculate; every record gains "
                        "no_repeat_ngram: N and ngram_bans, the generated positions with a non-empty ban set; not with --num_beams.  "
                        "Default 0: off, the path it always was (the WER effect on real corpora is unmeasured)")
    p.add_argument("--stop", choices=("off", "newline"), default="off",
                   help="newline: a sequence ends right behind the first token it generates whose text holds a newline — the harness "
                        "keeps the first line of the answer only, so what lies behind it is decoded and thrown away; the test runs inside "
                        "the sampling kernels, under both schedules and with every other flag; every record gains finish_reason (eos, "
                        "length or stop).  The predictions do not depend on it where the tokenizer decodes a token prefix to a prefix of "
                        "the text (true for the byte tokenizer, assumed for the others).  Default off: the path it always was (the "
                        "effect on real corpora is unmeasured)")
    p.add_argument("--stop_file", type=str, default=None, metavar="FILE",
                   help="a stop specification, one entry per line of token ids separated by blanks: a line of one id adds to the stop "
                        "set, a line of 2..8 ids is a stop sequence (at most 8 of them); blank lines and # comments are skipped; adds to "
                        "--stop; stop sequences do not go with --num_beams")
    p.add_argument("--temperature", type=float, default=0.2,
                   help="the sampler's temperature (inference/ger.py:71 decodes at 0.2); with the default --top_k 1 it changes no pick")
    p.add_argument("--top_k", type=int, default=1, metavar="K",
                   help="1: greedy arg-max, the path it always was; K > 1: sample among the K best tokens; 0: no crop by count")
    p.add_argument("--top_p", type=float, default=1.0, metavar="P",
                   help="P in (0, 1], with --top_k other than 1: nucleus sampling — the draw is made from the best tokens down to the one "
                        "whose mass crosses P of what --top_k keeps, ties kept together; the crop is taken inside the sampling kernels, "
                        "under both schedules and with every flag that goes with sampling.  Default 1.0: off")
    p.add_argument("--min_p", type=float, default=0.0, metavar="P",
                   help="P in [0, 1], with --top_k other than 1: only tokens whose probability is at least P times the best token's are "
                        "drawn from.  Default 0.0: off.  A run with any of --temperature, --top_k, --top_p, --min_p off its default "
                        "gives every record sampling: {temperature, top_k, top_p, min_p, seed}")
    p.add_argument("--repetition_penalty", type=float, default=1.0, metavar="T",
                   help="T in [1/8, 8]: the logit x of every token an utterance has already generated (its prompt stays free) becomes "
                        "x * T where negative and x / T otherwise before the pick; the values are computed inside the sampling kernels, "
                        "under both schedules and with --share_prefix, --constrain, --no_repeat_ngram, --stop, --logprobs, --top_logprobs, "
                        "--top_p, --min_p, --num_samples and fp8; not with --speculate or --num_beams.  Default 1.0: off")
    p.add_argument("--frequency_penalty", type=float, default=0.0, metavar="A",
                   help="A in [-8, 8]: A times the number of times the utterance has generated a token is taken off its logit; goes "
                        "with what --repetition_penalty goes with.  Default 0.0: off")
    p.add_argument("--presence_penalty", type=float, default=0.0, metavar="A",
                   help="A in [-8, 8]: A is taken off the logit of every token the utterance has generated; goes with what "
                        "--repetition_penalty goes with.  Default 0.0: off.  A run with any of the three penalties off its default gives "
                        "every record penalties: {repetition, frequency, presence}")
    p.add_argument("--bias_file", type=str, default=None, metavar="FILE",
                   help="contextual biasing: a list of phrases (names, product terms, jargon) whose continuations get a logit bonus inside "
                        "the sampling kernels.  One entry per line, ENTRY or BOOST<TAB>ENTRY; an entry made only of integers is a list "
                        "of token ids, anything else is text, encoded by the run's tokenizer with no BOS or EOS, and once more with one "
                        "leading space when that gives other ids (both forms count); at most 256 entries of 1 .. 8 tokens, shared by all "
                        "utterances.  Goes with both schedules and with --share_prefix, --constrain, --no_repeat_ngram, --stop, "
                        "--logprobs, --top_logprobs, --top_p, --min_p, the penalties, --num_samples and fp8; not with --speculate or "
                        "--num_beams.  Every record gains bias: {entries, default_boost} and bias_hits.  Default: off")
    p.add_argument("--bias_boost", type=float, default=4.0, metavar="B",
                   help="with --bias_file: the boost of a line that names none, finite, of either sign.  Default 4.0, an unmeasured "
                        "starting point: its effect on a real corpus' word error rate has not been measured")
    p.add_argument("--length_penalty", type=float, default=1.0,
                   help="with --num_beams: hypotheses are ranked by sum_logprob / n ** length_penalty, n their generated tokens")
    p.add_argument("--prefill_batch", type=int, default=64, help="utterances per packed prefill launch inside a decode batch")
    p.add_argument("--max_new_tokens", type=int, default=150, help="inference/ger.py:71")
    p.add_argument("--predict_dir", type=str, default=None)
    # RelPrompt (inference/relprompt.py): chunk geometry of the reliability masks; with --enc_features_dir (<dir>/<Uid>.pt =
    # {'audio': [T, whisper_dim], 'visual': [T, raven_dim]}: the encoders are upstream of this path) the masks are predicted
    p.add_argument("--mask_threshold", type=int, default=None)
    p.add_argument("--time_window", type=float, default=0.4)
    p.add_argument("--pool_size", type=int, default=10)
    p.add_argument("--enc_features_dir", type=str, default=None)
    return p


def parse_args(argv: Optional[Sequence[str]] = None):
    """The parsed flags, with the combinations that cannot run refused before anything is loaded."""
    p = build_parser()
    args = p.parse_args(argv)
    fp8_path = args.quantize in ("fp8", "mxfp4")             # mxfp4 is a weight format of the fp8 serving path: one engine, one set of refusals
    if args.kv_cache == "fp8" and not fp8_path:
        p.error("--kv_cache fp8 goes with --quantize fp8 (or mxfp4): the fp8 KV cache belongs to the fp8 serving path")
    if args.activations != "fp8" and args.quantize != "mxfp4":
        p.error(f"--activations {args.activations} goes with --quantize mxfp4: beside e4m3 or bf16 weights the narrow activations buy no MFMA rate")
    if args.speculate and fp8_path:                           # speculate.check_arguments refuses it too
        p.error(f"--speculate {args.speculate} does not go with --quantize {args.quantize}: an fp8 engine has no verify step")
    if args.speculate and args.schedule == "continuous":      # generate_stream refuses it too; here nothing has been loaded yet
        p.error(f"--speculate {args.speculate} goes with --schedule batch: continuous batching steps a row list one token at a time")
    draw = args.speculate_verify == "draw"                    # lifts the refusals of --speculate with the sampled path below
    if draw and not args.speculate:
        p.error("--speculate_verify draw goes with --speculate D: it says how a verify step confirms its drafts")
    if not 1 <= args.num_beams <= 4:
        p.error(f"--num_beams {args.num_beams}: W is 1 (greedy) or 2..4")
    if args.num_beams > 1:
        for on, flag, why in ((args.schedule == "continuous", "--schedule continuous", "continuous batching steps a row list one token at a time"),
                              (bool(args.speculate), f"--speculate {args.speculate}", "a verify step follows one greedy hypothesis"),
                              (fp8_path, f"--quantize {args.quantize}", "an fp8 engine's step changes its GEMM kernel with the row count"),
                              (args.share_prefix == "auto", "--share_prefix auto", "the beams' KV slots are forked from whole prompts"),
                              (bool(args.top_logprobs), f"--top_logprobs {args.top_logprobs}", "the records carry the beams instead")):
            if on:
                p.error(f"--num_beams {args.num_beams} does not go with {flag}: {why}")
    if not 1 <= args.num_samples <= 8:
        p.error(f"--num_samples {args.num_samples}: N is 1 (one answer) or 2..8")
    if args.select is not None and args.num_samples < 2:
        p.error(f"--select {args.select} goes with --num_samples N > 1: one answer leaves nothing to select among")
    if args.num_samples > 1:
        for on, flag, why in ((args.num_beams > 1, f"--num_beams {args.num_beams}", "beam search ranks hypotheses by score and draws nothing"),
                              (bool(args.speculate) and not draw, f"--speculate {args.speculate}", "a verify step confirms drafts against the greedy arg-max"),
                              (args.schedule == "continuous", "--schedule continuous", "an utterance's N decode slots are forked and stepped together"),
                              (args.top_k == 1, "--top_k 1", f"the arg-max gives {args.num_samples} equal candidates; sample with --top_k 0 or K > 1")):
            if on:
                p.error(f"--num_samples {args.num_samples} does not go with {flag}: {why}")
        if args.select is None:
            args.select = "avg_logprob"
    if args.share_prompt_kv:
        if args.speculate and args.num_samples > 1:         # sample_batch refuses it too
            p.error(f"--share_prompt_kv does not go with --speculate {args.speculate}: a verify step's rows are positions of one "
                    "sequence, not rows of an utterance")
        if args.num_samples < 2 and args.num_beams < 2:
            p.error("--share_prompt_kv goes with --num_samples N > 1 or --num_beams W > 1: one decode row per utterance shares its "
                    "prompt with nobody")
        if fp8_path:
            p.error(f"--share_prompt_kv does not go with --quantize {args.quantize}: an fp8 engine's step does not run the streaming "
                    "layers that launch the shared-prompt attention kernel")
    if args.beam_kv == "table":                             # beam_search_batch refuses both too; here nothing has been loaded yet
        if args.num_beams < 2:
            p.error("--beam_kv table goes with --num_beams W > 1: the table names, per tile, the sibling beam whose KV slot holds it")
        if not args.share_prompt_kv:
            p.error("--beam_kv table goes with --share_prompt_kv: the beams' private tiles are read through the table inside the "
                    "shared-prompt attention kernel")
    if not 0 <= args.no_repeat_ngram <= 8:
        p.error(f"--no_repeat_ngram {args.no_repeat_ngram}: N is 0 (off) or 1..8")
    dev_hist = args.beam_history == "device"                # the beams' histories on the device lift the next two refusals
    if dev_hist and args.num_beams < 2:
        p.error("--beam_history device goes with --num_beams W > 1: greedy decoding keeps its history in the token buffer")
    if args.no_repeat_ngram and args.num_beams > 1 and not dev_hist:    # beam_search_batch refuses it too; here nothing has been loaded yet
        p.error(f"--no_repeat_ngram {args.no_repeat_ngram} does not go with --num_beams {args.num_beams}: the beams' histories live on "
                "the host, so the sampling kernels cannot form a beam's ban set")
    if args.stop_file and args.num_beams > 1 and not dev_hist:          # beam_search_batch refuses it too; here nothing has been loaded yet
        from .stop import BEAM_REFUSAL, read_stop_file
        if read_stop_file(args.stop_file)[1]:
            p.error(f"--stop_file {args.stop_file} with --num_beams {args.num_beams}: {BEAM_REFUSAL}")
    if args.constrain_extra and args.constrain == "off":
        p.error("--constrain_extra goes with --constrain prompt")
    if args.constrain == "chain":
        if not 2 <= args.constrain_order <= 4:
            p.error(f"--constrain_order {args.constrain_order}: K is 2 .. 4")
        if args.constrain_extra:
            p.error("--constrain_extra goes with --constrain prompt: a chain automaton has no place for ids outside its prompt")
        if args.speculate and not draw:     # generate_batch refuses it too; here nothing has been loaded yet
            from .automaton import SPEC_REFUSAL as AUT_SPEC_REFUSAL
            p.error(f"--speculate {args.speculate} does not go with --constrain chain: {AUT_SPEC_REFUSAL}")
        if args.num_beams > 1:
            from .automaton import BEAM_REFUSAL as AUT_BEAM_REFUSAL
            p.error(f"--num_beams {args.num_beams} does not go with --constrain chain: {AUT_BEAM_REFUSAL}")
    elif args.constrain_order != 2:
        p.error("--constrain_order goes with --constrain chain")
    if not 0 <= args.top_logprobs <= 8:
        p.error(f"--top_logprobs {args.top_logprobs}: K is 0 (off) or 1..8")
    if args.top_logprobs:
        args.logprobs = True
    if not 0 <= args.speculate <= 7:
        p.error(f"--speculate {args.speculate}: D is 0 (off) or 1..7")
    from .nucleus import check_min_p, check_top_p
    for check, flag, value in ((check_top_p, "--top_p", args.top_p), (check_min_p, "--min_p", args.min_p)):
        try:
            check(value)
        except ValueError as e:
            p.error(f"{flag}: {e}")
    from .penalty import check_penalties, penalties_on
    try:
        pen = check_penalties(args.repetition_penalty, args.frequency_penalty, args.presence_penalty)
    except ValueError as e:
        p.error(f"--repetition_penalty / --frequency_penalty / --presence_penalty: {e}")
    if penalties_on(*pen):
        flags = f"--repetition_penalty {pen[0]} --frequency_penalty {pen[1]} --presence_penalty {pen[2]}"
        if args.speculate and not draw:     # generate_batch refuses it too; here nothing has been loaded yet
            p.error(f"--speculate {args.speculate} does not go with {flags}: a verify position's history would have to include the picks "
                    "of its own step")
        if args.num_beams > 1:
            p.error(f"--num_beams {args.num_beams} does not go with {flags}: " +
                    ("a penalised logit would change what a candidate's rank and a beam's score mean" if dev_hist else
                     "the beams' histories live on the host, so the sampling kernels cannot count them"))
    import math
    if not math.isfinite(args.bias_boost):
        p.error(f"--bias_boost {args.bias_boost}: the boost is finite")
    if args.bias_file:
        if args.speculate and not draw:     # generate_batch refuses it too; here nothing has been loaded yet
            from .bias import SPEC_REFUSAL
            p.error(f"--speculate {args.speculate} does not go with --bias_file {args.bias_file}: {SPEC_REFUSAL}")
        if args.num_beams > 1:
            from .bias import BEAM_REFUSAL
            p.error(f"--num_beams {args.num_beams} does not go with --bias_file {args.bias_file}: " +
                    ("a boosted logit would change what a candidate's rank and a beam's score mean" if dev_hist else BEAM_REFUSAL))
    if not args.temperature > 0.0:
        p.error(f"--temperature {args.temperature}: the temperature is positive")
    if args.top_k < 0:
        p.error(f"--top_k {args.top_k}: K is 0 (no crop), 1 (greedy) or more")
    if args.top_k != 1:
        if args.speculate and not draw:     # speculate.check_arguments refuses it too; here nothing has been loaded yet
            p.error(f"--speculate {args.speculate} does not go with --top_k {args.top_k}: a verify step confirms drafts against the greedy "
                    "arg-max, so it runs with --top_k 1 only")
        if args.num_beams > 1:
            p.error(f"--num_beams {args.num_beams} does not go with --top_k {args.top_k}: beam search ranks hypotheses by score and "
                    "draws nothing")
    return args


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """`python -m dualhyp_amd.inference --test_path x.json --model_path runs/exp/best_model.pth --llm_checkpoint
    checkpoints/TinyLlama/TinyLlama-1.1B-Chat-v1.0 --dual_hypotheses --prompts_format DualHyp` — the flags of
    inference/ger.py:129-153; `--d N` shards the utterances over N GPUs (one process each)."""
    import random
    from pathlib import Path
    args = parse_args(argv)
    rank, world, dev = init_distributed(args.d)
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    from .gpt import GPT
    from .relprompt import GPT as RelGPT
    from .tokenizer import load_tokenizer, apply_eos_override
    cfg = config_from_args(args)
    tokenizer = load_tokenizer(args.llm_checkpoint, args.tokenizer)
    apply_eos_override(tokenizer, cfg.name)        # inference/ger.py:196-198 (phi-): decoding stops at <|endoftext|>
    rel = args.prompts_format == "RelPrompt"
    if rel:
        cfg.pool_size = args.pool_size
    model = (RelGPT if rel else GPT)(cfg)
    if rel:                                        # inference/relprompt.py:341-342
        tokenizer.add_reliability_tokens(cfg.padded_vocab_size)
        model.resize_token_embeddings(3)
    if args.random_init:
        from .synth import synth_state_dict
        sd = synth_state_dict(cfg, seed=args.seed, embed_scale=50.0, head_tie=1.0)
        if rel:                                    # keep the freshly drawn reliability rows
            sd["transformer.wte.weight"] = torch.cat([sd["transformer.wte.weight"], model.transformer.wte.weight.data[-3:].to(torch.bfloat16)])
        model.load_state_dict(sd, strict=not rel)
    model = model.to(device=dev, dtype=torch.bfloat16)
    model.eval()
    if args.predict_dir is None:
        args.predict_dir = str(Path(args.model_path).parent / "predictions") if args.model_path else "predictions"
    out = result(args.model_path, model, tokenizer, args, rank, world)
    if rank == 0:
        print("Model: ", args.model_path, "WER: ", out["WER"] * 100, "WER_post: ", out["post_ST_wer"] * 100, "GTM: ", out["gtms"] * 100,
              "GTM_post: ", out["post_gtms"] * 100)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
