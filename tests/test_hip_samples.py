"""sample_batch on the GPU, pinned to its definition (include/dualhyp_hip.h, "Sampled candidates"): sample j of utterance u is row
u * N + j of generate_batch over the prompt list with every prompt repeated N times, under the same keyword arguments — the same
ids, log-probabilities, alternatives and done flags, bit for bit — from one prefill per utterance and one fork launch.  Every
check is exact.  Then the harness: --num_samples / --select through the CLI on the parity-harness fixture."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import Config, generate_batch, quantize_model_fp8, sample_batch
from dualhyp_amd.select import select
from dualhyp_amd.stop import finish_reasons
from dualhyp_amd.synth import synth_prompts

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_hip_prefix import DEV, ROOT, build, n_generated, sharing_prompts  # noqa: E402

pytestmark = pytest.mark.gpu
N = 3
NEW = 12
LENS = [17, 40, 64, 83, 100]            # ragged: below a tile, an exact multiple, and 100 + 12 positions fit parity-tiny's 128
# seed 99 was checked on the GPU to give an utterance whose three samples differ from each other on both models
# (test_samples_differ asserts it)
KW = dict(temperature=0.8, top_k=5, top_p=0.9, seed=99)


def bits(t):
    """NaN-filled float buffers compare by their bits"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def nfold(xs):
    return [x for x in xs for _ in range(N)]


def early_eos(free, prompts, vocab):
    """test_hip_prefix.early_eos at this file's budget: the token of the EOS-free run that ends the most rows in the first half of
    the budget while one runs to the end"""
    best, best_n = None, 0
    for eos in range(vocab):
        g = n_generated(free, prompts, eos, new=NEW)
        early = sum(a <= NEW // 2 for a in g)
        if max(g) == NEW and early > best_n:
            best, best_n = eos, early
    return best


def check_definition(m, prompts, what, mask=None, **kw):
    """sample_batch against the N-fold generate_batch call, row for row; returns (samples, timing)"""
    lens = [p.numel() for p in prompts]
    K = kw.get("top_logprobs", 0)
    # sample_batch first, on a new engine: its cache is zeroed, so a slot the fork did not fill cannot hold the right bytes by chance
    # (behind the N-fold call every slot would hold its prompt already)
    m.refresh_engine()
    tm = {}
    got, st_s = sample_batch(m, prompts, NEW, num_samples=N, return_state=True, timing=tm, **kw,
                             **({} if mask is None else dict(token_mask=mask)))
    st_s = {k: v.clone() for k, v in st_s.items()}
    ref = generate_batch(m, nfold(prompts), NEW, return_logprobs=True, return_state=True, **kw,
                         **({} if mask is None else dict(token_mask=nfold(mask))))
    want, want_lp, st = ref[0], ref[1], ref[-1]
    want_top = ref[2] if K else None
    assert len(got) == len(prompts) and all(len(g) == N for g in got)
    for key in st:     # the device state: ids, lengths, done flags, log-probabilities and alternatives, every row
        assert torch.equal(bits(st_s[key]), bits(st[key])), f"{what}: state[{key!r}] differs from the {N}-fold generate_batch call's"
    reasons = finish_reasons(st["done"])
    for u, n in enumerate(lens):
        for j in range(N):
            r, s = u * N + j, got[u][j]
            assert torch.equal(s["tokens"], want[r][n:].cpu()), f"{what}: ids of utterance {u} sample {j}"
            assert torch.equal(s["token_logprobs"], want_lp[r].cpu()) and not s["token_logprobs"].isnan().any(), f"{what}: log-probabilities of ({u}, {j})"
            assert s["finish_reason"] == reasons[r]
            assert s["sum_logprob"] == float(want_lp[r].double().sum()) and s["avg_logprob"] == s["sum_logprob"] / max(1, want_lp[r].numel())
            if K:
                assert all(torch.equal(a, b.cpu()) for a, b in zip(s["top_logprobs"], want_top[r])), f"{what}: alternatives of ({u}, {j})"
    return got, tm, st


@pytest.fixture(scope="module", params=["parity-tiny", "parity-hs128"])
def setup(request):
    cfg, m = build(request.param)
    V = cfg.padded_vocab_size
    prompts = [synth_prompts(1, n, V, seed=300 + i)[0].to(DEV) for i, n in enumerate(LENS)]
    free = [o.clone() for o in generate_batch(m, nfold(prompts), NEW, **KW)]
    eos = early_eos(free, nfold(prompts), V)
    assert eos is not None, "no token ends a row early"
    return cfg, m, prompts, free, eos


def test_sample_batch_is_the_n_fold_generate_batch(setup):
    cfg, m, prompts, free, eos = setup
    g = n_generated(free, nfold(prompts), eos, new=NEW)
    assert min(g) <= NEW // 2 and max(g) == NEW, "some rows must end early and one must run to its budget"
    got, tm, st = check_definition(m, prompts, "eos", eos_id=eos, **KW)
    assert tm["prefill_tokens"] == sum(LENS) and tm["shared_prefix"] == 0        # every prompt once, not N times
    assert 0.0 < tm["fork_ms"] < tm["prefill_ms"]
    assert 1 in st["done"].tolist() and set(st["done"].tolist()) & {0, 2}
    assert {s["finish_reason"] for ss in got for s in ss} == {"eos", "length"}
    # prefilled two utterances at a time, and without an EOS (one decode call): the same definition
    check_definition(m, prompts, "prefill_batch=2", eos_id=eos, prefill_batch=2, **KW)
    check_definition(m, prompts, "no eos", **KW)


def test_samples_differ(setup):
    cfg, m, prompts, free, eos = setup
    m.refresh_engine()
    got = sample_batch(m, prompts, NEW, num_samples=N, **KW)
    distinct = [len({tuple(s["tokens"].tolist()) for s in ss}) for ss in got]
    print("distinct samples per utterance:", distinct)
    assert max(distinct) == N, f"no utterance has {N} different samples under seed {KW['seed']}: {distinct}"
    # and it is the free run's rows
    assert all(torch.equal(s["tokens"], free[u * N + j][LENS[u]:].cpu()) for u, ss in enumerate(got) for j, s in enumerate(ss))


def test_share_prefix(setup):
    cfg, m, _, _, eos = setup
    prompts = sharing_prompts(cfg, [1, 9, 25, 12, 30], shared=40)          # 41 .. 70 tokens behind a shared tile: P = 32
    _, tm, _ = check_definition(m, prompts, "share_prefix", eos_id=eos, share_prefix=True, **KW)
    assert tm["shared_prefix"] == 32 and tm["prefill_tokens"] == sum(p.numel() for p in prompts) - 4 * 32


def test_token_mask(setup):
    cfg, m, prompts, _, eos = setup
    V = cfg.padded_vocab_size
    mask = [sorted(set(range(u % 3, V, 3)) | {eos}) for u in range(len(prompts))]      # a third of the vocabulary, another per utterance
    got, _, _ = check_definition(m, prompts, "token_mask", mask=mask, eos_id=eos, **KW)
    assert all(set(s["tokens"].tolist()) <= set(mask[u]) for u, ss in enumerate(got) for s in ss)


def test_no_repeat_ngram(setup):
    cfg, m, prompts, _, eos = setup
    check_definition(m, prompts, "no_repeat_ngram", eos_id=eos, no_repeat_ngram=2, **KW)


def test_stop(setup):
    cfg, m, prompts, free, eos = setup
    # a stop id and a stop sequence that the free run produces: the fourth token of row 1, tokens 6 and 7 of row 7
    a = int(free[1][LENS[0] + 3])
    b = free[7][LENS[2] + 5:LENS[2] + 7].tolist()
    got, _, st = check_definition(m, prompts, "stop", stop=[a, b], **KW)
    assert 3 in st["done"].tolist() and "stop" in {s["finish_reason"] for ss in got for s in ss}


def test_top_logprobs(setup):
    cfg, m, prompts, _, eos = setup
    got, _, _ = check_definition(m, prompts, "top_logprobs", eos_id=eos, top_logprobs=2, **KW)
    assert all(s["top_logprobs"][0].shape == (s["token_logprobs"].numel(), 2) for ss in got for s in ss)


def test_fp8_model_with_fp8_cache():
    cfg, m = build("parity-hs128")
    quantize_model_fp8(m, kv_cache="fp8")
    V = cfg.padded_vocab_size
    prompts = [synth_prompts(1, n, V, seed=300 + i)[0].to(DEV) for i, n in enumerate(LENS)]
    free = [o.clone() for o in generate_batch(m, nfold(prompts), NEW, **KW)]
    eos = early_eos(free, nfold(prompts), V)
    assert eos is not None
    check_definition(m, prompts, "fp8", eos_id=eos, **KW)
    assert m._engine.kv_cache_dtype == "fp8"


def test_fork_is_one_launch_without_a_host_synchronisation():
    """The fork under stream capture: a capture fails on any host synchronisation or staging upload, and the captured graph, replayed
    after the destinations were overwritten, restores them — the lengths are read on the device when the kernel runs."""
    cfg, m = build("parity-tiny")
    V = cfg.padded_vocab_size
    m.refresh_engine()
    eng = m.engine(2 * N, 128, 2 * N * 64, exact=True)
    lens = [40, 64]
    fill = [synth_prompts(1, 64, V, seed=20 + i)[0].to(DEV) for i in range(2 * N)]
    src = [synth_prompts(1, n, V, seed=60 + i)[0].to(DEV) for i, n in enumerate(lens)]
    plen = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def refill():
        eng.forward(torch.cat(fill), [64] * (2 * N), [0] * (2 * N), want_all=False, want_last=True)
        eng.forward_slots(torch.cat(src), lens, [0, N], prompt_phase=True)

    def cache():
        return torch.stack([eng.read(w, l, (2 * N, cfg.n_query_groups, 128 * cfg.head_size)) for l in range(cfg.n_layer) for w in (1, 2)])

    refill()
    eng.fork_slots(plen, N, 64)
    want = cache()
    refill()
    assert not torch.equal(cache(), want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.fork_slots(plen, N, 64)
    torch.cuda.synchronize()
    assert not torch.equal(cache(), want), "a captured launch must not have run"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cache(), want)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def test_harness_num_samples_and_select(tmp_path):
    """the fixture corpus of tests/test_harness.py through the CLI: --num_samples 3 --top_k 5 --temperature 0.8 alone and under each
    --select value — records carry samples and selected, the prediction is the selected sample's text, the selection is select()'s on
    the record's own candidates — and a run without --num_samples writes the file it always wrote (the decoder answers "up down")."""
    import test_harness as H
    items = H.merged_items(caps=H.CAPTIONS)
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    ckpt_dir = tmp_path / "checkpoints" / "parity-harness"
    ckpt_dir.mkdir(parents=True)
    cfg = Config.from_name("parity-harness", r=16, alpha=16, dropout=0.05, to_query=True, to_key=True, to_value=True, to_projection=True)
    sampled = ["--num_samples", "3", "--top_k", "5", "--temperature", "0.8"]
    files = {}
    for tag, extra in (("plain", []), ("default", sampled), ("avg_logprob", sampled + ["--select", "avg_logprob"]),
                       ("sum_logprob", sampled + ["--select", "sum_logprob"]), ("mbr", sampled + ["--select", "mbr"])):
        run_dir = tmp_path / "runs" / tag
        run_dir.mkdir(parents=True)
        torch.save({"model": H.speaking_state_dict(cfg, seed=31)}, run_dir / "best_model.pth")
        cmd = [sys.executable, "-m", "dualhyp_amd.inference", "--test_path", str(test_json), "--model_path", str(run_dir / "best_model.pth"),
               "--llm_checkpoint", str(ckpt_dir), "--prompts_format", "GER", "--tokenizer", "byte", "--max_new_tokens", str(H.NEW),
               "--decode_batch", "12"] + extra
        out = subprocess.run(cmd, cwd=tmp_path, env=H._env(), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        files[tag] = json.loads((run_dir / "predictions" / "best_model.json").read_text())
    plain = files["plain"]
    assert len(plain) == 7 + 2 and [p["inference"] for p in plain[:7]] == [H.SAYS] * 7
    assert plain[-2]["wer"] == pytest.approx(H.WANT_WER) and plain[-2]["gtms"] == f"{H.WANT_EXACT}/7"
    assert all(set(p) == {"inference", "ground_truth"} for p in plain[:7]), "the default run's records are the ones they always were"
    assert files["default"] == files["avg_logprob"]
    for how in ("avg_logprob", "sum_logprob", "mbr"):
        js = files[how]
        assert len(js) == 7 + 2
        for rec in js[:7]:
            assert len(rec["samples"]) == 3 and rec["inference"] == rec["samples"][rec["selected"]]["text"]
            assert all(set(s) == {"text", "sum_logprob", "avg_logprob", "finish_reason", "key"} for s in rec["samples"])
            assert rec["sampling"]["top_k"] == 5 and rec["sampling"]["temperature"] == 0.8
            best, keys = select(rec["samples"], [s["text"] for s in rec["samples"]], how)
            assert rec["selected"] == best and [s["key"] for s in rec["samples"]] == keys
        # the candidates do not depend on the selection rule
        assert [[(s["text"], s["sum_logprob"]) for s in r["samples"]] for r in js[:7]] == \
               [[(s["text"], s["sum_logprob"]) for s in r["samples"]] for r in files["avg_logprob"][:7]]
