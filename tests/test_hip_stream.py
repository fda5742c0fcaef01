"""Continuous batching on the GPU (dualhyp_amd.generate.generate_stream): finished decode rows retire, their KV slots are
refilled, the step is launched over the live rows.  The acceptance test is exact: the ids of generate_batch, bit for bit,
whatever the schedule — only the number of row-steps launched changes, and that number is checked as a count."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from dualhyp_amd import GPT, Config, generate_batch, generate_stream, quantize_model_fp8
from dualhyp_amd.schedule import predict
from dualhyp_amd.synth import synth_state_dict, synth_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
NEW = 24
LORA = dict(r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)


def build(name, fp8=False, seed=11):
    cfg = Config.from_name(name, **LORA)
    sd = synth_state_dict(cfg, seed=seed, norm_jitter=0.25, weight_scale=4.0, device=DEV)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(sd)
    m.eval()
    if fp8:
        quantize_model_fp8(m)
    return cfg, m


def ragged_prompts(cfg, n=48, seed=5):
    """n prompts of 1 .. ~100 tokens: the extremes and both sides of the 32- / 64-key tile edges are always present"""
    fixed = [1, 1, 2, 31, 32, 33, 63, 64, 65, 97, 100]
    ps = [synth_prompts(1, T, cfg.padded_vocab_size, seed=seed + i)[0] for i, T in enumerate(fixed)]
    ps += synth_prompts(n - len(fixed), 0, cfg.padded_vocab_size, seed=seed, ragged=True, lo=1, hi=100)
    return [p.to(DEV) for p in ps]


def n_generated(free, prompts, eos, new=NEW):
    """tokens each sequence produces with this EOS (the EOS counts, the budget caps), from the EOS-free run"""
    out = []
    for o, p in zip(free, prompts):
        hit = (o[p.numel():] == eos).nonzero().flatten()
        out.append(int(hit[0]) + 1 if hit.numel() else new)
    return out


def spread_eos(free, prompts, vocab, new=NEW):
    """An EOS id under which the sequences' lengths spread: the token of the EOS-free run that ends the most sequences in the
    first half of the budget while at least one sequence never produces it."""
    best, best_n = None, -1
    for eos in range(vocab):
        g = n_generated(free, prompts, eos, new)
        if not any(a == new and int(o[-1]) != eos for a, o in zip(g, free)):
            continue
        early = sum(a <= new // 2 for a in g)
        if early > best_n:
            best, best_n = eos, early
    return best


def spread_corpus(cfg, m, n=48, pool=320):
    """n prompts and an EOS id, both chosen from an EOS-free run of `pool` candidates (random weights produce any one token
    early in about 4 % of the sequences): the prompts of the extreme lengths, the candidates that the EOS ends in the first half
    of the budget (up to half of the corpus), and the following candidates in order."""
    cand = ragged_prompts(cfg, pool)
    free = [o.clone() for o in generate_batch(m, cand, NEW, temperature=0.2, top_k=1, prefill_batch=64)]
    eos = spread_eos(free, cand, cfg.padded_vocab_size)
    assert eos is not None, "no token of the EOS-free run spares a sequence"
    g = n_generated(free, cand, eos)
    keep = set(range(11))
    keep |= set([i for i in range(11, pool) if g[i] <= NEW // 2][:n // 2])
    keep |= set([i for i in range(11, pool) if i not in keep][:n - len(keep)])
    keep = sorted(keep)
    return [cand[i] for i in keep], [free[i] for i in keep], eos


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module", params=["parity-tiny", "parity-hs128", "parity-hs96"])
def corpus(request):
    cfg, m = build(request.param)
    ps, free, eos = spread_corpus(cfg, m)
    return cfg, m, ps, [o.clone() for o in free], eos


def test_same_ids_as_generate_batch(corpus):
    cfg, m, ps, free, eos = corpus
    g = n_generated(free, ps, eos)
    ended = [a < NEW or int(o[-1]) == eos for a, o in zip(g, free)]
    print(f"{cfg.name}: eos {eos}, tokens generated per sequence {sorted(g)}")
    # the inputs themselves: lengths must spread, or the schedule is not exercised
    assert len(ps) >= 48 and min(p.numel() for p in ps) == 1 and max(p.numel() for p in ps) >= 97
    assert sum(a <= NEW // 2 for a in g) * 4 >= len(ps), "fewer than a quarter of the sequences end in the first half of the budget"
    assert not all(ended), "no sequence runs to its budget"
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos)]
    assert [o.numel() - p.numel() for o, p in zip(want, ps)] == [a - 1 if e else a for a, e in zip(g, ended)]
    for max_rows in (4, 16, 64):
        for pb in (1, 8):
            got = generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=max_rows, prefill_batch=pb)
            bad = [i for i, (a, b) in enumerate(zip(want, got)) if not torch.equal(a, b)]
            assert not bad, f"max_rows {max_rows}, prefill_batch {pb}: sequences {bad} differ from generate_batch"


def test_eos_on_a_first_pick(corpus):
    """a sequence that ends on the pick of its prefill returns its prompt and never takes a decode row"""
    cfg, m, ps, free, eos = corpus
    first = int(free[7][ps[7].numel()])
    g = n_generated(free, ps, first)
    assert g[7] == 1
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=first)]
    tm = {}
    got = generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=first, max_rows=4, prefill_batch=8, timing=tm)
    assert same(want, got) and torch.equal(got[7], ps[7])
    assert tm["decode_row_steps"] == predict(g, NEW, 4, 8).decode_row_steps


def test_sampling_does_not_depend_on_the_schedule(corpus):
    cfg, m, ps, free, eos = corpus
    kw = dict(temperature=0.8, top_k=5, seed=4242, eos_id=eos)
    want = [o.clone() for o in generate_batch(m, ps, NEW, **kw)]
    assert not same(want, [o.clone() for o in generate_batch(m, ps, NEW, **dict(kw, seed=4243))]), "the draw ignores the seed"
    small = [o.clone() for o in generate_stream(m, ps, NEW, max_rows=4, prefill_batch=8, **kw)]
    large = [o.clone() for o in generate_stream(m, ps, NEW, max_rows=64, prefill_batch=8, **kw)]
    assert same(small, large), "sampled ids depend on max_rows"
    assert same(want, small), "sampled ids differ from generate_batch's"


def test_fewer_row_steps_exactly_counted(corpus):
    cfg, m, ps, free, eos = corpus
    g = n_generated(free, ps, eos)
    tb, ts = {}, {}
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, timing=tb)]
    got = generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=len(ps), prefill_batch=8, timing=ts)
    assert same(want, got)
    assert tb["decode_row_steps"] == len(ps) * tb["decode_steps"]
    print(f"{cfg.name}: row-steps batch {tb['decode_row_steps']}, stream {ts['decode_row_steps']}, rows {sorted(ts['launch_rows'])}")
    assert ts["decode_row_steps"] < tb["decode_row_steps"]
    sim = predict(g, NEW, len(ps), 8)
    assert ts["decode_row_steps"] == sim.decode_row_steps and ts["decode_steps"] == sim.decode_steps
    assert ts["launch_rows"] == sim.launch_rows and len(ts["launch_rows"]) <= 8
    assert ts["prefill_ms"] > 0 and ts["decode_ms"] > 0


def test_forward_slots_equals_forward_at():
    """a permuted slot list: the logits of forward_at, and each slot's K / V^T those of the contiguous run"""
    cfg, m = build("parity-hs128")
    lens = [1, 33, 64, 97, 5]
    ps = [synth_prompts(1, n, cfg.padded_vocab_size, seed=60 + i)[0].to(DEV) for i, n in enumerate(lens)]
    packed, S, B = torch.cat(ps), 128, 8
    G, hs, L = cfg.n_query_groups, cfg.head_size, cfg.n_layer

    def run(slots):
        m.refresh_engine()          # a fresh (zeroed) KV cache: the caches are compared whole
        eng = m.engine(B, S, int(packed.numel()), exact=True)
        if slots is None:
            _, last = eng.forward(packed, lens, [0] * len(ps), want_all=False, want_last=True, slot_base=2)
        else:
            last = eng.forward_slots(packed, lens, slots)
        return last.clone(), [eng.read(w, l, (B, G, S, hs)).clone() for l in range(L) for w in (1, 2)], eng

    at, kv_at, _ = run(None)
    same_slots, kv_same, _ = run([2, 3, 4, 5, 6])
    assert torch.equal(at, same_slots) and all(torch.equal(a, b) for a, b in zip(kv_at, kv_same))
    perm = [6, 0, 3, 7, 1]
    got, kv, eng = run(perm)
    assert torch.equal(at, got), "logits of the permuted slot list differ"
    for a, b in zip(kv_at, kv):
        for i, s in enumerate(perm):
            assert torch.equal(a[2 + i], b[s]), f"cache of sequence {i} (slot {s}) differs"
        for s in set(range(B)) - set(perm):
            assert not b[s].any(), f"slot {s} was written"
    # the identity array the plain decode relies on is untouched: a generate_batch on this engine equals a fresh one's
    after = [o.clone() for o in generate_batch(m, ps, 6, temperature=0.2, top_k=1)]
    m.refresh_engine()
    assert same(after, generate_batch(m, ps, 6, temperature=0.2, top_k=1))
    from dualhyp_amd._lib import DualHypHipError
    eng = m.engine(B, S, int(packed.numel()), exact=True)
    # a one-token prompt forwarded alone as a PROMPT: the bits it has in the pack (row 0 above), logits and cache
    alone = eng.forward_slots(ps[0], [1], [5], prompt_phase=True)
    assert torch.equal(alone[0], at[0])
    for l in range(L):
        for w in (1, 2):
            assert torch.equal(eng.read(w, l, (B, G, S, hs))[5], kv_at[2 * l + w - 1][2])
    with pytest.raises(DualHypHipError):
        eng.forward_slots(packed, lens, [0, 1, 1, 2, 3])        # a slot named twice
    with pytest.raises(DualHypHipError):
        eng.forward_slots(packed, lens, [0, 1, 2, 3, eng.max_batch])


@pytest.fixture(scope="module")
def tiny():
    return build("parity-tiny")


def test_budget_ends_on_the_last_cache_position(tiny):
    cfg, m = tiny
    ps = [synth_prompts(1, n, cfg.padded_vocab_size, seed=70 + n)[0].to(DEV) for n in (120, 3, 64, 120, 1)]
    new = 9                                   # 120 + 9 - 1 = 128 = block_size: the last forward runs on the last cache position
    want = [o.clone() for o in generate_batch(m, ps, new, temperature=0.2, top_k=1)]
    assert same(want, generate_stream(m, ps, new, temperature=0.2, top_k=1, max_rows=2, prefill_batch=1, check_every=3))
    with pytest.raises(NotImplementedError):
        generate_stream(m, ps, new + 1, temperature=0.2, top_k=1, max_rows=2)


def test_one_token_prompts_one_new_token_one_prompt(tiny):
    cfg, m = tiny
    ones = [torch.tensor([t], dtype=torch.int64, device=DEV) for t in (1, 5, 77, 200, 31, 9)]
    assert same([o.clone() for o in generate_batch(m, ones, 12, temperature=0.2, top_k=1)],
                generate_stream(m, ones, 12, temperature=0.2, top_k=1, max_rows=4, prefill_batch=8))
    ps = ragged_prompts(cfg, 20)
    tm = {}
    want = [o.clone() for o in generate_batch(m, ps, 1, temperature=0.2, top_k=1)]
    assert same(want, generate_stream(m, ps, 1, temperature=0.2, top_k=1, max_rows=4, prefill_batch=8, timing=tm))
    assert tm["decode_steps"] == 0 and tm["decode_row_steps"] == 0 and all(o.numel() == p.numel() + 1 for o, p in zip(want, ps))
    for new in (1, 7):
        assert same([o.clone() for o in generate_batch(m, ps[9:10], new, temperature=0.2, top_k=1)],
                    generate_stream(m, ps[9:10], new, temperature=0.2, top_k=1))


def test_eos_on_every_first_pick(tiny):
    cfg, m = tiny
    p = synth_prompts(1, 33, cfg.padded_vocab_size, seed=23)[0].to(DEV)
    first = int(generate_batch(m, [p], 1, temperature=0.2, top_k=1)[0][-1])
    tm = {}
    got = generate_stream(m, [p] * 6, 10, temperature=0.2, top_k=1, eos_id=first, max_rows=2, prefill_batch=2, timing=tm)
    assert all(torch.equal(o, p) for o in got) and tm["decode_steps"] == 0


def test_calls_back_to_back(tiny):
    """two generate_stream calls on one model (the engine and its captured steps are reused), then a generate_batch call
    that still equals a fresh run"""
    cfg, m = tiny
    ps = ragged_prompts(cfg, 24, seed=90)
    m.refresh_engine()
    fresh = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1)]
    eos = int(fresh[0][ps[0].numel() + 3])
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos)]
    m.refresh_engine()
    a = [o.clone() for o in generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=8, prefill_batch=8)]
    b = [o.clone() for o in generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=8, prefill_batch=8)]
    c = [o.clone() for o in generate_stream(m, list(reversed(ps)), NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=8, prefill_batch=3)]
    assert same(want, a) and same(want, b) and same(want, list(reversed(c)))
    assert same(fresh, generate_batch(m, ps, NEW, temperature=0.2, top_k=1))


def test_fp8_engine_same_row_class():
    """an fp8 engine below the 128-row boundary of its decode kernels: 48 prompts through 16 rows equal generate_batch's 48 rows"""
    cfg, m = build("parity-hs128", fp8=True)
    ps = ragged_prompts(cfg)
    free = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1)]
    eos = spread_eos(free, ps, cfg.padded_vocab_size)
    assert eos is not None
    g = n_generated(free, ps, eos)
    assert min(g) <= NEW // 2 and max(g) == NEW
    want = [o.clone() for o in generate_batch(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos)]
    tm = {}
    assert same(want, generate_stream(m, ps, NEW, temperature=0.2, top_k=1, eos_id=eos, max_rows=16, prefill_batch=8, timing=tm))
    assert max(tm["launch_rows"]) <= 128


@pytest.mark.parametrize("fmt", ["DualHyp", "GER"])
def test_harness_schedule_flag_changes_nothing(tmp_path, fmt):
    """the fixture corpus of tests/test_harness.py (a decoder that answers "up down": corpus WER 9/17) through the CLI with
    --schedule continuous and with --schedule batch: the same predictions file, the known WER"""
    sys.path.insert(0, str(ROOT / "tests"))
    import test_harness as H
    items = H.merged_items(caps=H.CAPTIONS)
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    ckpt_dir = tmp_path / "checkpoints" / "parity-harness"
    ckpt_dir.mkdir(parents=True)
    cfg = Config.from_name("parity-harness", r=16, alpha=16, dropout=0.05, to_query=True, to_key=True, to_value=True, to_projection=True)
    files = {}
    for schedule in ("continuous", "batch"):
        run_dir = tmp_path / "runs" / schedule
        run_dir.mkdir(parents=True)
        torch.save({"model": H.speaking_state_dict(cfg, seed=31)}, run_dir / "best_model.pth")
        cmd = [sys.executable, "-m", "dualhyp_amd.inference", "--test_path", str(test_json), "--model_path", str(run_dir / "best_model.pth"),
               "--llm_checkpoint", str(ckpt_dir), "--prompts_format", fmt, "--tokenizer", "byte", "--max_new_tokens", str(H.NEW),
               "--decode_batch", "4", "--schedule", schedule] + (["--dual_hypotheses"] if fmt == "DualHyp" else [])
        out = subprocess.run(cmd, cwd=tmp_path, env=H._env(), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        files[schedule] = json.loads((run_dir / "predictions" / "best_model.json").read_text())
    assert files["continuous"] == files["batch"]
    js = files["continuous"]
    assert len(js) == 7 + 2 and [p["inference"] for p in js[:7]] == [H.SAYS] * 7
    assert js[-2]["wer"] == pytest.approx(H.WANT_WER) and js[-2]["gtms"] == f"{H.WANT_EXACT}/7"
