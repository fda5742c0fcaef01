"""The fine-tune's micro-step WITH LoRA dropout on: loss and every LoRA gradient of the three training paths (eager autograd,
GraphedTrainStep, packed GraphedTrainStep) against oracle.ger_oracle.train_micro_step on the CPU under THE SAME masks — the
kernel's draws restated by tests/dropout_reference.py (seed = torch's initial seed, call id 2l for layer l's QKV branch and 2l + 1
for its proj branch, step = the model's device counter read after the HIP call, row b * T + t of the [B * T, d] activation) and
handed to the oracle's F.dropout calls in order.

Gate (that of test_hip_train.test_train_micro_step_matches_reference, the yardstick from the oracle's own two precisions): per LoRA
tensor e = max|g - g_fp32| / max|g_fp32| and e_hip <= max(1.3 * e_oracle_bf16, 0.02); |loss - l32| <= max(1.3 * |lbf - l32|, 1e-2).

The settings (dropout_reference.SETTINGS, p = 0.5) are the ones at which a backward that used the wrong layer's or site's mask, the
previous step's, none, or n1 for n1d moves some LoRA gradient by 11 - 67 gates: test_dropout_reference.py measures and asserts
that on the oracle alone.  Site 0's input gradient feeds only the frozen embedding and is dead by construction."""
import pytest
import torch

import dropout_reference as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234


def _model(key, dropout=R.P_MODEL):
    from dualhyp_amd import GPT
    from dualhyp_amd.finetune import FlatGradBucket
    from dualhyp_amd.train import prepare_for_training
    torch.manual_seed(SEED)
    cfg, sd = R.setting(key)
    cfg.dropout = dropout
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    m.cpu_rsqrt_vec_width = 32          # the oracle runs on the CPU (Q11)
    m.train()
    bucket = FlatGradBucket(prepare_for_training(m))
    return cfg, sd, m, bucket


def _seed():
    return torch.initial_seed() & (2 ** 63 - 1)


def _counter(m) -> int:
    return int(m._dropout_rng[1].item())


def _grads(m):
    return {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if "lora_" in n}


def _oracle(cfg, sd, ids, labels, step, accum, T_pad=None, row0=0):
    """Oracle pair for one [B, T] batch whose rows are row0 + b * T_pad + t of the HIP call's activation."""
    B, T = ids.shape
    T_pad = T if T_pad is None else T_pad
    assert B == 1 or T_pad == T
    rows = row0 + B * T_pad
    full = R.site_masks(2 * cfg.n_layer, rows, cfg.n_embd, R.P_MODEL, _seed(), step)
    return R.oracle_pair(cfg, sd, ids, labels, [m[row0:row0 + B * T] for m in full], accum)


def _compare(tag, loss, grads, ref, must_pass=True):
    """Print and record every distance, then apply the gate.  -> whether everything passed."""
    l32, g32, lbf, gbf = ref
    gate, e_hip = R.gates(g32, gbf), R.distances(grads, g32)
    figures, ok = {}, True
    for k, (e_ref, g) in gate.items():
        short = k.replace("transformer.h.", "h").replace(".attn.", ".")
        figures.update({f"{short}.e_hip": e_hip[k], f"{short}.e_oracle_bf16": e_ref, f"{short}.gate": g})
        ok &= e_hip[k] <= g
    loss_gate = max(1.3 * abs(lbf - l32), 1e-2)
    ok_loss = abs(loss - l32) <= loss_gate
    if must_pass:
        record_parity(tag, loss=loss, loss_fp32=l32, loss_bf16=lbf, loss_gate=loss_gate, **figures)
        assert ok_loss, f"{tag}: loss {loss} vs fp32 {l32}, bf16 {lbf}"
        for k, (e_ref, g) in gate.items():
            assert e_hip[k] <= g, f"{tag}: {k}: hip {e_hip[k]:.4f} vs oracle-bf16 {e_ref:.4f} of max|g| (gate {g:.4f})"
    return ok


@pytest.mark.parametrize("key", list(R.SETTINGS))
def test_eager_micro_steps_match_the_oracle_under_their_own_masks(key):
    """Two consecutive autograd micro-steps on one model: each matches the oracle under the masks of the counter it left behind,
    the counter rises by one per training forward, and the second does NOT match under the first's masks."""
    from dualhyp_amd.finetune import micro_loss
    cfg, sd, m, bucket = _model(key)
    s = R.SETTINGS[key]
    ids, labels = R.batch(cfg, s["B"], s["T"], seed=2)
    refs = {}
    for k in (1, 2):
        bucket.zero()
        loss = micro_loss(m, ids.to(DEV), labels.to(DEV), 8)
        (loss / 4).backward()
        assert _counter(m) == k
        refs[k] = _oracle(cfg, sd, ids, labels, k, 4)
        _compare(f"dropout_grads.eager.{key}.step{k}", loss.item(), _grads(m), refs[k])
    assert not _compare("", loss.item(), _grads(m), refs[1], must_pass=False), "step 2's gradients pass under step 1's masks"


@pytest.mark.parametrize("key", list(R.SETTINGS))
def test_graphed_micro_step_matches_the_oracle(key):
    """GraphedTrainStep, one sequence of 37 tokens padded to 64: the masks are indexed over the padded rows, the oracle gets rows
    0 .. 36.  The first call warms up, captures and replays (counter 2), the second replays (counter 3): each replay draws the
    masks of the counter it leaves behind."""
    from dualhyp_amd.train import GraphedTrainStep
    cfg, sd, m, bucket = _model(key)
    step = GraphedTrainStep(m, bucket)
    ids, labels = R.batch(cfg, 1, 37, seed=3)
    for call, want_counter in ((0, 2), (1, 3)):
        bucket.zero()
        loss = step(ids.to(DEV), labels.to(DEV), 0.25).item()
        assert _counter(m) == want_counter
        ref = _oracle(cfg, sd, ids, labels, want_counter, 4, T_pad=64)
        _compare(f"dropout_grads.graphed.{key}.call{call}", loss, _grads(m), ref)
    assert step.captures == 1


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "copy_back"])
@pytest.mark.parametrize("key", list(R.SETTINGS))
def test_packed_micro_steps_match_the_sum_of_the_oracles(key, direct, monkeypatch):
    """Two sequences (37 and 50 tokens, T_pad 64) in one packed launch: sequence p's masks are rows p * 64 + t of the padded
    activation; the bucket holds loss_scale * (the sum of the two micro-batch-1 gradients), each loss is its own sequence's.
    Once with the rank-16 gradients accumulated straight into the bucket, once copied back (DUALHYP_NO_DIRECT_GRADS)."""
    from dualhyp_amd.train import GraphedTrainStep
    if not direct:
        monkeypatch.setenv("DUALHYP_NO_DIRECT_GRADS", "1")
    cfg, sd, m, bucket = _model(key)
    step = GraphedTrainStep(m, bucket)
    lens, T_pad = (37, 50), 64
    ids = torch.zeros((2, max(lens)), dtype=torch.int64)
    labels = torch.full_like(ids, -1)
    for i, n in enumerate(lens):
        bi, bl = R.batch(cfg, 1, n, seed=10 + i)
        ids[i, :n], labels[i, :n] = bi[0], bl[0]
    bucket.zero()
    losses = step(ids.to(DEV), labels.to(DEV), 0.5, lengths=lens).tolist()
    c = _counter(m)
    assert c == 2
    parts = [_oracle(cfg, sd, ids[i:i + 1, :n], labels[i:i + 1, :n], c, 2, T_pad=T_pad, row0=i * T_pad) for i, n in enumerate(lens)]
    g32 = {k: parts[0][1][k].float() + parts[1][1][k].float() for k in parts[0][1]}
    gbf = {k: parts[0][3][k].float() + parts[1][3][k].float() for k in parts[0][3]}
    tag = f"dropout_grads.packed.{key}.{'direct' if direct else 'copy_back'}"
    for i, (l32, _, lbf, _) in enumerate(parts):
        print(f"[{tag}] sequence {i}: loss {losses[i]} fp32 {l32} bf16 {lbf}")
        assert abs(losses[i] - l32) <= max(1.3 * abs(lbf - l32), 1e-2), (i, losses[i], l32, lbf)
    _compare(tag, losses[1], _grads(m), (parts[1][0], g32, parts[1][2], gbf))


@pytest.mark.parametrize("key", list(R.SETTINGS))
def test_eval_mode_draws_nothing(key):
    """model.eval() on a dropout = 0.5 config: the logits of the same weights under dropout = 0.0, bit for bit, through the engine
    (no_grad) and through the autograd forward; the step counter stays where the last training forward left it."""
    cfg, sd, m, _ = _model(key)
    _, _, m0, _ = _model(key, dropout=0.0)
    s = R.SETTINGS[key]
    ids = R.batch(cfg, s["B"], s["T"], seed=2)[0].to(DEV)
    m(ids)                                  # one training forward: the counter exists and reads 1
    assert _counter(m) == 1 and getattr(m0, "_dropout_rng", None) is None
    m.eval()
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m(ids), m0(ids))
    lg, lg0 = m(ids), m0(ids)
    assert lg.requires_grad and torch.equal(lg, lg0)
    assert _counter(m) == 1
    m.train()
    m(ids)
    assert _counter(m) == 2
