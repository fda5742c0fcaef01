"""GPU tests of the cross-entropy kernels (csrc/loss.hip: ce_fwd_kernel, ce_bwd_kernel) against fp64, through the gates of
tests/loss_reference.py (derived there; tests/test_loss_reference.py shows what they reject).  At most 16 rows per case.

Contract stated by these tests: a row whose target lies outside [0, V) — the fine-tune's ignore index -1, but also V or
any other out-of-range id — is ignored: loss exactly 0, gradient exactly 0 whatever grad_row holds (NaN here).  A -inf logit
has probability 0: finite lse and loss (the target is finite), gradient exactly 0 at that column, as F.cross_entropy.  A
row with no finite logit is unspecified."""
import json

import pytest
import torch

import loss_reference as R
from conftest import GOLDEN, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


def _run(c):
    from dualhyp_amd import ops
    x, tg = c["logits"].to(DEV), c["targets"].to(DEV)
    loss, lse = ops.cross_entropy_fwd(x, tg)
    d = ops.cross_entropy_bwd(x, tg, lse, c["grow"].to(DEV))        # the lse the forward produced, as the training step
    assert loss.dtype == lse.dtype == torch.float32 and d.dtype == x.dtype and d.shape == x.shape
    return loss.cpu(), lse.cpu(), d.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", R.WIDTHS)
def test_ce_edge_rows(V, dtype):
    """Peaks and targets on every wave / stride edge column, ascending and descending strides, +-100 logits, ignored rows."""
    c = R.make_case(V, dtype)
    loss, lse, d = _run(c)
    f = R.fwd_gate(loss, lse, c["logits"], c["targets"])
    b = R.bwd_gate(d, c["logits"], c["targets"], c["grow"])
    print(f"V={V} {dtype}: fwd {f}\n  bwd {b}")
    record_parity(f"ce_edges.V{V}.{IDS[DTYPES.index(dtype)]}", lse_err=f["lse_err"], lse_bound=f["lse_tol"], lse_err_over_bound=f["lse_worst"],
                  loss_err_over_bound=f["loss_worst"], grad_bad=b["n_bad"],
                  **({"grad_err_over_tol": b["err_over_tol"]} if dtype == torch.float32 else {}))   # bf16: the band is gated after rounding
    assert f["ok"], f
    assert b["ok"], b
    ign = [i for i, k in enumerate(c["kinds"]) if k == "ignored"]
    assert bool((loss[ign] == 0).all()) and bool((d[ign] == 0).all()), "ignored rows (target -1 and target V) must be exactly 0"
    # the target column: -g (1 - p_t), so ~ -g where p_t ~ 0 and ~ 0 from the side of -g where p_t ~ 1
    g = c["grow"].double()
    for i, k in enumerate(c["kinds"]):
        if not k.startswith("peak"):
            continue
        dt = d[i, c["targets"][i]].double().item()
        if k == "peak":
            assert abs(dt + g[i].item()) <= 2.0 ** -7 * abs(g[i].item()), (i, dt, g[i].item())
        if k == "peak=t":
            assert dt * g[i].item() <= 0 and abs(dt) <= 1e-4 * abs(g[i].item()), (i, dt, g[i].item())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [3, 65, 257, 1000, 32064])
def test_ce_neg_inf_logits(V, dtype):
    """-inf at non-target columns: on a thread's first column, on a whole 256-column stride, everywhere but the target.  The
    forward used to return NaN when a thread met -inf before its first finite logit (V > 256)."""
    c = R.neg_inf_case(V, dtype)
    loss, lse, d = _run(c)
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all()), (c["kinds"], lse, loss)
    f = R.fwd_gate(loss, lse, c["logits"], c["targets"])
    b = R.bwd_gate(d, c["logits"], c["targets"], c["grow"])
    assert f["ok"], f
    assert b["ok"], b
    assert bool((d[torch.isinf(c["logits"])] == 0).all()), "the gradient at a -inf column must be exactly 0"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ce_finite_rows_keep_their_bits(dtype):
    """The -inf guard changes no finite row: lse and loss of the V = 32000 inputs of test_hip_train.test_cross_entropy_kernels
    are the bits the kernel produced before the guard (tests/golden/ce_v32000_bits.json, recorded from that build)."""
    from dualhyp_amd import ops
    from dualhyp_amd.synth import uniform, stream_id
    rows, V = 45, 32000
    lg = uniform((rows, V), 6.0, stream_id(21, "celg")).float().to(dtype)
    tg = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(3))
    tg[::4] = -1
    loss, lse = ops.cross_entropy_fwd(lg.to(DEV), tg.to(DEV))
    want = json.loads((GOLDEN / "ce_v32000_bits.json").read_text())[IDS[DTYPES.index(dtype)]]
    assert lse.cpu().view(torch.int32).tolist() == want["lse"]
    assert loss.cpu().view(torch.int32).tolist() == want["loss"]


@pytest.mark.parametrize("chunk_size", [0, 128])
def test_chunked_cross_entropy_ragged_width(chunk_size):
    """The public wrapper, forward and backward, at a ragged V with ignored rows: chunk_size 0 averages over the valid rows,
    any other over all rows (ignored ones count as 0)."""
    from dualhyp_amd.utils import chunked_cross_entropy
    B, T, V = 2, 7, 1000
    g = torch.Generator().manual_seed(11)
    x = ((torch.rand((B, T, V), generator=g, dtype=torch.float64) * 2 - 1) * 6).bfloat16()
    tg = torch.randint(0, V, (B, T), generator=g)
    tg[0, :3] = -1
    tg[1, -1] = -1
    xd = x.to(DEV).requires_grad_()
    out = chunked_cross_entropy(xd, tg.to(DEV), chunk_size=chunk_size)
    out.backward()
    x2, t2 = x.view(-1, V), tg.view(-1)
    t = R.truth(x2, t2)
    n = int(t["valid"].sum()) if chunk_size == 0 else B * T
    ref = t["loss"].sum() / n
    tol = t["tol_loss"][t["valid"]].sum() / n + (B * T + 1) * R.ulp32(ref)       # the rows' own tolerances + the fp32 sum and division
    assert abs(out.double().item() - ref.item()) <= tol.item(), (out.item(), ref.item(), tol.item())
    grow = torch.full((B * T,), 1.0 / n, dtype=torch.float32)
    res = R.bwd_gate(xd.grad.view(-1, V).cpu(), x2, t2, grow)
    assert res["ok"], res
    assert bool((xd.grad.view(-1, V).cpu()[~t["valid"]] == 0).all())
