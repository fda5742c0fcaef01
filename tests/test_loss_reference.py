"""The gates of tests/test_hip_loss.py have teeth (CPU only): an fp32 evaluation of the cross entropy that walks the row as
the kernel does passes them at every width, mutants — each one a bug the kernels could plausibly have — fail them, and the
loop without the -inf guard produces the NaN that the guard removes."""
import math

import pytest
import torch

import loss_reference as R

DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(V, dtype):
        if (V, dtype) not in cache:
            c = R.make_case(V, dtype)
            c["emu"] = R.emulate_fwd(c["logits"], c["targets"])
            cache[(V, dtype)] = c
        return cache[(V, dtype)]
    return get


def test_cases_cover_what_they_claim():
    for V in R.WIDTHS:
        for dtype in DTYPES:
            c = R.make_case(V, dtype)
            x, tg, kinds = c["logits"].double(), c["targets"], c["kinds"]
            assert x.size(0) <= 16 and bool(torch.isfinite(x).all())
            edges = R.edge_columns(V)
            peaks = {int(x[i].argmax()) for i, k in enumerate(kinds) if k.startswith("peak")}
            assert peaks == set(edges)
            assert {int(tg[i]) for i, k in enumerate(kinds) if k.startswith("peak")} == set(edges)
            for i, k in enumerate(kinds):
                if k.startswith("peak"):
                    assert x[i].max().item() == 22.5 and int((x[i] == -1.5).sum()) == V - 1
                if k in ("ascend", "descend") and V > 256:
                    col = x[i, 5::256]                                    # thread 5's columns
                    assert bool((col[1:] > col[:-1]).all() if k == "ascend" else (col[1:] < col[:-1]).all())
                if k == "large":
                    assert x[i].max().item() >= 89 and not bool(torch.isfinite(torch.exp(x[i].float()).sum()))
            assert kinds.count("ignored") == 2 and int(tg[-1]) == V and int(tg[-2]) == -1
    assert R.edge_columns(32064) == [0, 63, 64, 255, 256, 31999, 32000, 32063]
    assert R.edge_columns(256) == [0, 63, 64, 255] and R.edge_columns(1) == [0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", R.WIDTHS)
def test_fp32_evaluation_passes(cases, V, dtype):
    c = cases(V, dtype)
    loss, lse = c["emu"]
    res = R.fwd_gate(loss, lse, c["logits"], c["targets"])
    assert res["ok"], res
    assert res["lse_worst"] <= 0.25, f"the fp32 loop should sit well inside the bound: {res}"
    d = R.emulate_bwd(c["logits"], c["targets"], lse, c["grow"])
    res = R.bwd_gate(d, c["logits"], c["targets"], c["grow"])
    assert res["ok"], res
    # and the fp64 truth itself, stored in the logits' dtype
    t = R.truth(c["logits"], c["targets"], c["grow"])
    assert R.fwd_gate(t["loss"].float(), t["lse"].float(), c["logits"], c["targets"])["ok"]
    assert R.bwd_gate(t["grad"].to(dtype), c["logits"], c["targets"], c["grow"])["ok"]


def test_truth_is_torch_cross_entropy():
    F = torch.nn.functional
    c = R.make_case(1000, torch.float32)
    x = c["logits"].double().requires_grad_()
    tg = c["targets"].clone()
    tg[tg >= 1000] = -1
    per = F.cross_entropy(x, tg, ignore_index=-1, reduction="none")
    g = c["grow"].double().nan_to_num(nan=0.0)
    per.backward(g)
    t = R.truth(c["logits"], c["targets"], c["grow"])
    assert (per.detach() - t["loss"]).abs().max().item() <= 1e-12
    assert (x.grad - t["grad"]).abs().max().item() <= 1e-14


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [3, 65, 257, 1000, 32064])
@pytest.mark.parametrize("mutant", R.FWD_MUTANTS)
def test_forward_mutant_is_caught(cases, mutant, V, dtype):
    c = cases(V, dtype)
    loss, lse = R.mutant_fwd(c["logits"], c["targets"], mutant)
    res = R.fwd_gate(loss, lse, c["logits"], c["targets"])
    assert not res["ok"], f"{mutant} passed at V = {V}: {res}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [3, 65, 257, 1000, 32064])
@pytest.mark.parametrize("mutant", R.BWD_MUTANTS)
def test_backward_mutant_is_caught(cases, mutant, V, dtype):
    c = cases(V, dtype)
    res = R.bwd_gate(R.mutant_bwd(c["logits"], c["targets"], c["emu"][1], c["grow"], mutant), c["logits"], c["targets"], c["grow"])
    assert not res["ok"], f"{mutant} passed at V = {V}: {res}"


def test_one_dropped_column_of_a_peak_row_is_orders_beyond_the_bound():
    """The point of the peak rows: the peak column dropped moves lse by ~24 - log(V), its double count by log 2."""
    c = R.make_case(32064, torch.float32)
    t = R.truth(c["logits"], c["targets"])
    x = c["logits"].double()
    i = c["kinds"].index("peak")
    col = int(x[i].argmax())
    dropped = torch.logsumexp(torch.cat([x[i, :col], x[i, col + 1:]]), 0)
    doubled = torch.logsumexp(torch.cat([x[i], x[i, col:col + 1]]), 0)
    assert abs(dropped - t["lse"][i]).item() >= 1e4 * t["tol_lse"][i].item()
    assert abs(doubled - t["lse"][i]).item() >= 1e4 * t["tol_lse"][i].item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [3, 65, 257, 1000, 32064])
def test_neg_inf_columns(V, dtype):
    """A -inf logit at a thread's first column made the unguarded loop return NaN; -inf met later did not.  The guarded loop
    meets the gates, with exactly 0 gradient at the -inf columns; on finite rows the guard changes no bit."""
    c = R.neg_inf_case(V, dtype)
    x, tg = c["logits"], c["targets"]
    assert bool(torch.isfinite(x.gather(1, tg[:, None])).all()) and bool(torch.isfinite(x).any(-1).all())
    loss, lse = R.emulate_fwd(x, tg, skip_neg_inf=True)
    res = R.fwd_gate(loss, lse, x, tg)
    assert res["ok"], res
    d = R.emulate_bwd(x, tg, lse, c["grow"])
    assert R.bwd_gate(d, x, tg, c["grow"])["ok"]
    assert bool((d[torch.isinf(x)] == 0).all())
    old_loss, old_lse = R.emulate_fwd(x, tg, skip_neg_inf=False)
    hits = 0
    for i, kind in enumerate(c["kinds"]):
        # NaN exactly when some thread starts on -inf and meets a finite column later (a thread that never does is dropped
        # by the wave combine with its m = -inf, NaN sum and all): never at V <= 256
        hit = any(bool(torch.isinf(x[i, j])) and bool(torch.isfinite(x[i, j::256]).any()) for j in range(min(V, 256)))
        assert bool(torch.isnan(old_lse[i])) == hit, (kind, i)
        hits += hit
    assert (hits > 0) == (V > 256), hits
    assert R.fwd_gate(old_loss, old_lse, x, tg)["ok"] == (hits == 0)
    f = R.make_case(V, dtype)
    a, b = R.emulate_fwd(f["logits"], f["targets"], True), R.emulate_fwd(f["logits"], f["targets"], False)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_ulp32():
    x = torch.tensor([1.0, 1.5, 2.0, 1e-3, 100.0], dtype=torch.float64)
    want = torch.tensor([float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(math.inf, dtype=torch.float32)) - v)
                         for v in x.float().tolist()], dtype=torch.float64)
    assert torch.equal(R.ulp32(x.float().double()), want)
