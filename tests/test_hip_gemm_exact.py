"""Every route of the bf16 GEMM family against exact integer products, inside guard bands (tests/gemm_exact_reference.py).

One case = reset the route record, run the op on guarded integer operands under the case's tuning, then assert (1) the exact set
of kernels that ran, (2) the exact result — for SwiGLU the acceptance of swiglu_accept — and (3) intact guards: both margins of
every output still hold the sentinel and no sentinel is left inside.  Input margins hold NaN, so a row read out of range shows
as a NaN in the result.  The table (R.CASES) is checked on the CPU by tests/test_gemm_exact_reference.py.

Non-SwiGLU results are compared bit for bit (the fp64 references follow the same IEEE rules for the sign of a zero).  SwiGLU: the
acceptance of R.swiglu_accept, whose fp32 underflow range (g <= -88: a zero is accepted and counted as `flushed`) is stated
there; the counts go to the parity record."""
import pytest
import torch

import gemm_exact_reference as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI = {"plain": 0, "lora": 1, "swiglu": 2, "adapter": 3}


class _Data:
    """operands (guarded, on the GPU), references (on the GPU) and guarded outputs of the cases that share a data key"""

    def __init__(self, c: R.Case):
        cpu = R.operands(c)
        ref = R.reference(c, cpu)
        fp32 = c.op in ("partial", "pairs", "chain")
        self.inp = {k: R.Guarded(v.shape, torch.bfloat16, DEV, R.guard_rows(v.shape), v).t for k, v in cpu.items()}
        self.ref = {k: v.float().to(DEV) for k, v in ref.items()}
        odt = torch.float32 if fp32 else torch.bfloat16
        names = {"swiglu_train": ("act", "g", "u"), "linear_lora": ("y", "xa_work")}.get(c.op, ("parts",) if fp32 else ("y",))
        shapes = {"parts": ref["parts"].shape if fp32 else None, "xa_work": (c.M, 16 * R.n_seg(c))}
        self.out = {n: R.Guarded(shapes.get(n) or (c.M, c.N), odt, DEV, R.guard_rows(shapes.get(n) or (c.M, c.N))) for n in names}


def _call(c: R.Case, d: _Data):
    from dualhyp_amd import ops
    i, o = d.inp, {k: g.t for k, g in d.out.items()}
    if c.op == "linear":
        ops.linear(i["x"], i["w"], epilogue=EPI[c.epi], w2=i.get("w2"), xa=i.get("xa"), lora_b=i.get("lora_b"), lora_scale=c.lora_scale,
                   splits=c.splits, scale=i.get("scale"), bias=i.get("bias"), resid=i.get("resid"), out=o["y"])
    elif c.op == "linear_lora":
        ops.linear_lora(i["x"], i["w"], i["lora_a"], i["lora_b"], lora_scale=c.lora_scale, splits=c.splits, resid=i.get("resid"),
                        out=o["y"], xa_work=o["xa_work"])
    elif c.op == "linear_mul":
        ops.linear_mul(i["x"], i["w"], i["mul"], out=o["y"])
    elif c.op == "swiglu_train":
        ops.linear_swiglu_train(i["x"], i["w"], i["w2"], out=(o["act"], o["g"], o["u"]))
    else:
        fn = {"partial": ops.linear_partial, "pairs": ops.linear_partial_pairs, "chain": ops.linear_chain}[c.op]
        fn(i["x"], i["w"], i.get("w_ext"), c.ksplit, out=o["parts"][0] if c.op == "chain" else o["parts"])


def _same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """bit for bit: `want` (fp32 on the GPU, exactly representable in got's dtype) against got's bit pattern"""
    idt = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    ne = got.contiguous().view(idt) != want.to(got.dtype).view(idt)
    n = int(ne.sum())
    if n:
        at = tuple(ne.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {ne.numel()} elements differ from the exact result, first at {at}: got {got[at].item()}, "
                             f"exact {want[at].item()}; NaNs: {int(torch.isnan(got.float()).sum())}")


def _run(family: str, group: str) -> None:
    from dualhyp_amd import _lib
    lib = _lib.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cached, data, failures = None, None, []
    tally = {"neighbour": 0, "flushed": 0, "outputs": 0}
    for c in R.cases_of(family, group):
        if c.data_key != cached:
            data, cached = None, c.data_key               # (the previous case's buffers go first)
            data = _Data(c)
        try:
            _run_case(c, data, lib, n_cu, tally)
        except AssertionError as e:                       # every failing case of the group is named, not only the first
            failures.append(str(e))
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"{c.id}: {e} -- nothing more is started on a GPU that has faulted", 3)
            raise
    if tally["outputs"]:
        record_parity(f"gemm_exact.swiglu_neighbours.{family}.{group}", **tally)
    assert not failures, f"{len(failures)} failing cases:\n" + "\n".join(failures[:10])


def _run_case(c: R.Case, data: _Data, lib, n_cu: int, tally: dict) -> None:
    for g in data.out.values():
        g.refill()
    try:
        for k, v in c.tune:
            assert lib.dh_set_tuning(k, v) == 0, (k, v)
        lib.dh_debug_gemm_routes(1)
        _call(c, data)
        took = R.route_names(lib.dh_debug_gemm_routes(1))
    finally:
        for k, _ in c.tune:
            lib.dh_set_tuning(k, R.TUNING_DEFAULTS[k])
    torch.cuda.synchronize()
    want = R.expected_routes(c, n_cu)
    assert took == want, f"{c.id}: ran {sorted(took)}, expected {sorted(want)} ({n_cu} CUs)"
    o, ref, bad = {k: g.t for k, g in data.out.items()}, data.ref, []

    def attempt(fn, *args, **kw):                         # a wrong value does not hide a touched guard of the same case
        try:
            fn(*args, **kw)
        except AssertionError as e:
            bad.append(str(e))

    if c.epi == "swiglu":
        act = o["act"] if c.op == "swiglu_train" else o["y"]
        ok, n, flushed = R.swiglu_accept(act, ref["g"], ref["u"])
        if not bool(ok.all()):
            bad.append(f"{c.id}: " + R.swiglu_failures(act, ref["g"], ref["u"], ok))
        tally["neighbour"] += n
        tally["flushed"] += flushed
        tally["outputs"] += ok.numel()
        if c.op == "swiglu_train":
            attempt(_same, o["g"], ref["g"], f"{c.id}: g")
            attempt(_same, o["u"], ref["u"], f"{c.id}: u")
    elif c.op in ("partial", "pairs", "chain"):
        attempt(_same, o["parts"], ref["parts"], c.id)
    else:
        attempt(_same, o["y"], ref["y"], c.id)
    in_gemm = "w4_xa" in took                             # the down-projection rode in the GEMM: the work buffer is not touched
    if c.op == "linear_lora" and not in_gemm:
        attempt(_same, o["xa_work"], ref["xa_work"], f"{c.id}: xa_work")
    for name, g in data.out.items():
        attempt(g.check, f"{c.id}: {name}", written=not (name == "xa_work" and in_gemm))
    assert not bad, "\n".join(bad)


def _family(name):
    return pytest.mark.parametrize("group", R.groups(name))


@_family("t128")
def test_128_tile_kernel(group):
    """gemm_nt_kernel, 2 and 4 stages: K one to five stages deep, ragged M and N, every epilogue"""
    _run("t128", group)


@_family("w256")
def test_256_tile_kernels(group):
    """the 8-wave kernel's four loop forms and the 4-wave kernel per tile / persistent, at 135 tiles (last row band one row deep,
    last column tile 8 wide) and 289 tiles (more than CUs: the persistent walk), and the row split of a small last round"""
    _run("w256", group)


@_family("xa")
def test_lora_down_projection_inside_the_gemm(group):
    _run("xa", group)


@_family("mul")
def test_linear_mul(group):
    _run("mul", group)


@_family("swiglu_train")
def test_linear_swiglu_train(group):
    _run("swiglu_train", group)


@_family("k64_skinny_n")
def test_k64_and_skinny_n_kernels(group):
    _run("k64_skinny_n", group)


@_family("mid")
def test_gemm_mid(group):
    """1 / 2 / 4 row groups with and without the W ring; SwiGLU at K = 128, 384, 640 (a K-part of an odd number of k-steps) stays
    here up to 257 rows"""
    _run("mid", group)


@_family("dt")
def test_gemm_dt(group):
    _run("dt", group)


@_family("skinny")
def test_gemm_skinny(group):
    _run("skinny", group)


@_family("rows")
def test_partial_rows_kernel(group):
    """each K-slice is the exact product over its own k-steps"""
    _run("rows", group)


@_family("partial_waves")
def test_partial_k_split_over_waves(group):
    _run("partial_waves", group)


@_family("pairs")
def test_partial_pairs(group):
    _run("pairs", group)


@_family("chain")
def test_partial_chain(group):
    _run("chain", group)
