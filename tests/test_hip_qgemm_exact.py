"""Every route of the fp8 and MXFP4 GEMMs (csrc/fp8.hip, csrc/mxfp4.hip) against exact references, inside guard bands
(tests/qgemm_exact_reference.py; the table is checked on the CPU by tests/test_qgemm_exact_reference.py).

One case = reset the route record, run the op on guarded operands under the case's tuning, then assert (1) the exact set of
kernels that ran, (2) the exact bits of the result — for SwiGLU the acceptance of Q.swiglu_accept — and (3) intact guards: both
margins of the output still hold the sentinel and no sentinel is left inside.  The e4m3 operands sit between e4m3 NaN bytes,
the fp32 scales, the adapter vectors and the residual between NaNs, the MXFP4 scale bytes between E8M0 NaNs (255): a row, a
column or a block read out of range poisons the result.

The operands make every fp32 partial sum exact, so the K order is free and nothing else is: zero tolerance for the plain,
residual and adapter epilogues with real, index-dependent scales.  The last test runs real-valued data, where the order
matters, and asserts that a row's bits do not depend on the rows packed with it."""
import pytest
import torch

import gemm_exact_reference as R
import qgemm_exact_reference as Q
from conftest import record_parity
from test_hip_gemm_exact import _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI = {"plain": 0, "swiglu": 2, "adapter": 3}


def _guard(v: torch.Tensor, margin: int, sentinel=None) -> R.Guarded:
    g = R.Guarded(v.shape, v.dtype, DEV, margin)
    if sentinel is not None:
        g.sentinel = sentinel
        g.refill()
    g.t.copy_(v)
    return g


class _Data:
    """operands (guarded, on the GPU), references (on the GPU) and guarded outputs of the cases that share a data key"""

    def __init__(self, c: Q.Case):
        o = Q.operands(c)
        enc = Q.encode(c, o)
        self.ref = {k: v.to(DEV) for k, v in Q.reference(c, o).items()}
        i = {"xq": _guard(enc["xq"], 256 * c.K), "xs": _guard(o["xs"], 256)}
        for s in ("", "2"):
            if f"w{s}q" not in enc:
                continue
            if c.fmt == "fp8":
                i[f"w{s}q"] = _guard(enc[f"w{s}q"], 256 * c.K)
                i[f"w{s}sc"] = _guard(o["ws" + s], 256)
            else:                                            # two 16-row groups of margin on either side
                i[f"w{s}q"] = _guard(enc[f"w{s}q"], 2 * (c.K // 128) * 1024)
                i[f"w{s}sc"] = _guard(enc[f"w{s}sc"], 2 * (c.K // 128) * 64, Q.E8M0_SENTINEL)
        for k in ("a", "b"):
            if k in o:
                i[k] = _guard(o[k], 256)
        if "resid" in o:
            i["resid"] = _guard(o["resid"], R.guard_rows(o["resid"].shape))
        self.guards = i
        self.inp = {k: g.t for k, g in i.items()}
        self.out = {}

    def output(self, c: Q.Case) -> R.Guarded:
        dt = torch.float32 if c.op == "linear_f32" else torch.bfloat16
        if dt not in self.out:
            self.out[dt] = R.Guarded((c.M, c.N), dt, DEV, R.guard_rows((c.M, c.N)))
        return self.out[dt]


def _call(c: Q.Case, i: dict, out: torch.Tensor) -> None:
    from dualhyp_amd import ops
    fn = ops.linear_fp8 if c.fmt == "fp8" else ops.linear_mxfp4
    if c.op == "linear_f32":
        fn(i["xq"], i["xs"], i["wq"], i["wsc"], out32=True, out=out)
    else:
        fn(i["xq"], i["xs"], i["wq"], i["wsc"], epilogue=EPI[c.epi], w2q=i.get("w2q"), w2_scale=i.get("w2sc"), scale=i.get("a"),
           bias=i.get("b"), resid=i.get("resid"), kernel=c.kernel, out=out)


def _run(family: str, group: str) -> None:
    from dualhyp_amd import _lib
    lib = _lib.load()
    cached, data, failures = None, None, []
    tally = {"neighbour": 0, "flushed": 0, "outputs": 0}
    for c in Q.cases_of(family, group):
        if c.data_key != cached:
            data, cached = None, c.data_key               # (the previous case's buffers go first)
            data = _Data(c)
        try:
            _run_case(c, data, lib, tally)
        except AssertionError as e:                       # every failing case of the group is named, not only the first
            failures.append(str(e))
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"{c.id}: {e} -- nothing more is started on a GPU that has faulted", 3)
            raise
    if tally["outputs"]:
        record_parity(f"qgemm_exact.swiglu_neighbours.{family}.{group}", **tally)
    assert not failures, f"{len(failures)} failing cases:\n" + "\n".join(failures[:10])


def _run_case(c: Q.Case, data: _Data, lib, tally: dict) -> None:
    out = data.output(c)
    out.refill()
    try:
        for k, v in c.tune:
            assert lib.dh_set_tuning(k, v) == 0, (k, v)
        lib.dh_debug_gemm_routes(1)
        _call(c, data.inp, out.t)
        took = R.route_names(lib.dh_debug_gemm_routes(1))
    finally:
        for k, _ in c.tune:
            lib.dh_set_tuning(k, Q.TUNING_DEFAULTS[k])
    torch.cuda.synchronize()
    assert took == set(c.routes), f"{c.id}: ran {sorted(took)}, expected {sorted(c.routes)}"
    ref, bad = data.ref, []
    if c.epi == "swiglu":
        ok, n, flushed = Q.swiglu_accept(out.t, ref["g"], ref["u"], ref["cand"])
        if not bool(ok.all()):
            bad.append(f"{c.id}: " + R.swiglu_failures(out.t, ref["g"].float(), ref["u"].float(), ok))
        tally["neighbour"] += n
        tally["flushed"] += flushed
        tally["outputs"] += ok.numel()
    else:
        try:
            _same(out.t, ref["y"].float(), c.id)
        except AssertionError as e:                       # a wrong value does not hide a touched guard of the same case
            bad.append(str(e))
    try:
        out.check(c.id)
    except AssertionError as e:
        bad.append(str(e))
    assert not bad, "\n".join(bad)


def _family(name):
    return pytest.mark.parametrize("group", Q.groups(name))


@_family("small")
def test_up_to_128_rows_streaming_and_tiled(group):
    """1 .. 128 rows (the row-group boundaries, the last group one row deep) x every N class, K walking 1 .. 41 k-steps: the
    streaming kernels with 1 / 2 / 4 row groups (selector 0 and 2), their fp32-out forms, and the tiled kernel on the same
    operands (selector 1)"""
    _run("small", group)


@_family("tiled")
def test_tiled_kernels_4_stages(group):
    """ragged row and column tiles, five row tiles under a band of four, K one stage to 41"""
    _run("tiled", group)


@_family("two_stage")
def test_tiled_kernels_2_stages(group):
    """384 tiles of 128: the two-stage form, odd and even trip counts"""
    _run("two_stage", group)


@_family("dispatch")
def test_dispatch_thresholds(group):
    """128 | 129 rows, 383 | 384 tiles of 128, 496 | 512 tiles of 256: default selector, no tuning"""
    _run("dispatch", group)


@_family("tune")
def test_fp8_tile_and_band_tuning(group):
    """dh_set_tuning 19 (tile edge) and 20 (m-tiles per band of the tile walk) on ragged shapes: a wrong walk leaves a tile
    unwritten (a sentinel inside) or writes one twice at the wrong place"""
    _run("tune", group)


@_family("codes")
def test_every_code_of_each_format(group):
    """each non-NaN e4m3 byte (in x, then in w) and each e2m1 code under 17 block scales against a one-hot operand"""
    _run("codes", group)


# ---- row invariance on real-valued data ---------------------------------------------------------------------------------------
def _bytes(key, shape):
    """random e4m3 bytes with the top exponent bit clear: 2^-9 <= |value| <= 1.875 or zero, no NaN"""
    return torch.randint(0, 256, shape, generator=Q._gen(*key), dtype=torch.int32).to(torch.uint8) & 0xBF


INVARIANCE = [
    # fmt, M, N, K, epi, resid, kernel, tune, route, rows run alone
    ("fp8", 32, 132, 1152, "plain", False, 2, (), "fp8_stream_ng1", (0, 31)),
    ("fp8", 64, 132, 1152, "adapter", True, 2, (), "fp8_stream_ng2", (0, 33, 63)),
    ("fp8", 97, 132, 5248, "plain", True, 2, (), "fp8_stream_ng4", (0, 64, 96)),
    ("fp8", 97, 68, 2176, "swiglu", False, 2, (), "fp8_stream_ng4", (31, 96)),
    ("fp8", 257, 260, 640, "adapter", False, 0, (), "fp8_t128_s4", (0, 127, 256)),
    ("fp8", 1921, 2948, 384, "plain", False, 0, (), "fp8_t128_s2", (0, 1919, 1920)),
    ("fp8", 257, 260, 640, "plain", True, 0, ((19, 256),), "fp8_t256", (0, 255, 256)),
    ("fp8", 257, 132, 384, "swiglu", False, 0, ((19, 256),), "fp8_t256", (5, 256)),
    ("mx4", 32, 144, 1152, "plain", False, 2, (), "mx4_stream_ng1", (0, 31)),
    ("mx4", 64, 144, 1152, "adapter", True, 2, (), "mx4_stream_ng2", (0, 33, 63)),
    ("mx4", 97, 144, 5248, "plain", True, 2, (), "mx4_stream_ng4", (0, 64, 96)),
    ("mx4", 97, 80, 2176, "swiglu", False, 2, (), "mx4_stream_ng4", (31, 96)),
    ("mx4", 257, 272, 640, "adapter", False, 0, (), "mx4_t128_s4", (0, 127, 256)),
    ("mx4", 1921, 2960, 384, "plain", False, 0, (), "mx4_t128_s2", (0, 1919, 1920)),
]


@pytest.mark.parametrize("fmt,M,N,K,epi,resid,kernel,tune,route,rows", INVARIANCE, ids=[f"{c[8]}-{c[4]}" for c in INVARIANCE])
def test_a_rows_bits_do_not_depend_on_the_rows_packed_with_it(fmt, M, N, K, epi, resid, kernel, tune, route, rows):
    """Random e4m3 / e2m1 bytes and real scales: the fp32 sums round, so the summation order shows.  Row r of the M-row call equals
    the same row run alone through the same selector and tuning (alone it may take the sibling form of its family — one row
    group, or four stages for a one-tile grid — which the kernels document to keep the row's chain)."""
    from dualhyp_amd import _lib, ops
    from dualhyp_amd.quant import pack_mxfp4
    lib = _lib.load()
    c = Q.Case("inv", "inv", fmt, "linear", M, N, K, epi=epi, resid=resid)
    o = Q.operands(Q.Case("inv", "inv", fmt, "linear", M, N, 128, epi=epi, resid=resid))          # scales, vectors, residual
    i = {"xq": _bytes(("ix", M, K), (M, K)).to(DEV), "xs": o["xs"].to(DEV)}
    for s in ("", "2")[:2 if epi == "swiglu" else 1]:
        if fmt == "fp8":
            i[f"w{s}q"], i[f"w{s}sc"] = _bytes(("iw" + s, N, K), (N, K)).to(DEV), o["ws" + s].to(DEV)
        else:
            codes = torch.randint(0, 16, (N, K), generator=Q._gen("ic" + s, N, K)).to(torch.uint8)
            i[f"w{s}q"], i[f"w{s}sc"] = (t.to(DEV) for t in pack_mxfp4(codes, Q._scales4("w" + s, N, K, epi == "swiglu")))
    for k in ("a", "b", "resid"):
        if k in o:
            i[k] = o[k].to(DEV)

    def run(sel, n_rows):
        j = dict(i)
        if sel is not None:
            j.update(xq=i["xq"][sel:sel + 1].contiguous(), xs=i["xs"][sel:sel + 1].contiguous())
            if resid:
                j["resid"] = i["resid"][sel:sel + 1].contiguous()
        out = torch.empty((n_rows, N), dtype=torch.bfloat16, device=DEV)
        try:
            for k, v in tune:
                assert lib.dh_set_tuning(k, v) == 0
            lib.dh_debug_gemm_routes(1)
            _call(Q.Case("inv", "inv", fmt, "linear", n_rows, N, K, epi=epi, resid=resid, kernel=1 if kernel == 0 else kernel), j, out)
            return out, R.route_names(lib.dh_debug_gemm_routes(1))
        finally:
            for k, _ in tune:
                lib.dh_set_tuning(k, Q.TUNING_DEFAULTS[k])

    full, took = run(None, M)
    assert took == {route}, f"{c.id}: ran {sorted(took)}"
    assert not torch.isnan(full.float()).any()
    for r in rows:
        alone, took1 = run(r, 1)
        assert len(took1) == 1 and next(iter(took1)).split("_")[:2] == route.split("_")[:2], f"row alone ran {sorted(took1)}"
        assert torch.equal(alone[0].view(torch.int16), full[r].view(torch.int16)), f"{c.id}: row {r} differs when it runs alone ({sorted(took1)})"
