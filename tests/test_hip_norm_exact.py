"""rmsnorm_kernel, finish_norm_kernel / finish_norm_rows_kernel, rmsnorm_quant_fp8_block_kernel, the two row-quantisation kernels
and embed_kernel against the plain CPU references of tests/norm_reference.py, inside guard bands.

Acceptance (norm_reference.py states it and derives D_CHAIN): grid and spike rows bit for bit; realistic rows bit for bit where
the reference proves the row decided, otherwise the whole row equals one of its two candidate rows bit for bit.  x_out, sum_out,
e4m3 bytes, scales and embeddings are bit for bit always.  No ulp count and no share of elements anywhere.  Every failing row is
named.  Inputs and outputs live in guarded buffers (gemm_exact_reference.Guarded): input margins hold NaN, output margins must
be intact and no sentinel may be left inside.  The C entries are called directly so that the outputs are the guarded buffers.
tests/test_norm_reference.py checks the references, the inputs and the acceptance's sensitivity on the CPU."""
import pytest
import torch

import norm_reference as R
from conftest import record_parity
from gemm_exact_reference import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_():
    from dualhyp_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _margin(shape) -> int:
    return max(4 * int(shape[-1]), 4096)


def _in(t: torch.Tensor) -> Guarded:
    return Guarded(t.shape, t.dtype, DEV, _margin(t.shape), t)


def _out(shape, dtype) -> Guarded:
    return Guarded(shape, dtype, DEV, _margin(shape))


def _call(what: str, fn, *args) -> None:
    """one library call and its completion; a HIP error ends the run: nothing more is started on a GPU that has faulted"""
    _lib, _ = _lib_()
    try:
        _lib.check(fn(*args, _stream()))
        torch.cuda.synchronize()
    except RuntimeError as e:
        s = str(e)
        if "HIP error" in s or "illegal memory access" in s or "kernel launch failed" in s or "hipError" in s:
            pytest.exit(f"{what}: {e} -- nothing more is started on a GPU that has faulted", 3)
        raise


def _guards(failures, what, **outs) -> None:
    for name, g in outs.items():
        try:
            g.check(f"{what}: {name}")
        except AssertionError as e:
            failures.append(str(e))


def _record(family: str, c, want: R.NormWant) -> None:
    record_parity(f"norm_exact.{family}.{c.id.replace(' ', ',')}", undecided=int(want.undecided.sum()), rows=c.rows)


def _finish(failures) -> None:
    assert not failures, f"{len(failures)} failing rows / guards:\n" + "\n".join(failures[:40])


@pytest.fixture(autouse=True)
def _tuning_defaults_afterwards():
    yield
    _, lib = _lib_()
    for key, value in R.FINISH_TUNING_DEFAULTS.items():
        lib.dh_set_tuning(key, value)


# ---- RMSNorm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.NORM_D)
def test_rmsnorm(d):
    """rmsnorm_kernel: MAXC 1 / 4 / 8 / 16 with full and ragged rows, 1 .. 259 rows, the spike in every chunk (d <= 2056) or at
    the ends of every stride group, with and without the residual (sum_out given and null), row_tail none / all / mixed"""
    _, lib = _lib_()
    failures = []
    for c in R.norm_cases(d):
        o = R.norm_inputs(c)
        tail = R.tails(c.rows)[c.tail]
        want = R.norm_want(o["sum"], o["w"], R.EPS, tail, c.kind != "real").to(DEV)
        _record("rmsnorm", c, want)
        x, w, r = _in(o["x"]), _in(o["w"]), _in(o["r"]) if c.resid else None
        t = None if tail is None else tail.to(DEV)
        for with_sum in ((True, False) if c.resid else (False,)):
            what = f"rmsnorm {c.id}" + ("" if with_sum or not c.resid else " sum_out=null")
            out, s = _out((c.rows, d), torch.bfloat16), _out((c.rows, d), torch.bfloat16) if with_sum else None
            _call(what, lib.dh_rmsnorm_bf16, _p(x.t), _p(r.t) if r else None, _p(w.t), _p(out.t), _p(s.t) if s else None, c.rows, d, R.EPS, _p(t))
            failures += R.norm_accept(want, out.t, what)
            if s is not None:
                failures += R.same_rows(s.t, o["sum"].to(DEV), what + ": sum_out")
            _guards(failures, what, out=out, **({"sum_out": s} if s else {}))
    _finish(failures)


# ---- finish + norm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.FINISH_D)
def test_finish_norm(d):
    """finish_norm_kernel plain and hoisted and finish_norm_rows_kernel (2, 3, 4 and the default rows per block) against ONE
    independent reference: x_out bit for bit on every element, xn_out under the norm acceptance computed from the reference
    x_out; MAXC 1 / 2 / 4, every (n_part, pairs) the producers emit, LoRA on and off, both scales, 1 .. 259 rows, in place."""
    _, lib = _lib_()
    failures = []
    for c in R.finish_cases(d):
        o = R.finish_inputs(c)
        x1, want = R.finish_reference(c, o)
        x1, want = x1.to(DEV), want.to(DEV)
        _record("finish", c, want)
        tail = R.tails(c.rows)[c.tail]
        t = None if tail is None else tail.to(DEV)
        h, x, w, b = _in(o["h32"]), _in(o["x"]), _in(o["w"]), _in(o["b"]) if c.lora else None
        x_out, xn_out = _out((c.rows, d), torch.bfloat16), _out((c.rows, d), torch.bfloat16)
        for arm, k41, k43, k44 in R.FINISH_ARMS:
            what = f"finish {c.id} [{arm}]"
            for key, value in ((41, k41), (43, k43), (44, k44)):
                assert lib.dh_set_tuning(key, value) == 0, (key, value)
            x_out.refill()
            xn_out.refill()
            if c.in_place:
                x_out.t.copy_(o["x"])
            _call(what, lib.dh_finish_norm_bf16, _p(h.t), c.n_part, c.pairs, c.rows, d, 16 if c.lora else 0, _p(b.t) if b else None, c.scale,
                  _p(x_out.t if c.in_place else x.t), _p(w.t), _p(x_out.t), _p(xn_out.t), R.EPS, _p(t))
            failures += R.same_rows(x_out.t, x1, what + ": x_out")
            failures += R.norm_accept(want, xn_out.t, what + ": xn_out")
            _guards(failures, what, x_out=x_out, xn_out=xn_out)
    _finish(failures)


# ---- RMSNorm + fp8 quantisation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.NQ_D)
def test_rmsnorm_quant_fp8(d):
    """rmsnorm_quant_fp8_block_kernel, EPT 8 / 16 / 32: the bf16 row under the norm acceptance, bytes and scale bit for bit the
    oracle's quantisation of the accepted row; xn_out given and null, row_tail none and mixed"""
    _, lib = _lib_()
    failures = []
    for c in R.norm_quant_cases(d):
        o = R.norm_quant_inputs(c)
        tail = R.tails(c.rows)[c.tail]
        want = R.norm_want(o["x"], o["w"], R.EPS, tail, c.kind != "real", quant=True).to(DEV)
        _record("rmsnorm_quant_fp8", c, want)
        what = f"rmsnorm_quant_fp8 {c.id}"
        x, w = _in(o["x"]), _in(o["w"])
        t = None if tail is None else tail.to(DEV)
        xn = _out((c.rows, d), torch.bfloat16) if c.xn else None
        q, s = _out((c.rows, d), torch.uint8), _out((c.rows,), torch.float32)
        _call(what, lib.dh_rmsnorm_quant_fp8, _p(x.t), _p(w.t), _p(xn.t) if xn else None, _p(q.t), _p(s.t), c.rows, d, R.EPS, _p(t))
        failures += R.norm_accept(want, xn.t if xn else None, what, q.t, s.t)
        _guards(failures, what, q=q, scale=s, **({"xn_out": xn} if xn else {}))
    _finish(failures)


# ---- row quantisation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.QUANT_K)
def test_quant_rows_fp8(K):
    """quant_rows_fp8_block_kernel (<= 256 rows) and quant_rows_fp8_kernel (above; last blocks of 1, 3 and 2 rows): bytes and
    scales bit for bit on realistic rows, an all-zero row, a row of e4m3 subnormals and amax in each chunk in turn"""
    _, lib = _lib_()
    failures = []
    pool, sweep = R.quant_inputs(K), R.quant_sweep(K)
    for name, src, counts in (("rows", pool, R.QUANT_ROWS), ("sweep", sweep, (sweep.size(0),))):
        q_ref, s_ref = R.quant_rows(src)
        q_ref, s_ref = q_ref.to(DEV), s_ref.to(DEV)
        for rows in counts:
            what = f"quant_rows_fp8 K={K} {name} rows={rows}"
            x = _in(src[:rows])
            q, s = _out((rows, K), torch.uint8), _out((rows,), torch.float32)
            _call(what, lib.dh_quant_rows_fp8, _p(x.t), _p(q.t), _p(s.t), rows, K)
            failures += R.same_rows(q.t, q_ref[:rows], what + ": bytes")
            failures += R.same_rows(s.t.view(-1, 1), s_ref[:rows].view(-1, 1), what + ": scale")
            _guards(failures, what, q=q, scale=s)
    _finish(failures)


# ---- embedding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.EMBED_D)
def test_embed_clamps_ids(d):
    """embed_kernel: ids -1, vocab and vocab + 7 read rows 0 and vocab - 1, nothing outside the table (its margins hold NaN)"""
    _, lib = _lib_()
    failures = []
    wte_cpu = R.real_rows(f"wte{d}", R.EMBED_VOCAB, d, 1.0)
    wte = _in(wte_cpu)
    for n_tok in R.EMBED_NTOK:
        what = f"embed d={d} n_tok={n_tok}"
        ids = torch.tensor(R.EMBED_IDS[:n_tok], dtype=torch.int64)
        ids_dev = ids.to(DEV)
        out = _out((n_tok, d), torch.bfloat16)
        _call(what, lib.dh_embed_bf16, _p(ids_dev), _p(wte.t), _p(out.t), n_tok, d, R.EMBED_VOCAB)
        failures += R.same_rows(out.t, R.embed_want(wte_cpu, ids).to(DEV), what)
        _guards(failures, what, out=out)
    _finish(failures)
