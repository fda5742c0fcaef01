"""GPU tests of MXFP6 activations beside MXFP4 weights (csrc/mxfp6.hip, dualhyp_amd.quant; include/dualhyp_hip.h "MXFP6 activations").

The two quantiser kernels bit for bit against the fp64 quantiser of tests/mxfp6_reference.py; the operand map of
v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 x e2m3 pair and both block scales, with one-hot operands and exact integer grids
through both GEMM kernels; the GEMMs (streaming and tiled, every epilogue) against the fp64 product; row and grid-class invariance;
the decoder end to end against oracle.OracleGPT with its block linears over MXFP6-quantised activations; batch invariance, the fp8
KV cache, two activation formats in one process, and the command line."""
import functools
import json

import pytest
import torch

import mxfp4_reference as R4
import mxfp6_reference as R
from conftest import ulp_diff, record_parity, bf16_ulp
from dualhyp_amd.synth import uniform, stream_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def U(shape, bound, name, seed=79):
    return uniform(shape, bound, stream_id(seed, name))


def dv(t):
    return t.to(DEV)


def _packed_w(codes, scales):
    from dualhyp_amd.quant import pack_mxfp4
    wq, ws = pack_mxfp4(codes, scales)
    return dv(wq), dv(ws)


def _packed_x(codes, scales, fill=0):
    from dualhyp_amd.quant import pack_mxfp6
    xq, xs = pack_mxfp6(codes, scales, fill=fill)
    return dv(xq), dv(xs)


# ---------------------------------------------------------------------------------------------- quantiser kernels
def _quant_input(rows, K):
    """Random rows over many binades with the blocks of the hand-made edge row in front (as many of its 12 as fit)."""
    g = torch.Generator().manual_seed(rows * 131 + K)
    x = U((rows, K), 1.5, f"q{rows}x{K}")
    x = (x.float() * torch.exp2(torch.randint(-12, 12, (rows, K // 32), generator=g).float()).repeat_interleave(32, dim=1)).bfloat16()
    edge = R.edge_row().view(12, 32)
    nb = min(12, rows * K // 32)
    first = (rows + K // 128) % 12                              # which edge blocks a small case gets differs from case to case
    x.view(-1, 32)[:nb] = edge[(torch.arange(nb) + first) % 12]
    return x


@pytest.mark.parametrize("K", [128, 384, 2048])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 130])
def test_quantiser_kernels_match_the_host_reference(rows, K):
    from dualhyp_amd import ops
    from dualhyp_amd.quant import unpack_mxfp6
    x = _quant_input(rows, K)
    rc, rs = R.quantize_blocks(x)
    xq, xs = ops.quant_rows_mxfp6(dv(x))
    c, s = R.unpack(xq, xs, rows, K)                            # the header's index arithmetic
    assert torch.equal(s, rs), f"E8M0 bytes differ at {(s != rs).nonzero()[:4].tolist()}"
    assert torch.equal(c, rc), f"e2m3 codes differ at {(c != rc).nonzero()[:4].tolist()}"
    c2, s2 = unpack_mxfp6(xq.cpu(), xs.cpu(), rows)
    assert torch.equal(c2, rc) and torch.equal(s2, rs)
    G = (rows + 15) // 16                                       # the rows past `rows` keep the zeros the buffers were made with
    assert all(int(t[rows:].max()) == 0 for t in unpack_mxfp6(xq.cpu(), xs.cpu(), G * 16) if rows < G * 16)
    # the rmsnorm form quantises, bit for bit, the bf16 row dh_rmsnorm_bf16 produces
    xin, w = U((rows, K), 2.0, f"n{rows}x{K}"), (1 + U((K,), 0.5, f"nw{K}").float()).bfloat16()
    xn = ops.rmsnorm(dv(xin), dv(w), 1e-5)
    xn2, q2, sc2 = ops.rmsnorm_quant_mxfp6(dv(xin), dv(w), 1e-5)
    assert torch.equal(xn2, xn), "the bf16 row differs from dh_rmsnorm_bf16's"
    q1, sc1 = ops.quant_rows_mxfp6(xn)
    assert torch.equal(q2, q1) and torch.equal(sc2, sc1), "the fused form differs from the plain quantiser on dh_rmsnorm_bf16's row"
    nc, ns = R.quantize_blocks(xn.cpu())
    assert torch.equal(R.unpack(q2, sc2, rows, K)[0], nc) and torch.equal(R.unpack(q2, sc2, rows, K)[1], ns)


def test_rows_past_m_are_never_written_and_never_read_into_an_output():
    """M = 17: the last group of 16 has 15 rows that are no row of the matrix.  Pre-filled with 0xFF (codes 63, scale byte NaN) or
    with zeros, the quantisers leave them as they are, write the same bytes for the rows below M, and both GEMM kernels give the
    same outputs."""
    from dualhyp_amd import ops
    from dualhyp_amd.quant import unpack_mxfp6
    M, N, K = 17, 48, 384
    x, w = U((M, K), 1.5, "px"), U((N, K), 0.05, "pw")
    wq, ws = _packed_w(*R4.quantize_blocks(w))
    outs = []
    for fill in (0, 0xFF):
        xq, xs = ops.quant_rows_mxfp6(dv(x), fill=fill)
        c, s = unpack_mxfp6(xq.cpu(), xs.cpu(), 32)
        assert (c[M:] == (fill & 63)).all() and (s[M:] == fill).all(), "the quantiser wrote a row past M"
        _, xq2, xs2 = ops.rmsnorm_quant_mxfp6(dv(x), dv(torch.ones(K, dtype=torch.bfloat16)), 1e-5, fill=fill)
        c2, s2 = unpack_mxfp6(xq2.cpu(), xs2.cpu(), 32)
        assert (c2[M:] == (fill & 63)).all() and (s2[M:] == fill).all(), "the rmsnorm quantiser wrote a row past M"
        outs.append((c[:M], s[:M], c2[:M], s2[:M], ops.linear_mxfp4a6(xq, xs, M, wq, ws, kernel=1), ops.linear_mxfp4a6(xq, xs, M, wq, ws, kernel=2),
                     ops.linear_mxfp4a6(xq, xs, M, wq, ws, out32=True)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[1][4].float()).all() and outs[1][4].float().abs().max() > 0


# ---------------------------------------------------------------------------------------------- exact products
UNIT = 2.0 ** -5                                        # the smallest product: 0.125 * 2^-1 (x) times 0.5 * 2^0 (w)


@functools.lru_cache(maxsize=None)
def _integer_operands(K):
    """x: all 64 codes with scale bytes 126..128; w: all 16 codes with scale bytes 127..129; the rules differ between even and odd k,
    between the four MX blocks of a k-step and between k-steps, so a wrong bit position, plane, block or scale byte moves a sum."""
    M, N = 257, 144
    m, n, k = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    q, blk = (k // 32) % 4, torch.arange(K // 32).view(1, -1)
    xc = ((5 * m + 7 * k + (k & 1) * (m + 3) + q * (q + m) + 11 * (k // 128)) % 64).to(torch.uint8)
    xs = (126 + ((m + blk + blk // 4) % 3)).to(torch.uint8)
    wc = ((3 * n + 5 * k + (k & 1) * (n + 2) + q * (q + n)) % 16).to(torch.uint8)
    ws = (127 + ((n + 2 * blk + blk // 4) % 3)).to(torch.uint8)
    assert sorted(xc.unique().tolist()) == list(range(64)) and sorted(xs.unique().tolist()) == [126, 127, 128]
    assert sorted(wc.unique().tolist()) == list(range(16)) and sorted(ws.unique().tolist()) == [127, 128, 129]
    xd, wd = R.dequantize_blocks(xc, xs), R4.dequantize_blocks(wc, ws)
    # every term is a multiple of UNIT and the sum of their magnitudes stays below 2^24 units: fp32 is exact in any order
    assert torch.equal(xd / 2.0 ** -4, (xd / 2.0 ** -4).round()) and torch.equal(wd * 2, (wd * 2).round())
    assert ((xd.abs() @ wd.abs().T) / UNIT).max() < 2 ** 24
    return xc, xs, wc, ws, (xd @ wd.T).float().bfloat16()


@pytest.mark.parametrize("M", [1, 16, 17, 33, 65, 128, 129, 257])
def test_mxfp4a6_operand_map_exact_integers(M):
    """K = 128, 256, 384, 640 are 1, 2, 3 and 5 k-steps: every branch of the 4-stage prologue and its steady state; M = 33, 65 and 128
    sit on the row-group boundaries of the streaming kernel, 129 and 257 are tiled only; N = 16, 48, 144 is one W fragment, part of
    a tile and more than one tile."""
    from dualhyp_amd import ops
    for K in (128, 256, 384, 640):
        xc, xs_, wc, ws_, want = _integer_operands(K)
        xq, xs = _packed_x(xc[:M], xs_[:M], fill=0xFF)
        for N in (16, 48, 144):
            wq, ws = _packed_w(wc[:N], ws_[:N])
            w = want[:M, :N]
            for kernel in (1, 2):
                if kernel == 2 and M > 128:
                    continue
                y = ops.linear_mxfp4a6(xq, xs, M, wq, ws, kernel=kernel).cpu()
                assert torch.equal(y, w), f"M={M} N={N} K={K} kernel={kernel}: not the exact product; first at {(y != w).nonzero()[:4].tolist()}"
            auto = ops.linear_mxfp4a6(xq, xs, M, wq, ws).cpu()
            assert torch.equal(auto, w)
            if M <= 128:
                assert torch.equal(ops.linear_mxfp4a6(xq, xs, M, wq, ws, out32=True).cpu(), w.float()), f"fp32-out kernel, M={M} N={N} K={K}"


def test_mxfp4a6_one_hot_operands():
    """A single 1.0 per x row against every w code, and a single 1.0 per w row against every x code: each output is one element of the
    other operand, so the k a bit position stands for is pinned for every element position of a block, every block and k-step."""
    from dualhyp_amd import ops
    K = 384
    xc, xs_, wc, ws_, _ = _integer_operands(K)
    M, N = 128, 48
    km = (3 * torch.arange(M) + 1) % K                                    # 3 is coprime to 32 and to 384 / 32: every position of a block
    hot_x = torch.zeros((M, K), dtype=torch.uint8)
    hot_x[torch.arange(M), km] = 8                                        # e2m3 code of 1.0
    unit = torch.full((M, K // 32), 127, dtype=torch.uint8)
    wd = R4.dequantize_blocks(wc[:N], ws_[:N])
    want = wd[:, km].T.float().bfloat16()
    xq, xs = _packed_x(hot_x, unit)
    wq, ws = _packed_w(wc[:N], ws_[:N])
    for kernel in (1, 2):
        assert torch.equal(ops.linear_mxfp4a6(xq, xs, M, wq, ws, kernel=kernel).cpu(), want), f"one-hot x, kernel {kernel}"
    kn = (5 * torch.arange(N) + 2) % K
    hot_w = torch.zeros((N, K), dtype=torch.uint8)
    hot_w[torch.arange(N), kn] = 2                                        # e2m1 code of 1.0
    xd = R.dequantize_blocks(xc[:M], xs_[:M])
    want = xd[:, kn].float().bfloat16()
    xq, xs = _packed_x(xc[:M], xs_[:M])
    wq, ws = _packed_w(hot_w, torch.full((N, K // 32), 127, dtype=torch.uint8))
    for kernel in (1, 2):
        assert torch.equal(ops.linear_mxfp4a6(xq, xs, M, wq, ws, kernel=kernel).cpu(), want), f"one-hot w, kernel {kernel}"


# ---------------------------------------------------------------------------------------------- real values
def _first_rows(xq, xs, rows):
    """The buffers of the first `rows` rows: whole groups, so the last one keeps the bytes of real rows past `rows`."""
    g = (rows + 15) // 16
    return xq[:g].contiguous(), xs[:g].contiguous()


@pytest.mark.parametrize("M,N,K", [(7, 512, 512), (40, 256, 384), (96, 1024, 2048), (130, 1024, 4096), (257, 512, 1792)])
def test_linear_mxfp4a6_matches_the_fp64_product(M, N, K):
    """The operands are the same codes on both sides and every product is exact: only the fp32 summation order differs from the fp64
    sum, with mxfp4.hip's accumulation structure, so the gates are those of test_linear_mxfp4_matches_the_fp64_product.  Up to 128
    rows both kernels are checked, and a row's bits do not depend on how many rows ride along."""
    from dualhyp_amd import ops
    F = torch.nn.functional
    x, w, w2 = U((M, K), 1.5, "mx"), U((N, K), 0.05, "mw"), U((N, K), 0.05, "mw2")
    (c1, s1), (c2, s2) = R4.quantize_blocks(w), R4.quantize_blocks(w2)
    wq, ws = _packed_w(c1, s1)
    w2q, w2s = _packed_w(c2, s2)
    xq, xs = ops.quant_rows_mxfp6(dv(x))
    xc, xsc = R.unpack(xq, xs, M, K)
    y0, y2 = R.linear(xc, xsc, c1, s1).float().bfloat16(), R.linear(xc, xsc, c2, s2).float().bfloat16()
    r = U((M, N), 1.0, "mr")
    sc, bi = (1 + U((N,), 0.5, "ms").float()).bfloat16(), U((N,), 0.5, "mb")

    def chk(got, want, what, floor=1.0 / 16, max_ulp=2, max_frac=0.01):
        u = ulp_diff(got.float().cpu(), want.float(), floor)
        f = (u > 0).float().mean().item()
        record_parity(f"mxfp4a6_linear.{what}.M{M}N{N}K{K}", max_ulp=u.max().item(), bit_exact_frac=1.0 - f)
        assert u.max().item() <= max_ulp and f <= max_frac, f"{what}: max {u.max().item()} ulp, {f:.3%} differ"
    lin = functools.partial(ops.linear_mxfp4a6, xq, xs, M, wq, ws)
    for kernel, tag in ((2, "stream."), (1, "tiled.")) if M <= 128 else ((0, ""),):
        chk(lin(kernel=kernel), y0, tag + "plain")
        chk(lin(resid=dv(r), kernel=kernel), r + y0, tag + "resid", floor=1.0)
        chk(lin(epilogue=ops.EPI_SWIGLU, w2q=w2q, w2_scale=w2s, kernel=kernel), F.silu(y0) * y2, tag + "swiglu", max_ulp=4, max_frac=0.025)
        chk(lin(epilogue=ops.EPI_ADAPTER, scale=dv(sc), bias=dv(bi), kernel=kernel), sc * (y0 + bi), tag + "adapter", floor=1.0, max_ulp=4)
    # a row's bits do not depend on M within the streaming class (1 / 2 / 4 row groups) nor within the tiled class
    for kernel in (1, 2) if M <= 128 else (1,):
        full = lin(kernel=kernel)
        for rows in {1, min(M, 17), min(M, 33), min(M, 65), min(M, 129)}:
            pq, ps = _first_rows(xq, xs, rows)
            part = ops.linear_mxfp4a6(pq, ps, rows, wq, ws, kernel=kernel)
            assert torch.equal(part, full[:rows]), f"kernel {kernel}: rows 0..{rows} depend on the row count ({M} vs {rows})"
    if M <= 128:
        assert torch.equal(lin(out32=True), lin(kernel=2).float()), "the fp32-out kernel differs from the streaming kernel"


@pytest.mark.parametrize("epilogue", ["plain", "swiglu"])
def test_tiled_grid_classes_are_bit_identical(epilogue):
    """Grids of 384 tiles and more run the tiled kernel with two LDS stages and two blocks per CU, smaller ones with four stages;
    both walk k ascending in one accumulator, so a 128-row tile of the big call equals the same rows computed alone (the
    four-stage form the tests above hold against fp64)."""
    from dualhyp_amd import ops
    M, N, K = (1536, 4096, 384) if epilogue == "plain" else (768, 4096, 384)      # 12 x 32 and 6 x 64 tiles
    x, w, w2 = U((M, K), 1.5, "gx"), U((N, K), 0.05, "gw"), U((N, K), 0.05, "gw2")
    wq, ws = _packed_w(*R4.quantize_blocks(w))
    kw = dict(kernel=1)
    if epilogue == "swiglu":
        w2q, w2s = _packed_w(*R4.quantize_blocks(w2))
        kw.update(epilogue=ops.EPI_SWIGLU, w2q=w2q, w2_scale=w2s)
    xq, xs = ops.quant_rows_mxfp6(dv(x))
    lib = ops._lib.load()
    lib.dh_debug_gemm_routes(1)
    full = ops.linear_mxfp4a6(xq, xs, M, wq, ws, **kw)
    big = lib.dh_debug_gemm_routes(1)
    for r0 in (0, M - 128):
        part = ops.linear_mxfp4a6(xq[r0 // 16:r0 // 16 + 8].contiguous(), xs[r0 // 16:r0 // 16 + 8].contiguous(), 128, wq, ws, **kw)
        assert torch.equal(part, full[r0:r0 + 128]), f"rows {r0}.. of the {M}-row call differ from the same rows alone"
    small = lib.dh_debug_gemm_routes(1)
    # the five routes are appended behind mxfp4.hip's: stream ng1 / ng2 / ng4 = 35 / 36 / 37, tiled 4 stages = 38, 2 stages = 39
    assert big == 1 << 39 and small == 1 << 38, f"routes taken: {big:#x} (2 stages expected), {small:#x} (4 stages expected)"
    assert full.float().abs().max().item() > 0


# ---------------------------------------------------------------------------------------------- decoder end to end
from test_hip_mxfp4 import _tiny, rel_rms, T, G          # noqa: E402  the model, weights, prompts and oracles of the MXFP4 tests, built once


def _model(cfg, sd, kv_cache="bf16", activations="mxfp6"):
    from dualhyp_amd import GPT, quantize_model_mxfp4
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    m.eval()
    m.cpu_rsqrt_vec_width = 32
    quantize_model_mxfp4(m, kv_cache=kv_cache, activations=activations)
    return m


@functools.lru_cache(maxsize=None)
def _a6(kv_cache="bf16"):
    """The MXFP6-activation model over _tiny()'s weights and the oracle whose block linears see MXFP6-quantised activations."""
    import kv8_reference as R8
    from oracle import ger_oracle as O
    t = _tiny()
    inner = O.OracleGPT(t["cfg"], t["sdq"]) if kv_cache == "bf16" else R8.OracleGPTKV8(t["cfg"], t["sdq"])
    return dict(m=_model(t["cfg"], t["sd"], kv_cache=kv_cache), o=R.OracleA6(O, inner, [t["sdq"][k] for k in t["blocks"]]))


def _decisive(logits):
    """the restatement decides a step when its best logit leads the second by at least 4 bf16 ulps."""
    top = logits.float().topk(2).values
    return (top[0] - top[1]).item() >= 4 * bf16_ulp(top[0]).item()


@pytest.mark.parametrize("kv_cache", ["bf16", "fp8"])
def test_mxfp6_decoder_vs_oracle_restatement(kv_cache):
    """The gates of test_mxfp4_decoder_vs_oracle_restatement, measured against the restatement's own distance to the fp32 oracle;
    arg-max equality on the steps the restatement decides."""
    t, a = _tiny(), _a6(kv_cache)
    m, o, o32, idx = a["m"], a["o"], t["o32"], t["idx"]
    assert m.fp8 and m.weight_format == "mxfp4" and m.activation_format == "mxfp6" and m.kv_cache_dtype == kv_cache
    with torch.no_grad():
        got = m(torch.stack(idx).to(DEV)).float().cpu()
        want_q, want_32, want_a8 = o(torch.stack(idx)).float(), o32(torch.stack(idx)), t["oq"](torch.stack(idx)).float()
    assert m._engine.activation_format == "mxfp6" and m._engine.kv_cache_dtype == kv_cache
    d_hip, d_orc, d_pair, d_a8 = rel_rms(got, want_32), rel_rms(want_q, want_32), rel_rms(got, want_q), rel_rms(want_a8, want_32)
    record_parity(f"mxfp6_decoder.tiny.nocache.kv_{kv_cache}", rel_rms_hip_vs_fp32=d_hip, rel_rms_oracle_mxfp6_vs_fp32=d_orc,
                  rel_rms_hip_vs_oracle_mxfp6=d_pair, rel_rms_oracle_fp8_activations_vs_fp32=d_a8)
    assert d_hip <= 1.1 * d_orc and d_pair <= d_orc
    steps, agree = [], 0
    with torch.no_grad():
        m.reset_cache()
        o.reset_cache()
        lp = m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV)).float().cpu()
        rp = o(idx[0].view(1, -1), torch.arange(T)).float()
        d_prefill = rel_rms(lp, rp)
        tok = int(rp[0, -1].argmax())
        for sstep in range(G):
            ld = m(torch.tensor([[tok]], device=DEV), torch.tensor([T + sstep], device=DEV))[0, 0].float().cpu()
            rd = o(torch.tensor([[tok]]), torch.tensor([T + sstep]))[0, 0].float()
            steps.append((rel_rms(ld, rd), int(ld.argmax()), int(rd.argmax()), _decisive(rd)))
            agree += int(ld.argmax()) == int(rd.argmax())
            tok = int(rd.argmax())
        m.reset_cache()
        o.reset_cache()
    record_parity(f"mxfp6_decoder.tiny.cached.kv_{kv_cache}", rel_rms_prefill_hip_vs_oracle=d_prefill,
                  rel_rms_decode_steps_hip_vs_oracle=[s[0] for s in steps], argmax_equal=agree, decisive_steps=sum(s[3] for s in steps), steps=G)
    assert d_prefill <= d_orc
    for d, got_tok, want_tok, decisive in steps:
        assert d <= 1.25 * d_orc and (got_tok == want_tok or not decisive)
    assert any(s[3] for s in steps), "no step of the restatement is decisive: the arg-max gate checked nothing"


@pytest.mark.parametrize("kv_cache", ["bf16", "fp8"])
def test_mxfp6_batch_invariance(kv_cache):
    """generate_batch equals one-at-a-time for 33, 40 and 128 joint rows and for 96 ragged rows, with either KV cache."""
    from dualhyp_amd import generate, generate_batch
    m, idx = _a6(kv_cache)["m"], _tiny()["idx"]
    kw = dict(temperature=0.2, top_k=1)
    p0, p1 = idx[0][:23].to(DEV), idx[1].to(DEV)
    alone = [generate(m, p, p.numel() + 5, **kw).cpu() for p in (p0, p1)]
    assert m._engine.kv_cache_dtype == kv_cache and m._engine.activation_format == "mxfp6"
    both = [o.cpu() for o in generate_batch(m, [p0, p1], 5, **kw)]
    assert all(torch.equal(a, b) for a, b in zip(alone, both))
    for n, pb in ((33, 33), (40, 16), (128, 32)):
        joint = generate_batch(m, [p1] * n, 5, prefill_batch=pb, **kw)
        assert all(torch.equal(o.cpu(), alone[1]) for o in joint), f"{n}-row joint decode differs from the alone run"
    mixed = generate_batch(m, [p0, p1] * 48, 5, prefill_batch=32, **kw)      # 96 ragged rows
    assert all(torch.equal(o.cpu(), alone[i % 2]) for i, o in enumerate(mixed))


def test_two_activation_formats_in_one_process():
    """An e4m3-activation MXFP4 engine and an MXFP6-activation one generate in turn: each gives the ids it gives alone; a repeat call of
    quantize_model_mxfp4 switches an existing model over, engine included."""
    from dualhyp_amd import generate, quantize_model_mxfp4
    t = _tiny()
    cfg, sd, p = t["cfg"], t["sd"], t["idx"][1].to(DEV)
    kw = dict(temperature=0.2, top_k=1)
    models = {"fp8": t["m"], "mxfp6": _a6()["m"]}
    alone = {}
    for how in models:
        m = _model(cfg, sd, activations=how)
        alone[how] = generate(m, p, T + G, **kw).cpu()
        assert m._engine.activation_format == how
        del m
    for _ in range(2):
        for how, m in models.items():
            assert torch.equal(generate(m, p, T + G, **kw).cpu(), alone[how]), f"the {how}-activation model's ids change next to the other engine"
    m = _model(cfg, sd, activations="fp8")
    assert torch.equal(generate(m, p, T + G, **kw).cpu(), alone["fp8"])
    quantize_model_mxfp4(m, activations="mxfp6")
    assert torch.equal(generate(m, p, T + G, **kw).cpu(), alone["mxfp6"]) and m._engine.activation_format == "mxfp6"
    with torch.no_grad():   # the logits differ: the two formats are two models
        a = models["fp8"](p.view(1, -1)).float()
        b = models["mxfp6"](p.view(1, -1)).float()
    assert not torch.equal(a, b)
    for mm in models.values():
        mm.reset_cache()


def test_cli_quantize_mxfp4_activations_mxfp6(tmp_path):
    """`python -m dualhyp_amd.inference --random_init --quantize mxfp4 --activations mxfp6` on the merged-schema fixture of
    test_harness.py: the predictions of generate_batch on a model quantised through the API with the same settings; every record says
    which activation format produced it."""
    from test_harness import merged_items, CAPTIONS
    from dualhyp_amd import GPT, generate_batch, quantize_model_mxfp4
    from dualhyp_amd import inference as I
    from dualhyp_amd.data import HypothesesDataset
    from dualhyp_amd.synth import synth_state_dict
    from dualhyp_amd.tokenizer import ByteTokenizer
    items = merged_items(caps=CAPTIONS)
    test_json = tmp_path / "test.json"
    test_json.write_text(json.dumps(items))
    ckpt_dir = tmp_path / "checkpoints" / "parity-harness"
    ckpt_dir.mkdir(parents=True)
    new = 10
    argv = ["--test_path", str(test_json), "--llm_checkpoint", str(ckpt_dir), "--prompts_format", "DualHyp", "--dual_hypotheses",
            "--tokenizer", "byte", "--random_init", "--quantize", "mxfp4", "--activations", "mxfp6", "--max_new_tokens", str(new),
            "--decode_batch", "4", "--predict_dir", str(tmp_path / "predictions")]
    out = I.main(argv)
    preds = [p["inference"] for p in out["predictions"]]
    assert len(preds) == len(items) and all(p.get("activations") == "mxfp6" for p in out["predictions"])
    args = I.parse_args(argv)
    cfg = I.config_from_args(args)
    torch.manual_seed(args.seed)
    m = GPT(cfg)
    m.load_state_dict(synth_state_dict(cfg, seed=args.seed, embed_scale=50.0, head_tie=1.0))
    m = m.to(device=DEV, dtype=torch.bfloat16).eval()
    quantize_model_mxfp4(m, activations="mxfp6")
    tok = ByteTokenizer()
    ds = HypothesesDataset(str(test_json), tok, prompts_format="DualHyp", seed=args.seed)
    exs = [ds[i] for i in range(len(ds))]
    want = []
    for b in range(0, len(exs), 4):
        ps = [e["input_ids_no_response"].to(DEV) for e in exs[b:b + 4]]
        outs = generate_batch(m, ps, new, temperature=0.2, top_k=1, eos_id=tok.eos_token_id, prefill_batch=4)
        want += [I.extract_answer(tok.decode(o.cpu()), tok.decode(p.cpu())) for o, p in zip(outs, ps)]
    assert m._engine.activation_format == "mxfp6" and m.weight_format == "mxfp4"
    assert preds == want
