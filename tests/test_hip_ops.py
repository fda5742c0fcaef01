"""GPU parity of each HIP kernel against the oracle's op on the same seeded inputs, through the
C ABI (dualhyp_amd.ops -> libdualhyp_hip.so).  Tolerances are in bf16 ulps: the kernels round
at the reference's rounding points, so differences can only come from fp32 summation order
(a result landing on the other side of a bf16 rounding boundary)."""
import math

import pytest
import torch

from conftest import ulp_diff, record_parity
from dualhyp_amd.synth import uniform, stream_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def U(shape, bound, name, seed=11):
    return uniform(shape, bound, stream_id(seed, name))


def check_ulp(got, want, max_ulp, max_frac, what, floor_frac=1.0):
    """floor_frac = 1: yardstick is the bf16 ulp at max(|a|,|b|,rms) — right for results that are
    sums of O(rms) rounded intermediates (residual adds, LoRA adds, attention averages)."""
    u = ulp_diff(got.float().cpu(), want.float(), floor_frac)
    frac = (u > 0).float().mean().item()
    assert u.max().item() <= max_ulp and frac <= max_frac, f"{what}: max {u.max().item():.2f} ulp, {frac:.3%} of elements differ"
    return u.max().item(), frac


@pytest.mark.parametrize("rows,d", [(37, 2048), (5, 256), (3, 4096), (64, 512)])
def test_rmsnorm(dev, rows, d):
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    # (row by row and bit for bit, every MAXC class, ragged d and guard bands: tests/test_hip_norm_exact.py::test_rmsnorm)
    x = U((rows, d), 2.0, f"x{d}")
    w = (1 + U((d,), 0.25, f"w{d}").float()).bfloat16()
    # torch's CPU bf16 rsqrt rounds differently in its vector loop and its scalar tail (the last
    # rows % 32 of the call); row_tail reproduces that, so the match is bit-exact
    # up to fp32 summation order in the mean.
    tail = (torch.arange(rows) >= rows // 32 * 32).to(torch.uint8)
    got = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5, row_tail=tail.to(dev))
    check_ulp(got, O.rmsnorm(x, w, 1e-5), 1, 0.002, "rmsnorm")
    r = U((rows, d), 1.0, f"r{d}")
    got, s = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5, resid=r.to(dev), return_sum=True, row_tail=tail.to(dev))
    assert torch.equal(s.cpu(), x + r)
    check_ulp(got, O.rmsnorm(x + r, w, 1e-5), 1, 0.002, "add+rmsnorm")
    # without flags every row uses the single-rounding form
    xf = x.float()
    rb = lambda v: v.bfloat16().float()
    rr = rb(1 / torch.sqrt(rb(rb(rb(xf * xf).sum(-1, keepdim=True) / d) + 1e-5)))
    want = rb(w.float() * rb(xf * rr))
    got = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5)
    assert (got.float().cpu() != want).float().mean().item() < 0.002


def test_embed(dev):
    from dualhyp_amd import ops
    wte = U((300, 256), 1.0, "wte")
    ids = torch.tensor([0, 5, 299, 7, 7, 123], dtype=torch.int64)
    assert torch.equal(ops.embed(ids.to(dev), wte.to(dev)).cpu(), wte[ids])


@pytest.mark.parametrize("M,N,K", [(100, 384, 256), (1, 128, 64), (257, 2560, 2048), (33, 136, 128), (640, 256, 5632)])
def test_linear_plain_and_resid(dev, M, N, K):
    from dualhyp_amd import ops
    x, w = U((M, K), 1.0, "lx"), U((N, K), 0.05, "lw")
    want = torch.nn.functional.linear(x, w)
    check_ulp(ops.linear(x.to(dev), w.to(dev)), want, 1, 0.002, "linear", floor_frac=1 / 16)
    r = U((M, N), 1.0, "lr")
    check_ulp(ops.linear(x.to(dev), w.to(dev), resid=r.to(dev)), r + want, 2, 0.002, "linear+resid")


@pytest.mark.parametrize("M,d,r", [(70, 256, 4), (130, 2048, 16), (300, 256, 4), (517, 2048, 16)])
def test_linear_lora(dev, M, d, r):
    """ger/lora.py:159-166 (proj) and :367-402 (qkv, contiguous [Q|K|V] delta, quirk Q2)."""
    from dualhyp_amd import ops
    from dualhyp_amd.gpt import _pad_rank
    from oracle import ger_oracle as O
    kv = d // 2
    N = d + 2 * kv
    x = U((1, M, d), 1.0, "qx")
    W = U((N, d), 0.05, "qw")
    A = U((3 * r, d), 1 / math.sqrt(d), "qa")
    B = U((N, r), 0.05, "qb")
    s = 2.0
    want = O.lora_qkv_linear(x, W, A, B, s, (d, kv, kv))
    A48 = torch.zeros(48, d, dtype=torch.bfloat16)
    for seg in range(3):
        A48[16 * seg:16 * seg + r] = A[seg * r:(seg + 1) * r]
    B16 = _pad_rank(B, r, 1)
    xd = x.to(dev)
    xa = ops.linear(xd, A48.to(dev))
    got = ops.linear(xd, W.to(dev), epilogue=ops.EPI_LORA, xa=xa, lora_b=B16.to(dev), lora_scale=s, splits=(d, d + kv))
    check_ulp(got, want, 2, 0.002, "qkv lora")
    # single-segment (attn.proj) with fused residual
    Wp, Ap, Bp = U((d, d), 0.05, "pw"), U((r, d), 1 / math.sqrt(d), "pa"), U((d, r), 0.05, "pb")
    res = U((1, M, d), 1.0, "pr")
    want = res + O.lora_linear(x, Wp, Ap, Bp, s)
    xa = ops.linear(xd, _pad_rank(Ap, r, 0).to(dev))
    got = ops.linear(xd, Wp.to(dev), epilogue=ops.EPI_LORA, xa=xa, lora_b=_pad_rank(Bp, r, 1).to(dev), lora_scale=s,
                     resid=res.to(dev))
    check_ulp(got, want, 2, 0.002, "proj lora + resid")


def test_linear_tile_size_invariant(dev):
    """dh_linear_impl sends a prompt that runs alone (M = 512) to the 128-tile kernel and the same rows packed with
    31 others (M = 16384) to the 256-tile kernel.  Both use mfma 16x16x32 with one accumulator per output and k
    ascending in steps of 32, so a row must come out bit-identical either way — for every epilogue the prefill uses."""
    from dualhyp_amd import ops
    d, I, big, small, m0 = 2048, 5632, 16384, 512, 7 * 512
    x = U((big, d), 1.0, "tx").to(dev)
    xs = x[m0:m0 + small].contiguous()
    w = U((2560, d), 0.05, "tw").to(dev)
    assert torch.equal(ops.linear(x, w)[m0:m0 + small], ops.linear(xs, w)), "PLAIN: 128-tile and 256-tile kernels differ"
    r = U((big, 2560), 1.0, "tr").to(dev)
    assert torch.equal(ops.linear(x, w, resid=r)[m0:m0 + small], ops.linear(xs, w, resid=r[m0:m0 + small].contiguous()))
    A48, B16 = U((48, d), 1 / math.sqrt(d), "ta").to(dev), U((2560, 16), 0.05, "tb").to(dev)
    xa = ops.linear(x, A48)
    xas = ops.linear(xs, A48)
    assert torch.equal(xa[m0:m0 + small], xas)
    kw = dict(epilogue=ops.EPI_LORA, lora_b=B16, lora_scale=2.0, splits=(2048, 2304))
    assert torch.equal(ops.linear(x, w, xa=xa, **kw)[m0:m0 + small], ops.linear(xs, w, xa=xas, **kw)), "LORA differs"
    w1, w2 = U((I, d), 0.05, "t1").to(dev), U((I, d), 0.05, "t2").to(dev)
    assert torch.equal(ops.linear(x, w1, epilogue=ops.EPI_SWIGLU, w2=w2)[m0:m0 + small],
                       ops.linear(xs, w1, epilogue=ops.EPI_SWIGLU, w2=w2)), "SWIGLU differs"
    act = U((big, I), 1.0, "tact").to(dev)
    wp = U((d, I), 0.05, "tp").to(dev)
    rr = U((big, d), 1.0, "trr").to(dev)
    assert torch.equal(ops.linear(act, wp, resid=rr)[m0:m0 + small],
                       ops.linear(act[m0:m0 + small].contiguous(), wp, resid=rr[m0:m0 + small].contiguous())), "K = 5632 differs"
    # a ragged tail: M not a multiple of either tile
    xt = x[: 16384 - 77].contiguous()
    assert torch.equal(ops.linear(xt, w)[-300:], ops.linear(xt[-300:].contiguous(), w))


def test_linear_256_tile_variants_bit_equal(dev):
    """The 256-tile prefill GEMM's loop variants (dh_set_tuning key 1: 2 = 8 waves in phase, 1 = 8 waves ping-pong, 5 = the
    default four waves with 128 x 128 each, full-line stages and asm MFMAs; key 22: its persistent-block modes) run the same chain per
    output — one accumulator, k ascending in steps of 32 — and share one epilogue: every epilogue must come out bit-identical, on
    full tiles, on the ragged last row band (M = 8192 - 77: the run-time-bounded epilogue) and with more tiles than CUs (the
    persistent walk, next tile's first stages requested in front of the epilogue)."""
    from dualhyp_amd import ops, _lib
    lib = _lib.load()
    d, I, M = 2048, 1408, 8192 - 77
    x = U((M, d), 1.0, "vx").to(dev)
    w = U((2560, d), 0.05, "vw").to(dev)
    r = U((M, 2560), 1.0, "vr").to(dev)
    A48, B16 = U((48, d), 1 / math.sqrt(d), "va").to(dev), U((2560, 16), 0.05, "vb").to(dev)
    w1, w2 = U((I, d), 0.05, "v1").to(dev), U((I, d), 0.05, "v2").to(dev)
    act, wp, rr = U((M, I), 1.0, "vact").to(dev), U((d, I), 0.05, "vp").to(dev), U((M, d), 1.0, "vrr").to(dev)
    xa = ops.linear(x, A48)

    def run():
        return [ops.linear(x, w), ops.linear(x, w, resid=r),
                ops.linear(x, w, epilogue=ops.EPI_LORA, xa=xa, lora_b=B16, lora_scale=2.0, splits=(2048, 2304)),
                ops.linear(x, w, epilogue=ops.EPI_LORA, xa=xa, lora_b=B16, lora_scale=1.0, splits=(2048, 2304), resid=r),
                ops.linear(x, w1, epilogue=ops.EPI_SWIGLU, w2=w2), ops.linear(act, wp, resid=rr)]
    # ragged N: the last column tile is partly outside the matrix (N = 2464 = 9.6 tiles; 1344 SwiGLU pairs = 10.5 tiles of 128)
    wr, rrr = w[:2464].contiguous(), r[:, :2464].contiguous()
    w1r, w2r = w1[:1344].contiguous(), w2[:1344].contiguous()

    def run_ragged():
        return [ops.linear(x, wr), ops.linear(x, wr, resid=rrr), ops.linear(x, w1r, epilogue=ops.EPI_SWIGLU, w2=w2r)]
    _run = run
    run = lambda: _run() + run_ragged()
    names = ["plain", "plain + resid", "lora", "lora + resid", "swiglu", "K = 1408 + resid", "plain N = 2464", "plain + resid N = 2464", "swiglu I = 1344"]
    try:
        lib.dh_set_tuning(1, 2)
        want = run()
        assert float(want[0].float().abs().sum()) > 0
        for variant, persist in ((1, 1), (5, 0), (5, 1), (5, 2)):
            lib.dh_set_tuning(1, variant)
            lib.dh_set_tuning(22, persist)
            for nm, a, b in zip(names, want, run()):
                assert torch.equal(a, b), f"variant {variant} persist {persist}: {nm} differs from the in-phase 8-wave kernel"
    finally:
        lib.dh_set_tuning(1, 5)
        lib.dh_set_tuning(22, 1)


@pytest.mark.parametrize("M", [8192, 8192 - 77, 700])
def test_linear_lora_down_projection_in_the_gemm(dev, M):
    """dh_linear_lora_bf16 / dh_linear_qkv_lora_rope_cache_bf16 (ABI 4): the LoRA down-projection bf16(x A^T) computed by the library —
    inside the 4-wave 256-tile kernel's K loop for large M with tile-aligned segments (M = 8192, and 8192 - 77 with a ragged last row
    band), by a separate launch otherwise (M = 700: the 128-tile kernel; segment boundaries off the 256 grid) — must give the bits of
    the caller-side two-step form xa = linear(x, A); linear(x, W, EPI_LORA, xa)."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    d, kv = 2048, 256
    N = d + 2 * kv
    x = U((M, d), 1.0, "fx").to(dev)
    w, wp = U((N, d), 0.05, "fw").to(dev), U((d, d), 0.05, "fwp").to(dev)
    A48, B16 = U((48, d), 1 / math.sqrt(d), "fa").to(dev), U((N, 16), 0.05, "fb").to(dev)
    A16, Bp = U((16, d), 1 / math.sqrt(d), "fap").to(dev), U((d, 16), 0.05, "fbp").to(dev)
    res = U((M, d), 1.0, "fr").to(dev)
    # QKV-shaped: three segments at 2048 / 2304 (multiples of 256)
    want = ops.linear(x, w, epilogue=ops.EPI_LORA, xa=ops.linear(x, A48), lora_b=B16, lora_scale=2.0, splits=(d, d + kv))
    got_qkv = ops.linear_lora(x, w, A48, B16, lora_scale=2.0, splits=(d, d + kv))
    assert torch.equal(got_qkv, want)
    # attn.proj-shaped: one segment, fused residual, lora_scale 1 (its own code path in the epilogue)
    want = ops.linear(x, wp, epilogue=ops.EPI_LORA, xa=ops.linear(x, A16), lora_b=Bp, lora_scale=1.0, resid=res)
    got_proj = ops.linear_lora(x, wp, A16, Bp, lora_scale=1.0, resid=res)
    assert torch.equal(got_proj, want)
    # ... and DIRECTLY against the oracle's LoRA layers at this M (the in-GEMM form was tied to the
    # oracle only through the two-launch form at M <= 517): ger/lora.py:367-402 (QKV, contiguous [Q|K|V] delta) and :159-166
    # (proj) + the residual add of ger/model.py:313.  r = 16 here, so A48 / B16 are the reference's own A (3r, d) / B (N, r).
    xc = x.cpu().unsqueeze(0)
    want_o = O.lora_qkv_linear(xc, w.cpu(), A48.cpu(), B16.cpu(), 2.0, (d, kv, kv))[0]
    mu, fr = check_ulp(got_qkv, want_o, 2, 0.002, f"in-GEMM qkv lora vs oracle, M={M}")
    record_parity(f"linear_lora_in_gemm.qkv.M{M}", max_ulp=mu, differing_frac=fr)
    want_o = (res.cpu().unsqueeze(0) + O.lora_linear(xc, wp.cpu(), A16.cpu(), Bp.cpu(), 1.0))[0]
    mu, fr = check_ulp(got_proj, want_o, 2, 0.002, f"in-GEMM proj lora + resid vs oracle, M={M}")
    record_parity(f"linear_lora_in_gemm.proj_resid.M{M}", max_ulp=mu, differing_frac=fr)
    # with the 8-wave kernel selected the library must take the two-launch path by itself
    from dualhyp_amd import _lib
    try:
        _lib.load().dh_set_tuning(1, 1)
        assert torch.equal(ops.linear_lora(x, wp, A16, Bp, lora_scale=1.0, resid=res), want)
    finally:
        _lib.load().dh_set_tuning(1, 5)
    # segment boundaries off the 256-column grid: the library falls back to the separate launch
    want = ops.linear(x, w, epilogue=ops.EPI_LORA, xa=ops.linear(x, A48), lora_b=B16, lora_scale=2.0, splits=(d - 32, d + kv + 32))
    assert torch.equal(ops.linear_lora(x, w, A48, B16, lora_scale=2.0, splits=(d - 32, d + kv + 32)), want)
    if M < 8192 - 77:
        return
    # the fused QKV projection + rope + cache append
    hs, n_head, n_groups, s_max = 64, 32, 4, 512
    cos, sin = O.build_rope_cache(s_max, hs)
    cos, sin = cos.to(dev), sin.to(dev)
    i32 = torch.int32
    nseq = (M + s_max - 1) // s_max
    lens = [s_max] * (nseq - 1) + [M - s_max * (nseq - 1)]
    slot = torch.cat([torch.full((n,), i, dtype=i32) for i, n in enumerate(lens)]).to(dev)
    pos = torch.cat([torch.arange(n, dtype=i32) for n in lens]).to(dev)
    mk = lambda: (torch.zeros((nseq, n_groups, s_max, hs), dtype=torch.bfloat16, device=dev),
                  torch.zeros((nseq, n_groups, hs, s_max), dtype=torch.bfloat16, device=dev))
    kc1, vt1 = mk()
    kc2, vt2 = mk()
    q1 = ops.linear_qkv_rope_cache(x, w, cos, sin, slot, pos, kc1, vt1, n_head, n_groups, xa=ops.linear(x, A48), lora_b=B16, lora_scale=2.0)
    q2 = ops.linear_qkv_lora_rope_cache(x, w, A48, B16, cos, sin, slot, pos, kc2, vt2, n_head, n_groups, lora_scale=2.0)
    assert torch.equal(q1, q2) and torch.equal(kc1, kc2) and torch.equal(vt1, vt2)
    assert float(kc2.float().abs().sum()) > 0


@pytest.mark.parametrize("hs,n_head,n_groups,lora", [(64, 32, 4, True), (128, 32, 8, True), (64, 32, 4, False)])
def test_qkv_gemm_with_rope_and_cache_epilogue(dev, hs, n_head, n_groups, lora):
    """dh_linear_qkv_rope_cache_bf16 (rope + KV append inside the 256-tile QKV GEMM's epilogue) against the two-step
    form dh_linear_bf16(EPI_LORA) + dh_qkv_rope_cache_bf16 on a packed ragged batch: rotated q and both caches bit for bit."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    d = n_head * hs
    kv = n_groups * hs
    N = d + 2 * kv
    lens = [512] * 30 + [300, 212, 640, 384]                       # 16384 packed tokens, ragged tail
    M, s_max = sum(lens), 640
    x = U((M, d), 1.0, f"rq{hs}").to(dev)
    w = U((N, d), 0.03, f"rw{hs}").to(dev)
    A48, B16 = U((48, d), 1 / math.sqrt(d), f"ra{hs}").to(dev), U((N, 16), 0.05, f"rb{hs}").to(dev)
    cos, sin = O.build_rope_cache(s_max, hs)
    cos, sin = cos.to(dev), sin.to(dev)
    i32 = torch.int32
    slot = torch.cat([torch.full((n,), i, dtype=i32) for i, n in enumerate(lens)]).to(dev)
    pos = torch.cat([torch.arange(n, dtype=i32) for n in lens]).to(dev)
    B = len(lens)
    mk = lambda: (torch.zeros((B, n_groups, s_max, hs), dtype=torch.bfloat16, device=dev),
                  torch.zeros((B, n_groups, hs, s_max), dtype=torch.bfloat16, device=dev))
    kc1, vt1 = mk()
    xa = ops.linear(x, A48) if lora else None
    if lora:
        qkv = ops.linear(x, w, epilogue=ops.EPI_LORA, xa=xa, lora_b=B16, lora_scale=2.0, splits=(d, d + kv))
    else:
        qkv = ops.linear(x, w)
    q1 = ops.qkv_rope_cache(qkv, cos, sin, slot, pos, kc1, vt1, n_head, n_groups)
    assert float(kc1.float().abs().sum()) > 0 and float(vt1.float().abs().sum()) > 0
    # the default (four waves, block per tile), the same with persistent blocks (640 tiles on 256 CUs), and the 8-wave kernel
    from dualhyp_amd import _lib
    lib = _lib.load()
    try:
        for variant, persist in ((5, 1), (5, 2), (1, 1)):
            lib.dh_set_tuning(1, variant)
            lib.dh_set_tuning(22, persist)
            kc2, vt2 = mk()
            q2 = ops.linear_qkv_rope_cache(x, w, cos, sin, slot, pos, kc2, vt2, n_head, n_groups, xa=xa, lora_b=B16 if lora else None, lora_scale=2.0)
            assert torch.equal(q1, q2), f"variant {variant} persist {persist}: rotated q differs"
            assert torch.equal(kc1, kc2), f"variant {variant} persist {persist}: K cache differs"
            assert torch.equal(vt1, vt2), f"variant {variant} persist {persist}: V^T cache differs"
    finally:
        lib.dh_set_tuning(1, 5)
        lib.dh_set_tuning(22, 1)
    if lora:
        # round 4: the ABI-4 entry point with the LoRA down-projection inside the K loop runs the rebuilt epilogue (v_dot2 arithmetic,
        # one loop over the row strips, V^T through LDS as 16-byte stores where a strip is 16 aligned positions of one slot, the
        # scatter elsewhere): same bits as the two-step form, both head sizes, lora_scale 2 and 1 (the epilogue's two instantiations),
        # and with the last sequences shifted so that their strips are NOT aligned (512-token sequences are; 300 / 212 / 640 / 384
        # start on multiples of 4 only)
        for scale in (2.0, 1.0):
            kc0, vt0 = mk()
            q0 = ops.qkv_rope_cache(ops.linear(x, w, epilogue=ops.EPI_LORA, xa=xa, lora_b=B16, lora_scale=scale, splits=(d, d + kv)),
                                    cos, sin, slot, pos, kc0, vt0, n_head, n_groups)
            kc2, vt2 = mk()
            q2 = ops.linear_qkv_lora_rope_cache(x, w, A48, B16, cos, sin, slot, pos, kc2, vt2, n_head, n_groups, lora_scale=scale)
            assert torch.equal(q0, q2), f"in-GEMM LoRA, scale {scale}: rotated q differs"
            assert torch.equal(kc0, kc2), f"in-GEMM LoRA, scale {scale}: K cache differs"
            assert torch.equal(vt0, vt2), f"in-GEMM LoRA, scale {scale}: V^T cache differs"
        # a cached prefix: positions start at 37 (no strip is aligned to 16 keys): the scatter path everywhere
        s_big = s_max + 64
        cosb, sinb = (t.to(dev) for t in O.build_rope_cache(s_big, hs))
        mkb = lambda: (torch.zeros((B, n_groups, s_big, hs), dtype=torch.bfloat16, device=dev),
                       torch.zeros((B, n_groups, hs, s_big), dtype=torch.bfloat16, device=dev))
        pos37 = pos + 37
        kc0, vt0 = mkb()
        q0 = ops.qkv_rope_cache(ops.linear(x, w, epilogue=ops.EPI_LORA, xa=xa, lora_b=B16, lora_scale=2.0, splits=(d, d + kv)),
                                cosb, sinb, slot, pos37, kc0, vt0, n_head, n_groups)
        kc2, vt2 = mkb()
        q2 = ops.linear_qkv_lora_rope_cache(x, w, A48, B16, cosb, sinb, slot, pos37, kc2, vt2, n_head, n_groups, lora_scale=2.0)
        assert torch.equal(q0, q2) and torch.equal(kc0, kc2) and torch.equal(vt0, vt2), "in-GEMM LoRA, shifted positions"


@pytest.mark.parametrize("M,d,I", [(50, 256, 384), (200, 2048, 5632), (300, 256, 384), (515, 2048, 5632)])
def test_linear_swiglu_and_adapter(dev, M, d, I):
    from dualhyp_amd import ops
    x, w1, w2 = U((M, d), 1.0, "sx"), U((I, d), 0.05, "s1"), U((I, d), 0.05, "s2")
    F = torch.nn.functional
    want = F.silu(F.linear(x, w1)) * F.linear(x, w2)
    check_ulp(ops.linear(x.to(dev), w1.to(dev), epilogue=ops.EPI_SWIGLU, w2=w2.to(dev)), want, 2, 0.003, "swiglu")
    sc = (1 + U((I,), 0.5, "sc").float()).bfloat16()
    bi = U((I,), 0.5, "bi")
    want = sc * (F.linear(x, w1) + bi)
    check_ulp(ops.linear(x.to(dev), w1.to(dev), epilogue=ops.EPI_ADAPTER, scale=sc.to(dev), bias=bi.to(dev)), want,
              2, 0.002, "adapter")


@pytest.mark.parametrize("M", [1, 7, 32])
@pytest.mark.parametrize("d,I,r", [(256, 384, 4), (2048, 5632, 16)])
def test_linear_decode_shapes(dev, M, d, I, r):
    """M <= 32 takes the weight-streaming kernel (gemm_skinny.hip): all four epilogues."""
    from dualhyp_amd import ops
    from dualhyp_amd.gpt import _pad_rank
    from oracle import ger_oracle as O
    F = torch.nn.functional
    x = U((1, M, d), 1.0, f"dx{M}")
    kv = d // 2
    N = d + 2 * kv
    W, A, B = U((N, d), 0.05, "dw"), U((3 * r, d), 1 / math.sqrt(d), "da"), U((N, r), 0.05, "db")
    A48 = torch.zeros(48, d, dtype=torch.bfloat16)
    for seg in range(3):
        A48[16 * seg:16 * seg + r] = A[seg * r:(seg + 1) * r]
    xd = x.to(dev)
    xa = ops.linear(xd, A48.to(dev))
    check_ulp(xa[..., :r], F.linear(x, A)[..., :r], 1, 0.01, "xa", floor_frac=1 / 16)
    got = ops.linear(xd, W.to(dev), epilogue=ops.EPI_LORA, xa=xa, lora_b=_pad_rank(B, r, 1).to(dev), lora_scale=2.0,
                     splits=(d, d + kv))
    check_ulp(got, O.lora_qkv_linear(x, W, A, B, 2.0, (d, kv, kv)), 2, 0.01, "decode qkv lora")
    w1, w2, wp = U((I, d), 0.05, "d1"), U((I, d), 0.05, "d2"), U((d, I), 0.05, "dp")
    act_ref = F.silu(F.linear(x, w1)) * F.linear(x, w2)
    act = ops.linear(xd, w1.to(dev), epilogue=ops.EPI_SWIGLU, w2=w2.to(dev))
    check_ulp(act, act_ref, 2, 0.01, "decode swiglu")
    res = U((1, M, d), 1.0, "dres")
    got = ops.linear(act_ref.to(dev), wp.to(dev), resid=res.to(dev))
    check_ulp(got, res + F.linear(act_ref, wp), 2, 0.01, "decode mlp proj + resid")
    sc, bi = (1 + U((N,), 0.5, "dsc").float()).bfloat16(), U((N,), 0.5, "dbi")
    got = ops.linear(xd, W.to(dev), epilogue=ops.EPI_ADAPTER, scale=sc.to(dev), bias=bi.to(dev))
    check_ulp(got, sc * (F.linear(x, W) + bi), 2, 0.01, "decode adapter")


@pytest.mark.parametrize("M", [33, 100, 256, 640])
@pytest.mark.parametrize("N,n_ext,K,ks", [(2560, 48, 2048, 8), (2048, 0, 5632, 11), (2048, 16, 2048, 8), (384, 16, 256, 1), (256, 16, 384, 2)])
def test_linear_partial_wide_rows(dev, M, N, n_ext, K, ks):
    """Several 32-row groups in one launch (joint decode of several batches): every group's partial
    sums are bit-identical to the same rows in a launch of their own."""
    from dualhyp_amd import ops
    x = U((M, K), 1.0, f"wx{M}{K}").to(dev)
    W = U((N, K), 0.05, f"ww{N}{K}").to(dev)
    A = U((n_ext, K), 0.05, f"wa{K}").to(dev) if n_ext else None
    wide = ops.linear_partial(x, W, A, ksplit=ks)
    assert wide.shape == (ks, M, N + n_ext)
    for m0 in range(0, M, 32):
        alone = ops.linear_partial(x[m0:m0 + 32].contiguous(), W, A, ksplit=ks)
        assert torch.equal(alone, wide[:, m0:m0 + 32]), f"rows {m0}.. differ"
    ref = x.float() @ torch.cat([W, A]).float().T if n_ext else x.float() @ W.float().T
    got = wide.sum(0)
    assert (got - ref).abs().max().item() <= 1e-3 * ref.abs().max().item() + 1e-4
    # the tiled kernels (gemm_dt.hip) deliver the same slices already combined, bit for bit, in the decode family's ONE
    # order (include/dualhyp_hip.h): adjacent slices in pairs, pair sums in index order — the split-K kernel emits the
    # pair sums (what every decode step above 128 rows runs), the chain kernel the total
    if K % 64 == 0 and (K // 32 + ks - 1) // ks in (8, 16):
        pair_sums = torch.stack([wide[i] + wide[i + 1] if i + 1 < ks else wide[i] for i in range(0, ks, 2)])
        from dualhyp_amd import _lib
        for wn in (2, 4, 0):                    # 128 x 128 tiles on 4 waves, 128 x 256 on 8, the default choice
            _lib.load().dh_set_tuning(17, wn)
            try:
                pairs = ops.linear_partial_pairs(x, W, A, ksplit=ks)
            finally:
                _lib.load().dh_set_tuning(17, 0)
            assert pairs.shape == ((ks + 1) // 2, M, N + n_ext)
            assert torch.equal(pairs, pair_sums), f"split-K tiles (wn={wn}): pair sums differ from the streamed slices added in pairs"
        total = ops.combine_partials(wide, pairs=True)
        assert torch.equal(total, ops.combine_partials(pair_sums, pairs=False))
        if M >= 65:
            _lib.load().dh_set_tuning(7, 65)
            try:
                chain = ops.linear_chain(x, W, A, ksplit=ks)
            finally:
                _lib.load().dh_set_tuning(7, 1 << 30)
            assert torch.equal(chain, total), "tiled chain sum differs from the family's combine order of the streamed slices"
        # the consumers: slices (pairs flag) and pair sums give the same bits
        if N == 2048 and n_ext == 0:
            xres = U((M, N), 1.0, f"wr{M}").to(dev)
            wn_ = (1 + U((N,), 0.25, "wwn").float()).bfloat16().to(dev)
            a = ops.finish_norm(wide, N, xres, wn_, 1e-5, pairs=True)
            b = ops.finish_norm(pair_sums, N, xres, wn_, 1e-5, pairs=False)
            c = ops.finish_norm(total.unsqueeze(0), N, xres, wn_, 1e-5, pairs=False)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    else:
        with pytest.raises(Exception):
            ops.linear_chain(x, W, A, ksplit=ks)
        with pytest.raises(Exception):
            ops.linear_partial_pairs(x, W, A, ksplit=ks)


@pytest.mark.parametrize("d,I,V", [(2048, 5632, 32000), (256, 384, 256), (512, 768, 512)])
def test_decode_phase_linear_rows_invariant(dev, d, I, V):
    """Decode-phase GEMMs with fused epilogues: <= 64 rows stream the weights (gemm_mid.hip), more rows take
    the tiled kernel (gemm_dt.hip) — every row comes out bit-identical either way."""
    from dualhyp_amd import ops, _lib
    lib = _lib.load()
    M = 200
    x = U((M, d), 1.0, f"ix{d}").to(dev)
    w1, w2 = U((I, d), 0.05, f"i1{d}").to(dev), U((I, d), 0.05, f"i2{d}").to(dev)
    wl = U((V, d), 0.05, f"il{d}").to(dev)
    sc, bi = (1 + U((V,), 0.5, "isc").float()).bfloat16().to(dev), U((V,), 0.5, "ibi").to(dev)
    act = U((M, I), 1.0, f"ia{d}").to(dev)
    wp, res = U((d, I), 0.05, f"ip{d}").to(dev), U((M, d), 1.0, f"ir{d}").to(dev)
    calls = {
        "swiglu": lambda xs, sl: ops.linear(xs, w1, epilogue=ops.EPI_SWIGLU, w2=w2),
        "adapter": lambda xs, sl: ops.linear(xs, wl, epilogue=ops.EPI_ADAPTER, scale=sc, bias=bi),
        "plain+resid": lambda xs, sl: ops.linear(act[sl].contiguous(), wp, resid=res[sl].contiguous()),
    }
    lib.dh_set_tuning(4, 2)          # public dh_linear_bf16 in the decode phase
    lib.dh_set_tuning(6, 65)         # tiled kernel from 65 rows on (default 129; lm_head 65)
    try:
        for name, fn in calls.items():
            whole = fn(x, slice(0, M))
            for a in (0, 64, 150):
                sl = slice(a, min(a + 32, M))
                part = fn(x[sl].contiguous(), sl)
                assert torch.equal(part, whole[sl]), f"{name}: rows {a}.. differ between the tiled and the streaming kernel"
            sl = slice(100, 164)     # 64 rows: still the streaming kernel, two row groups
            assert torch.equal(fn(x[sl].contiguous(), sl), whole[sl]), name
    finally:
        lib.dh_set_tuning(4, 0)
        lib.dh_set_tuning(6, 129)


def _attn_setup(dev, hs, n_head, n_groups, lens, pos0, s_max, seed):
    """Random qkv for a ragged batch -> (ops outputs, oracle-side q/k/v per sequence)."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    qpk = n_head // n_groups
    width = (n_head + 2 * n_groups) * hs
    n_tok = sum(lens)
    qkv = U((n_tok, width), 1.0, f"aqkv{seed}")
    cos, sin = O.build_rope_cache(s_max, hs)
    slot = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)])
    pos = torch.cat([torch.arange(p, p + n, dtype=torch.int32) for p, n in zip(pos0, lens)])
    B = len(lens)
    kc = torch.zeros((B, n_groups, s_max, hs), dtype=torch.bfloat16, device=dev)
    vt = torch.zeros((B, n_groups, hs, s_max), dtype=torch.bfloat16, device=dev)
    q = ops.qkv_rope_cache(qkv.to(dev), cos.to(dev), sin.to(dev), slot.to(dev), pos.to(dev), kc, vt, n_head, n_groups)
    # oracle split/rope per sequence (ger/model.py:216-246)
    ref = []
    t0 = 0
    for n, p in zip(lens, pos0):
        x = qkv[t0:t0 + n].view(1, n, n_groups, qpk + 2, hs).permute(0, 2, 3, 1, 4)
        qq, kk, vv = x.split((qpk, 1, 1), dim=2)
        qq = qq.reshape(1, -1, n, hs)
        kk = kk.reshape(1, -1, n, hs)
        vv = vv.reshape(1, -1, n, hs)
        c, s = cos[p:p + n], sin[p:p + n]
        ref.append((O.apply_rope(qq, c, s), O.apply_rope(kk, c, s), vv))
        t0 += n
    return q, kc, vt, ref


# "long": BASELINE config 5's context (10-best x 2 prompts of ~1.5k tokens, hs 128): 24-27 key tiles of the online
# softmax per query block in the prefill kernel, 12+ split-KV partials in the decode kernels
LONG_LENS = [1700, 65, 1536]


@pytest.mark.parametrize("hs,n_head,n_groups,case", [(64, 32, 4, "short"), (64, 4, 2, "short"), (128, 8, 2, "short"), (128, 8, 2, "long"),
                                                     (64, 8, 2, "long")])
def test_qkv_rope_cache_and_prefill_attention(dev, hs, n_head, n_groups, case):
    from dualhyp_amd import ops
    lens, pos0, s_max = [70, 1, 33, 128], [0, 0, 0, 0], 192
    if case == "long":
        lens, pos0, s_max = LONG_LENS, [0, 0, 0], 1792
    q, kc, vt, ref = _attn_setup(dev, hs, n_head, n_groups, lens, pos0, s_max, seed=hs + n_head)
    qpk = n_head // n_groups
    t0 = 0
    for i, (n, (rq, rk, rv)) in enumerate(zip(lens, ref)):
        assert torch.equal(q[t0:t0 + n].cpu().permute(1, 0, 2), rq[0]), "rotated q"
        assert torch.equal(ops.kcache_to_plain(kc)[i, :, :n].cpu(), rk[0]), "k cache"
        assert torch.equal(ops.vcache_to_plain(vt)[i, :, :, :n].cpu().transpose(1, 2), rv[0]), "v^T cache"
        t0 += n
    i32 = torch.int32
    starts = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)[:-1]), dtype=i32)
    y = ops.attn_prefill(q, kc, vt, torch.arange(len(lens), dtype=i32).to(dev), starts.to(dev),
                         torch.tensor(lens, dtype=i32).to(dev), torch.tensor(pos0, dtype=i32).to(dev), max(lens))
    t0 = 0
    worst = 0.0
    for n, (rq, rk, rv) in zip(lens, ref):
        k = rk.repeat_interleave(qpk, dim=1)
        v = rv.repeat_interleave(qpk, dim=1)
        want = torch.nn.functional.scaled_dot_product_attention(rq, k, v, is_causal=True, scale=1 / math.sqrt(hs))
        want = want.transpose(1, 2).reshape(n, n_head * hs)
        # fp32 ground truth decides what "close" means: both are roundings of it
        truth = torch.nn.functional.scaled_dot_product_attention(rq.float(), k.float(), v.float(), is_causal=True,
                                                                 scale=1 / math.sqrt(hs)).transpose(1, 2).reshape(n, -1)
        got = y[t0:t0 + n].float().cpu()
        err_hip = (got - truth).abs().max().item()
        err_ref = (want.float() - truth).abs().max().item()
        assert err_hip <= max(2 * err_ref, 2e-2), f"prefill attention: hip err {err_hip} vs reference-kernel err {err_ref}"
        u = ulp_diff(got, want.float(), 1.0)
        worst = max(worst, u.max().item())
        # the reference's CPU kernel takes one KV block (<= 512 keys) against the final row max; this kernel
        # walks 64-key tiles with a running max, so P is rounded to bf16 at a different scale on
        # rows whose max moves: 1-ulp differences on up to ~15% of outputs at T = 128
        # (beyond 512 keys the reference's kernel walks 512-key blocks with a running max too, at block edges other than this
        # kernel's 64-key ones; and a long row's output is an average of many values, small against the rms floor of the ulp)
        frac = (u > 0).float().mean().item()
        if case == "short":
            assert u.max().item() <= 2.5 and frac < 0.20, f"{u.max().item()} ulp, {frac:.2%} differ"
        else:
            # At 1.5k keys neither bf16 kernel is "the" answer: each is 2-3 ulps from the fp32 result on its worst element, at
            # different elements (their P roundings differ in every one of the 24-27 tiles), so they sit up to ~5 ulps apart.
            # The gate is ACCURACY, in ulps against the fp32 truth: HIP's worst and mean error no larger than the reference
            # kernel's (x1.25 / +0.5 ulp of slack), and the two bf16 results no further apart than their errors add up to.
            u_ht, u_rt = ulp_diff(got, truth, 1.0), ulp_diff(want.float(), truth, 1.0)
            record_parity(f"attention.prefill_vs_oracle_bf16.hs{hs}.T{n}", max_ulp_hip_vs_oracle=u.max().item(), differing_frac=frac,
                          max_ulp_hip_vs_fp32=u_ht.max().item(), max_ulp_oracle_vs_fp32=u_rt.max().item(),
                          mean_ulp_hip_vs_fp32=u_ht.mean().item(), mean_ulp_oracle_vs_fp32=u_rt.mean().item())
            assert u_ht.max().item() <= 1.25 * u_rt.max().item() + 0.5 and u_ht.mean().item() <= 1.25 * u_rt.mean().item() + 0.02, \
                f"T={n}: HIP {u_ht.max().item():.2f} / {u_ht.mean().item():.3f} ulp (max / mean) from fp32, reference kernel {u_rt.max().item():.2f} / {u_rt.mean().item():.3f}"
            assert u.max().item() <= u_ht.max().item() + u_rt.max().item() + 1e-6
        t0 += n


@pytest.mark.parametrize("hs,n_head,n_groups,case", [(64, 32, 4, "short"), (128, 8, 2, "short"), (128, 8, 2, "long"), (64, 8, 2, "long")])
def test_chunked_prefill_and_decode_attention(dev, hs, n_head, n_groups, case):
    """Prefill T-1 tokens, then one decode token per sequence at ragged positions; the decode
    kernel must agree with the prefill kernel run on the same cache and with fp32 attention."""
    from dualhyp_amd import ops
    lens, s_max = [100, 37, 64, 1, 129], 192
    if case == "long":
        lens, s_max = [1700, 1601, 1537, 129, 1536], 1792
    q, kc, vt, ref = _attn_setup(dev, hs, n_head, n_groups, lens, [0] * len(lens), s_max, seed=3)
    qpk = n_head // n_groups
    i32 = torch.int32
    ends = torch.tensor(lens).cumsum(0)
    last_rows = (ends - 1).tolist()
    qd = q[last_rows].contiguous()                       # the last token of each sequence as a decode query
    kv_len = torch.tensor(lens, dtype=i32).to(dev)
    y = ops.attn_decode(qd, kc, vt, torch.arange(len(lens), dtype=i32).to(dev), kv_len)
    # the prefill kernel on the same cache: each sequence's last token as a 1-token chunk at position len-1
    starts1 = torch.arange(len(lens), dtype=i32).to(dev)
    y_pre = ops.attn_prefill(qd, kc, vt, torch.arange(len(lens), dtype=i32).to(dev), starts1, torch.ones(len(lens), dtype=i32).to(dev),
                             torch.tensor([n - 1 for n in lens], dtype=i32).to(dev), 1)
    worst = worst_pd = 0.0
    for i, (n, (rq, rk, rv)) in enumerate(zip(lens, ref)):
        k = rk.repeat_interleave(qpk, dim=1)
        v = rv.repeat_interleave(qpk, dim=1)
        sdpa = lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, scale=1 / math.sqrt(hs)).transpose(1, 2).reshape(-1)
        want = sdpa(rq[:, :, -1:], k, v).float()                       # the oracle's op in bf16: what the reference returns
        truth = sdpa(rq[:, :, -1:].float(), k.float(), v.float())
        got = y[i].float().cpu()
        err_hip, err_ref = (got - truth).abs().max().item(), (want - truth).abs().max().item()
        assert err_hip <= max(2 * err_ref, 2e-2), f"decode attention seq {i}: hip err {err_hip} vs reference-kernel err {err_ref}"
        u = ulp_diff(got, want, 1.0)
        worst = max(worst, u.max().item())
        # split-KV partials merged at the end vs the reference's single pass: same 2.5-ulp envelope as the prefill kernel
        # (a one-row softmax average is small against the rms floor of the ulp: most outputs differ by a fraction of it)
        assert u.max().item() <= 2.5 and u.mean().item() <= 0.5, f"seq {i}: max {u.max().item()} / mean {u.mean().item():.2f} ulp vs the oracle's bf16 SDPA"
        upd = ulp_diff(got, y_pre[i].float().cpu(), 1.0)
        worst_pd = max(worst_pd, upd.max().item())
        assert upd.max().item() <= 2.0, f"seq {i}: decode and prefill kernels differ by {upd.max().item()} ulp on the same cache"
    from conftest import record_parity
    record_parity(f"attention.decode_vs_oracle_bf16.hs{hs}.{case}", max_ulp=worst, max_ulp_decode_vs_prefill_kernel=worst_pd, max_keys=max(lens))


@pytest.mark.parametrize("hs,n_head,n_groups,r,case", [(64, 32, 4, 16, "short"), (64, 4, 2, 4, "short"), (128, 8, 2, 16, "short"),
                                                       (128, 8, 2, 16, "long"), (64, 8, 2, 16, "long")])
def test_fused_decode_kernels(dev, hs, n_head, n_groups, r, case):
    """The 3 kernels of the fused decode layer against the oracle ops they replace: partial-sum GEMM with the
    LoRA A rows appended, fused LoRA-finish + rope + cache append + attention, LoRA-finish + residual + norm."""
    from dualhyp_amd import ops
    from dualhyp_amd.gpt import _pad_rank
    from oracle import ger_oracle as O
    F = torch.nn.functional
    d = n_head * hs
    qpk = n_head // n_groups
    kv = n_groups * hs
    N = d + 2 * kv
    lens = [40, 1, 97, 64, 33]                      # kv_len per sequence INCLUDING the new token
    B, s_max, s = len(lens), 128, 2.0
    if case == "long":                              # config 5's context: 50+ 32-key tiles per (sequence, group), VERDICT r03 #2
        lens, s_max = [1601, 1, 1537, 1700, 129], 1792
    xn = U((B, d), 1.0, "fx")
    W, A, Bm = U((N, d), 0.05, "fw"), U((3 * r, d), 1 / math.sqrt(d), "fa"), U((N, r), 0.05, "fb")
    A48 = torch.zeros(48, d, dtype=torch.bfloat16)
    for seg in range(3):
        A48[16 * seg:16 * seg + r] = A[seg * r:(seg + 1) * r]
    for ks in (1, 2):
        y32 = ops.linear_partial(xn.to(dev), W.to(dev), A48.to(dev), ksplit=ks)
        want = xn.float() @ torch.cat([W, A48]).float().T
        assert (y32.sum(0).cpu() - want).abs().max().item() <= 2e-5 * want.abs().max().item() + 1e-5
    # ---- past context through the prefill kernels' cache writer, then the fused decode kernel
    cos, sin = O.build_rope_cache(s_max, hs)
    kc = torch.zeros((B, n_groups, s_max, hs), dtype=torch.bfloat16, device=dev)
    vt = torch.zeros((B, n_groups, hs, s_max), dtype=torch.bfloat16, device=dev)
    past = [U((n - 1, N), 1.0, f"past{i}") for i, n in enumerate(lens)]
    i32 = torch.int32
    for i, p in enumerate(past):
        if p.size(0):
            ops.qkv_rope_cache(p.to(dev), cos.to(dev), sin.to(dev), torch.full((p.size(0),), i, dtype=i32, device=dev),
                               torch.arange(p.size(0), dtype=i32, device=dev), kc, vt, n_head, n_groups)
    kv_len = torch.tensor(lens, dtype=i32, device=dev)
    y = ops.attn_decode_fused(y32, N, _pad_rank(Bm, r, 1).to(dev), s, (d, d + kv), cos.to(dev), sin.to(dev),
                              torch.arange(B, dtype=i32, device=dev), kv_len, kc, vt, n_head)
    qkv_new = O.lora_qkv_linear(xn.view(B, 1, d), W, A, Bm, s, (d, kv, kv))[:, 0]     # (B, N) bf16, reference rounding
    for i, n in enumerate(lens):
        full = torch.cat([past[i], qkv_new[i:i + 1]]).view(1, n, n_groups, qpk + 2, hs).permute(0, 2, 3, 1, 4)
        qq, kk, vv = full.split((qpk, 1, 1), dim=2)
        qq, kk, vv = qq.reshape(1, -1, n, hs), kk.reshape(1, -1, n, hs), vv.reshape(1, -1, n, hs)
        qq, kk = O.apply_rope(qq, cos[:n], sin[:n]), O.apply_rope(kk, cos[:n], sin[:n])
        # past rows untouched; the appended row may flip 1 ulp where the K-split partial sums round differently
        kcp, vtp = ops.kcache_to_plain(kc), ops.vcache_to_plain(vt)
        assert torch.equal(kcp[i, :, :n - 1].cpu(), kk[0][:, :n - 1]), "k cache: past rows"
        assert torch.equal(vtp[i, :, :, :n - 1].cpu().transpose(1, 2), vv[0][:, :n - 1]), "v^T cache: past rows"
        check_ulp(kcp[i, :, n - 1], kk[0][:, n - 1], 1, 0.01, "k cache: appended row")
        check_ulp(vtp[i, :, :, n - 1], vv[0][:, n - 1], 1, 0.01, "v^T cache: appended row")
        kb, vb = kk.repeat_interleave(qpk, dim=1), vv.repeat_interleave(qpk, dim=1)
        truth = F.scaled_dot_product_attention(qq[:, :, -1:].float(), kb.float(), vb.float(), scale=1 / math.sqrt(hs)).transpose(1, 2).reshape(-1)
        want = F.scaled_dot_product_attention(qq[:, :, -1:], kb, vb, scale=1 / math.sqrt(hs)).transpose(1, 2).reshape(-1).float()
        got = y[i].float().cpu()
        err, err_ref = (got - truth).abs().max().item(), (want - truth).abs().max().item()
        assert err <= max(2 * err_ref, 2e-2), f"fused decode attention seq {i}: err {err} vs reference-kernel err {err_ref}"
        u = ulp_diff(got, want, 1.0)          # the new token's q/k/v may already differ by 1 ulp from the oracle's (K-split sums)
        assert u.max().item() <= 3.0 and u.mean().item() <= 0.5, f"fused decode attention seq {i}: max {u.max().item()} / mean {u.mean().item():.2f} ulp vs the oracle's bf16 SDPA"
        if case == "long":
            record_parity(f"attention.fused_decode_vs_oracle_bf16.hs{hs}.keys{n}", max_ulp=u.max().item(), mean_ulp=u.mean().item(),
                          max_abs_hip_vs_fp32=err, max_abs_oracle_vs_fp32=err_ref)
    # ---- proj LoRA finish + residual + norm
    att = U((B, d), 1.0, "fatt")
    Wp, Ap, Bp = U((d, d), 0.05, "fwp"), U((r, d), 1 / math.sqrt(d), "fap"), U((d, r), 0.05, "fbp")
    xres = U((B, d), 1.0, "fres")
    wn = (1 + U((d,), 0.25, "fwn").float()).bfloat16()
    h32 = ops.linear_partial(att.to(dev), Wp.to(dev), _pad_rank(Ap, r, 0).to(dev), ksplit=2)
    tail = torch.ones(B, dtype=torch.uint8, device=dev)
    x1, n2 = ops.finish_norm(h32, d, xres.to(dev), wn.to(dev), 1e-5, lora_b=_pad_rank(Bp, r, 1).to(dev), lora_scale=s, row_tail=tail)
    x1_ref = xres + O.lora_linear(att, Wp, Ap, Bp, s)
    check_ulp(x1, x1_ref, 2, 0.002, "finish: proj lora + resid")
    # the norm is checked on the kernel's own x1 (single-row calls take torch's scalar rsqrt path, Q11)
    n2_ref = torch.cat([O.rmsnorm(x1.cpu()[i:i + 1], wn, 1e-5) for i in range(B)])
    check_ulp(n2, n2_ref, 1, 0.002, "finish: norm")
    # no-LoRA variant (mlp proj + residual + next norm)
    h32 = ops.linear_partial(att.to(dev), Wp.to(dev), None, ksplit=1)
    x2, _ = ops.finish_norm(h32, d, xres.to(dev), wn.to(dev), 1e-5)
    check_ulp(x2, xres + F.linear(att, Wp), 2, 0.002, "finish: plain resid")


def test_sampling_argmax_ties_and_eos(dev):
    """generate/base.py:62-80 tail: lowest-index arg-max after the bf16 temperature divide
    (Q6), EOS flag (Q7), frozen finished sequences."""
    from dualhyp_amd import ops
    V = 32000
    lg = U((4, V), 3.0, "slog")
    lg[0, 777] = 9.0
    lg[0, 31999] = 9.0          # exact tie -> lowest index
    lg[1, 5] = 8.0
    lg[2, V - 1] = 8.5
    lg[3, 100] = 7.0
    tokens = torch.zeros((4, 8), dtype=torch.int64, device=dev)
    length = torch.tensor([3, 1, 2, 4], dtype=torch.int32, device=dev)
    done = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev)
    ops.sample(lg.to(dev), tokens, length, done, temperature=0.2, top_k=1, eos_id=5)
    assert tokens.cpu()[0, 3] == 777 and tokens.cpu()[1, 1] == 5 and tokens.cpu()[2, 2] == V - 1
    assert length.tolist() == [4, 2, 3, 4] and done.tolist() == [0, 1, 0, 1]
    # ties created by the bf16 rounding of logit/temperature
    row = torch.zeros(V, dtype=torch.bfloat16)
    row[10], row[20] = 1.0, 1.0039062   # distinct logits ...
    want = int(torch.nonzero((row / 0.2) == (row / 0.2).max())[0])
    tokens.zero_(); length.fill_(0); done.zero_()
    ops.sample(row.view(1, -1).repeat(4, 1).to(dev), tokens, length, done, temperature=0.2, top_k=1)
    assert tokens[0, 0].item() == want


def test_sampling_topk_distribution(dev):
    from dualhyp_amd import ops
    V, k, n = 1000, 5, 4096
    base = torch.full((V,), -2.0)
    base[[3, 50, 400, 800, 999]] = torch.tensor([2.0, 1.5, 1.0, 0.5, 0.0])
    lg = base.bfloat16().view(1, -1).repeat(n, 1).to(dev)
    tokens = torch.zeros((n, 1), dtype=torch.int64, device=dev)
    length = torch.zeros(n, dtype=torch.int32, device=dev)
    done = torch.zeros(n, dtype=torch.int32, device=dev)
    ops.sample(lg, tokens, length, done, temperature=1.0, top_k=k, seed=99, step=0)
    picks = tokens.view(-1).cpu()
    assert set(picks.tolist()) <= {3, 50, 400, 800, 999}
    p = torch.softmax(torch.tensor([2.0, 1.5, 1.0, 0.5, 0.0]), 0)
    freq = torch.tensor([(picks == t).float().mean() for t in (3, 50, 400, 800, 999)])
    assert (freq - p).abs().max() < 0.03, (freq, p)


def test_noise_mask_classifier(dev):
    """RelPrompt reliability predictor on the HIP path vs the reference module's own outputs
    (tests/golden/noise_mask_classifier: ger/relprompt.py:126-147 run on the CPU, bf16 and fp32)."""
    from conftest import load_golden
    from dualhyp_amd.relprompt import NoiseMaskClassifier
    from dualhyp_amd.synth import uniform, stream_id
    t, meta = load_golden("noise_mask_classifier")
    for tag, mt in meta.items():
        C, pool, T = mt["C"], mt["pool"], mt["T"]
        m = NoiseMaskClassifier(C, pool_size=pool).eval()
        sd = {k: uniform(tuple(shape), 1.0 / math.sqrt(math.prod(shape[1:]) if len(shape) > 1 else 256.0), stream_id(mt["seed"], tag + k)).float()
              for k, shape in mt["shapes"].items()}
        m.load_state_dict(sd)
        m = m.to(dev)
        x = uniform((2, T, C), 1.5, stream_id(mt["seed"], tag + "x")).to(dev)
        got = m(x).float().cpu()
        want_b, want_f = t[f"{tag}.logits_bf16"].float(), t[f"{tag}.logits_fp32"]
        assert got.shape == want_f.shape == (2, (T + pool - 1) // pool, 3)
        e_hip, e_ref = (got - want_f).abs().max().item(), (want_b - want_f).abs().max().item()
        print(f"[parity] classifier {tag}: |hip-fp32|max {e_hip:.3e} vs |ref_bf16-fp32|max {e_ref:.3e}; "
              f"bit-exact vs ref bf16 {(got == want_b).float().mean().item():.1%}")
        assert e_hip <= 1.5 * e_ref + 1e-3
        assert torch.equal(got.argmax(-1), want_f.argmax(-1)) or (got - want_f).abs().max() < 0.02


@pytest.mark.parametrize("M,N,K", [(4480, 48, 2048), (17920, 16, 2048), (1000, 64, 2560), (700, 32, 128), (1000, 520, 64), (4480, 2048, 64)])
def test_skinny_n_gemm_keeps_the_tiled_kernels_bits(dev, M, N, K):
    """dh_linear_bf16 with 16-64 output columns and many rows (the LoRA down-projections of the fine-tune, x . A^T of a prefill) runs on
    gemm_skinny_n_kernel, with K = 64 and a wide N (the rank-padded up-projections) on gemm_k64_kernel: the bits of the tiled kernels
    (dh_set_tuning(31, 0)) and the oracle's F.linear to one bf16 rounding."""
    from dualhyp_amd import ops, _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(dev)
    got = ops.linear(x, w)
    try:
        lib.dh_set_tuning(31, 0)
        want = ops.linear(x, w)
    finally:
        lib.dh_set_tuning(31, 1)
    assert torch.equal(got, want)
    ref = (x.float() @ w.float().T)
    assert (got.float() - ref).abs().max().item() <= 2 ** -7 * ref.abs().max().item()


@pytest.mark.parametrize("M", [8192, 8115, 700])
def test_persistent_lora_and_residual_tiles_keep_the_bits(dev, M):
    """Round 4: the attn-proj (LoRA with the in-GEMM down-projection + residual) and mlp-proj (plain + residual) GEMMs run persistent
    blocks whose epilogue requests the next tile's first stages (dh_set_tuning(30, 1), the default) and start a tile with a counted
    wait that leaves the previous tile's last stores in flight (dh_set_tuning(24, bit 2)): bit-equal to one block per tile with
    vmcnt(0), on full and ragged row counts."""
    from dualhyp_amd import ops, _lib
    lib = _lib.load()
    d, I = 2048, 5632
    x, act, res = U((M, d), 1.0, f"px{M}").to(dev), U((M, I), 1.0, f"pa{M}").to(dev), U((M, d), 1.0, f"pr{M}").to(dev)
    Wp, Wm = U((d, d), 0.05, "pwp").to(dev), U((d, I), 0.05, "pwm").to(dev)
    A16, Bp = U((16, d), 0.05, "pa16").to(dev), U((d, 16), 0.05, "pbp").to(dev)
    run = lambda: (ops.linear_lora(x, Wp, A16, Bp, lora_scale=2.0, resid=res), ops.linear(act, Wm, resid=res))
    got = run()
    try:
        lib.dh_set_tuning(30, 0)
        lib.dh_set_tuning(24, 3)
        want = run()
    finally:
        lib.dh_set_tuning(30, 1)
        lib.dh_set_tuning(24, 7)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
