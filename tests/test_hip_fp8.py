"""GPU tests of the fp8 serving path (csrc/fp8.hip, dualhyp_amd.quant; BASELINE config 5): the quantisation kernels
bit for bit against the oracle's torch-e4m3fn restatement, the fp8 MFMA's operand map with exact integer data, the
W8A8 GEMMs (streaming and tiled, every epilogue) against oracle.linear_fp8, and the whole decoder in fp8 mode:
its distance to the fp32 function must not exceed the oracle fp8 restatement's, and greedy ids must be the
reference's."""
import math

import functools
import json

import pytest
import torch

from conftest import ulp_diff, record_parity
from dualhyp_amd.synth import uniform, stream_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def U(shape, bound, name, seed=77):
    return uniform(shape, bound, stream_id(seed, name))


def test_row_quantisation_is_the_oracles():
    from dualhyp_amd import ops
    from dualhyp_amd.quant import quantize_rows_fp8
    from oracle import ger_oracle as O
    for rows, K in ((5, 512), (33, 4096), (3, 14336), (64, 2048)):
        x = U((rows, K), 3.0, f"q{K}")
        x[0, :] = 0                                    # an all-zero row: amax clamps to 1e-12
        x[1, :8] = torch.tensor([1e-3, -2e-3, 4e-4, 3.0, -3.0, 1e-5, 2.9, 0.0]).bfloat16()   # e4m3 subnormals after scaling
        q_ref, s_ref = O.quantize_rows_fp8(x)
        q, s = ops.quant_rows_fp8(x.to(DEV))
        assert torch.equal(s.cpu(), s_ref.view(-1)), "activation scales differ from the oracle's"
        assert torch.equal(q.cpu(), q_ref.view(torch.uint8)), "e4m3 bytes differ from torch's conversion"
        qw, sw = quantize_rows_fp8(x.to(DEV))          # the weight quantiser (torch ops on the device)
        assert torch.equal(qw.cpu(), q_ref.view(torch.uint8)) and torch.equal(sw.cpu(), s_ref.view(-1))
    # fused with RMSNorm (bit for bit against a CPU reference at every EPT, with row_tail: tests/test_hip_norm_exact.py)
    d = 4096
    w = (1 + U((d,), 0.25, "nw").float()).bfloat16()
    for rows in (37, 300):
        xr = U((rows, d), 2.0, f"nx{rows}")
        xn, q, s = ops.rmsnorm_quant_fp8(xr.to(DEV), w.to(DEV), 1e-5)
        want = ops.rmsnorm(xr.to(DEV), w.to(DEV), 1e-5)            # the bf16 kernel: same rounding points, another summation order
        u = ulp_diff(xn.float().cpu(), want.float().cpu(), 1.0)
        assert u.max().item() <= 1 and (u > 0).float().mean().item() <= 0.002
        q_ref, s_ref = O.quantize_rows_fp8(xn.cpu())               # quantisation of the row the kernel itself produced
        assert torch.equal(q.cpu(), q_ref.view(torch.uint8)) and torch.equal(s.cpu(), s_ref.view(-1))
    # a row's result does not depend on how many rows ride along
    xa = U((300, d), 2.0, "nx300").to(DEV)
    one = ops.rmsnorm_quant_fp8(xa[7:8].contiguous(), w.to(DEV), 1e-5)
    many = ops.rmsnorm_quant_fp8(xa, w.to(DEV), 1e-5)
    assert torch.equal(one[0][0], many[0][7]) and torch.equal(one[1][0], many[1][7]) and torch.equal(one[2], many[2][7:8])


@pytest.mark.parametrize("M", [1, 19, 32, 33, 96, 128, 200])
def test_fp8_mfma_operand_map_exact_integers(M):
    """Values in {-1, 0, 1} placed by an asymmetric rule in (row, k): every product and partial sum is exact, so any
    wrong lane -> (row, k) assumption of v_mfma_scale_f32_16x16x128_f8f6f4 shows as a wrong integer."""
    from dualhyp_amd import ops
    N, K = 80, 384
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    w = torch.randint(-1, 2, (N, K), generator=g).float()
    x[:, ::7] = 1.0                                       # break symmetry between k positions and between operands
    w[:, ::5] = -1.0
    xq, wq = x.to(torch.float8_e4m3fn).view(torch.uint8), w.to(torch.float8_e4m3fn).view(torch.uint8)
    ones_m, ones_n = torch.ones(M), torch.ones(N)
    want = x @ w.T
    assert want.abs().max() <= 256
    # every kernel that can take this row count: streaming (NG = 1, 2, 4 row groups: M <= 32 / 64 / 128) and tiled
    for kernel in (0, 1, 2):
        if kernel == 2 and M > 128:
            continue
        y = ops.linear_fp8(xq.to(DEV), ones_m.to(DEV), wq.to(DEV), ones_n.to(DEV), kernel=kernel)
        assert torch.equal(y.float().cpu(), want), f"fp8 GEMM (M={M}, kernel={kernel}) is not the exact integer product"


@pytest.mark.parametrize("M,N,K", [(7, 512, 512), (32, 2560, 2048), (40, 256, 384), (96, 1024, 2048), (128, 2560, 4096), (300, 2560, 2048),
                                   (130, 1024, 4096), (257, 512, 1792)])
def test_linear_fp8_matches_the_oracle(M, N, K):
    """Streaming kernel: M <= 32 (NG 1), <= 64 (NG 2), 65..128 (NG 4: the bench's 4 x 32-row decode step); tiled above.
    Up to 128 rows BOTH kernels are checked (the engine pins tiled for a prefill of any size)."""
    from dualhyp_amd import ops
    from oracle import ger_oracle as O
    x, w, w2 = U((M, K), 1.5, "fx"), U((N, K), 0.05, "fw"), U((N, K), 0.05, "fw2")
    wq, ws = O.quantize_rows_fp8(w)
    w2q, w2s = O.quantize_rows_fp8(w2)
    xq, xs = ops.quant_rows_fp8(x.to(DEV))
    dv = lambda t: t.to(DEV)
    wqd, wsd, w2qd, w2sd = dv(wq.view(torch.uint8)), dv(ws.view(-1)), dv(w2q.view(torch.uint8)), dv(w2s.view(-1))

    def chk(got, want, what, floor=1.0 / 16, max_ulp=2, max_frac=0.01):
        # same e4m3 operands on both sides: the only freedom is the fp32 summation order (MFMA vs the CPU's blocked
        # matmul) of K exact products of magnitude up to 2e5 — a result lands on the other side of a bf16 rounding
        # boundary in ~0.5 % of the outputs
        u = ulp_diff(got.float().cpu(), want.float(), floor)
        f = (u > 0).float().mean().item()
        record_parity(f"fp8_linear.{what}.M{M}N{N}K{K}", max_ulp=u.max().item(), bit_exact_frac=1.0 - f)
        assert u.max().item() <= max_ulp and f <= max_frac, f"{what}: max {u.max().item()} ulp, {f:.3%} differ"
    y0 = O.linear_fp8(x, wq, ws.view(-1))
    r = U((M, N), 1.0, "fr")
    F = torch.nn.functional
    sc, bi = (1 + U((N,), 0.5, "fs").float()).bfloat16(), U((N,), 0.5, "fb")
    for kernel, tag in ((2, "stream."), (1, "tiled.")) if M <= 128 else ((0, ""),):
        chk(ops.linear_fp8(xq, xs, wqd, wsd, kernel=kernel), y0, tag + "plain")
        chk(ops.linear_fp8(xq, xs, wqd, wsd, resid=dv(r), kernel=kernel), r + y0, tag + "resid", floor=1.0)   # a sum of two O(rms) terms
        chk(ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_SWIGLU, w2q=w2qd, w2_scale=w2sd, kernel=kernel),
            F.silu(y0) * O.linear_fp8(x, w2q, w2s.view(-1)), tag + "swiglu", max_ulp=4, max_frac=0.025)      # a product of two rounded values: their boundary flips add up
        chk(ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_ADAPTER, scale=dv(sc), bias=dv(bi), kernel=kernel), sc * (y0 + bi), tag + "adapter",
            floor=1.0, max_ulp=4)    # y0 + bias cancels: ulps at max(|a|, |b|, rms)
    if M > 128:
        # the 256 x 256 tile on sixteen waves (large prefills) runs the same fp32 chain per output as the 128-tile: bit-identical
        from dualhyp_amd import _lib
        base = {"plain": ops.linear_fp8(xq, xs, wqd, wsd), "resid": ops.linear_fp8(xq, xs, wqd, wsd, resid=dv(r)),
                "swiglu": ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_SWIGLU, w2q=w2qd, w2_scale=w2sd),
                "adapter": ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_ADAPTER, scale=dv(sc), bias=dv(bi))}
        _lib.load().dh_set_tuning(19, 256)
        try:
            big = {"plain": ops.linear_fp8(xq, xs, wqd, wsd), "resid": ops.linear_fp8(xq, xs, wqd, wsd, resid=dv(r)),
                   "swiglu": ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_SWIGLU, w2q=w2qd, w2_scale=w2sd),
                   "adapter": ops.linear_fp8(xq, xs, wqd, wsd, epilogue=ops.EPI_ADAPTER, scale=dv(sc), bias=dv(bi))}
        finally:
            _lib.load().dh_set_tuning(19, 0)
        for k in base:
            assert torch.equal(base[k], big[k]), f"256-tile fp8 GEMM differs from the 128-tile ({k}, M={M} N={N} K={K})"
    if M <= 128:
        # a row's bits do not depend on how many rows ride along, inside either kernel (1 row vs all M, across the
        # 32- and 64-row group boundaries of the streaming kernel)
        for kernel in (1, 2):
            full = ops.linear_fp8(xq, xs, wqd, wsd, kernel=kernel)
            for rows in {1, min(M, 33), min(M, 65)}:
                part = ops.linear_fp8(xq[:rows].contiguous(), xs[:rows].contiguous(), wqd, wsd, kernel=kernel)
                assert torch.equal(part, full[:rows]), f"kernel {kernel}: rows 0..{rows} depend on the row count ({M} vs {rows})"


def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def test_fp8_decoder_vs_oracle_restatement():
    """Tiny decoder (hs 128, LoRA r 16 merged), fp8 mode end to end: prefill + decode logits against the oracle's fp8
    restatement and against the fp32 function; greedy ids equal the bf16 oracle's (tied-head weights: margins of tens
    of ulps); batched ragged generate equals one-at-a-time."""
    from dualhyp_amd import GPT, Config, generate, generate_batch, quantize_model_fp8
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    from oracle import ger_oracle as O
    cfg = Config.from_name("parity-hs128", r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
    sd = synth_state_dict(cfg, seed=3, norm_jitter=0.25, weight_scale=4.0, embed_scale=64.0, head_tie=1.0)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    m.eval()
    m.cpu_rsqrt_vec_width = 32
    quantize_model_fp8(m)
    assert m.transformer.h[0].mlp.fc_1.linear.weight.numel() == 0 and m.transformer.h[0].mlp.fc_1.linear.weight_fp8.dtype == torch.uint8
    oq = O.OracleGPT(cfg, O.quantize_state_dict_fp8(sd, cfg))
    o32 = O.OracleGPT(cfg, {k: v.float() for k, v in sd.items()})
    obf = O.OracleGPT(cfg, sd)
    T, G = 40, 10
    idx = synth_prompts(2, T, cfg.padded_vocab_size, seed=9)
    with torch.no_grad():
        got = m(torch.stack(idx).to(DEV)).float().cpu()
        want_q, want_32 = oq(torch.stack(idx)).float(), o32(torch.stack(idx))
    d_hip, d_orc, d_pair = rel_rms(got, want_32), rel_rms(want_q, want_32), rel_rms(got, want_q)
    record_parity("fp8_decoder.tiny.nocache", rel_rms_hip_vs_fp32=d_hip, rel_rms_oracle_fp8_vs_fp32=d_orc, rel_rms_hip_vs_oracle_fp8=d_pair)
    # e4m3 steps are 6 %: a 1-ulp bf16 difference upstream moves some activation into the next fp8 bucket, so two
    # implementations of the SAME scheme differ by about half of what separates either from the fp32 function
    assert d_hip <= 1.1 * d_orc and d_pair <= d_orc
    # the weights the engine streams are the oracle's bytes
    q_ref = O.quantize_state_dict_fp8(sd, cfg)
    k = "transformer.h.1.attn.attn.linear.weight"
    assert torch.equal(m.transformer.h[1].attn.attn.linear.weight_fp8.cpu(), q_ref[k].view(torch.uint8))
    assert torch.equal(m.transformer.h[1].attn.attn.linear.weight_scale.cpu(), q_ref[k + "_scale"])
    # cached prefill + decode steps
    with torch.no_grad():
        m.reset_cache()
        lp = m(idx[0].view(1, -1).to(DEV), torch.arange(T, device=DEV)).float().cpu()
        rp = oq(idx[0].view(1, -1), torch.arange(T)).float()
        assert rel_rms(lp, rp) <= d_orc
        tok = int(rp[0, -1].argmax())
        for sstep in range(3):
            ld = m(torch.tensor([[tok]], device=DEV), torch.tensor([T + sstep], device=DEV))[0, 0].float().cpu()
            rd = oq(torch.tensor([[tok]]), torch.tensor([T + sstep]))[0, 0].float()
            assert rel_rms(ld, rd) <= 1.25 * d_orc and int(ld.argmax()) == int(rd.argmax())
            tok = int(rd.argmax())
        m.reset_cache()
    ids_bf = O.generate(obf, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    oq.reset_cache()
    ids_q = O.generate(oq, idx[1], T + G, temperature=0.2, top_k=1, mode="argmax")
    got_ids = generate(m, idx[1].to(DEV), T + G, temperature=0.2, top_k=1).cpu()
    record_parity("fp8_decoder.tiny.generate_ids", generated=G, equal_to_bf16_oracle=int((got_ids[T:] == ids_bf[T:]).sum()),
                  equal_to_fp8_oracle=int((got_ids[T:] == ids_q[T:]).sum()))
    assert torch.equal(got_ids, ids_q) and torch.equal(got_ids, ids_bf)
    p0, p1 = idx[0][:23].to(DEV), idx[1].to(DEV)
    alone = [generate(m, p, p.numel() + 5, temperature=0.2, top_k=1).cpu() for p in (p0, p1)]
    both = [o.cpu() for o in generate_batch(m, [p0, p1], 5, temperature=0.2, top_k=1)]
    assert all(torch.equal(a, b) for a, b in zip(alone, both))
    # joint decodes of 33 (streaming NG 2, just past the 32-row fused-attention launch), 40 and 128 prompts (NG 4: the
    # llama3-8b-fp8 bench's four batches per decode loop): same ids as the prompt alone.  The prefill is tiled whatever
    # the packing (a 40-token prompt alone, 16 of them packed), the decode streams up to 128 rows: kernels are pinned
    # by phase, csrc/engine.hip fp8_kernel
    for n, pb in ((33, 33), (40, 16), (128, 32)):
        joint = generate_batch(m, [idx[1].to(DEV)] * n, 5, temperature=0.2, top_k=1, prefill_batch=pb)
        assert all(torch.equal(o.cpu(), alone[1]) for o in joint), f"{n}-row joint decode differs from the alone run"
    mixed = generate_batch(m, [p0, p1] * 48, 5, temperature=0.2, top_k=1, prefill_batch=32)      # 96 ragged rows
    assert all(torch.equal(o.cpu(), alone[i % 2]) for i, o in enumerate(mixed))


@functools.lru_cache(maxsize=1)
def _oracle_fp8(cfg_json, kw_json):
    """The oracle's fp8 restatement of a synthetic model (quantising ~1 GB of weights on the CPU takes a minute: the two fixtures of
    test_fp8_llama3_shape_vs_reference share the configuration and the seed, so they share it)."""
    from dualhyp_amd import Config
    from dualhyp_amd.synth import synth_state_dict
    from oracle import ger_oracle as O
    cfg = Config(**json.loads(cfg_json))
    # generated on the GPU and copied: the counter-based generator gives the same tensors on both devices (checked once below on a
    # small tensor), 0.7 s against two minutes on the host cores for the 1.1 G parameters of this shape
    sd = {k: v.cpu() for k, v in synth_state_dict(cfg, device=DEV, **json.loads(kw_json)).items()}
    small = Config(**{**json.loads(cfg_json), "n_layer": 1, "padded_vocab_size": 512, "vocab_size": 512, "n_embd": 256, "intermediate_size": 512,
                      "n_head": 2, "n_query_groups": 1})
    a, b = synth_state_dict(small, **json.loads(kw_json)), synth_state_dict(small, device=DEV, **json.loads(kw_json))
    assert all(torch.equal(a[k], b[k].cpu()) for k in a)
    return O.OracleGPT(cfg, O.quantize_state_dict_fp8(sd, cfg))


@pytest.mark.parametrize("name", ["llama3_shape", "llama3_shape_1536"])
def test_fp8_llama3_shape_vs_reference(golden, name):
    """BASELINE config 5's layer shape (Llama-3-8B: d 4096, hs 128, 8 groups, I 14336, V 128256; 2 layers) in fp8 mode
    against the REFERENCE's tensors (tests/golden/llama3_shape at T = 96, llama3_shape_1536 at the configuration's real
    1536-token prompt + 16 decode steps): distance to the reference's fp32 logits no larger than the oracle fp8
    restatement's, and every one of the reference's greedy ids reproduced."""
    from dualhyp_amd import GPT, Config, generate, quantize_model_fp8
    from dualhyp_amd.synth import synth_state_dict
    from oracle import ger_oracle as O
    from conftest import load_golden
    t, meta = load_golden(name)
    cfg = Config(**meta["config"])
    kw = dict(seed=meta["seed"], embed_scale=meta["embed_scale"], head_tie=meta["head_tie"])
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, device=DEV, **kw))
    m.eval()
    m.cpu_rsqrt_vec_width = 32
    quantize_model_fp8(m)
    T, G = meta["T"], meta["G"]
    ids = t["generate_ids"]
    with torch.no_grad():
        lg = m(t["idx"].view(1, -1).to(DEV), torch.arange(T, device=DEV))[0, -4:, :4096].float().cpu()
    m.reset_cache()
    f32, bf = t["prefill_logits_last4_v4096_fp32"].float(), t["prefill_logits_last4_v4096"].float()
    oq = _oracle_fp8(json.dumps(meta["config"], sort_keys=True), json.dumps(kw, sort_keys=True))
    with torch.no_grad():      # the head on the four compared rows only (activations are quantised per token: rows are independent)
        want_q = oq.lm_head(oq.hidden(t["idx"].view(1, -1), torch.arange(T))[:, -4:])[0, :, :4096].float()
    d_hip, d_orc, d_bf = rel_rms(lg, f32), rel_rms(want_q, f32), rel_rms(bf, f32)
    record_parity(f"fp8_decoder.{name}.prefill", rel_rms_hip_fp8_vs_ref_fp32=d_hip, rel_rms_oracle_fp8_vs_ref_fp32=d_orc,
                  rel_rms_ref_bf16_vs_ref_fp32=d_bf, rel_rms_hip_vs_oracle_fp8=rel_rms(lg, want_q))
    assert d_hip <= 1.1 * d_orc and rel_rms(lg, want_q) <= d_orc
    free = generate(m, t["idx"].to(DEV), T + G, temperature=0.2, top_k=1).cpu()
    record_parity(f"fp8_decoder.{name}.generate_ids", generated=G, equal_to_reference=int((free[T:] == ids[T:]).sum()))
    assert torch.equal(free, ids)

