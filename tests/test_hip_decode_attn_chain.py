"""The decode step's short-chain kernels against the kernels they replace (csrc/decode_fused.hip).

attn_decode_chain_kernel (hs 64) and finish_norm_kernel<, true> change WHEN a block asks for its operands, never what it computes:
every output bit has to equal the parent kernels', which stay in the library behind dh_set_tuning 40 (attention) and 41
(finish_norm's hoisted loads from that many rows on) as the A/B arm.  The verify step's attention was not touched and still has to
give the bits of plain steps."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D_MODEL, N_HEAD, N_GROUPS, N_LAYER, S_MAX = 2048, 32, 4, 2, 576
LENS = (1, 31, 32, 33, 63, 64, 65, 511, 512, 545)   # one tile, tile edges, fewer tiles than waves, 17 tiles
ROWS = (1, 3, 32, 33, 129, 640)
KSPLIT = {1: 1, 3: 2}                                # K-slices of the partial-sum GEMMs: 1, 2 and 8 reach the <., 2, .> and <., 8, .> kernels
EPS = 1e-5


def _tuning(attn_chain, finish_hoist_rows):
    from dualhyp_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dh_set_tuning(40, attn_chain))
    _lib.check(lib.dh_set_tuning(41, finish_hoist_rows))


PARENT, NEW = (0, 0), (1, 1)       # NEW hoists finish_norm's loads at every row count, so each row count runs the new code


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    _tuning(1, -1)


def _weights(hs, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s, k=0.02: (torch.randn(*s, device=DEV, generator=g) * k).bfloat16()
    qkv_dim = (N_HEAD + 2 * N_GROUPS) * hs
    d_att = N_HEAD * hs
    return [dict(wqkv=r(qkv_dim, D_MODEL), aqkv=r(48, D_MODEL), bqkv=r(qkv_dim, 16, k=0.05), wproj=r(D_MODEL, d_att), aproj=r(16, d_att),
                 bproj=r(D_MODEL, 16, k=0.05), norm=(1 + r(D_MODEL, k=0.25).float()).bfloat16()) for _ in range(N_LAYER)]


def _inputs(rows, hs, lens, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed + rows)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    kv_len = torch.tensor([lens[(7 * i + i // len(lens)) % len(lens)] for i in range(rows)], dtype=torch.int32, device=DEV)
    return dict(x=r(rows, D_MODEL), xn=r(rows, D_MODEL), kv_len=kv_len, slot=torch.arange(rows, dtype=torch.int32, device=DEV).flip(0).contiguous(),
                cos=r(S_MAX, hs), sin=r(S_MAX, hs), kc=[r(rows, N_GROUPS, S_MAX, hs) for _ in range(N_LAYER)],
                vt=[r(rows, N_GROUPS, hs, S_MAX) for _ in range(N_LAYER)])


def _step(arm, W, I, hs, ksplit):
    """Attention sub-layer of N_LAYER decode layers from the ops: partial GEMM -> fused attention -> partial GEMM -> finish_norm."""
    from dualhyp_amd import ops
    _tuning(*arm)
    qkv_dim = (N_HEAD + 2 * N_GROUPS) * hs
    x, xn = I["x"].clone(), I["xn"].clone()
    kc, vt = [t.clone() for t in I["kc"]], [t.clone() for t in I["vt"]]
    out = dict(att=[], x=[], xn=[], kc=kc, vt=vt)
    for l, w in enumerate(W):
        q32 = ops.linear_partial(xn, w["wqkv"], w["aqkv"], ksplit=ksplit)
        att = ops.attn_decode_fused(q32, qkv_dim, w["bqkv"], 2.0, (N_HEAD * hs, (N_HEAD + N_GROUPS) * hs), I["cos"], I["sin"], I["slot"],
                                    I["kv_len"], kc[l], vt[l], N_HEAD)
        p32 = ops.linear_partial(att, w["wproj"], w["aproj"], ksplit=ksplit)
        x, xn = ops.finish_norm(p32, D_MODEL, x, w["norm"], EPS, lora_b=w["bproj"], lora_scale=2.0)
        out["att"].append(att); out["x"].append(x); out["xn"].append(xn)
    torch.cuda.synchronize()
    return out


def _same(a, b, rows, I, hs):
    from dualhyp_amd import ops
    for l in range(N_LAYER):
        for k in ("att", "x", "xn"):
            assert torch.isfinite(a[k][l].float()).all(), f"layer {l}: {k} of the parent arm is not finite"
            bad = (a[k][l] != b[k][l]).any(dim=1).nonzero().flatten().tolist()
            assert not bad, f"layer {l}: {k} differs in rows {bad[:8]} (kv_len {[int(I['kv_len'][r]) for r in bad[:8]]})"
        # the K tile and the V^T tile that hold the appended position, and everything else in the caches
        assert torch.equal(a["kc"][l], b["kc"][l]) and torch.equal(a["vt"][l], b["vt"][l]), f"layer {l}: the caches differ"
        kp, k0 = ops.kcache_to_plain(b["kc"][l]), ops.kcache_to_plain(I["kc"][l])
        vp, v0 = ops.vcache_to_plain(b["vt"][l]), ops.vcache_to_plain(I["vt"][l])
        for r in range(0, rows, max(1, rows // 16)):
            s, pos = int(I["slot"][r]), int(I["kv_len"][r]) - 1
            keep = torch.ones(S_MAX, dtype=torch.bool, device=DEV)
            keep[pos] = False
            assert torch.equal(kp[s][:, keep], k0[s][:, keep]) and torch.equal(vp[s][:, :, keep], v0[s][:, :, keep]), \
                f"layer {l} row {r}: the append wrote outside position {pos}"


@pytest.fixture(scope="module")
def weights64():
    return _weights(64)


@pytest.mark.parametrize("rows", ROWS)
def test_step_equals_parent_kernels(weights64, rows):
    I = _inputs(rows, 64, LENS)
    ks = KSPLIT.get(rows, 8)
    a, b = _step(PARENT, weights64, I, 64, ks), _step(NEW, weights64, I, 64, ks)
    _same(a, b, rows, I, 64)
    # the default selection (finish_norm's crossover by row count) gives the same bits as well
    _same(a, _step((1, -1), weights64, I, 64, ks), rows, I, 64)


@pytest.mark.parametrize("n_part,pairs", ((11, True), (6, False)))
def test_attention_with_many_partials(n_part, pairs):
    """The <., 16, .> instantiation (more than 8 partials) and partials that already are pair sums, on synthetic partial sums."""
    from dualhyp_amd import ops
    rows, hs = 33, 64
    I = _inputs(rows, hs, LENS)
    qkv_dim = (N_HEAD + 2 * N_GROUPS) * hs
    g = torch.Generator(device=DEV).manual_seed(9)
    q32 = torch.randn(n_part, rows, qkv_dim + 48, device=DEV, generator=g) * 0.3
    bq = (torch.randn(qkv_dim, 16, device=DEV, generator=g) * 0.05).bfloat16()
    res = []
    for arm in (PARENT, NEW):
        _tuning(*arm)
        kc, vt = I["kc"][0].clone(), I["vt"][0].clone()
        for lora in (bq, None):
            att = ops.attn_decode_fused(q32, qkv_dim, lora, 2.0, (N_HEAD * hs, (N_HEAD + N_GROUPS) * hs), I["cos"], I["sin"], I["slot"],
                                        I["kv_len"], kc, vt, N_HEAD, pairs=pairs)
            res.append((att, kc.clone(), vt.clone()))
    torch.cuda.synchronize()
    for (a, ak, av), (b, bk, bv) in zip(res[:2], res[2:]):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b) and torch.equal(ak, bk) and torch.equal(av, bv)


@pytest.mark.parametrize("hs", (128, 96))
def test_other_head_sizes(hs):
    """hs 96 and 128 keep attn_decode_fused_kernel whatever key 40 says; finish_norm's hoisted instantiation serves them too."""
    rows = 33
    W, I = _weights(hs), _inputs(rows, hs, (31, 65, 545))
    _same(_step(PARENT, W, I, hs, 8), _step(NEW, W, I, hs, 8), rows, I, hs)


def test_verify_step_equals_plain_steps():
    """speculate=3 against the plain run at hs 64: attn_verify_fused_kernel still gives, position by position, the bits of the
    single-token kernel that now is attn_decode_chain_kernel (the smallest case of tests/test_hip_speculate.py).
    The op itself, row by row against plain launches of the single-token op: tests/test_hip_verify_attn.py."""
    from dualhyp_amd import GPT, Config, generate_batch
    from dualhyp_amd.synth import synth_state_dict, synth_prompts
    new, kw = 24, dict(temperature=0.2, top_k=1)
    cfg = Config.from_name("parity-tiny", r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True, to_projection=True)
    assert cfg.head_size == 64
    # the shapes attn_decode_chain_kernel takes (one finish item per thread of its 512): otherwise the plain run is the parent kernel's
    assert (cfg.n_head // cfg.n_query_groups + 1) * 32 + 64 <= 512
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=11, norm_jitter=0.25, weight_scale=4.0, device=DEV))
    m.eval()
    ps = [synth_prompts(1, n, cfg.padded_vocab_size, seed=70 + i)[0].to(DEV) for i, n in enumerate((1, 30, 31, 32, 33, 47, 64))]
    want, st0 = generate_batch(m, ps, new, return_state=True, **kw)
    want, st0 = [o.clone() for o in want], {k: v.clone() for k, v in st0.items()}
    drafts = torch.zeros((len(ps), new), dtype=torch.int64, device=DEV)
    for u, p in enumerate(ps):
        drafts[u] = st0["tokens"][u, p.numel():p.numel() + new]
    drafts[:, 2::3] = (drafts[:, 2::3] + 1) % cfg.padded_vocab_size            # every third draft is wrong
    got, st1 = generate_batch(m, ps, new, speculate=3, drafts=drafts, return_state=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert torch.equal(st0["tokens"], st1["tokens"]) and torch.equal(st0["length"], st1["length"])
