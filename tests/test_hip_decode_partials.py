"""The decode step's fp32 partial sums: the one-launch total on the register-lean tile (csrc/gemm_dt.hip, gemm_dt_chain_kernel)
and finish_norm over several rows per block (csrc/decode_fused.hip, finish_norm_rows_kernel).

Neither changes an output bit.  The chain tile gives the slices of the streaming kernel and the pair sums of the split-K kernel,
combined in the family's order; finish_norm_rows_kernel gives what finish_norm_kernel gives, which stays in the library behind
dh_set_tuning 43 (0: never the rows kernel) as the A/B arm; 44 sets the rows per block."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
CHAIN_OFF = 1 << 30
CHAIN_DEFAULT, PAIRS_DEFAULT = 1536, 288      # the library's defaults of keys 7 and 18 (gemm_dt.hip, gemm_skinny.hip)


def _lib_():
    from dualhyp_amd import _lib
    return _lib, _lib.load()


def _set(key, value):
    _lib, lib = _lib_()
    _lib.check(lib.dh_set_tuning(key, value))


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    _, lib = _lib_()
    for key, value in ((7, CHAIN_DEFAULT), (18, PAIRS_DEFAULT), (43, -1), (44, 0)):
        lib.dh_set_tuning(key, value)


def _rand(shape, scale, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


# ------------------------------------------------------------------------------------------ the chain tile
SHAPES = ((2560, 48, 2048, 8), (2048, 16, 2048, 8), (2048, 0, 5632, 11))     # the last: 11 slices, an unpaired last one


@pytest.fixture(scope="module")
def chain_operands():
    out = {}
    for n_main, n_ext, K, ks in SHAPES:
        out[(n_main, K)] = (_rand((257, K), 1.0, K + n_main).bfloat16(), _rand((n_main, K), 0.05, K + 1).bfloat16(),
                            _rand((n_ext, K), 0.05, K + 2).bfloat16() if n_ext else None)
    return out


@pytest.mark.parametrize("M", (1, 33, 129, 257))          # ragged last m-tiles; N = 2608 and 2064 are ragged last n-tiles
@pytest.mark.parametrize("n_main,n_ext,K,ks", SHAPES)
def test_chain_tile_equals_both_partial_routes(chain_operands, M, n_main, n_ext, K, ks):
    from dualhyp_amd import ops
    x, W, A = chain_operands[(n_main, K)]
    x = x[:M].contiguous()
    _set(7, 1)
    _set(18, 1)
    total = ops.linear_chain(x, W, A, ksplit=ks)
    slices = ops.linear_partial(x, W, A, ksplit=ks)
    pair_sums = ops.linear_partial_pairs(x, W, A, ksplit=ks)
    torch.cuda.synchronize()
    assert total.shape == (M, n_main + n_ext) and slices.shape[0] == ks and pair_sums.shape[0] == (ks + 1) // 2
    assert torch.isfinite(total).all() and total.abs().max().item() > 0
    assert torch.equal(total, ops.combine_partials(slices, pairs=True)), "chain tile differs from the streamed slices in the family's order"
    assert torch.equal(total, ops.combine_partials(pair_sums, pairs=False)), "chain tile differs from the split-K pair sums added in order"


# ------------------------------------------------------------------------------------------ finish_norm
ROWS = (1, 2, 3, 5, 130, 641)
PARTS = ((1, 0), (4, 0), (6, 0), (11, 1), (16, 1))        # what the producers emit: pair sums / the total with pairs = 0, raw slices with 1
MAX_ROWS = max(ROWS)


@pytest.fixture(scope="module")
def finish_operands():
    out = {}
    for d in (2048, 3072, 4096):
        out[d] = dict(h=_rand((16, MAX_ROWS, d + 16), 0.3, d), x=_rand((MAX_ROWS, d), 1.0, d + 1).bfloat16(),
                      w=(1 + _rand((d,), 0.25, d + 2)).bfloat16(), b=_rand((d, 16), 0.05, d + 3).bfloat16())
    return out


def _finish(arm, rpb, F, rows, d, n_part, pairs, lora, tail):
    from dualhyp_amd import ops
    _set(43, arm)
    _set(44, rpb)
    h = F["h"][:n_part, :rows].contiguous()
    if not lora:
        h = h[:, :, :d].contiguous()
    return ops.finish_norm(h, d, F["x"][:rows].contiguous(), F["w"], EPS, lora_b=F["b"] if lora else None, lora_scale=2.0,
                           row_tail=tail, pairs=bool(pairs))


@pytest.mark.parametrize("d", (2048, 3072, 4096))
@pytest.mark.parametrize("rows", ROWS)
def test_finish_norm_rows_kernel_equals_finish_norm_kernel(finish_operands, rows, d):
    """Both arms of key 43 at every (n_part, pairs), LoRA on and off, row_tail None and a mixed pattern; the rows kernel with 2, 3
    and 4 rows per block (a last block of 1, 2 and 3 rows among them) and with its default choice."""
    F = finish_operands[d]
    mixed = (torch.arange(rows, device=DEV) % 3 == 1).to(torch.uint8)
    for n_part, pairs in PARTS:
        for lora in (True, False):
            for tail in (None, mixed):
                old = _finish(0, 0, F, rows, d, n_part, pairs, lora, tail)
                assert torch.isfinite(old[0].float()).all() and torch.isfinite(old[1].float()).all()
                for rpb in (2, 3, 4, 0):
                    new = _finish(1, rpb, F, rows, d, n_part, pairs, lora, tail)
                    for name, a, b in (("x_out", old[0], new[0]), ("xn_out", old[1], new[1])):
                        bad = (a != b).any(dim=1).nonzero().flatten().tolist()
                        assert not bad, (f"{name} differs in rows {bad[:8]}: n_part {n_part} pairs {pairs} lora {lora} "
                                         f"tail {tail is not None} rows per block {rpb}")
                dflt = _finish(-1, 0, F, rows, d, n_part, pairs, lora, tail)
                assert torch.equal(old[0], dflt[0]) and torch.equal(old[1], dflt[1])


def test_finish_norm_in_place(finish_operands):
    """The engine's call: x_out is x_resid.  A block reads its rows' residuals a row ahead of writing them."""
    from dualhyp_amd import _lib, ops
    F, rows, d = finish_operands[2048], 130, 2048
    h = F["h"][:4, :rows].contiguous()
    want = _finish(0, 0, F, rows, d, 4, 0, True, None)
    _set(43, 1)
    x = F["x"][:rows].clone()
    xn = torch.empty_like(x)
    _lib.check(_lib.load().dh_finish_norm_bf16(ops._p(h), 4, 0, rows, d, 16, ops._p(F["b"]), 2.0, ops._p(x), ops._p(F["w"]), ops._p(x), ops._p(xn),
                                               EPS, None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(x, want[0]) and torch.equal(xn, want[1])


# ------------------------------------------------------------------------------------------ engine level
def test_engine_step_with_chain_tile():
    """A two-layer TinyLlama-shaped engine, one decode step at 130 rows: the chain route (key 7 = 128) against the default
    routes, logits and both caches; row 37 decoded alone against row 37 of the joint step."""
    from dualhyp_amd import GPT, Config
    from dualhyp_amd.synth import synth_state_dict
    rows, P = 130, 12
    cfg = Config.from_name("tiny-llama-1.1b-chat", n_layer=2, r=16, alpha=16, dropout=0.0, to_query=True, to_key=True, to_value=True,
                           to_projection=True)
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(cfg, seed=11, norm_jitter=0.25, weight_scale=4.0, device=DEV))
    m.eval()
    g = torch.Generator().manual_seed(3)
    prompts = torch.randint(3, cfg.padded_vocab_size, (rows, P), generator=g).to(DEV)
    nxt = torch.randint(3, cfg.padded_vocab_size, (rows,), generator=g).to(DEV)
    eng = m.engine(need_batch=rows, need_pos=64, need_tokens=rows * P, exact=True)
    G, hs = cfg.n_query_groups, cfg.head_size

    def step(chain_rows, which):
        _set(7, CHAIN_OFF)
        eng.forward_slots(prompts[which], [P] * len(which), which, prompt_phase=True)
        _set(7, chain_rows)
        logits = eng.forward_slots(nxt[which], [1] * len(which), which, pos0=P).clone()
        caches = [eng.read(what, layer, (eng.max_batch, G, eng.s_max, hs) if what == 1 else (eng.max_batch, G, hs, eng.s_max))
                  for layer in range(cfg.n_layer) for what in (1, 2)]
        torch.cuda.synchronize()
        return logits, caches

    every = list(range(rows))
    off, off_c = step(CHAIN_OFF, every)
    on, on_c = step(128, every)
    assert torch.isfinite(off.float()).all()
    assert torch.equal(on, off), "logits differ between the chain route and the default routes"
    assert all(torch.equal(a, b) for a, b in zip(on_c, off_c)), "the caches differ between the chain route and the default routes"
    alone, alone_c = step(128, [37])
    assert torch.equal(alone[0], on[37]), "row 37 alone differs from row 37 of the 130-row step"
    assert all(torch.equal(a[37], b[37]) for a, b in zip(alone_c, on_c)), "slot 37's cache differs between the two"
