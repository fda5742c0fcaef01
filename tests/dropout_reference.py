"""CPU restatement of the LoRA-branch dropout draw (include/dualhyp_hip.h, "LoRA-branch dropout"), in numpy uint64 arithmetic and
torch-CPU bf16: helpers of test_dropout_reference.py, test_hip_dropout.py and test_hip_dropout_grads.py.  Nothing here calls the
library.

Element i of a call has chunk c = i / 8, half h = (i % 8) / 4, lane e = i % 4.  Its draw is word e of Philox4x32-10 (Salmon et
al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) on
    counter = {lo32(c), hi32(c) * 2 + h, lo32(step), hi32(step)},
    key     = {lo32(seed) ^ (call_id * 0x9E3779B9 mod 2^32), (hi32(seed) + call_id) mod 2^32};
keep iff draw >= thresh(p) = min(floor((double)(float)p * 2^32), 0xffffffff); m = bf16_rne(1.0f / (1.0f - (float)p)); a kept
element is bf16_rne(fp32(x) * fp32(m)), a dropped one +0 in both y and mask.

`injected_dropout` is the oracle-side half: it hands masks of this definition to oracle.ger_oracle's LoRA functions in call order
(layer l QKV = site 2l, layer l proj = site 2l + 1: the call ids dualhyp_amd/train.py uses), optionally with one of the backward
mutations the model-level tests must be able to see."""
import contextlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
MASK32 = 0xFFFFFFFF


# --------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10_scalar(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """Pure-Python integers: one counter block (4 words), one key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(v) & MASK32 for v in counter)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox4x32_10(counters: np.ndarray, key) -> np.ndarray:
    """Vectorised: counters [..., 4] and key [..., 2] (or one key for all) of 32-bit words -> uint64 [..., 4] holding 32-bit words."""
    c = np.asarray(counters, dtype=np.uint64) & np.uint64(MASK32)
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & np.uint64(MASK32), c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1)


# --------------------------------------------------------------------------- threshold, scale, key
def thresh(p: float) -> int:
    """keep iff draw >= thresh: min(floor((double)(float)p * 2^32), 0xffffffff)."""
    t = float(np.float32(p)) * 4294967296.0          # a float32 times a power of two: exact in double
    return MASK32 if t >= 4294967295.0 else int(t)


def scale_bits(p: float) -> int:
    """The bf16 bit pattern of round-to-nearest-even(1.0f / (1.0f - (float)p)), the division and subtraction in fp32."""
    v = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    u = int(np.asarray(v, dtype=np.float32).view(np.uint32))
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def scale(p: float) -> torch.Tensor:
    """The mask value of a kept element as a 0-d bf16 tensor."""
    return torch.tensor([scale_bits(p)], dtype=torch.int16).view(torch.bfloat16)[0]          # positive: the sign bit is clear


def key_words(seed: int, call_id: int) -> Tuple[int, int]:
    seed, call_id = int(seed) & (2 ** 64 - 1), int(call_id) & MASK32
    return (seed & MASK32) ^ ((call_id * W0) & MASK32), ((seed >> 32) + call_id) & MASK32


def counter_words(i: int, step: int) -> Tuple[int, int, int, int]:
    """Counter block of element i (scalar form of the definition)."""
    c, h, step = i // 8, (i % 8) // 4, int(step) & (2 ** 64 - 1)
    return c & MASK32, ((c >> 32) * 2 + h) & MASK32, step & MASK32, step >> 32


def draws(n: int, seed: int, call_id: int, step: Optional[int]) -> np.ndarray:
    """uint64 [n]: the 32-bit draw of every element of an n-element call (n % 8 == 0).  step None = a null step_dev = step 0."""
    assert n % 8 == 0 and n >= 0
    step = 0 if step is None else int(step) & (2 ** 64 - 1)
    c = np.arange(n // 8, dtype=np.uint64)
    ctr = np.empty((n // 8, 2, 4), dtype=np.uint64)
    ctr[:, :, 0] = (c & np.uint64(MASK32))[:, None]
    ctr[:, :, 1] = ((c >> np.uint64(32)) * np.uint64(2))[:, None] + np.arange(2, dtype=np.uint64)[None, :]
    ctr[:, :, 2] = step & MASK32
    ctr[:, :, 3] = step >> 32
    return philox4x32_10(ctr, key_words(seed, call_id)).reshape(n)


def keep_mask(n: int, p: float, seed: int, call_id: int, step: Optional[int]) -> torch.Tensor:
    """bool [n]: which elements a call keeps."""
    return torch.from_numpy(draws(n, seed, call_id, step) >= np.uint64(thresh(p)))


def dropout(x: torch.Tensor, p: float, seed: int, call_id: int, step: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """x bf16 (CPU, any shape, numel % 8 == 0) -> (y, mask) bf16 of x's shape."""
    assert x.dtype == torch.bfloat16 and not x.is_cuda
    keep = keep_mask(x.numel(), p, seed, call_id, step).view(x.shape)
    m = scale(p)
    zero = torch.zeros((), dtype=torch.bfloat16)
    y = torch.where(keep, (x.float() * m.float()).to(torch.bfloat16), zero)          # a dropped -0, inf or NaN is +0
    return y, torch.where(keep, m, zero)


def site_masks(n_sites: int, rows: int, d: int, p: float, seed: int, step: int) -> List[torch.Tensor]:
    """The scaled masks (fp32 [rows, d]: 0 or the bf16 scale) of call ids 0 .. n_sites-1 on a [rows, d] activation."""
    s = scale(p).float()
    return [keep_mask(rows * d, p, seed, cid, step).view(rows, d).float() * s for cid in range(n_sites)]


# --------------------------------------------------------------------------- the oracle under given masks
class _IgnoredInBackward(torch.autograd.Function):
    """x * m whose input gradient forgets the mask (what a backward that skipped one site's mask would compute)."""

    @staticmethod
    def forward(ctx, x, m):
        return x * m

    @staticmethod
    def backward(ctx, g):
        return g, None


class _FunctionalWithMasks:
    """Stands in for `torch.nn.functional` inside oracle.ger_oracle: `dropout` hands out the given masks in call order, everything
    else is torch's.  Mutations (all leave the forward VALUES alone unless they say otherwise):
      ignore_dx = {sites}: those sites' masks are skipped on the input-gradient path only;
      a_grad_unmasked = {QKV sites}: lora_A's gradient is contracted with the undropped input (n1 where it needs n1d)."""

    def __init__(self, masks: Sequence[torch.Tensor], ignore_dx=(), a_grad_unmasked=()):
        import torch.nn.functional as real
        self._real, self._masks, self._next = real, list(masks), 0
        self._ignore_dx, self._a_unmasked = set(ignore_dx), set(a_grad_unmasked)
        self._pending = None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def dropout(self, x, p=0.5, training=True, inplace=False):
        assert training and not inplace, "the oracle draws LoRA dropout in training mode only"
        assert self._next < len(self._masks), f"dropout call {self._next}: only {len(self._masks)} masks were given"
        site, m = self._next, self._masks[self._next]
        self._next += 1
        assert tuple(m.shape) == tuple(x.shape), f"site {site}: mask {tuple(m.shape)} for an input {tuple(x.shape)}"
        m = m.to(x.dtype)
        xd = _IgnoredInBackward.apply(x, m) if site in self._ignore_dx else x * m
        if site in self._a_unmasked:
            self._pending = (xd, x)
        return xd

    def linear(self, x, w, bias=None):
        if self._pending is not None and x is self._pending[0]:
            xd, x0 = self._pending
            self._pending = None
            wrong = self._real.linear(x0.detach(), w)          # carries lora_A's gradient, from the undropped input
            return self._real.linear(xd, w.detach(), bias) + (wrong - wrong.detach())
        return self._real.linear(x, w, bias)

    def all_consumed(self) -> bool:
        return self._next == len(self._masks) and self._pending is None


@contextlib.contextmanager
def injected_dropout(masks: Sequence[torch.Tensor], **mutation):
    """Inside the block the oracle's `F.dropout` calls return x * masks[k] for the k-th call (shape checked); on a clean exit all
    masks must have been used.  The oracle module is restored whatever happens."""
    from oracle import ger_oracle as O
    real, fake = O.F, _FunctionalWithMasks(masks, **mutation)
    O.F = fake
    try:
        yield fake
        assert fake.all_consumed(), f"{fake._next} of {len(masks)} masks were consumed"
    finally:
        O.F = real


def oracle_micro_step(cfg, sd: Dict[str, torch.Tensor], ids: torch.Tensor, labels: torch.Tensor, masks: Sequence[torch.Tensor],
                      grad_accum: float, chunk: int = 8, **mutation):
    """oracle.ger_oracle.train_micro_step with the LoRA dropout masks given: masks[k] is [B, T, d] (or [B*T, d], row b*T + t) for
    call k.  -> (loss, {name: gradient})."""
    from oracle import ger_oracle as O
    B, T = ids.shape
    masks = [m.reshape(B, T, -1) for m in masks]
    with injected_dropout(masks, **mutation):
        return O.train_micro_step(cfg, sd, ids, labels, grad_accum=grad_accum, lm_head_chunk_size=chunk)


# --------------------------------------------------------------------------- the model-level settings
# Chosen so that a backward that mishandles ONE site's mask moves some LoRA gradient by many times its gate (measured and asserted
# in test_dropout_reference.py); at the default tiny settings (alpha = 2r, weight_scale 1) such a bug hides inside the 2 % gate.
P_MODEL = 0.5          # scale exactly 2, threshold 2^31
SETTINGS = {
    "tiny_r4": dict(config="parity-tiny", r=4, alpha=32, weight_scale=2.0, B=2, T=64),            # copy-back gradient path
    "hs128_r16": dict(config="parity-hs128", r=16, alpha=128, weight_scale=1.0, B=2, T=37),       # direct-accumulate path
}


def setting(key: str, device="cpu"):
    """-> (cfg, bf16 state dict on `device`) of one of SETTINGS."""
    from dualhyp_amd.config import Config
    from dualhyp_amd.synth import synth_state_dict
    s = SETTINGS[key]
    cfg = Config.from_name(s["config"], r=s["r"], alpha=s["alpha"], dropout=P_MODEL, to_query=True, to_key=True, to_value=True,
                           to_projection=True)
    return cfg, synth_state_dict(cfg, seed=5, weight_scale=s["weight_scale"], device=device)


def batch(cfg, B: int, T: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Random ids [B, T] and labels that carry the second half of every row."""
    ids = torch.randint(3, cfg.padded_vocab_size, (B, T), generator=torch.Generator().manual_seed(seed))
    labels = ids.clone()
    labels[:, : T // 2] = -1
    return ids, labels


def oracle_pair(cfg, sd, ids, labels, masks, grad_accum: float):
    """The oracle in fp32 and in bf16 under the same masks -> (l32, g32, lbf, gbf)."""
    l32, g32 = oracle_micro_step(cfg, {k: v.float() for k, v in sd.items()}, ids, labels, masks, grad_accum)
    lbf, gbf = oracle_micro_step(cfg, {k: v.bfloat16() for k, v in sd.items()}, ids, labels, masks, grad_accum)
    return l32.item(), g32, lbf.item(), gbf


def gates(g32: Dict[str, torch.Tensor], gbf: Dict[str, torch.Tensor]) -> Dict[str, Tuple[float, float]]:
    """Per LoRA tensor (e_oracle_bf16, gate): e = max|g - g_fp32| / max|g_fp32|, gate = max(1.3 * e_oracle_bf16, 0.02) — the gate of
    test_hip_train.test_train_micro_step_matches_reference with the oracle's own two precisions as the yardstick."""
    out = {}
    for k, g in g32.items():
        e = (gbf[k].float() - g.float()).abs().max().item() / g.float().abs().max().item()
        out[k] = (e, max(1.3 * e, 0.02))
    return out


def distances(g: Dict[str, torch.Tensor], g32: Dict[str, torch.Tensor]) -> Dict[str, float]:
    return {k: (g[k].float() - v.float()).abs().max().item() / v.float().abs().max().item() for k, v in g32.items()}
