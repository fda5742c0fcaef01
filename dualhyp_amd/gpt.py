"""Host-side mirror of the reference's LoRA decoder (ger/lora.py GPT + ger/model.py).

Same constructor, parameter names, state-dict keys and `forward()` signature as
`ger.lora.GPT` (ger/lora.py:475-549) so `finetune.ger` / `inference.ger`-style callers work
unchanged — but the modules only HOLD parameters.  All arithmetic runs in libdualhyp_hip.so:
`GPT.forward` hands the packed batch to the native engine (dualhyp_amd/csrc/engine.hip), which
sequences the HIP kernels for every layer.  There is no eager/PyTorch fallback: on CPU tensors
or without the built library, forward raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib, ops
from .config import Config

KVCache = Tuple[torch.Tensor, torch.Tensor]
RoPECache = Tuple[torch.Tensor, torch.Tensor]


def build_rope_cache(seq_len: int, n_elem: int, dtype: torch.dtype = torch.bfloat16, device="cpu",
                     base: int = 10000, condense_ratio: int = 1) -> RoPECache:
    """cos/sin tables [seq_len, n_elem] (ger/model.py:319-346).  Built once on the host with the
    same fp32 formula as the reference and rounded to bf16 whatever the model dtype (quirk Q1),
    then moved to `device`; the kernels only read them."""
    theta = 1.0 / (base ** (torch.arange(0, n_elem, 2) / n_elem))
    ang = torch.outer(torch.arange(seq_len) / condense_ratio, theta).repeat(1, 2)
    cos, sin = torch.cos(ang), torch.sin(ang)
    if dtype == torch.bfloat16:
        cos, sin = cos.bfloat16(), sin.bfloat16()
    elif dtype in (torch.float16, torch.int8):
        cos, sin = cos.half(), sin.half()
    return cos.to(device), sin.to(device)


def map_old_state_dict_weights(state_dict: Dict, mapping: Dict[str, str], prefix: str) -> Dict:
    """Rename pre-LoRA checkpoint keys (ger/utils.py:466-472)."""
    for old, new in mapping.items():
        k = prefix + old
        if k in state_dict:
            state_dict[prefix + new] = state_dict.pop(k)
    return state_dict


# ------------------------------------------------------------------------------------------ modules
class RMSNorm(nn.Module):
    """ger/rmsnorm.py: weight-only RMS norm, computed in the storage dtype by dh_rmsnorm_bf16."""

    def __init__(self, size: int, dim: int = -1, eps: float = 1e-5) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(size))
        self.eps = eps
        self.dim = dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.rmsnorm(x, self.weight, self.eps)

    def reset_parameters(self) -> None:
        nn.init.ones_(self.weight)


class _FrozenLinear(nn.Module):
    """Parameter holder for a bias-free dense layer ('linear.weight' in the state dict)."""

    def __init__(self, in_features: int, out_features: int) -> None:
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))


class AdapterV2Linear(nn.Module):
    """lm_head wrapper: scale * (W x + bias) (ger/lora.py:63-75); scale=1, bias=0, frozen."""

    def __init__(self, in_features: int, out_features: int, **_: Any) -> None:
        super().__init__()
        self.linear = _FrozenLinear(in_features, out_features)
        self.adapter_bias = nn.Parameter(torch.zeros(out_features), requires_grad=False)
        self.adapter_scale = nn.Parameter(torch.ones(out_features), requires_grad=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear(x, self.linear.weight, epilogue=ops.EPI_ADAPTER, scale=self.adapter_scale,
                          bias=self.adapter_bias)

    def reset_parameters(self) -> None:
        nn.init.zeros_(self.adapter_bias)
        nn.init.ones_(self.adapter_scale)


class LoRALayer(nn.Module):
    def __init__(self, r: int, lora_alpha: int, lora_dropout: float) -> None:
        super().__init__()
        assert r >= 0
        self.r, self.lora_alpha, self.lora_dropout_p = r, lora_alpha, float(lora_dropout)
        self.merged = False


def _pad_rank(t: torch.Tensor, r: int, dim: int) -> torch.Tensor:
    """Zero-pad the rank axis to 16 (what the rank-16 MFMA epilogue consumes); exact."""
    if r == 16:
        return t
    shape = list(t.shape)
    shape[dim] = 16
    out = t.new_zeros(shape)
    out.narrow(dim, 0, r).copy_(t)
    return out


class LoRALinear(LoRALayer):
    """y = W x + (alpha/r) B A x (ger/lora.py:103-166); r == 0 is a plain linear."""

    def __init__(self, in_features: int, out_features: int, r: int = 0, lora_alpha: int = 1,
                 lora_dropout: float = 0.0, **_: Any) -> None:
        super().__init__(r, lora_alpha, lora_dropout)
        self.linear = _FrozenLinear(in_features, out_features)
        if r > 0:
            self.lora_A = nn.Parameter(torch.zeros(r, in_features))
            self.lora_B = nn.Parameter(torch.zeros(out_features, r))
            self.scaling = lora_alpha / r
            self.reset_parameters()

    def reset_parameters(self) -> None:
        if hasattr(self, "lora_A"):
            nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
            nn.init.zeros_(self.lora_B)

    @property
    def lora_active(self) -> bool:
        return self.r > 0 and not self.merged and hasattr(self, "lora_A")

    def padded_lora(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(A [16, in], B [out, 16]) contiguous, rank zero-padded."""
        bf = torch.bfloat16   # LoRA parameters may be fp32 masters while fine-tuning; kernels take bf16
        return (_pad_rank(self.lora_A.data.to(bf), self.r, 0).contiguous(),
                _pad_rank(self.lora_B.data.to(bf), self.r, 1).contiguous())

    def merge(self) -> None:
        """W += (B A) * scaling (ger/lora.py:152-157)."""
        if self.r > 0 and not self.merged:
            self.linear.weight.data += (self.lora_B.data @ self.lora_A.data) * self.scaling
            self.merged = True

    def forward(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not self.lora_active:
            return ops.linear(x, self.linear.weight, resid=resid)
        A, B = self.padded_lora()
        xa = ops.linear(x, A)
        return ops.linear(x, self.linear.weight, epilogue=ops.EPI_LORA, xa=xa, lora_b=B,
                          lora_scale=self.scaling, resid=resid)


class LoRAQKVLinear(LoRALinear):
    """Fused q/k/v projection with per-matrix LoRA (ger/lora.py:169-402).  The base weight rows
    are group-interleaved, the LoRA delta is laid out contiguously [Q|K|V] and added as is
    (quirk Q2) — dh_linear_bf16's `splits` reproduce that."""

    def __init__(self, in_features: int, out_features: int, n_head: int, n_query_groups: int, r: int = 0,
                 lora_alpha: int = 1, lora_dropout: float = 0.0,
                 enable_lora: Union[bool, Tuple[bool, bool, bool]] = False, **_: Any) -> None:
        LoRALayer.__init__(self, r, lora_alpha, lora_dropout)
        self.linear = _FrozenLinear(in_features, out_features)
        self.n_head, self.n_query_groups = n_head, n_query_groups
        if isinstance(enable_lora, bool):
            enable_lora = [enable_lora] * 3
        assert len(enable_lora) == 3
        self.enable_lora = list(enable_lora)
        self.kv_embd_size = in_features // (n_head // n_query_groups)
        if r > 0 and any(self.enable_lora):
            shapes = (in_features * self.enable_lora[0], self.kv_embd_size * self.enable_lora[1],
                      self.kv_embd_size * self.enable_lora[2])
            self.qkv_shapes = [s for s in shapes if s]
            self.lora_A = nn.Parameter(torch.zeros(r * sum(self.enable_lora), in_features))
            self.lora_B = nn.Parameter(torch.zeros(sum(self.qkv_shapes), r))
            self.scaling = lora_alpha / r
            self.reset_parameters()

    @property
    def splits(self) -> Tuple[int, int]:
        d = self.linear.in_features
        return d, d + self.kv_embd_size

    def padded_lora(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(A [48, in], B [out, 16]); disabled q/k/v segments are zero rows, which reproduces
        zero_pad (ger/lora.py:272-312) exactly."""
        bf = torch.bfloat16
        if self.r == 16 and all(self.enable_lora):
            return self.lora_A.data.to(bf).contiguous(), self.lora_B.data.to(bf).contiguous()
        d_in, r = self.linear.in_features, self.r
        A = torch.zeros(48, d_in, dtype=bf, device=self.lora_A.device)
        B = torch.zeros(self.linear.out_features, 16, dtype=bf, device=self.lora_B.device)
        seg_rows = (d_in, self.kv_embd_size, self.kv_embd_size)
        a_off = b_off = row0 = 0
        for seg, en in enumerate(self.enable_lora):
            if en:
                A[16 * seg:16 * seg + r] = self.lora_A.data[a_off:a_off + r]
                B[row0:row0 + seg_rows[seg], :r] = self.lora_B.data[b_off:b_off + seg_rows[seg]]
                a_off += r
                b_off += seg_rows[seg]
            row0 += seg_rows[seg]
        return A, B

    def delta_w(self) -> torch.Tensor:
        """Dense (out, in) LoRA update before scaling, contiguous [Q|K|V] rows (ger/lora.py:357-364)."""
        A, B = self.padded_lora()
        d_in = self.linear.in_features
        segs = (d_in, self.kv_embd_size, self.kv_embd_size)
        parts, row0 = [], 0
        for seg, n in enumerate(segs):
            parts.append(B[row0:row0 + n].float() @ A[16 * seg:16 * seg + 16].float())
            row0 += n
        return torch.cat(parts, dim=0)

    def merge(self) -> None:
        if self.r > 0 and any(self.enable_lora) and not self.merged:
            self.linear.weight.data += (self.delta_w() * self.scaling).to(self.linear.weight.dtype)
            self.merged = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not (self.lora_active and any(self.enable_lora)):
            return ops.linear(x, self.linear.weight)
        A, B = self.padded_lora()
        xa = ops.linear(x, A)
        return ops.linear(x, self.linear.weight, epilogue=ops.EPI_LORA, xa=xa, lora_b=B,
                          lora_scale=self.scaling, splits=self.splits)


class CausalSelfAttention(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        shape = (config.n_head + 2 * config.n_query_groups) * config.head_size
        self.attn = LoRAQKVLinear(config.n_embd, shape, n_head=config.n_head, n_query_groups=config.n_query_groups,
                                  r=config.r, lora_alpha=config.alpha, lora_dropout=config.dropout,
                                  enable_lora=(config.to_query, config.to_key, config.to_value))
        self.proj = LoRALinear(config.n_embd, config.n_embd, r=(config.r if config.to_projection else 0),
                               lora_alpha=config.alpha, lora_dropout=config.dropout)
        self.config = config

    def _load_from_state_dict(self, state_dict: Dict, prefix: str, *args: Any, **kwargs: Any) -> None:
        mapping = {"attn.weight": "attn.linear.weight", "proj.weight": "proj.linear.weight"}
        super()._load_from_state_dict(map_old_state_dict_weights(state_dict, mapping, prefix), prefix, *args, **kwargs)


class LLaMAMLP(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        r = config.r if config.to_mlp else 0
        self.fc_1 = LoRALinear(config.n_embd, config.intermediate_size, r=r, lora_alpha=config.alpha)
        self.fc_2 = LoRALinear(config.n_embd, config.intermediate_size, r=r, lora_alpha=config.alpha)
        self.proj = LoRALinear(config.intermediate_size, config.n_embd, r=r, lora_alpha=config.alpha)

    def forward(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """proj(silu(fc_1 x) * fc_2 x) (ger/model.py:312-316) as two launches."""
        act = ops.linear(x, self.fc_1.linear.weight, epilogue=ops.EPI_SWIGLU, w2=self.fc_2.linear.weight)
        return ops.linear(act, self.proj.linear.weight, resid=resid)

    def _load_from_state_dict(self, state_dict: Dict, prefix: str, *args: Any, **kwargs: Any) -> None:
        mapping = {f"{n}.weight": f"{n}.linear.weight" for n in ("fc_1", "fc_2", "proj")}
        super()._load_from_state_dict(map_old_state_dict_weights(state_dict, mapping, prefix), prefix, *args, **kwargs)


class Block(nn.Module):
    def __init__(self, config: Config, block_idx: int = 0) -> None:
        super().__init__()
        self.norm_1 = RMSNorm(config.n_embd, eps=config.norm_eps)
        self.attn = CausalSelfAttention(config)
        self.norm_2 = RMSNorm(config.n_embd, eps=config.norm_eps)
        self.mlp = LLaMAMLP(config)
        self.config = config


# ------------------------------------------------------------------------------------------ engine handle
class _Engine:
    """Owns a dh_engine* and the derived (rank-padded) LoRA tensors it points at."""

    def __init__(self, model: "GPT", max_batch: int, s_max: int, max_tokens: int) -> None:
        cfg = model.config
        lib = _lib.load()
        self.keep: List[torch.Tensor] = []      # tensors whose storage the engine references
        layers = (_lib.LayerWeights * cfg.n_layer)()

        def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
            if t is None:
                return None
            if not t.is_cuda or t.dtype != torch.bfloat16:
                raise _lib.DualHypHipError(
                    "GPT parameters must be bf16 tensors on the GPU for the HIP path "
                    f"(found {t.dtype} on {t.device}); there is no CPU fallback")
            t = t.contiguous()
            self.keep.append(t)
            return t.data_ptr()

        fp8 = bool(getattr(model, "fp8", False))
        mx4 = fp8 and getattr(model, "weight_format", "") == "mxfp4"      # block weights MXFP4, lm_head e4m3 (quantize_model_mxfp4)
        self.kv_cache_dtype = getattr(model, "kv_cache_dtype", "bf16")
        if self.kv_cache_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_cache_dtype is 'bf16' or 'fp8', got {self.kv_cache_dtype!r}")
        if self.kv_cache_dtype == "fp8" and not fp8:
            raise _lib.DualHypHipError("an fp8 KV cache needs an fp8 model: quantize_model_fp8(model, kv_cache='fp8')")
        self.activation_format = getattr(model, "activation_format", "fp8")    # "mxfp6": quantize_model_mxfp4(model, activations="mxfp6")
        if self.activation_format not in ("fp8", "mxfp6"):
            raise ValueError(f"activation_format is 'fp8' or 'mxfp6', got {self.activation_format!r}")
        if self.activation_format == "mxfp6" and not mx4:
            raise _lib.DualHypHipError("MXFP6 activations need an mxfp4 model: quantize_model_mxfp4(model, activations='mxfp6')")

        def wptr(lin) -> Optional[int]:
            """bf16 weight, or the e4m3 bytes of a quantised layer (dualhyp_amd.quant)"""
            if not fp8:
                return ptr(lin.weight.data)
            t = lin.weight_mx4 if hasattr(lin, "weight_mx4") else lin.weight_fp8
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
            self.keep.append(t)
            return t.data_ptr()

        def sptr(lin) -> Optional[int]:
            if not fp8:
                return None
            if hasattr(lin, "weight_mx4"):
                t = lin.weight_mx4_scale       # E8M0 bytes behind the float pointer of dh_layer_weights (dh_engine_create_q)
                assert mx4 and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
                self.keep.append(t)
                return t.data_ptr()
            t = lin.weight_scale
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            self.keep.append(t)
            return t.data_ptr()

        scale = 0.0
        for l, blk in enumerate(model.transformer.h):
            w = layers[l]
            w.norm_1, w.norm_2 = ptr(blk.norm_1.weight.data), ptr(blk.norm_2.weight.data)
            qkv, proj = blk.attn.attn, blk.attn.proj
            w.attn_w, w.proj_w = wptr(qkv.linear), wptr(proj.linear)
            w.attn_ws, w.proj_ws = sptr(qkv.linear), sptr(proj.linear)
            if qkv.lora_active and any(qkv.enable_lora):
                A, B = qkv.padded_lora()
                w.attn_lora_a, w.attn_lora_b = ptr(A), ptr(B)
                scale = qkv.scaling
            if proj.lora_active:
                A, B = proj.padded_lora()
                w.proj_lora_a, w.proj_lora_b = ptr(A), ptr(B)
                scale = proj.scaling
            w.fc_1, w.fc_2 = wptr(blk.mlp.fc_1.linear), wptr(blk.mlp.fc_2.linear)
            w.mlp_proj = wptr(blk.mlp.proj.linear)
            w.fc_1_ws, w.fc_2_ws, w.mlp_proj_ws = sptr(blk.mlp.fc_1.linear), sptr(blk.mlp.fc_2.linear), sptr(blk.mlp.proj.linear)
        cos, sin = model.rope_cache
        desc = _lib.ModelDesc(
            n_layer=cfg.n_layer, n_head=cfg.n_head, n_groups=cfg.n_query_groups, head_size=cfg.head_size,
            n_embd=cfg.n_embd, intermediate=cfg.intermediate_size, vocab=model.lm_head.adapter_scale.size(0),
            block_size=cfg.block_size, norm_eps=cfg.norm_eps, lora_scale=scale,
            wte=ptr(model.transformer.wte.weight.data), wte_rows=model.transformer.wte.weight.size(0),
            ln_f=ptr(model.transformer.ln_f.weight.data), rope_cos=ptr(cos), rope_sin=ptr(sin),
            lm_head=wptr(model.lm_head.linear), adapter_scale=ptr(model.lm_head.adapter_scale.data),
            adapter_bias=ptr(model.lm_head.adapter_bias.data), h_layers=layers, lm_head_ws=sptr(model.lm_head.linear))
        self.max_batch, self.s_max, self.max_tokens = max_batch, s_max, max_tokens
        self.vocab = desc.vocab
        self.kv_dims = (cfg.n_query_groups, cfg.head_size)
        self.device = model.transformer.wte.weight.device
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.dh_engine_create_qa(C.byref(desc), max_batch, s_max, max_tokens, int(self.kv_cache_dtype == "fp8"),
                                               int(mx4), int(self.activation_format == "mxfp6"), C.byref(handle)))
        self.handle = handle
        self.lib = lib
        self.signature = model._param_signature()

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.dh_engine_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def forward(self, ids: torch.Tensor, seq_len: List[int], pos0: List[int], want_all: bool,
                want_last: bool, slot_base: int = 0) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        n = len(seq_len)
        n_tok = int(sum(seq_len))
        ids = ids.reshape(-1)
        assert ids.numel() == n_tok and ids.dtype == torch.int64 and ids.is_cuda
        ids = ids.contiguous()
        la = torch.empty((n_tok, self.vocab), dtype=torch.bfloat16, device=self.device) if want_all else None
        ll = torch.empty((n, self.vocab), dtype=torch.bfloat16, device=self.device) if want_last else None
        a_len = (C.c_int32 * n)(*seq_len)
        a_pos = (C.c_int32 * n)(*pos0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_forward_at(self.handle, ids.data_ptr(), a_len, a_pos, n, int(slot_base),
                                                     ops._p(la), ops._p(ll), torch.cuda.current_stream().cuda_stream))
        return la, ll

    def decode(self, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, n_steps: int, temperature: float,
               top_k: Optional[int], eos_id: Optional[int], seed: int, first_step: int = 0) -> None:
        self._check_logprobs(tokens)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_decode(
                self.handle, tokens.data_ptr(), tokens.size(1), length.data_ptr(), done.data_ptr(), tokens.size(0),
                int(n_steps), float(temperature), 0 if top_k is None else int(top_k),
                -1 if eos_id is None else int(eos_id), int(seed) & ((1 << 64) - 1), int(first_step),
                torch.cuda.current_stream().cuda_stream))

    def forward_slots(self, ids: torch.Tensor, seq_len: List[int], slots: List[int], prompt_phase: bool = False,
                      pos0: int = 0, want_all: bool = False) -> torch.Tensor:
        """Prompt forward of sequence i into KV slot slots[i], its tokens at positions pos0.. (0: whole prompts; P: what follows
        a shared prefix that copy_prefix has put into the slots): the last positions' logits (dh_engine_forward_slots).
        prompt_phase: prefill kernels even when every sequence has one token.
        want_all: the logits of every packed row, [sum(seq_len), vocab], instead of the last positions'."""
        n = len(seq_len)
        ids = ids.reshape(-1)
        assert len(slots) == n and ids.numel() == int(sum(seq_len)) and ids.dtype == torch.int64 and ids.is_cuda
        ids = ids.contiguous()
        ll = torch.empty((ids.numel() if want_all else n, self.vocab), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_forward_slots(self.handle, ids.data_ptr(), (C.c_int32 * n)(*seq_len), (C.c_int32 * n)(*([int(pos0)] * n)),
                                                        (C.c_int32 * n)(*slots), n, int(prompt_phase), ll.data_ptr() if want_all else None,
                                                        None if want_all else ll.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return ll

    def copy_prefix(self, src_slot: int, dst_slots: List[int], n_pos: int) -> None:
        """Cache positions [0, n_pos) of KV slot src_slot, every layer, into each slot of dst_slots (dh_engine_copy_prefix)."""
        n = len(dst_slots)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_copy_prefix(self.handle, int(src_slot), (C.c_int32 * n)(*dst_slots), n, int(n_pos),
                                                      torch.cuda.current_stream().cuda_stream))

    def fork_slots(self, prompt_len: torch.Tensor, n_copies: int, max_len: int) -> None:
        """The prompt cache of slot u * n_copies — the tiles that hold its first prompt_len[u] positions, every layer — into the
        n_copies - 1 slots behind it, for every utterance u, by one launch that reads the lengths on the device
        (dh_engine_fork_slots).  prompt_len: int32 [n_utt] on the GPU; max_len: its maximum as the host knows it."""
        if prompt_len.dtype != torch.int32 or not prompt_len.is_cuda or not prompt_len.is_contiguous() or prompt_len.dim() != 1:
            raise TypeError("fork_slots takes the prompt lengths as a contiguous 1-D int32 tensor on the GPU")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_fork_slots(self.handle, prompt_len.data_ptr(), prompt_len.numel(), int(n_copies), int(max_len),
                                                     torch.cuda.current_stream().cuda_stream))

    def read_kv8(self, what: int, layer: int) -> torch.Tensor:
        """An fp8-KV engine's stored cache of `layer` (test hook, dh_engine_read): 9 / 10 the K / V^T bytes [max_batch, g, s_max * hs]
        uint8, 11 / 12 the K / V exponents [max_batch, g, s_max] int8."""
        assert what in (9, 10, 11, 12)
        G, hs = self.kv_dims
        out = torch.empty((self.max_batch, G, self.s_max * (hs if what <= 10 else 1)), dtype=torch.uint8 if what <= 10 else torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_read(self.handle, what, layer, out.data_ptr(), out.numel(), torch.cuda.current_stream().cuda_stream))
        return out

    def row_arrays(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The (row_seq, row_slot) device arrays of decode_rows: allocated once per engine, so their addresses stay
        what the captured steps were keyed by."""
        if getattr(self, "_rows", None) is None:
            self._rows = (torch.zeros(self.max_batch, dtype=torch.int32, device=self.device),
                          torch.zeros(self.max_batch, dtype=torch.int32, device=self.device))
        return self._rows

    def decode_rows(self, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, limit: torch.Tensor, max_new_tokens: int,
                    n_rows: int, n_steps: int, temperature: float, top_k: Optional[int], eos_id: Optional[int], seed: int) -> None:
        """n_steps decode steps over the first n_rows entries of row_arrays() (dh_engine_decode_rows)."""
        row_seq, row_slot = self.row_arrays()
        assert 0 < n_rows <= self.max_batch and length.numel() == done.numel() == limit.numel() == tokens.size(0)
        self._check_logprobs(tokens)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_decode_rows(
                self.handle, tokens.data_ptr(), tokens.size(1), length.data_ptr(), done.data_ptr(), limit.data_ptr(), tokens.size(0),
                int(max_new_tokens), row_seq.data_ptr(), row_slot.data_ptr(), int(n_rows), int(n_steps), float(temperature),
                0 if top_k is None else int(top_k), -1 if eos_id is None else int(eos_id), int(seed) & ((1 << 64) - 1),
                torch.cuda.current_stream().cuda_stream))

    def reserve_rows(self, rows: int) -> None:
        """Size the single-token-step workspaces for `rows` rows (dh_engine_reserve_rows): a verify step has (D + 1) rows per sequence."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_reserve_rows(self.handle, int(rows)))

    def decode_spec(self, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, limit: torch.Tensor, max_new_tokens: int,
                    n_draft: int, drafts: Optional[torch.Tensor], counters: torch.Tensor, n_steps: int, temperature: float,
                    eos_id: Optional[int], first_step: int = 0) -> None:
        """n_steps verify steps of n_draft drafts per sequence (dh_engine_decode_spec); drafts None: the prompt-lookup proposer."""
        B = tokens.size(0)
        assert length.numel() == done.numel() == limit.numel() == B and counters.numel() >= 3 and counters.dtype == torch.int32
        assert drafts is None or (drafts.dtype == torch.int64 and drafts.is_contiguous() and tuple(drafts.shape) == (B, int(max_new_tokens)))
        self._check_logprobs(tokens)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_decode_spec(
                self.handle, tokens.data_ptr(), tokens.size(1), length.data_ptr(), done.data_ptr(), limit.data_ptr(), B,
                int(max_new_tokens), int(n_draft), None if drafts is None else drafts.data_ptr(), counters.data_ptr(), int(n_steps),
                float(temperature), -1 if eos_id is None else int(eos_id), int(first_step), torch.cuda.current_stream().cuda_stream))

    def decode_spec_draw(self, tokens: torch.Tensor, length: torch.Tensor, done: torch.Tensor, limit: torch.Tensor, max_new_tokens: int,
                         n_draft: int, drafts: Optional[torch.Tensor], counters: torch.Tensor, n_steps: int, temperature: float,
                         top_k: Optional[int], eos_id: Optional[int], seed: int, first_step: int = 0) -> None:
        """decode_spec whose positions draw as decode's steps draw (dh_engine_decode_spec_draw, "Sampled verification" of the header): any
        top_k, the call's seed, and the nucleus, penalties, bias and automaton that are set."""
        B = tokens.size(0)
        assert length.numel() == done.numel() == limit.numel() == B and counters.numel() >= 3 and counters.dtype == torch.int32
        assert drafts is None or (drafts.dtype == torch.int64 and drafts.is_contiguous() and tuple(drafts.shape) == (B, int(max_new_tokens)))
        self._check_logprobs(tokens)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_decode_spec_draw(
                self.handle, tokens.data_ptr(), tokens.size(1), length.data_ptr(), done.data_ptr(), limit.data_ptr(), B,
                int(max_new_tokens), int(n_draft), None if drafts is None else drafts.data_ptr(), counters.data_ptr(), int(n_steps),
                float(temperature), 0 if top_k is None else int(top_k), -1 if eos_id is None else int(eos_id),
                int(seed) & ((1 << 64) - 1), int(first_step), torch.cuda.current_stream().cuda_stream))

    def reserve_beams(self, num_beams: int, max_new_tokens: int) -> None:
        """Size the KV re-parenting scratch and the candidates' workspace of decode_beam (dh_engine_reserve_beams)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_reserve_beams(self.handle, int(num_beams), int(max_new_tokens)))

    def reserve_beam_tiles(self, num_beams: int, max_new_tokens: int) -> None:
        """reserve_beams for decode_beam calls under a tile table (set_beam_tiles): the candidates' workspace and a scratch of one
        tile per (row, layer's K and V^T, group), whatever max_new_tokens is (dh_engine_reserve_beam_tiles)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_reserve_beam_tiles(self.handle, int(num_beams), int(max_new_tokens)))

    def set_beam_tiles(self, table: Optional[torch.Tensor]) -> None:
        """The tile table of later decode_beam calls (dh_engine_set_beam_tiles; include/dualhyp_hip.h, "Beam KV tile table"): the int32
        [2, n_utt, W, NT] planes of a dualhyp_amd.beam.BeamState (tile_table()); None turns it off.  While set, a beam step's attention
        reads every closed tile from the sibling slot that holds it and its re-parenting copies the one open tile; it needs
        set_shared_prompt(W, ...) and reserve_beam_tiles.  Part of a beam step's key.  The caller keeps the planes alive while set."""
        if table is not None and (table.dtype != torch.int32 or not table.is_cuda or not table.is_contiguous() or table.dim() != 4
                                  or table.size(0) != 2):
            raise TypeError("set_beam_tiles takes a contiguous int32 [2, n_utt, W, NT] tensor on the GPU, or None")
        _lib.check(self.lib.dh_engine_set_beam_tiles(self.handle, None if table is None else table.data_ptr(),
                                                     0 if table is None else table.size(3)))
        self._beam_tiles = table

    def decode_beam(self, state, prompt_len: torch.Tensor, n_steps: int, eos_id: Optional[int], first_step: int) -> None:
        """n_steps beam steps of state.n_utt utterances x state.W beams, the first one step number first_step >= 1
        (dh_engine_decode_beam; `state` is a dualhyp_amd.beam.BeamState, prompt_len int32 [n_utt] on the GPU)."""
        assert prompt_len.dtype == torch.int32 and prompt_len.is_cuda and prompt_len.is_contiguous() and prompt_len.numel() == state.n_utt
        mask = getattr(self, "_token_mask", None)
        assert mask is None or mask.size(0) == state.n_utt, "the token mask has one row per utterance"
        hist = getattr(self, "_beam_history", None)
        assert hist is None or tuple(hist.shape) == (2, state.n_utt, state.W, state.max_new), "the history planes are another state's"
        tiles = getattr(self, "_beam_tiles", None)
        assert tiles is None or tuple(tiles.shape[:3]) == (2, state.n_utt, state.W), "the tile table is another state's"
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_decode_beam(
                self.handle, C.byref(state.c_struct()), prompt_len.data_ptr(), state.n_utt, state.W, state.max_new, int(n_steps),
                -1 if eos_id is None else int(eos_id), int(first_step), torch.cuda.current_stream().cuda_stream))

    def set_logprobs(self, buf: Optional[torch.Tensor]) -> None:
        """The float32 buffer, shaped like the decode calls' `tokens`, that later decode / decode_rows / decode_spec calls write each
        appended token's log-probability into (dh_engine_set_logprobs); None turns it off.  The caller keeps it alive while set."""
        if buf is not None and (buf.dtype != torch.float32 or not buf.is_cuda or not buf.is_contiguous() or buf.dim() != 2):
            raise TypeError("set_logprobs takes a contiguous 2-D float32 tensor on the GPU, or None")
        self._logprobs = buf
        _lib.check(self.lib.dh_engine_set_logprobs(self.handle, None if buf is None else buf.data_ptr()))

    def set_top_logprobs(self, ids: Optional[torch.Tensor], lp: Optional[torch.Tensor] = None) -> None:
        """The int32 / float32 buffers, [rows of `tokens`, tok_ld, K] with 1 <= K <= 8, that later decode / decode_rows / decode_spec
        calls write each appended token's K alternatives into (dh_engine_set_top_logprobs; it goes with set_logprobs); None turns
        it off.  The caller keeps them alive while set."""
        if ids is None:
            self._top = None
            _lib.check(self.lib.dh_engine_set_top_logprobs(self.handle, 0, None, None))
            return
        if (lp is None or ids.dtype != torch.int32 or lp.dtype != torch.float32 or not (ids.is_cuda and lp.is_cuda) or ids.dim() != 3
                or tuple(ids.shape) != tuple(lp.shape) or not (ids.is_contiguous() and lp.is_contiguous())):
            raise TypeError("set_top_logprobs takes contiguous 3-D int32 ids and float32 values of one shape on the GPU, or None")
        if not 1 <= ids.size(2) <= ops.MAX_TOP_LOGPROBS:
            raise ValueError(f"set_top_logprobs: K = {ids.size(2)} is outside 1 .. {ops.MAX_TOP_LOGPROBS}")
        self._top = (ids, lp)
        _lib.check(self.lib.dh_engine_set_top_logprobs(self.handle, ids.size(2), ids.data_ptr(), lp.data_ptr()))

    def set_token_mask(self, mask: Optional[torch.Tensor]) -> None:
        """The int32 token mask, [sequences or utterances of the decode calls, ceil(vocab / 32)], under which later decode /
        decode_rows / decode_spec / decode_beam calls pick (dh_engine_set_token_mask; include/dualhyp_hip.h, "Token masks"); None
        turns it off.  The caller keeps it alive while set."""
        if mask is not None and (mask.dtype != torch.int32 or not mask.is_cuda or not mask.is_contiguous() or mask.dim() != 2):
            raise TypeError("set_token_mask takes a contiguous 2-D int32 tensor on the GPU, or None")
        self._token_mask = mask
        _lib.check(self.lib.dh_engine_set_token_mask(self.handle, None if mask is None else mask.data_ptr(),
                                                     0 if mask is None else mask.size(1)))

    def set_no_repeat_ngram(self, ngram: int, start: Optional[torch.Tensor] = None) -> None:
        """no_repeat_ngram = ngram (1..8) for later decode / decode_rows / decode_spec calls, with start, the int32 prompt lengths of
        their sequences (dh_engine_set_no_repeat_ngram; include/dualhyp_hip.h, "No-repeat n-grams"); 0 turns it off.  decode_beam
        refuses to run while it is set.  The caller keeps start alive while set."""
        if ngram and (start is None or start.dtype != torch.int32 or not start.is_cuda or not start.is_contiguous() or start.dim() != 1):
            raise TypeError("set_no_repeat_ngram takes a contiguous 1-D int32 tensor of prompt lengths on the GPU beside ngram > 0")
        _lib.check(self.lib.dh_engine_set_no_repeat_ngram(self.handle, int(ngram), start.data_ptr() if ngram else None))
        self._ngram_start = start if ngram else None

    def set_stop(self, stop, start: Optional[torch.Tensor] = None, beam_fin_tok: Optional[torch.Tensor] = None) -> None:
        """The stop specification (a dualhyp_amd.stop.StopSpec on the engine's device; include/dualhyp_hip.h, "Stop conditions") for
        later decode / decode_rows / decode_spec / decode_beam calls; None turns it off.  start: the int32 prompt lengths of their
        sequences, needed with stop sequences; beam_fin_tok: a beam call's int32 [n_utt, W] ending ids, needed there with a stop set
        (dh_engine_set_stop).  The caller keeps all three alive while set."""
        if stop is not None and not stop:
            stop = None
        for t, name in ((start, "start"), (beam_fin_tok, "beam_fin_tok")):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous()):
                raise TypeError(f"set_stop takes {name} as a contiguous int32 tensor on the GPU")
        if stop is not None and stop.sequences and start is None:
            raise ValueError("stop sequences need start, the int32 prompt lengths: a match never reaches back into the prompt")
        _lib.check(self.lib.dh_engine_set_stop(self.handle, None if stop is None else C.byref(stop.c_struct()),
                                               None if stop is None or start is None else start.data_ptr(),
                                               None if stop is None or beam_fin_tok is None else beam_fin_tok.data_ptr()))
        self._stop = (stop, start, beam_fin_tok) if stop is not None else None

    def set_beam_history(self, history: Optional[torch.Tensor], ngram: int = 0) -> None:
        """Device histories for later decode_beam calls (dh_engine_set_beam_history; include/dualhyp_hip.h, "Beam histories"): the
        int64 [2, n_utt, W, max_new] planes of a dualhyp_amd.beam.BeamState (history_buffer()) and the beam steps' no_repeat_ngram,
        0 .. 8; None turns it off.  While set, decode_beam bans under ngram and takes the stop sequences of set_stop; the planes and
        ngram are part of a beam step's key.  The caller keeps the planes alive while set."""
        if history is not None and (history.dtype != torch.int64 or not history.is_cuda or not history.is_contiguous() or history.dim() != 4
                                    or history.size(0) != 2):
            raise TypeError("set_beam_history takes a contiguous int64 [2, n_utt, W, max_new] tensor on the GPU, or None")
        _lib.check(self.lib.dh_engine_set_beam_history(self.handle, None if history is None else history.data_ptr(), int(ngram)))
        self._beam_history = history

    def set_nucleus(self, top_p: Optional[float] = None, min_p: Optional[float] = None) -> None:
        """top_p and min_p (include/dualhyp_hip.h, "Nucleus and min-p") for later decode / decode_rows calls with top_k != 1; None, 1.0
        and 0.0 turn them off (dh_engine_set_nucleus).  Both are part of a captured step's key."""
        from .nucleus import check_nucleus
        top_p, min_p = check_nucleus(top_p, min_p)
        _lib.check(self.lib.dh_engine_set_nucleus(self.handle, top_p, min_p))

    def set_penalties(self, repetition: Optional[float] = None, frequency: Optional[float] = None, presence: Optional[float] = None,
                      start: Optional[torch.Tensor] = None) -> None:
        """The repetition, frequency and presence penalties (include/dualhyp_hip.h, "Penalties") for later decode / decode_rows calls;
        None, 1.0 and 0.0 turn them off (dh_engine_set_penalties).  start: the int32 [n_seq] prompt lengths on the engine's device, the
        array set_no_repeat_ngram / set_stop take; kept alive here while set.  The values are part of a captured step's key.  While
        set, decode_spec and decode_beam refuse."""
        from .penalty import check_penalties, penalties_on
        r, f, p = check_penalties(repetition, frequency, presence)
        if not penalties_on(r, f, p):
            _lib.check(self.lib.dh_engine_set_penalties(self.handle, None, None))
            self._pen_start = None
            return
        if start is None:
            raise ValueError("penalties need start, the int32 prompt lengths: the history they count begins there")
        if not start.is_cuda or start.dtype != torch.int32 or not start.is_contiguous() or start.dim() != 1:
            raise TypeError("set_penalties takes start as a contiguous 1-D int32 tensor of prompt lengths on the GPU")
        args = _lib.PenaltyArgs(r, f, p)
        _lib.check(self.lib.dh_engine_set_penalties(self.handle, C.byref(args), start.data_ptr()))
        self._pen_start = start

    def set_bias(self, bias=None, start: Optional[torch.Tensor] = None) -> None:
        """The bias (a dualhyp_amd.bias.BiasSpec on the engine's device; include/dualhyp_hip.h, "Contextual biasing") for later decode /
        decode_rows calls; None turns it off (dh_engine_set_bias).  start: the int32 [n_seq] prompt lengths on the engine's device, the
        array set_no_repeat_ngram / set_stop / set_penalties take; it and the spec are kept alive here while set.  The spec's arrays
        are part of a captured step's key.  While set, decode_spec and decode_beam refuse."""
        if bias is None:
            _lib.check(self.lib.dh_engine_set_bias(self.handle, None, None))
            self._bias = None
            return
        if start is None:
            raise ValueError("a bias needs start, the int32 prompt lengths: a match never reaches back into the prompt")
        if not start.is_cuda or start.dtype != torch.int32 or not start.is_contiguous() or start.dim() != 1:
            raise TypeError("set_bias takes start as a contiguous 1-D int32 tensor of prompt lengths on the GPU")
        _lib.check(self.lib.dh_engine_set_bias(self.handle, C.byref(bias.c_struct()), start.data_ptr()))
        self._bias = (bias, start)

    def set_automaton(self, automaton=None, start: Optional[torch.Tensor] = None) -> None:
        """The automaton set (a dualhyp_amd.automaton.AutomatonSet on the engine's device, a start state per sequence of the decode calls;
        include/dualhyp_hip.h, "Automaton constraints") for later decode / decode_rows calls; None turns it off
        (dh_engine_set_automaton).  start: the int32 [n_seq] prompt lengths on the engine's device, the array the other history readers
        take; it and the set, whose state buffer the steps write, are kept alive here while set.  The set's arrays are part of a
        captured step's key.  While set, decode_spec and decode_beam refuse, and a decode call needs an eos_id."""
        if automaton is None:
            _lib.check(self.lib.dh_engine_set_automaton(self.handle, None, None))
            self._automaton = None
            return
        if start is None:
            raise ValueError("an automaton needs start, the int32 prompt lengths: a sequence is in its start state while it has generated nothing")
        if not start.is_cuda or start.dtype != torch.int32 or not start.is_contiguous() or start.dim() != 1:
            raise TypeError("set_automaton takes start as a contiguous 1-D int32 tensor of prompt lengths on the GPU")
        _lib.check(self.lib.dh_engine_set_automaton(self.handle, C.byref(automaton.c_struct()), start.data_ptr()))
        self._automaton = (automaton, start)

    def set_shared_prompt(self, group_rows: int = 0, prompt_len: Optional[torch.Tensor] = None) -> None:
        """Shared-prompt attention (include/dualhyp_hip.h) for later decode / decode_beam calls whose rows u * group_rows + j are the
        candidates or beams of utterance u: prompt_len, the int32 [n_utt] prompt lengths on the engine's device (what fork_slots
        takes), kept alive here while set; 0 / None turns it off (dh_engine_set_shared_prompt).  Part of a captured step's key.
        While set, decode_rows and decode_spec refuse."""
        if not group_rows or prompt_len is None:
            _lib.check(self.lib.dh_engine_set_shared_prompt(self.handle, 0, None))
            self._shared_prompt = None
            return
        if not prompt_len.is_cuda or prompt_len.dtype != torch.int32 or not prompt_len.is_contiguous() or prompt_len.dim() != 1:
            raise TypeError("set_shared_prompt takes the prompt lengths as a contiguous 1-D int32 tensor on the GPU")
        _lib.check(self.lib.dh_engine_set_shared_prompt(self.handle, int(group_rows), prompt_len.data_ptr()))
        self._shared_prompt = (int(group_rows), prompt_len)

    def _check_logprobs(self, tokens: torch.Tensor) -> None:
        buf = getattr(self, "_logprobs", None)
        assert buf is None or tuple(buf.shape) == tuple(tokens.shape), "the logprobs buffer must have the shape of tokens"
        top = getattr(self, "_top", None)
        assert top is None or (buf is not None and tuple(top[0].shape[:2]) == tuple(tokens.shape)), \
            "the top_logprobs buffers go with a logprobs buffer and have the shape of tokens, times K"
        mask = getattr(self, "_token_mask", None)
        assert mask is None or mask.size(0) == tokens.size(0), "the token mask has one row per row of tokens"
        start = getattr(self, "_ngram_start", None)
        assert start is None or start.numel() == tokens.size(0), "no_repeat_ngram's start has one prompt length per row of tokens"
        stop = getattr(self, "_stop", None)
        assert stop is None or stop[1] is None or stop[1].numel() == tokens.size(0), "stop's start has one prompt length per row of tokens"

    def graph_count(self, n_draft: int = -1) -> int:
        """Captured decode steps kept for n_draft drafts (0: the plain steps, -1: all)."""
        return int(self.lib.dh_engine_graph_count(self.handle, int(n_draft)))

    def read_spec(self, n_seq: int, n_draft: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(drafts [n_seq, n_draft], length [n_seq]) of the last verify step: what its proposer drafted and from how many tokens."""
        S = n_draft + 1
        ids = torch.empty((n_seq, S), dtype=torch.int64, device=self.device)
        kv = torch.empty(n_seq, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(self.lib.dh_engine_read(self.handle, 4, 0, ids.data_ptr(), ids.numel() * 8, st))
            _lib.check(self.lib.dh_engine_read(self.handle, 5, 0, kv.data_ptr(), kv.numel() * 4, st))
        return ids[:, 1:].contiguous(), kv

    def read_step_logits(self, n_rows: int) -> torch.Tensor:
        """The bf16 logits rows [n_rows, vocab] of the last single-token step (test hook, dh_engine_read what 8)."""
        out = torch.empty((n_rows, self.vocab), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(self.lib.dh_engine_read(self.handle, 8, 0, out.data_ptr(), out.numel() * 2, st))
        return out

    def set_rsqrt_emulation(self, vec_width: int, whole_call: bool) -> None:
        _lib.check(self.lib.dh_engine_set_cpu_rsqrt_emulation(self.handle, int(vec_width), int(whole_call)))

    def set_timing(self, on: bool) -> None:
        _lib.check(self.lib.dh_engine_set_timing(self.handle, int(on)))

    def get_timing(self, which: int) -> Tuple[float, int]:
        """(milliseconds, launches) of kernel class `which` since set_timing(True); see dh_engine_get_timing."""
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.lib.dh_engine_get_timing(self.handle, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def read(self, what: int, layer: int, shape) -> torch.Tensor:
        """Copy of engine state (dh_engine_read): 0 ln_f(x), 1 K cache, 2 V^T cache, 3 residual x; 6 / 7 the K / V^T cache of an
        fp8-KV engine expanded to bf16."""
        out = torch.empty(shape, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dh_engine_read(self.handle, what, layer, out.data_ptr(), out.numel() * 2,
                                               torch.cuda.current_stream().cuda_stream))
        return out


# ------------------------------------------------------------------------------------------ GPT
class GPT(nn.Module):
    """Drop-in for ger.lora.GPT (ger/lora.py:475-565)."""

    def __init__(self, config: Config) -> None:
        super().__init__()
        assert config.padded_vocab_size is not None
        config.check_supported()
        self.config = config
        self.lm_head = AdapterV2Linear(config.n_embd, config.padded_vocab_size)
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
            h=nn.ModuleList(Block(config, i) for i in range(config.n_layer)),
            ln_f=RMSNorm(config.n_embd, eps=config.norm_eps),
        ))
        self.rope_cache: Optional[RoPECache] = None
        self.max_seq_length = config.block_size
        self.mask_cache: Optional[torch.Tensor] = None   # never built: causality is implicit in the kernels
        self.kv_caches: List[KVCache] = []                # kept for API parity; the engine owns the cache
        # 0 (the product default): RMSNorm rounds rsqrt once, as a GPU run of the reference does.  Tests that
        # compare with the reference's CPU tensors set 32 (AVX-512 hosts; 16 = AVX2): torch's CPU bf16 rsqrt
        # rounds twice in its scalar tail loop and dh_rmsnorm_bf16 can reproduce that per row.
        self.cpu_rsqrt_vec_width = 0
        self.kv_cache_dtype = "bf16"                      # "fp8": quantize_model_fp8(model, kv_cache="fp8")
        self.activation_format = "fp8"                    # "mxfp6": quantize_model_mxfp4(model, activations="mxfp6"); read by quantised models only
        self._engine: Optional[_Engine] = None
        self._capacity = dict(max_batch=1, s_max=0, max_tokens=0)
        self._cache_len: List[int] = []                   # tokens currently valid per cache slot

    # ---- construction helpers --------------------------------------------------------------
    @classmethod
    def from_name(cls, name: str, **kwargs: Any) -> "GPT":
        return cls(Config.from_name(name, **kwargs))

    def _load_from_state_dict(self, state_dict: Dict, prefix: str, *args: Any, **kwargs: Any) -> None:
        mapping = {"lm_head.weight": "lm_head.linear.weight"}
        super()._load_from_state_dict(map_old_state_dict_weights(state_dict, mapping, prefix), prefix, *args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # accept both 'x.linear.weight' (reference key) and our holder's 'x.linear.weight' (identical)
        if getattr(self, "fp8", False):
            raise RuntimeError("load_state_dict: this model was quantised (quantize_model_fp8 / quantize_model_mxfp4): its bf16 weights no longer "
                               "exist; load the checkpoint into a fresh GPT and quantise that")
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._drop_engine()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._drop_engine()
        self.rope_cache = None
        return out

    def build_rope_cache(self, idx: torch.Tensor) -> RoPECache:
        return build_rope_cache(self.config.block_size, self.config.rope_n_elem, torch.bfloat16, idx.device)

    def reset_cache(self) -> None:
        """Forget the cached keys/values (ger/model.py:58-63).  Stale cache contents are never
        attended to (causal bound), so nothing has to be cleared."""
        self.kv_caches.clear()
        self._cache_len = []

    # ---- engine management -----------------------------------------------------------------
    def _param_signature(self) -> Tuple:
        # data_ptr + version: in-place updates of LoRA parameters (optimizer steps) invalidate the
        # engine's rank-padded copies too
        return tuple((p.data_ptr(), p.dtype, str(p.device), p._version) for p in self.parameters())

    def _drop_engine(self) -> None:
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
            self._engine = None
        self._cache_len = []

    def refresh_engine(self) -> None:
        """Call after changing LoRA parameters in place (the engine keeps rank-padded copies)."""
        self._drop_engine()

    def set_capacity(self, max_batch: int, s_max: Optional[int] = None, max_tokens: Optional[int] = None) -> None:
        """Pre-size the KV cache / workspace: `max_batch` sequences of up to `s_max` positions
        (default: max_seq_length, as the reference allocates, ger/lora.py:542) and `max_tokens`
        packed tokens per forward.  Re-sizing drops the cache contents."""
        s_max = self.max_seq_length if s_max is None else s_max
        s_max = -(-min(s_max, self.config.block_size) // 64) * 64
        max_tokens = max_batch * min(s_max, 1024) if max_tokens is None else max_tokens
        cap = dict(max_batch=max_batch, s_max=s_max, max_tokens=max(max_tokens, max_batch))
        if cap != self._capacity:
            self._capacity = cap
            self._drop_engine()

    def engine(self, need_batch: int = 1, need_pos: int = 1, need_tokens: int = 1, exact: bool = False) -> _Engine:
        """The engine, grown (cache contents dropped) when the request does not fit.  By default the cache is
        sized like the reference's (max_seq_length positions, ger/lora.py:542: later calls at higher positions
        must not re-allocate) with room for max_batch x 1024 packed tokens; `exact=True` (generate_batch, which
        knows its whole need up front) allocates what was asked for — 2048 sequences x 640 positions is 30 GB,
        at max_seq_length it would be 94 GB plus 77 GB of workspace."""
        cap = self._capacity
        if cap["s_max"] == 0 or need_batch > cap["max_batch"] or need_pos > cap["s_max"] or need_tokens > cap["max_tokens"]:
            mb = max(cap["max_batch"], need_batch)
            if exact:   # nothing inherited from an earlier, reference-sized allocation
                self.set_capacity(need_batch, need_pos, max(need_tokens, need_batch))
            else:
                s_need = max(cap["s_max"], need_pos, self.max_seq_length)
                self.set_capacity(mb, s_need, max(cap["max_tokens"], need_tokens, mb * min(s_need, 1024)))
        if self._engine is not None and (self._engine.signature != self._param_signature()
                                         or self._engine.kv_cache_dtype != getattr(self, "kv_cache_dtype", "bf16")
                                         or self._engine.activation_format != getattr(self, "activation_format", "fp8")):
            self._drop_engine()
        if self._engine is None:
            w = self.transformer.wte.weight
            if not w.is_cuda:
                raise _lib.DualHypHipError("dualhyp_amd.GPT runs only on the GPU (model.to('cuda')); no CPU fallback")
            if self.rope_cache is None or self.rope_cache[0].device != w.device:
                self.rope_cache = self.build_rope_cache(w)
            self._engine = _Engine(self, **self._capacity)
        return self._engine

    # ---- forward ---------------------------------------------------------------------------
    def forward(self, idx: torch.Tensor, input_pos: Optional[torch.Tensor] = None,
                lm_head_chunk_size: int = 0) -> Union[torch.Tensor, List[torch.Tensor]]:
        """ger/lora.py:504-549.  With `input_pos` (consecutive positions) the batch runs through
        the KV cache; without, every row is a fresh causal sequence."""
        B, T = idx.shape
        block_size = self.config.block_size
        use_kv_cache = input_pos is not None
        if use_kv_cache:
            assert self.max_seq_length >= T, f"Cannot forward sequence of length {T}, max seq length is only {self.max_seq_length}"
        assert self.max_seq_length <= block_size, f"Cannot attend to {self.max_seq_length}, block size is only {block_size}"
        assert block_size >= T, f"Cannot forward sequence of length {T}, block size is only {block_size}"
        if not use_kv_cache and torch.is_grad_enabled():
            # autograd path (LoRA fine-tune, finetune/ger.py:278): only the no-cache forward trains, and only
            # when there is an active LoRA parameter asking for a gradient.  A cached call (input_pos given) is
            # incremental decoding whatever the grad mode — the reference allows it outside no_grad() — and
            # runs through the engine below, which returns logits without a graph.
            from .train import forward_train, lora_parameters
            if not getattr(self, "fp8", False) and any(p.requires_grad for p in lora_parameters(self)):
                return forward_train(self, idx, lm_head_chunk_size)
        if use_kv_cache:
            pos = input_pos.tolist() if input_pos.numel() <= 2 else [int(input_pos[0]), int(input_pos[-1])]
            p0 = pos[0]
            if pos[-1] - p0 + 1 != T or input_pos.numel() != T:
                raise NotImplementedError("input_pos must be T consecutive positions")
            if p0 + T > self.max_seq_length:
                raise NotImplementedError(f"position {p0 + T - 1} exceeds max_seq_length {self.max_seq_length}")
        else:
            p0 = 0
        eng = self.engine(B, p0 + T, B * T)
        if use_kv_cache:
            if p0 > 0 and (len(self._cache_len) < B or any(c != p0 for c in self._cache_len[:B])):
                raise RuntimeError(f"KV cache holds {self._cache_len[:B]} tokens but input_pos starts at {p0}")
        eng.set_rsqrt_emulation(self.cpu_rsqrt_vec_width, whole_call=True)
        la, _ = eng.forward(idx, [T] * B, [p0] * B, want_all=True, want_last=False)
        self._cache_len = [p0 + T] * B if use_kv_cache else []
        logits = la.view(B, T, -1)
        if lm_head_chunk_size > 0:
            return list(logits.split(lm_head_chunk_size, dim=1))
        return logits


def mark_only_lora_as_trainable(model: nn.Module, bias: str = "none") -> None:
    """ger/lora.py:405-439."""
    for n, p in model.named_parameters():
        if "lora_" not in n:
            p.requires_grad = False
    if bias == "none":
        return
    if bias == "all":
        for n, p in model.named_parameters():
            if "bias" in n:
                p.requires_grad = True
    elif bias == "lora_only":
        for m in model.modules():
            if isinstance(m, LoRALayer) and getattr(m, "bias", None) is not None:
                m.bias.requires_grad = True
    else:
        raise NotImplementedError


def lora_filter(key: str, value: Any) -> bool:
    return "lora_" in key


def merge_lora_weights(model: GPT) -> None:
    """Fold every LoRA update into its base weight (ger/lora.py:707-711)."""
    for m in model.modules():
        if isinstance(m, LoRALinear):
            m.merge()
    model.refresh_engine()
