"""Layer modules of the hot path (reference transformer_layers.py:16-169) as thin hosts over the HIP
operators.  Parameter names and shapes are the reference's (checkpoint keys load unchanged); every
`forward` dispatches to libmistral_hip -- there is no torch compute path here.

These module-level forwards exist for callers that drive a block themselves; `Transformer.forward_partial`
bypasses them and hands the whole local layer stack to the native runner (`mi_forward`)."""
from typing import Optional

import torch
from torch import nn

from . import _hip
from .args import LoraArgs, MoeArgs, QuantizationArgs
from .cache import CacheView
from .lora import LoRALinear, maybe_lora
from .moe import MoeLayer
from .quant import QuantLinear, linear_quant, quantized_linear_cls, refusal

LORA_MOE_REFUSAL = ("un-merged LoRA on a MoE model (adapters inside the experts) is not implemented; merge the adapter into the "
                    "checkpoint first (what the reference's default CLI path does, lora.py:118-139)")


def _no_lora(lora: Optional[LoraArgs], moe: Optional[MoeArgs]) -> None:
    """The one refused combination at construction time (fp16 / fp32 storage is refused where the dtype is known: the first
    forward, `_hip.lora_linear` / `HipStackBackend`)."""
    if lora is not None and moe is not None:
        raise NotImplementedError(LORA_MOE_REFUSAL)


def _linear_cls(lora: Optional[LoraArgs], quantization: Optional[QuantizationArgs]):
    """nn.Linear, LoRALinear (un-merged adapters), or Fp8Linear / Mxfp4Linear (weight-only FP8 / MXFP4, by format); adapters and
    quantisation do not combine."""
    if quantization is not None:
        if lora is not None:
            raise NotImplementedError(refusal("lora", quantization))
        return quantized_linear_cls(quantization)
    return maybe_lora(lora)


def _adapters(*mods):
    """(lora_A weights, lora_B weights) of LoRALinear modules, for `_hip.lora_linear`."""
    return tuple(m.lora_A.weight for m in mods), tuple(m.lora_B.weight for m in mods)


class RMSNorm(nn.Module):
    """bf16( bf16(x_f32 * rsqrt(mean(x_f32^2) + eps)) * weight )  (reference transformer_layers.py:109-120)."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _hip.rmsnorm(x, self.weight, self.eps)


class FeedForward(nn.Module):
    """w2( silu(w1 x) * w3 x ) with bf16 rounding after every step (reference transformer_layers.py:96-106):
    gate/up projections + SiLU*mul are one kernel, the down projection another."""

    def __init__(self, dim: int, hidden_dim: int, lora: Optional[LoraArgs] = None,
                 quantization: Optional[QuantizationArgs] = None):
        super().__init__()
        linear = _linear_cls(lora, quantization)
        self.w1 = linear(dim, hidden_dim, bias=False)
        self.w2 = linear(hidden_dim, dim, bias=False)
        self.w3 = linear(dim, hidden_dim, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if isinstance(self.w1, LoRALinear):  # gate | up with their two adapters in one lora_up launch, then down
            a, b = _adapters(self.w1, self.w3)
            hid = _hip.lora_linear(x, (self.w1.weight, self.w3.weight), a, b, self.w1.scaling, _hip.EPI_SWIGLU)
            return self.w2(hid)
        if isinstance(self.w1, QuantLinear):  # the same two launches on quantised weights (csrc/gemv_w8.hip, gemv_w4.hip)
            return self.w2(linear_quant(x, (self.w1, self.w3), _hip.EPI_SWIGLU))
        hid = _hip.linear(x, (self.w1.weight, self.w3.weight), _hip.EPI_SWIGLU)
        return _hip.linear(hid, (self.w2.weight,), _hip.EPI_STORE)


class Attention(nn.Module):
    """Reference transformer_layers.py:30-93.  q|k|v are ONE projection launch over the three weight
    matrices, GQA is resolved inside the attention kernels (no repeat_kv), and the three xformers masks
    are the kernels' position test."""

    def __init__(self, dim: int, n_heads: int, head_dim: int, n_kv_heads: int, lora: Optional[LoraArgs] = None,
                 quantization: Optional[QuantizationArgs] = None):
        super().__init__()
        self.n_heads, self.head_dim, self.n_kv_heads = n_heads, head_dim, n_kv_heads
        self.repeats = n_heads // n_kv_heads
        self.scale = head_dim ** -0.5
        linear = _linear_cls(lora, quantization)
        self.wq = linear(dim, n_heads * head_dim, bias=False)
        self.wk = linear(dim, n_kv_heads * head_dim, bias=False)
        self.wv = linear(dim, n_kv_heads * head_dim, bias=False)
        self.wo = linear(n_heads * head_dim, dim, bias=False)

    def forward(self, x: torch.Tensor, freqs_cis: torch.Tensor, cache: Optional[CacheView] = None,
                mask=None) -> torch.Tensor:
        assert mask is None or cache is None
        T = x.shape[0]
        H, Hkv, Dh = self.n_heads, self.n_kv_heads, self.head_dim
        nq, nkv = H * Dh, Hkv * Dh
        cs = torch.view_as_real(freqs_cis).contiguous()  # rows already gathered by position (transformer.py:199)
        rows = torch.arange(T, dtype=torch.int32, device=x.device)
        lora = isinstance(self.wq, LoRALinear)
        quant = isinstance(self.wq, QuantLinear)
        if quant and T <= _hip.GEMV_MAX_T:  # the plain model's launches on quantised weights (csrc/gemv_w8.hip, gemv_w4.hip)
            qkv = _hip.qkv_rope_kvwrite_quant(self.wq.hip, x, self.wq.weight, self.wk.weight, self.wv.weight, self.wq.qscale_weight,
                                              self.wk.qscale_weight, self.wv.qscale_weight, Dh, cs, rows)
        elif quant:
            qkv = linear_quant(x, (self.wq, self.wk, self.wv), _hip.EPI_STORE)
            _hip.rope_inplace(qkv, H, Hkv, Dh, cs, rows)
        elif lora:  # q | k | v with their three adapters: base product, lora_down, lora_up; RoPE as its own pass
            a, b = _adapters(self.wq, self.wk, self.wv)
            qkv = _hip.lora_linear(x, (self.wq.weight, self.wk.weight, self.wv.weight), a, b, self.wq.scaling, _hip.EPI_STORE)
            _hip.rope_inplace(qkv, H, Hkv, Dh, cs, rows)
        elif T <= _hip.GEMV_MAX_T:  # decode-sized: projection + RoPE in the one weight-streaming launch
            qkv = _hip.qkv_rope_kvwrite(x, self.wq.weight, self.wk.weight, self.wv.weight, Dh, cs, rows)
        else:
            qkv = _hip.linear(x, (self.wq.weight, self.wk.weight, self.wv.weight), _hip.EPI_STORE)
            _hip.rope_inplace(qkv, H, Hkv, Dh, cs, rows)
        if cache is None:
            # reference quirk: the block never forwards `mask` (transformer_layers.py:165) -> unmasked
            out = _hip.attn_prefill(qkv, H, Hkv, Dh, None, None, T, None, None, 1, T, causal=False)
        else:
            b = cache.metadata.batch
            assert b is not None
            if cache.prefill:
                out = _hip.attn_prefill(qkv, H, Hkv, Dh, cache.cache_k, cache.cache_v, cache.max_seq_len, b.q_start,
                                        b.kv_before, len(b.seqlens), b.max_q_len, causal=True)
                cache.update(qkv[:, nq:nq + nkv], qkv[:, nq + nkv:])
            else:
                cache.update(qkv[:, nq:nq + nkv], qkv[:, nq + nkv:])
                out = _hip.attn_decode(qkv, cache.cache_k, cache.cache_v, H, b.tok_pos)
        if lora or quant:
            return self.wo(out)
        return _hip.linear(out, (self.wo.weight,), _hip.EPI_STORE)


class TransformerBlock(nn.Module):
    """Pre-norm residual block (reference transformer_layers.py:123-169)."""

    def __init__(self, dim: int, hidden_dim: int, n_heads: int, n_kv_heads: int, head_dim: int, norm_eps: float,
                 lora: Optional[LoraArgs] = None, moe: Optional[MoeArgs] = None,
                 quantization: Optional[QuantizationArgs] = None):
        super().__init__()
        _no_lora(lora, moe)
        if quantization is not None and moe is not None:
            raise NotImplementedError(refusal("moe", quantization))
        self.n_heads = n_heads
        self.dim = dim
        self.attention = Attention(dim=dim, n_heads=n_heads, head_dim=head_dim, n_kv_heads=n_kv_heads, lora=lora,
                                   quantization=quantization)
        self.attention_norm = RMSNorm(dim, eps=norm_eps)
        self.ffn_norm = RMSNorm(dim, eps=norm_eps)
        self.feed_forward: nn.Module
        if moe is not None:
            self.feed_forward = MoeLayer(
                experts=[FeedForward(dim=dim, hidden_dim=hidden_dim, lora=lora) for _ in range(moe.num_experts)],
                gate=nn.Linear(dim, moe.num_experts, bias=False), moe_args=moe)
        else:
            self.feed_forward = FeedForward(dim=dim, hidden_dim=hidden_dim, lora=lora, quantization=quantization)

    def forward(self, x: torch.Tensor, freqs_cis: torch.Tensor, cache: Optional[CacheView] = None,
                mask=None) -> torch.Tensor:
        r = self.attention.forward(self.attention_norm(x), freqs_cis, cache)
        h = x + r
        r = self.feed_forward.forward(self.ffn_norm(h))
        return h + r
