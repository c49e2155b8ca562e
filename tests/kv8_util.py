"""Shared by tests/test_kv8_host.py and tests/test_gpu_kv8.py (FP8 K/V rings, include/mistral_hip.h MI_KV_E4M3): the bf16 patterns
of the exhaustive rule test, rings of e4m3 bytes in either layout, and the oracle's attention block restated on an e4m3 ring."""
from typing import List, Optional

import torch
import torch.nn.functional as F

import mistral_oracle as mo

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def all_finite_bf16() -> torch.Tensor:
    """Every finite bf16 bit pattern once, in ascending order of the pattern (65 280 values; +-0 are two of them)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    return bits[torch.isfinite(bits)]


def e4m3_ring(host_bf16: torch.Tensor, head_major: bool, device="cuda") -> torch.Tensor:
    """Host ring [B, W, Hkv, Dh] of bf16 values -> device ring of e4m3 bytes (quantised by the rule on the host) in the
    requested layout.  The bytes travel as uint8: no float8 kernel of torch's is part of what is tested."""
    from mistral_inference.cache import kv_quantize
    q = kv_quantize(host_bf16).view(torch.uint8)
    if head_major:
        return q.permute(0, 2, 1, 3).contiguous().to(device).permute(0, 2, 1, 3).view(F8)
    return q.contiguous().to(device).view(F8)


def host_values(ring8: torch.Tensor) -> torch.Tensor:
    """bf16 host tensor [B, W, Hkv, Dh] of the values an e4m3 ring (any device, either layout) holds: the read rule on the host."""
    from mistral_inference.cache import kv_dequantize
    return kv_dequantize(ring8.view(torch.uint8).cpu().contiguous().view(F8), BF)


def attention_block_kv8(x: torch.Tensor, wq, wk, wv, wo, cs: torch.Tensor, args: mo.OracleArgs, seqlens: List[int],
                        cache: Optional[mo.OracleCache], layer: int) -> torch.Tensor:
    """mistral_oracle.attention_block on a cache whose rings hold e4m3 bytes (OracleCache(dtype=torch.float8_e4m3fn)).

    Rounding points, the reference's own (transformer_layers.py:72-81): the ring write rounds by the rule; at decode (every
    sequence adds one token to a cache that has seen some) the step's own row goes through the ring - written, then read - so it
    is rounded before the attention; at prefill the chunk's own rows are the activations, unrounded; old keys are the ring's
    dequantised bytes."""
    from mistral_inference.cache import kv_dequantize, kv_quantize
    T = x.shape[0]
    H, Hkv, Dh = args.n_heads, args.n_kv_heads, args.head_dim
    q = mo.apply_rope(F.linear(x, wq).view(T, H, Dh), cs)
    k = mo.apply_rope(F.linear(x, wk).view(T, Hkv, Dh), cs)
    v = F.linear(x, wv).view(T, Hkv, Dh)
    if cache is None:
        return mo.attention_block(x, wq, wk, wv, wo, cs, args, seqlens, None, layer)
    assert cache.k[layer].dtype == F8
    decode = cache.seen[0] > 0 and all(s == 1 for s in seqlens)   # cache.py:236-254
    W = cache.sizes[layer]
    ring_k, ring_v = cache.k[layer].view(torch.uint8), cache.v[layer].view(torch.uint8)
    deq = lambda b8: kv_dequantize(b8.view(F8), x.dtype)  # noqa: E731
    outs = []
    start = 0
    for b, s in enumerate(seqlens):
        p = cache.seen[b]
        qb, kb, vb = q[start:start + s], k[start:start + s], v[start:start + s]
        k8, v8 = kv_quantize(kb).view(torch.uint8), kv_quantize(vb).view(torch.uint8)
        if decode:
            kb, vb = deq(k8), deq(v8)
        n_old = min(p, W)
        old_pos = torch.arange(p - n_old, p)
        keys = torch.cat([deq(ring_k[b, old_pos % W]), kb]) if n_old else kb
        vals = torch.cat([deq(ring_v[b, old_pos % W]), vb]) if n_old else vb
        kpos = torch.cat([old_pos, torch.arange(p, p + s)])
        qpos = torch.arange(p, p + s)
        outs.append(mo._attend(qb, keys, vals, qpos, kpos, W, causal=True))
        keep = torch.arange(s) >= s - W
        slots = (qpos % W)[keep]
        ring_k[b, slots] = k8[keep]
        ring_v[b, slots] = v8[keep]
        start += s
    return F.linear(torch.cat(outs), wo)
