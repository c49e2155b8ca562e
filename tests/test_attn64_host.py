"""mi_attn_prefill with 64-wide heads, before any launch (no GPU, fake pointers): the one form csrc/attn_prefill64.hip has is the
cache-less non-causal one with n_heads == n_kv_heads; every other head_dim 64 call, and every other width, is MI_ERR_SHAPE by name."""
import pytest


# (cache_k, cache_v, n_heads, n_kv_heads, head_dim, causal) -> words of the message
@pytest.mark.parametrize("ck, cv, H, Hkv, dh, causal, words", [
    (None, None, 4, 4, 64, 1, (b"head_dim 64", b"non-causal")),
    (1, 1, 4, 4, 64, 0, (b"head_dim 64", b"cache-less")),
    (None, None, 4, 2, 64, 0, (b"head_dim 64", b"n_kv_heads must equal n_heads")),
    (None, None, 4, 4, 96, 0, (b"head_dim must be 128, or 64",)),
], ids=["causal", "ring", "gqa", "width96"])
def test_attn_prefill_refuses_by_name(ck, cv, H, Hkv, dh, causal, words):
    from mistral_inference import _hip
    L = _hip.lib()
    assert L.mi_attn_prefill(1, 1, 3 * H * dh, ck, cv, 16, 1, 4, H, Hkv, dh, 1, 1, causal, 0.0, 0, None) == _hip.MI_ERR_SHAPE
    detail = L.mi_last_error_detail()
    assert b"mi_attn_prefill" in detail and all(w in detail for w in words), detail
