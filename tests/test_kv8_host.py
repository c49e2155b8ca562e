"""FP8 (e4m3) K/V rings, host side (no GPU): the written rule, `BufferCache` with dtype=float8_e4m3fn on the CPU, and what the
library decides before any launch (sizes, layout codes, refusals)."""
import ctypes as C
import types

import pytest
import torch

from kv8_util import BF, F8, all_finite_bf16
from test_abi import _tiny_model, _valid_decode_batch


def _cache_mod():
    from mistral_inference import cache
    return cache


# ------------------------------------------------------------------------------------------------ the rule
def test_rule_over_every_finite_bf16_pattern():
    c = _cache_mod()
    x = all_finite_bf16()
    assert x.numel() == 65280
    q = c.kv_quantize(x)
    b = q.view(torch.uint8)
    assert q.dtype == F8 and not bool(((b == 0x7F) | (b == 0xFF)).any())          # no NaN code from a finite input
    d32, d16 = c.kv_dequantize(q, torch.float32), c.kv_dequantize(q, BF)
    assert d16.dtype == BF and torch.equal(d16.float(), d32)                       # every dequantised value is exact in bf16
    assert torch.equal(c.kv_quantize(d16).view(torch.uint8), b)                    # idempotent
    assert float(d32.abs().max()) == 448.0
    # round to nearest: no e4m3 value lies closer to x than the one chosen (checked against the whole code table)
    table = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).float()
    table = table[torch.isfinite(table)]
    xc = x.float().clamp(-448, 448)
    best = (xc[:, None] - table[None, :]).abs().amin(1)
    assert torch.equal((xc - d32).abs(), best)


def test_rule_saturates_infinities_and_keeps_nan():
    c = _cache_mod()
    x = torch.tensor([float("inf"), float("-inf"), 1e30, -1e30, 448.0, 464.0, 480.0], dtype=BF)
    assert c.kv_dequantize(c.kv_quantize(x), torch.float32).tolist() == [448.0, -448.0, 448.0, -448.0, 448.0, 448.0, 448.0]
    assert bool(torch.isnan(x.to(F8).float())[[0, 1, 2, 3, 6]].all())              # torch's bare cast makes NaN of them
    assert bool(torch.isnan(c.kv_dequantize(c.kv_quantize(torch.tensor([float("nan")], dtype=BF)), torch.float32)).all())


# ------------------------------------------------------------------------------------------------ BufferCache on the CPU
@pytest.mark.parametrize("layout", ["0", "1"])
def test_buffer_cache_with_e4m3_rings(layout, monkeypatch):
    from mistral_inference import _hip
    c = _cache_mod()
    monkeypatch.setenv("MI_KV_LAYOUT", layout)
    cache = c.BufferCache(2, 3, 64, 2, 128, sliding_window=16, dtype=F8)
    ref = c.BufferCache(2, 3, 64, 2, 128, sliding_window=16, dtype=BF)
    for l in range(2):
        k = cache.cache_k[l]
        assert k.dtype == F8 and k.shape == ref.cache_k[l].shape == (3, 16, 2, 128) and k.stride() == ref.cache_k[l].stride()
        assert _hip.kv_layout_of(k) == int(layout) and _hip.kv_layout_code(k) == (int(layout) | _hip.KV_E4M3)
        assert not bool(k.view(torch.uint8).any()) and not bool(cache.cache_v[l].view(torch.uint8).any())   # zero-filled
    assert cache.kv_layout == (int(layout) | 0x10) and ref.kv_layout == int(layout)
    # .to() both ways goes by the rule, and keeps the layout
    vals = (torch.randn(3, 16, 2, 128, generator=torch.Generator().manual_seed(1)) * 300).to(BF)   # some beyond +-448
    assert float(vals.float().abs().max()) > 448
    for l in range(2):
        ref.cache_k[l].copy_(vals)
        ref.cache_v[l].copy_(-vals)
    ref.to("cpu", F8)
    assert ref.kv_layout == (int(layout) | 0x10)
    assert torch.equal(ref.cache_k[0].view(torch.uint8), c.kv_quantize(vals).view(torch.uint8))
    assert not bool(torch.isnan(ref.cache_k[0].float()).any())
    ref.to("cpu", BF)
    assert ref.kv_layout == int(layout) and ref.cache_k[1].dtype == BF
    assert torch.equal(ref.cache_v[1], c.kv_dequantize(c.kv_quantize(-vals), BF))


def test_cache_view_on_e4m3_rings():
    c = _cache_mod()
    cache = c.BufferCache(1, 2, 64, 2, 128, sliding_window=8, dtype=F8)
    vals = (torch.randn(2, 8, 2, 128, generator=torch.Generator().manual_seed(2)) * 4).to(BF)
    cache.cache_k[0].view(torch.uint8).copy_(c.kv_quantize(vals).view(torch.uint8))
    cache.cache_v[0].view(torch.uint8).copy_(c.kv_quantize(-vals).view(torch.uint8))
    cache.init_kvseqlens(2)
    cache.update_seqlens([11, 3])            # sequence 0 has wrapped, sequence 1 has not
    view = cache.get_view(0, cache.get_input_metadata([2, 1])[0])
    assert view.key.dtype == F8 and view.value.dtype == F8 and view.key.shape == (2, 8, 2, 128)       # the raw rings
    xk = torch.ones(3, 2, 128, dtype=BF)
    ik, iv = view.interleave_kv(xk, 2 * xk)
    assert ik.dtype == BF and iv.dtype == BF and ik.shape == (8 + 2 + 3 + 1, 2, 128)
    deq = c.kv_dequantize(c.kv_quantize(vals), BF)
    old0 = torch.stack([deq[0, p % 8] for p in range(3, 11)])
    assert torch.equal(ik[:8], old0) and torch.equal(ik[8:10], xk[:2]) and torch.equal(ik[10:13], deq[1, :3])
    assert torch.equal(iv[:8], -old0)


# ------------------------------------------------------------------------------------------------ the library, before any launch
def test_new_symbols_are_exported_and_the_abi_version_stays():
    from mistral_inference import _hip
    L = _hip.lib()
    assert L.mi_abi_version() == 9
    for name in ("mi_kv_dequant", "mi_workspace_bytes_kv"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(L, name)
    assert _hip.KV_E4M3 == 0x10


@pytest.mark.parametrize("model_kw", [dict(dim=512, hidden_dim=1024, vocab=512), dict(dim=512, hidden_dim=1024, vocab=512, E=8, k=2)])
def test_workspace_bytes_kv(model_kw):
    from mistral_inference import _hip
    L = _hip.lib()
    m = _tiny_model(**model_kw)
    w8, w4 = _hip.MiW8Model(), _hip.MiW4Model()
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for T, B, W in ((1, 1, 64), (8, 2, 1), (8, 8, 64), (9, 9, 4096), (300, 3, 4096), (5, 1, 17)):
        plain = L.mi_workspace_bytes(C.byref(m), T, B, W)
        assert plain > 4096
        quant = {0: plain, 1: L.mi_workspace_bytes_w8(C.byref(m), C.byref(w8), T, B, W)}
        assert quant[1] == L.mi_workspace_bytes_w4(C.byref(m), C.byref(w4), T, B, W)
        scratch = align(2 * B * m.n_kv_heads * W * m.head_dim * 2)          # K and V rings of B sequences, bf16
        for qz in (0, 1):
            for lay in (0, 1):
                assert L.mi_workspace_bytes_kv(C.byref(m), qz, T, B, W, lay) == quant[qz], (T, B, W, qz, lay)
                assert L.mi_workspace_bytes_kv(C.byref(m), qz, T, B, W, lay | 0x10) == quant[qz] + scratch, (T, B, W, qz, lay)
    assert L.mi_workspace_bytes_kv(C.byref(m), 0, 1, 1, 64, 2) == 0 and L.mi_workspace_bytes_kv(None, 0, 1, 1, 64, 0) == 0


def test_layout_codes_of_the_forward_entries():
    """0x10 / 0x11 pass mi_forward's layout check - the call then fails on the workspace, which must hold the dequantisation
    scratch - while 2 and 7 (and the flag on top of them) still fail on kv_layout; mi_forward_generic refuses the flag by name."""
    from mistral_inference import _hip
    L = _hip.lib()
    m = _tiny_model()
    for lay in (0x10, 0x11):
        bt = _valid_decode_batch(workspace_bytes=64)
        bt.kv_layout = lay
        assert L.mi_forward(C.byref(m), C.byref(bt), None) == -3 and b"workspace 64 < required" in L.mi_last_error_detail()
        need = L.mi_workspace_bytes_kv(C.byref(m), 0, 1, 1, 16, lay)
        bt.workspace_bytes = need - 1                      # what a bf16 cache needs is not enough
        assert need > L.mi_workspace_bytes(C.byref(m), 1, 1, 16)
        assert L.mi_forward(C.byref(m), C.byref(bt), None) == -3 and f"required {need}".encode() in L.mi_last_error_detail()
        bt.workspace_bytes = 1 << 30
        assert L.mi_forward_generic(C.byref(m), C.byref(bt), 1, None) == -4
        detail = L.mi_last_error_detail()
        assert b"mi_forward_generic" in detail and b"MI_KV_E4M3" in detail and b"e4m3" in detail
    for lay in (2, 7, 0x12, 0x20, 0x31):
        bt = _valid_decode_batch()
        bt.kv_layout = lay
        assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1 and b"mi_forward: kv_layout" in L.mi_last_error_detail()
        assert L.mi_forward_generic(C.byref(m), C.byref(bt), 1, None) == -1 and b"kv_layout" in L.mi_last_error_detail()


def test_leaves_decide_on_the_flag_before_any_launch():
    from mistral_inference import _hip
    L = _hip.lib()
    assert L.mi_attn_prefill(1, 1, 768, 1, 1, 16, 1, 4, 4, 2, 128, 1, 1, 1, 0.0, 0x11, None) == -4
    assert b"mi_kv_dequant" in L.mi_last_error_detail() and b"MI_KV_E4M3" in L.mi_last_error_detail()
    assert L.mi_attn_prefill(1, 1, 768, 1, 1, 16, 1, 4, 4, 2, 128, 1, 1, 1, 0.0, 2, None) == -1
    assert L.mi_kv_dequant(1, 1, 1, 1, 16, 1, 2, 128, 2, None) == -1
    assert L.mi_kv_dequant(1, 1, None, 1, 16, 1, 2, 128, 0x11, None) == -1
    assert L.mi_kv_dequant(1, 1, 1, 1, 3, 1, 1, 8, 0x10, None) == -2 and b"multiple of 16" in L.mi_last_error_detail()
    assert L.mi_attn_decode(1, 1, 128, 1, 1, 16, 1, 4, 2, 128, 1, 1, 0x12, None) == -1


def test_unknown_kv_dtype_is_refused_by_name():
    from mistral_inference.generate import generate
    from mistral_inference.main import demo, interactive
    model = types.SimpleNamespace(dtype=BF)        # refused before the model is touched
    with pytest.raises(NotImplementedError, match=r"kv_dtype=torch\.float16.*torch\.bfloat16.*torch\.float8_e4m3fn"):
        generate([[1, 2, 3]], model, max_tokens=1, temperature=0.0, kv_dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="float8_e5m2"):
        generate([[1, 2, 3]], model, max_tokens=1, temperature=0.0, kv_dtype=torch.float8_e5m2)
    with pytest.raises(TypeError):                 # keyword-only
        generate([[1, 2, 3]], model, [], 1, 0.0, None, None, None, F8)
    for tool in (interactive, demo):
        with pytest.raises(NotImplementedError, match=r"kv_dtype='fp8'.*'bf16', 'fp8_e4m3'"):
            tool("/nonexistent", kv_dtype="fp8")   # before anything is loaded
    from mistral_inference.cache import kv_dtype_arg
    assert kv_dtype_arg(None) is None and kv_dtype_arg("fp8_e4m3") == F8 and kv_dtype_arg("bf16") == BF
