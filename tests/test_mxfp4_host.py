"""Weight-only MXFP4 (OCP e2m1 codes, e8m0 block scales) on the host: the quantiser, packing, the checkpoint writer, params.json
parsing and refusals, a meta-built quantised model, the argument checks of the new C entry points, and the teeth of the exact
GPU test family - nothing here needs a device."""
import ctypes as C
import json
import os

import pytest
import torch
import safetensors
from safetensors.torch import save_file

import mistral_oracle as mo
from hip_util import write_checkpoint
from mistral_inference import _hip
from mistral_inference.args import QFORMAT_MXFP4, QuantizationArgs, TransformerArgs
from mistral_inference.quant import (QSCALE_KEY, Fp8Linear, Mxfp4Linear, check_quantize_arg, dequantize_mxfp4, quantize_blocks,
                                     quantize_checkpoint)
from mistral_inference.transformer import Transformer
from mxfp4_cases import EXACT_SHAPES, exact_case, exact_reference

ARGS = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                     sliding_window=16)
LINEARS = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2", "feed_forward.w3")
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _codes(packed):
    """[out, in / 2] bytes -> [out, in] codes, the low nibble at the even k"""
    return torch.stack((packed & 15, packed >> 4), dim=2).reshape(packed.shape[0], -1)


@pytest.mark.parametrize("K", [32, 512, 4096])
def test_quantiser_properties_on_gaussian_rows(K):
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(24, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    w[3, :32] = 0.0                                           # an all-zero block
    packed, scale = quantize_blocks(w)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (24, K // 2)
    assert scale.dtype == torch.uint8 and tuple(scale.shape) == (24, K // 32)
    amax = w.float().reshape(24, K // 32, 32).abs().amax(dim=2)
    sc = torch.ldexp(torch.ones_like(amax), scale.to(torch.int32) - 127)
    nz = amax > 0
    ratio = amax[nz] / sc[nz]
    assert bool((ratio > 3).all()) and bool((ratio <= 6).all()), (float(ratio.min()), float(ratio.max()))
    assert int(scale[3, 0]) == 127 and int(packed[3, :16].max()) == 0, "an all-zero block: byte 127 and zero codes"
    deq = dequantize_mxfp4(packed, scale)
    assert deq.dtype == torch.bfloat16 and tuple(deq.shape) == (24, K)
    # exact bf16: the same values computed in fp64 from the bytes
    tab = torch.tensor(E2M1 + [-x for x in E2M1], dtype=torch.float64)
    want = tab[_codes(packed).long()].reshape(24, K // 32, 32) * torch.ldexp(torch.ones(24, K // 32, dtype=torch.float64),
                                                                            scale.to(torch.int32) - 127)[:, :, None]
    assert torch.equal(deq.double(), want.reshape(24, K))
    assert torch.equal(deq.float().to(torch.bfloat16), deq)
    # nearest code: no other representable magnitude of the block's grid is closer
    v = (w.float().reshape(24, K // 32, 32) / sc[:, :, None]).abs()
    got = (deq.float().reshape(24, K // 32, 32) / sc[:, :, None]).abs()
    grid = torch.tensor(E2M1)
    best = (v[..., None] - grid).abs().amin(dim=-1)
    assert bool(((v - got).abs() == best).all())
    # re-quantising the dequantised weights reproduces the values (not the bytes: a block whose maximum rounded to 3 rescales)
    p2, s2 = quantize_blocks(deq)
    assert torch.equal(dequantize_mxfp4(p2, s2), deq)
    # relative rms error: the format's noise (0.116 - 0.118 on Gaussian rows)
    rel = float((deq.float() - w.float()).pow(2).sum().sqrt() / w.float().pow(2).sum().sqrt())
    assert 0.09 < rel < 0.14, rel


def test_ties_go_to_the_even_code_and_a_hand_made_block_saturates():
    w = torch.zeros(2, 32)
    w[0, :8] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])   # amax 6: scale 1
    w[0, 8:15] = -torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[1, :4] = torch.tensor([6.0, 5.5, -5.75, 0.24])
    packed, scale = quantize_blocks(w)
    assert scale.flatten().tolist() == [127, 127]
    deq = dequantize_mxfp4(packed, scale).float()
    assert deq[0, :8].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert deq[0, 8:15].tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert deq[1, :4].tolist() == [6.0, 6.0, -6.0, 0.0]
    assert int(_codes(packed).max()) <= 15 and float(deq.abs().max()) == 6.0
    # a block holding bf16 max: the code steps down instead of dequantising to inf
    big = torch.zeros(1, 32)
    big[0, 0] = float(torch.finfo(torch.bfloat16).max)
    p, s = quantize_blocks(big.to(torch.bfloat16))
    assert bool(torch.isfinite(dequantize_mxfp4(p, s).float()).all()) and float(dequantize_mxfp4(p, s)[0, 0]) == 3.0 * 2.0 ** 126
    for bad in (float("inf"), float("nan")):
        w = torch.zeros(1, 32)
        w[0, 5] = bad
        with pytest.raises(ValueError):
            quantize_blocks(w)
    with pytest.raises(ValueError, match="48"):
        quantize_blocks(torch.zeros(2, 48))


def test_scale_exponent_is_integer_arithmetic_at_every_magnitude():
    for e in (-30, -1, 0, 7, 40):
        for m, up in ((1.0, 0), (1.5, 0), (1.5078125, 1), (1.9921875, 1)):
            w = torch.zeros(1, 32)
            w[0, 7] = m * 2.0 ** e
            _, scale = quantize_blocks(w.to(torch.bfloat16))
            assert int(scale) - 127 == e - 2 + up, (e, m)   # ceil(log2(m 2^e / 6))


def test_packing_low_nibble_is_the_even_k():
    w = torch.zeros(1, 32)
    w[0, 0::2] = 6.0       # code 7 at every even k
    w[0, 1::2] = -1.0      # code 8 | 2 at every odd k
    packed, scale = quantize_blocks(w)
    assert packed.flatten().tolist() == [0xA7] * 16 and int(scale) == 127
    hand = torch.tensor([[0x21] + [0] * 15], dtype=torch.uint8)      # low nibble 1 (0.5) at k = 0, high nibble 2 (1.0) at k = 1
    deq = dequantize_mxfp4(hand, torch.tensor([[128]], dtype=torch.uint8)).float()
    assert deq[0, :3].tolist() == [1.0, 2.0, 0.0]


def _quantized_folder(tmp_path):
    w = mo.synth_weights(ARGS, seed=11)
    src = write_checkpoint(tmp_path / "bf16", ARGS, w)
    dst = quantize_checkpoint(src, tmp_path / "mxfp4", qformat="mxfp4")
    return w, src, dst


def test_quantize_checkpoint_round_trip(tmp_path):
    w, src, dst = _quantized_folder(tmp_path)
    params = json.load(open(dst / "params.json"))
    assert params["quantization"] == {"qformat_weight": "mxfp4"}
    assert {k: v for k, v in params.items() if k != "quantization"} == json.load(open(os.path.join(src, "params.json")))
    lin = {f"layers.{l}.{n}.weight" for l in range(ARGS.n_layers) for n in LINEARS}
    want = set(w) | {k[:-len("weight")] + QSCALE_KEY for k in lin}
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        assert set(f.keys()) == want
        for k in f.keys():
            sl, t = f.get_slice(k), f.get_tensor(k)
            if k in lin:
                out, inn = w[k].shape
                assert sl.get_dtype() == "U8" and tuple(t.shape) == (out, inn // 2)
                packed, scale = quantize_blocks(w[k])
                assert torch.equal(t, packed)
                assert torch.equal(f.get_tensor(k[:-len("weight")] + QSCALE_KEY), scale)
            elif k.endswith(QSCALE_KEY):
                out, inn = w[k[:-len(QSCALE_KEY)] + "weight"].shape
                assert sl.get_dtype() == "U8" and tuple(t.shape) == (out, inn // 32)
            else:
                assert sl.get_dtype() == "BF16" and torch.equal(t, w[k])
    lin_n = sum(w[k].numel() for k in lin)
    rest_b = 2 * sum(v.numel() for k, v in w.items() if k not in lin)
    expect = lin_n * (1 / 2 + 1 / 32) + rest_b
    dst_sz = os.path.getsize(dst / "consolidated.safetensors")
    assert abs(dst_sz - expect) < 0.02 * expect, (dst_sz, expect)
    with pytest.raises(ValueError, match="already quantised"):
        quantize_checkpoint(dst, tmp_path / "again", qformat="mxfp4")
    with pytest.raises(ValueError, match="already quantised"):
        quantize_checkpoint(dst, tmp_path / "again8")
    fp8 = quantize_checkpoint(src, tmp_path / "fp8")
    with pytest.raises(ValueError, match="already quantised"):
        quantize_checkpoint(fp8, tmp_path / "again4", qformat="mxfp4")
    assert json.load(open(fp8 / "params.json"))["quantization"] == {"qformat_weight": "fp8_e4m3"}   # the default is unchanged
    # a folder of one format under the other's params.json is not accepted
    for a, b, name in ((fp8, "mxfp4", "fp8_as_mxfp4"), (dst, "fp8_e4m3", "mxfp4_as_fp8")):
        mixed = tmp_path / name
        mixed.mkdir()
        os.symlink(a / "consolidated.safetensors", mixed / "consolidated.safetensors")
        json.dump({**mo.params_json(ARGS), "quantization": {"qformat_weight": b}}, open(mixed / "params.json", "w"))
        with pytest.raises(ValueError):
            Transformer.from_folder(mixed, device="cpu")
    m = Transformer.from_folder(dst, device="cpu")      # the folder loads as it is
    mod = m.layers["0"].attention.wq
    assert isinstance(mod, Mxfp4Linear) and torch.equal(mod.weight, quantize_blocks(w["layers.0.attention.wq.weight"])[0])
    assert torch.equal(mod.dequantized(), dequantize_mxfp4(*quantize_blocks(w["layers.0.attention.wq.weight"])))


def test_params_json_block_and_refusals(tmp_path):
    base = mo.params_json(ARGS)
    a = TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "mxfp4"}})
    assert a.quantization == QuantizationArgs("mxfp4") and QFORMAT_MXFP4 == "mxfp4"
    with pytest.raises(NotImplementedError, match="int4_awq"):
        TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "int4_awq"}})
    check_quantize_arg("mxfp4")
    with pytest.raises(NotImplementedError, match="nf4"):
        check_quantize_arg("nf4")

    def folder(name, extra):   # refused by name before any tensor is read: the folders hold params.json only
        d = tmp_path / name
        d.mkdir()
        json.dump({**base, "quantization": {"qformat_weight": "mxfp4"}, **extra}, open(d / "params.json", "w"))
        return d
    with pytest.raises(NotImplementedError, match="LoRA.*MXFP4"):
        Transformer.from_folder(folder("lora", {"lora": {"rank": 8, "scaling": 2.0}}), device="cpu")
    with pytest.raises(NotImplementedError, match="MXFP4.*MoE"):
        Transformer.from_folder(folder("moe", {"moe": {"num_experts": 4, "num_experts_per_tok": 2}}), device="cpu")
    with pytest.raises(NotImplementedError, match="MXFP4.*fp16 / fp32"):
        Transformer.from_folder(folder("f16", {}), device="cpu", dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="MXFP4.*fp16 / fp32"):
        Transformer.from_folder(folder("f32", {}), device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="1040"):
        Transformer.from_folder(folder("odd", {"hidden_dim": 1040}), device="cpu")      # in % 32 != 0
    plain = tmp_path / "plain"
    plain.mkdir()
    json.dump(base, open(plain / "params.json", "w"))
    with pytest.raises(NotImplementedError, match="MXFP4.*fp16 / fp32"):
        Transformer.from_folder(plain, device="cpu", dtype=torch.float16, quantize="mxfp4")


def test_scale_byte_255_in_a_checkpoint_is_refused(tmp_path):
    w, src, dst = _quantized_folder(tmp_path)
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys()}
    sd["layers.1.feed_forward.w2.qscale_weight"][3, 1] = 255
    save_file(sd, str(dst / "consolidated.safetensors"))
    with pytest.raises(ValueError, match="255"):
        Transformer.from_folder(dst, device="cpu")
    lin = Mxfp4Linear(64, 4)
    with pytest.raises(ValueError, match="255"):
        lin.load_quantized(torch.zeros(4, 32, dtype=torch.uint8), torch.full((4, 2), 255, dtype=torch.uint8))
    with pytest.raises(ValueError, match="48"):
        Mxfp4Linear(48, 4)


def _meta_model(rank=1, ranks=2):
    a = TransformerArgs.from_dict({**mo.params_json(ARGS), "quantization": {"qformat_weight": "mxfp4"}})
    with torch.device("meta"):
        return Transformer(a, pipeline_rank=rank, num_pipeline_ranks=ranks).to(torch.bfloat16)


def test_meta_built_quantised_model_on_a_later_pipeline_rank():
    m = _meta_model()
    assert m.dtype == torch.bfloat16       # not the code bytes of its first layer
    assert list(m.layers.keys()) == ["1"]
    blk = m.layers["1"]
    dims = {"attention.wq": (512, 512), "attention.wk": (256, 512), "attention.wv": (256, 512), "attention.wo": (512, 512),
            "feed_forward.w1": (1024, 512), "feed_forward.w2": (512, 1024), "feed_forward.w3": (1024, 512)}
    for name in LINEARS:
        mod = blk.get_submodule(name)
        assert isinstance(mod, Mxfp4Linear) and not isinstance(mod, Fp8Linear)
        out, inn = dims[name]
        assert (mod.out_features, mod.in_features) == (out, inn)
        assert sum(p.numel() * p.element_size() for p in mod.parameters()) == out * inn // 2 + out * inn // 32
        assert mod.weight.dtype == torch.uint8 and mod.qscale_weight.dtype == torch.uint8  # the bf16 cast touched neither
    assert isinstance(m.output, torch.nn.Linear) and m.output.weight.dtype == torch.bfloat16  # the LM head is not quantised
    with pytest.raises(NotImplementedError, match="merging an adapter into MXFP4"):
        m.load_lora("/nonexistent/lora.safetensors")


def test_dtype_casts_leave_codes_and_scales_alone():
    lin = Mxfp4Linear(64, 16)
    packed, scale = quantize_blocks(torch.randn(16, 64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16))
    lin.load_quantized(packed, scale)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        lin = lin.to(dt)
        assert lin.weight.dtype == torch.uint8 and lin.qscale_weight.dtype == torch.uint8
        assert torch.equal(lin.weight, packed) and torch.equal(lin.qscale_weight, scale)


# ---- the C entry points' argument checks (no device work happens before them)
_vp = C.c_void_p
FAKE = 0x10000  # never dereferenced: every call below is refused before any launch


def _w4_call(K=64, M=2, w0=FAKE, s0=FAKE, out=FAKE, x=FAKE, epi=_hip.EPI_STORE):
    wp = (_vp * 3)(w0, None, None)
    sp = (_vp * 3)(s0, None, None)
    nr = (C.c_int * 3)(64, 0, 0)
    return _hip.lib().mi_linear_w4(out, 64, x, K, M, K, wp, nr, epi, None, None, 0.0, sp, None, 0, None)


def test_mi_linear_w4_argument_checks():
    L = _hip.lib()
    assert _w4_call(out=None) == -1 and _w4_call(x=None) == -1 and _w4_call(w0=None) == -1 and _w4_call(s0=None) == -1
    assert _w4_call(K=48) == _hip.MI_ERR_SHAPE
    assert "mi_linear_w4" in L.mi_last_error_detail().decode() and "48" in L.mi_last_error_detail().decode()
    assert _w4_call(epi=_hip.EPI_LOGITS) == -4      # the LM head is not quantised
    assert _w4_call(epi=_hip.EPI_RESIDUAL) == -1    # residual epilogue without a residual
    assert _w4_call(M=16) == -3                     # more than 8 rows: needs the dequantisation scratch
    nr = (C.c_int * 3)(64, 32, 0)
    assert L.mi_linear_w4_scratch_bytes(8, 64, nr, _hip.EPI_STORE) == 0
    assert L.mi_linear_w4_scratch_bytes(9, 64, nr, _hip.EPI_STORE) == 96 * 64 * 2
    assert L.mi_linear_w4_scratch_bytes(9, 64, nr, _hip.EPI_SWIGLU) == 128 * 64 * 2
    rc = L.mi_qkv_rope_kvwrite_w4(FAKE, 512, FAKE, 48, 1, 48, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 1, 128, None, 0.0, FAKE, 16, FAKE,
                                  None, None, None, 0, 0, None)
    assert rc == _hip.MI_ERR_SHAPE and "mi_qkv_rope_kvwrite_w4" in L.mi_last_error_detail().decode()
    assert "48" in L.mi_last_error_detail().decode()


def _model(**kw):
    layers = (_hip.MiLayer * 2)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 2
    m.norm_eps = 1e-5
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    for k, v in kw.items():
        setattr(m, k, v)
    return m, layers


def _w4():
    scales = (_hip.MiW4Layer * 2)()
    w4 = _hip.MiW4Model()
    w4.format, w4.layers = _hip.MI_W4_MXFP4, C.cast(scales, C.POINTER(_hip.MiW4Layer))
    return w4, scales


def test_mi_forward_w4_refuses_moe_and_lora_by_name_and_sizes_a_plain_model_as_ever():
    L = _hip.lib()
    w4, _keep = _w4()
    bt = _hip.MiBatch()
    moe, _k1 = _model(num_experts=8, top_k=2)
    assert L.mi_forward_w4(C.byref(moe), C.byref(w4), C.byref(bt), None) == -4
    detail = L.mi_last_error_detail().decode()
    assert "MoE" in detail and "MXFP4" in detail and "mi_forward_w4" in detail
    lora, _k2 = _model(lora_rank=8, lora_scaling=2.0)
    assert L.mi_forward_w4(C.byref(lora), C.byref(w4), C.byref(bt), None) == -4
    assert "LoRA" in L.mi_last_error_detail().decode() and "MXFP4" in L.mi_last_error_detail().decode()
    dense, _k3 = _model()
    for fmt in (1, 3):
        bad = _hip.MiW4Model()
        bad.format, bad.layers = fmt, w4.layers
        assert L.mi_forward_w4(C.byref(dense), C.byref(bad), C.byref(bt), None) == -4
    # mi_forward_w8 keeps refusing the new format value
    w8 = _hip.MiW8Model()
    w8.format, w8.layers = _hip.MI_W4_MXFP4, C.cast((_hip.MiW8Layer * 2)(), C.POINTER(_hip.MiW8Layer))
    assert L.mi_forward_w8(C.byref(dense), C.byref(w8), C.byref(bt), None) == -4
    odd, _k4 = _model(hidden_dim=1040)
    assert L.mi_forward_w4(C.byref(odd), C.byref(w4), C.byref(bt), None) == _hip.MI_ERR_SHAPE
    for T, B, W in ((1, 1, 16), (3, 3, 4096), (12, 1, 16), (4096, 1, 4096)):
        plain = L.mi_workspace_bytes(C.byref(dense), T, B, W)
        assert L.mi_workspace_bytes_w4(C.byref(dense), None, T, B, W) == plain
        extra = L.mi_workspace_bytes_w4(C.byref(dense), C.byref(w4), T, B, W) - plain
        # the dequantisation scratch: the largest linear group (w1|w3: 2 F D bf16 elements), for more than 8 rows only
        assert extra == (2 * 1024 * 512 * 2 if T > 8 else 0), (T, extra)


def test_the_symbols_are_exported():
    for name in ("mi_linear_w4_scratch_bytes", "mi_linear_w4", "mi_qkv_rope_kvwrite_w4", "mi_workspace_bytes_w4", "mi_forward_w4"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(_hip.lib(), name)


# ---- teeth of the exact family of tests/test_gpu_mxfp4.py: its fp64 reference moves in every output row under either mutation
@pytest.mark.parametrize("K,N", EXACT_SHAPES)
def test_exact_family_reference_sees_shifted_scales_and_swapped_nibbles(K, N):
    packed, scale, x = exact_case(K, N, M=3)
    ref = exact_reference(packed, scale, x)
    assert float(ref.abs().max()) * 16 < 2 ** 24
    rolled = (scale + 1) if K == 32 else torch.roll(scale, 1, dims=1)
    swapped = (packed << 4) | (packed >> 4)
    for mutant in (exact_reference(packed, rolled, x), exact_reference(swapped, scale, x)):
        changed = (mutant != ref).any(dim=0)     # ref is [M, N]
        assert int(changed.sum()) == N, (K, N, int(changed.sum()))
