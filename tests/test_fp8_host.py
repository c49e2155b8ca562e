"""Weight-only FP8 (OCP e4m3) on the host: the quantiser, the checkpoint writer, params.json parsing and refusals, a meta-built
quantised model, and the argument checks of the new C entry points - nothing here needs a device."""
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
from mistral_inference.args import QuantizationArgs, TransformerArgs
from mistral_inference.quant import QSCALE_KEY, Fp8Linear, dequantize, quantize_checkpoint, quantize_rows
from mistral_inference.transformer import Transformer

ARGS = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                     sliding_window=16)
LINEARS = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2", "feed_forward.w3")
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def _rows():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(40, 64, generator=g)
    w *= torch.logspace(-6, 6, 40, base=2.0)[:, None] * 0.37   # row maxima over 12 octaves, none a power of two
    w[5] = 0.0                                                  # an all-zero row
    w[6, :] = 0.0
    w[6, 3] = 448.0                                             # amax / scale == 448 exactly
    w[7, :] = 1e-3
    w[7, 9] = -BF16_MAX                                         # a row holding bf16 max
    w[8, 0], w[8, 1] = 1.0, 2.0 ** -20                          # an entry below half the row's smallest e4m3 subnormal (2^-17)
    return w.to(torch.bfloat16)


def test_quantize_rows_scales_codes_and_exact_dequantisation():
    w = _rows()
    q, scale = quantize_rows(w)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and tuple(scale.shape) == (40,)
    mant, _ = torch.frexp(scale)
    assert bool((mant == 0.5).all()), "row scales are powers of two"
    amax = w.float().abs().amax(dim=1)
    nz = amax > 0
    ratio = amax[nz] / scale[nz]
    assert bool((ratio > 224).all()) and bool((ratio <= 448).all()), ratio
    assert float(scale[5]) == 1.0 and int(q[5].view(torch.uint8).max()) == 0        # zero row: scale 1, zero codes
    assert float(amax[6] / scale[6]) == 448.0
    codes = q.view(torch.uint8)
    assert not bool(((codes & 0x7F) == 0x7F).any()), "the NaN codes 0x7F / 0xFF are never produced"
    deq = dequantize(q, scale)
    assert deq.dtype == torch.bfloat16
    assert torch.equal(deq.float(), q.float() * scale[:, None]), "bf16(scale * e4m3) is exact for power-of-two scales"
    assert torch.equal(dequantize(codes, scale), deq)                                # bytes or float8: the same
    # relative error of a normal e4m3 value: half an ulp of 3 mantissa bits
    big = w.float().abs() >= (2.0 ** -6) * scale[:, None]
    rel = ((deq.float() - w.float()).abs() / w.float().abs().clamp_min(1e-30))[big]
    assert float(rel.max()) <= 2.0 ** -4
    # a row holding bf16 max saturates: with the scale 2^120 the entry is 255 * scale, which e4m3 would round UP to 256 * scale
    # = 2^128 = inf; it becomes the largest code below, 240 * scale - finite, inside +-448 * scale, within one e4m3 step
    assert float(scale[7]) == 2.0 ** 120 and bool(torch.isfinite(deq[7].float()).all())
    assert float(deq[7].float().abs().max()) <= 448.0 * float(scale[7])
    assert float(deq[7, 9]) == -240.0 * 2.0 ** 120 and abs(float(deq[7, 9]) + BF16_MAX) <= 2.0 ** -4 * BF16_MAX
    assert float(deq[8, 1]) == 0.0 and float(deq[8, 0]) == 1.0


def test_e4m3_cast_is_guarded_against_the_nan_codes():
    """torch's cast to float8_e4m3fn turns anything that rounds above 448 into the NaN code; quantize_rows clamps first."""
    assert int(torch.tensor([500.0]).to(torch.float8_e4m3fn).view(torch.uint8)) == 0x7F   # what the clamp is for
    w = torch.tensor([[447.0, -448.0, 3.0, 0.0] * 4]).to(torch.bfloat16)                  # bf16(447) = 448
    q, scale = quantize_rows(w)
    assert float(scale) == 1.0 and q.view(torch.uint8)[0, :2].tolist() == [0x7E, 0xFE]
    with pytest.raises(ValueError):
        quantize_rows(torch.tensor([[float("inf")] * 16]))


def test_quantize_rows_is_the_same_on_every_row_magnitude():
    """Exponent arithmetic on integers (frexp / ldexp): exact at powers of two and at 1.75 * 2^e, where a log2 could round."""
    for e in (-20, -1, 0, 7, 30):
        for m, up in ((1.0, 0), (1.75, 0), (1.7578125, 1), (1.9921875, 1)):
            w = torch.zeros(1, 16)
            w[0, 0] = m * 2.0 ** e
            _, scale = quantize_rows(w.to(torch.bfloat16))
            assert float(scale) == 2.0 ** (e - 8 + up), (e, m)


def _quantized_folder(tmp_path):
    w = mo.synth_weights(ARGS, seed=11)
    src = write_checkpoint(tmp_path / "bf16", ARGS, w)
    dst = quantize_checkpoint(src, tmp_path / "fp8")
    return w, src, dst


def test_quantize_checkpoint_round_trip(tmp_path):
    w, src, dst = _quantized_folder(tmp_path)
    params = json.load(open(dst / "params.json"))
    assert params["quantization"] == {"qformat_weight": "fp8_e4m3"}
    assert {k: v for k, v in params.items() if k != "quantization"} == json.load(open(os.path.join(src, "params.json")))
    lin = {f"layers.{l}.{n}.weight" for l in range(ARGS.n_layers) for n in LINEARS}
    want = set(w) | {k[:-len("weight")] + QSCALE_KEY for k in lin}
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        assert set(f.keys()) == want
        for k in f.keys():
            sl, t = f.get_slice(k), f.get_tensor(k)
            if k in lin:
                assert sl.get_dtype() == "F8_E4M3" and tuple(t.shape) == tuple(w[k].shape)
                q, scale = quantize_rows(w[k])
                assert torch.equal(t.view(torch.uint8), q.view(torch.uint8))
                assert torch.equal(f.get_tensor(k[:-len("weight")] + QSCALE_KEY), scale)
            elif k.endswith(QSCALE_KEY):
                assert sl.get_dtype() == "F32" and tuple(t.shape) == (w[k[:-len(QSCALE_KEY)] + "weight"].shape[0],)
            else:
                assert sl.get_dtype() == "BF16" and torch.equal(t, w[k])
    # about half: the linears halve (+ 4 bytes per row), embeddings / LM head / norms stay
    lin_b = sum(w[k].numel() for k in lin)
    rest_b = 2 * sum(v.numel() for k, v in w.items() if k not in lin)
    src_sz = os.path.getsize(os.path.join(src, "consolidated.safetensors"))
    dst_sz = os.path.getsize(dst / "consolidated.safetensors")
    assert abs(dst_sz - (lin_b + rest_b)) < 0.02 * src_sz and dst_sz < 0.6 * src_sz, (src_sz, dst_sz)
    with pytest.raises(ValueError, match="already quantised"):
        quantize_checkpoint(dst, tmp_path / "again")


def test_params_json_block_and_refusals(tmp_path):
    base = mo.params_json(ARGS)
    a = TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "fp8_e4m3"}})
    assert a.quantization == QuantizationArgs("fp8_e4m3")
    assert TransformerArgs.from_dict(base).quantization is None
    with pytest.raises(NotImplementedError, match="int4_awq"):
        TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "int4_awq"}})

    # refused by name before any tensor is read: the folders hold params.json only
    def folder(name, extra):
        d = tmp_path / name
        d.mkdir()
        json.dump({**base, "quantization": {"qformat_weight": "fp8_e4m3"}, **extra}, open(d / "params.json", "w"))
        return d
    with pytest.raises(NotImplementedError, match="LoRA"):
        Transformer.from_folder(folder("lora", {"lora": {"rank": 8, "scaling": 2.0}}), device="cpu")
    with pytest.raises(NotImplementedError, match="MoE"):
        Transformer.from_folder(folder("moe", {"moe": {"num_experts": 4, "num_experts_per_tok": 2}}), device="cpu")
    with pytest.raises(NotImplementedError, match="fp16 / fp32"):
        Transformer.from_folder(folder("f16", {}), device="cpu", dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="fp16 / fp32"):
        Transformer.from_folder(folder("f32", {}), device="cpu", dtype=torch.float32)
    plain = tmp_path / "plain"
    plain.mkdir()
    json.dump(base, open(plain / "params.json", "w"))
    with pytest.raises(NotImplementedError, match="int8"):
        Transformer.from_folder(plain, device="cpu", quantize="int8")
    with pytest.raises(NotImplementedError, match="fp16 / fp32"):
        Transformer.from_folder(plain, device="cpu", dtype=torch.float16, quantize="fp8_e4m3")


def _meta_model(rank=1, ranks=2):
    a = TransformerArgs.from_dict({**mo.params_json(ARGS), "quantization": {"qformat_weight": "fp8_e4m3"}})
    with torch.device("meta"):
        return Transformer(a, pipeline_rank=rank, num_pipeline_ranks=ranks).to(torch.bfloat16)


def test_meta_built_quantised_model_on_a_later_pipeline_rank():
    m = _meta_model()
    assert m.dtype == torch.bfloat16       # not the e4m3 bytes of its first layer
    assert list(m.layers.keys()) == ["1"]
    blk = m.layers["1"]
    dims = {"attention.wq": (512, 512), "attention.wk": (256, 512), "attention.wv": (256, 512), "attention.wo": (512, 512),
            "feed_forward.w1": (1024, 512), "feed_forward.w2": (512, 1024), "feed_forward.w3": (1024, 512)}
    for name in LINEARS:
        mod = blk.get_submodule(name)
        assert isinstance(mod, Fp8Linear)
        out, inn = dims[name]
        assert (mod.out_features, mod.in_features) == (out, inn)
        assert sum(p.numel() * p.element_size() for p in mod.parameters()) == out * inn + 4 * out
        assert mod.weight.dtype == torch.uint8 and mod.qscale_weight.dtype == torch.float32  # the bf16 cast touched neither
    assert isinstance(m.output, torch.nn.Linear) and m.output.weight.dtype == torch.bfloat16  # the LM head is not quantised
    with pytest.raises(NotImplementedError, match="merging an adapter into FP8"):
        m.load_lora("/nonexistent/lora.safetensors")


def test_dtype_casts_leave_bytes_and_scales_alone():
    lin = Fp8Linear(32, 16)
    q, scale = quantize_rows(torch.randn(16, 32, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16))
    lin.load_quantized(q, scale * 1.25)   # a scale that bf16 cannot hold
    before = (lin.weight.clone(), lin.qscale_weight.clone())
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        lin = lin.to(dt)
        assert lin.weight.dtype == torch.uint8 and lin.qscale_weight.dtype == torch.float32
        assert torch.equal(lin.weight, before[0]) and torch.equal(lin.qscale_weight, before[1])
    lin.load_quantized(q, torch.tensor(0.5))  # a scalar scale is broadcast
    assert tuple(lin.qscale_weight.shape) == (16,) and bool((lin.qscale_weight == 0.5).all())


def test_activation_scale_key_is_a_foreign_key(tmp_path):
    w, src, dst = _quantized_folder(tmp_path)
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys()}
    sd["layers.0.attention.wq.qscale_act"] = torch.ones(1)
    save_file(sd, str(dst / "consolidated.safetensors"))
    with pytest.raises(ValueError, match="Unexpected key layers.0.attention.wq.qscale_act"):
        Transformer.from_folder(dst, device="cpu")


# ---- the C entry points' argument checks (no device work happens before them)
_vp = C.c_void_p
FAKE = 0x10000  # never dereferenced: every call below is refused before any launch


def _w8_call(K=32, M=2, w0=FAKE, s0=FAKE, out=FAKE, x=FAKE, epi=_hip.EPI_STORE):
    wp = (_vp * 3)(w0, None, None)
    sp = (_vp * 3)(s0, None, None)
    nr = (C.c_int * 3)(64, 0, 0)
    return _hip.lib().mi_linear_w8(out, 64, x, K, M, K, wp, nr, epi, None, None, 0.0, sp, None, 0, None)


def test_mi_linear_w8_argument_checks():
    L = _hip.lib()
    assert _w8_call(out=None) == -1 and _w8_call(x=None) == -1 and _w8_call(w0=None) == -1 and _w8_call(s0=None) == -1
    assert _w8_call(K=24) == _hip.MI_ERR_SHAPE
    assert "mi_linear_w8" in L.mi_last_error_detail().decode() and "24" in L.mi_last_error_detail().decode()
    assert _w8_call(epi=_hip.EPI_LOGITS) == -4      # the LM head is not quantised
    assert _w8_call(epi=_hip.EPI_RESIDUAL) == -1    # residual epilogue without a residual
    assert _w8_call(M=16) == -3                     # more than 8 rows: needs the dequantisation scratch
    nr = (C.c_int * 3)(64, 32, 0)
    assert L.mi_linear_w8_scratch_bytes(8, 32, nr, _hip.EPI_STORE) == 0
    assert L.mi_linear_w8_scratch_bytes(9, 32, nr, _hip.EPI_STORE) == 96 * 32 * 2
    assert L.mi_linear_w8_scratch_bytes(9, 32, nr, _hip.EPI_SWIGLU) == 128 * 32 * 2
    rc = L.mi_qkv_rope_kvwrite_w8(FAKE, 512, FAKE, 24, 1, 24, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 1, 128, None, 0.0, FAKE, 16, FAKE,
                                  None, None, None, 0, 0, None)
    assert rc == _hip.MI_ERR_SHAPE and "mi_qkv_rope_kvwrite_w8" in L.mi_last_error_detail().decode()


def _model(**kw):
    layers = (_hip.MiLayer * 2)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 2
    m.norm_eps = 1e-5
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    for k, v in kw.items():
        setattr(m, k, v)
    return m, layers


def _w8():
    scales = (_hip.MiW8Layer * 2)()
    w8 = _hip.MiW8Model()
    w8.format, w8.layers = _hip.MI_W8_FP8_E4M3, C.cast(scales, C.POINTER(_hip.MiW8Layer))
    return w8, scales


def test_mi_forward_w8_refuses_moe_and_lora_by_name_and_sizes_a_plain_model_as_ever():
    L = _hip.lib()
    w8, _keep = _w8()
    bt = _hip.MiBatch()
    moe, _k1 = _model(num_experts=8, top_k=2)
    assert L.mi_forward_w8(C.byref(moe), C.byref(w8), C.byref(bt), None) == -4
    assert "MoE" in L.mi_last_error_detail().decode() and "mi_forward_w8" in L.mi_last_error_detail().decode()
    lora, _k2 = _model(lora_rank=8, lora_scaling=2.0)
    assert L.mi_forward_w8(C.byref(lora), C.byref(w8), C.byref(bt), None) == -4
    assert "LoRA" in L.mi_last_error_detail().decode()
    dense, _k3 = _model()
    bad = _hip.MiW8Model()
    bad.format, bad.layers = 2, w8.layers
    assert L.mi_forward_w8(C.byref(dense), C.byref(bad), C.byref(bt), None) == -4
    odd, _k4 = _model(hidden_dim=1032)
    assert L.mi_forward_w8(C.byref(odd), C.byref(w8), C.byref(bt), None) == _hip.MI_ERR_SHAPE
    for T, B, W in ((1, 1, 16), (3, 3, 4096), (12, 1, 16), (4096, 1, 4096)):
        plain = L.mi_workspace_bytes(C.byref(dense), T, B, W)
        assert L.mi_workspace_bytes_w8(C.byref(dense), None, T, B, W) == plain
        extra = L.mi_workspace_bytes_w8(C.byref(dense), C.byref(w8), T, B, W) - plain
        # the dequantisation scratch: the largest linear group (w1|w3: 2 F D bf16 elements), for more than 8 rows only
        assert extra == (2 * 1024 * 512 * 2 if T > 8 else 0), (T, extra)
