"""FP8 (e4m3) MoE experts on the host: the checkpoint round trip with `experts=True`, the new refusals by name and the unchanged
one without the switch, and the argument checks of the new C entries (fake pointers, codes checked before any launch)."""
import ctypes as C
import json
import os

import pytest
import torch
import safetensors

import mistral_oracle as mo
from hip_util import write_checkpoint
from mistral_inference import _hip
from mistral_inference.quant import QSCALE_KEY, dequantize, quantize_checkpoint
from mistral_inference.transformer import Transformer

ARGS = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                     num_experts=4, num_experts_per_tok=2)
FAKE = C.c_void_p(0x1000)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("moe_fp8")
    w = mo.synth_weights(ARGS, seed=5)
    src = write_checkpoint(root / "bf16", ARGS, w)
    return root, src, w, str(quantize_checkpoint(src, root / "fp8", experts=True))


def test_checkpoint_round_trip_with_experts(folders):
    _, src, w, dst = folders
    params = json.load(open(os.path.join(dst, "params.json")))
    assert params["quantization"] == {"qformat_weight": "fp8_e4m3", "experts": True} and params["moe"]["num_experts"] == 4
    with safetensors.safe_open(os.path.join(dst, "consolidated.safetensors"), framework="pt") as f:
        keys = set(f.keys())
        for name, t in w.items():
            quantised = ".attention.w" in name or ".experts." in name
            assert (name[:-len("weight")] + QSCALE_KEY in keys) == quantised, name
            got = f.get_tensor(name)
            if not quantised:  # the router gate, norms, embeddings and the LM head stay bf16
                assert got.dtype == torch.bfloat16 and torch.equal(got, t), name
                continue
            s = f.get_tensor(name[:-len("weight")] + QSCALE_KEY)
            assert got.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and tuple(s.shape) == (t.shape[0],)
            assert float(((dequantize(got, s).float() - t.float()).abs() / t.float().abs().clamp_min(2.0 ** -6 * s[:, None])).max()) <= 2.0 ** -4
    size = lambda d: os.path.getsize(os.path.join(d, "consolidated.safetensors"))  # noqa: E731
    bf16_rest = 2 * sum(t.numel() for n, t in w.items() if not (".attention.w" in n or ".experts." in n))
    assert abs(size(dst) - (size(src) + bf16_rest) / 2) < 0.02 * size(src), (size(src), size(dst))
    model = Transformer.from_folder(dst, device="cpu")
    assert type(model.layers["0"].feed_forward.experts[0].w2).__name__ == "Fp8Linear"
    assert isinstance(model.layers["0"].feed_forward.gate, torch.nn.Linear)


def test_refusals_by_name(folders):
    root, src, w, dst = folders
    dense = write_checkpoint(root / "dense", mo.OracleArgs(**{**ARGS.__dict__, "num_experts": 0, "num_experts_per_tok": 0}),
                             {k: v for k, v in w.items() if "feed_forward" not in k})
    load = lambda f, **kw: Transformer.from_folder(f, device="cpu", **kw)  # noqa: E731  (every refusal comes before anything is read)
    with pytest.raises(NotImplementedError, match="MoE model is not implemented .the expert kernels read bf16 weights."):
        load(src, quantize="fp8_e4m3")                                       # without the switch: today's refusal, word for word
    params = json.load(open(os.path.join(dst, "params.json")))
    params["quantization"] = {"qformat_weight": "fp8_e4m3"}
    os.makedirs(root / "noflag", exist_ok=True)
    json.dump(params, open(root / "noflag" / "params.json", "w"))
    with pytest.raises(NotImplementedError, match="the expert kernels read bf16 weights"):
        load(root / "noflag")                                                # a quantization block without "experts": true
    with pytest.raises(NotImplementedError, match="MXFP4 expert weights"):
        load(src, quantize="mxfp4", quantize_experts=True)
    with pytest.raises(NotImplementedError, match="dense model"):
        load(dense, quantize="fp8_e4m3", quantize_experts=True)
    with pytest.raises(NotImplementedError, match="fp16 / fp32"):
        load(src, quantize="fp8_e4m3", quantize_experts=True, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="quantize_experts=True needs quantize"):
        load(src, quantize_experts=True)
    with pytest.raises(NotImplementedError, match="prefill_fp8=True on a MoE model with FP8 experts"):
        load(dst, prefill_fp8=True)
    with pytest.raises(NotImplementedError, match="MXFP4 expert weights"):
        quantize_checkpoint(src, root / "w4", "mxfp4", experts=True)
    model = load(dst)
    with pytest.raises(NotImplementedError, match="load_lora.*FP8"):
        model.load_lora(root / "none.safetensors")
    with pytest.raises(NotImplementedError, match="FP8 experts"):
        model.refuse_verify(None, model_only=True)


def _decode(**kw):
    a = dict(out=FAKE, x=FAKE, tab=FAKE, stab=FAKE, T=1, D=272, F=528, k=2)
    a.update(kw)
    return _hip.lib().mi_moe_experts_decode_w8(a["out"], FAKE, a["x"], a["D"], a["T"], a["D"], a["F"], a["tab"], a["stab"], FAKE, FAKE, a["k"],
                                               None, 0.0, FAKE, None)


def _grouped(**kw):
    a = dict(tab=FAKE, stab=FAKE, T=16, D=272, F=528, E=4, k=2, scratch=FAKE, nbytes=1 << 40)
    a.update(kw)
    return _hip.lib().mi_moe_grouped_gemm_w8(FAKE, FAKE, FAKE, a["D"], a["T"], a["D"], a["F"], a["E"], a["k"], a["tab"], a["stab"], FAKE, FAKE,
                                             a["scratch"], a["nbytes"], None)


def test_leaf_argument_checks():
    L = _hip.lib()
    detail = lambda: L.mi_last_error_detail().decode()  # noqa: E731
    for call in (_decode, _grouped):
        assert call(tab=None) == -1 and call(stab=None) == -1 and "scale table" in detail()
        assert call(D=264) == _hip.MI_ERR_SHAPE and "multiples of 16" in detail()
        assert call(F=520) == _hip.MI_ERR_SHAPE
        assert call(k=3) == _hip.MI_ERR_SHAPE
        assert call(F=16400) == _hip.MI_ERR_SHAPE and "too large for the decode combine kernel" in detail()
    assert _decode(out=None) == -1 and _decode(T=9) == -4 and "mi_moe_grouped_gemm_w8" in detail()
    assert _grouped(E=17) == _hip.MI_ERR_SHAPE and _grouped(scratch=None) == -1
    need = L.mi_moe_grouped_gemm_w8_scratch_bytes(16, 272, 528, 4, 2)
    plain = L.mi_moe_grouped_gemm_scratch_bytes(16, 272, 528, 4, 2)
    images = 4 * 2 * 528 * 272 * 2  # the larger family, W1 | W3, of every expert as bf16
    assert images <= need - plain <= images + 2 * 256 + 16 * 3 * 8, (need, plain)
    assert _grouped(nbytes=need - 1) == -3


def _model(**kw):
    layers = (_hip.MiLayer * 2)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 2
    m.num_experts, m.top_k, m.norm_eps = 4, 2, 1e-5
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    for k, v in kw.items():
        setattr(m, k, v)
    return m, layers


def test_forward_entry_refusals_and_workspace():
    L = _hip.lib()
    detail = lambda: L.mi_last_error_detail().decode()  # noqa: E731
    scales, experts, bt, vo = (_hip.MiW8Layer * 2)(), (_hip.MiMoeW8Layer * 2)(), _hip.MiBatch(), _hip.MiVerifyOut()
    w8 = _hip.MiW8Model()
    w8.format, w8.layers = _hip.MI_W8_FP8_E4M3, C.cast(scales, C.POINTER(_hip.MiW8Layer))
    fwd = lambda m, q=w8, ex=experts, v=None, a8=0: L.mi_forward_moe_w8(C.byref(m), C.byref(q), ex, None, C.byref(bt), v, a8, None)  # noqa: E731
    moe, _k = _model()
    assert L.mi_forward_w8(C.byref(moe), C.byref(w8), C.byref(bt), None) == -4 and "the experts stay bf16" in detail()  # as ever
    assert fwd(moe, ex=None) == -1
    w4 = _hip.MiW8Model()
    w4.format, w4.layers = _hip.MI_W4_MXFP4, w8.layers
    assert fwd(moe, q=w4) == -4 and "MXFP4 experts" in detail()
    lora, _k2 = _model(lora_rank=8, lora_scaling=2.0)
    assert fwd(lora) == -4 and "LoRA" in detail()
    assert fwd(moe, a8=1) == -4 and "prefill" in detail()
    assert fwd(moe, v=C.byref(vo)) == -4 and "verify step" in detail()
    dense, _k3 = _model(num_experts=0, top_k=0)
    assert fwd(dense) == -1 and "dense model" in detail()
    odd, _k4 = _model(hidden_dim=1032)
    assert fwd(odd) == _hip.MI_ERR_SHAPE
    assert fwd(moe) == -1 and "batch" in detail()               # the checks passed: the empty batch is next
    for T, B, W in ((1, 1, 16), (3, 3, 4096), (12, 1, 16)):
        base = L.mi_workspace_bytes_kv(C.byref(moe), 1, T, B, W, 0)
        extra = L.mi_workspace_bytes_moe_w8(C.byref(moe), C.byref(w8), experts, None, T, B, W, 0) - base
        assert extra == (0 if T <= 8 else 4 * 2 * 1024 * 512 * 2 + 512), (T, extra)  # the images and the pointer table, T > 8 only
        assert L.mi_workspace_bytes(C.byref(moe), T, B, W) == L.mi_workspace_bytes_kv(C.byref(moe), 0, T, B, W, 0)
