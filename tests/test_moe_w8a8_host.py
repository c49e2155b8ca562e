"""Token-grouped W8A8 prefill GEMMs on FP8 experts, on the host: the new symbols, the leaf's own argument checks (fake pointers,
codes checked before any launch), the scratch and workspace formulas, and the refusals of `prefill_fp8_experts` by name."""
import ctypes as C
import json
import os

import pytest
import torch

from mistral_inference import _hip, quant
from mistral_inference.args import TransformerArgs
from mistral_inference.transformer import Transformer
from test_moe_fp8_host import FAKE, _model

up = lambda n: (n + 255) // 256 * 256  # noqa: E731  (csrc/api.hip align_up)
detail = lambda: _hip.lib().mi_last_error_detail().decode()  # noqa: E731


def _leaf(fn="mi_moe_grouped_gemm_w8a8", **kw):
    a = dict(x=FAKE, tab=FAKE, stab=FAKE, T=300, D=384, F=640, E=4, k=2, nbytes=1 << 40)
    a.update(kw)
    return getattr(_hip.lib(), fn)(FAKE, FAKE, a["x"], a["D"], a["T"], a["D"], a["F"], a["E"], a["k"], a["tab"], a["stab"], FAKE, FAKE,
                                   FAKE, a["nbytes"], None)


def test_symbols_leaf_argument_checks_and_scratch():
    L = _hip.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "mistral_hip.h")).read()
    for name in ("mi_moe_grouped_gemm_w8a8_scratch_bytes", "mi_moe_grouped_gemm_w8a8", "mi_workspace_bytes_moe_w8a8", "mi_forward_moe_w8a8"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(L, name) and f" {name}(" in header, name
    assert L.mi_abi_version() == 9
    assert _leaf(tab=None) == -1 and _leaf(stab=None) == -1 and "scale table" in detail()
    assert _leaf(x=C.c_void_p(0x1008)) == -1 and "16-byte aligned" in detail()
    for kw in (dict(D=264), dict(T=255, F=520), dict(T=16, k=3)):    # outside the predicate: mi_moe_grouped_gemm_w8's errors, never a new one
        assert _leaf(**kw) == _leaf("mi_moe_grouped_gemm_w8", **kw) == _hip.MI_ERR_SHAPE, kw
    T, D, F, E, k = 300, 384, 640, 4, 2
    need = L.mi_moe_grouped_gemm_w8a8_scratch_bytes(T, D, F, E, k)
    extra = need - L.mi_moe_grouped_gemm_scratch_bytes(T, D, F, E, k)
    assert extra == up(T * D) + up(T * 4) + up(T * k * F) + up(T * k * 4) < E * 2 * F * D * 2    # x_q | s_x | h_q | s_h, no images
    assert _leaf(nbytes=need - 1) == -3


def test_workspace_at_300_rows_is_the_w8_figure_less_the_images():
    scales, experts, w8 = (_hip.MiW8Layer * 2)(), (_hip.MiMoeW8Layer * 2)(), _hip.MiW8Model()
    w8.format, w8.layers = _hip.MI_W8_FP8_E4M3, C.cast(scales, C.POINTER(_hip.MiW8Layer))
    moe, _k = _model()
    q = lambda fn, T: getattr(_hip.lib(), fn)(C.byref(moe), C.byref(w8), experts, None, T, 1, 16, 0)  # noqa: E731
    # T = 300, dim 512, hidden 1024, E = 4, k = 2: the pointer table and the images leave; x_q [T, 1024] | s_x | h_q [T k, F] | s_h come
    assert q("mi_workspace_bytes_moe_w8", 300) - q("mi_workspace_bytes_moe_w8a8", 300) == \
        512 + 4 * 2 * 1024 * 512 * 2 - (up(300 * 1024) + up(300 * 4) + up(600 * 1024) + up(600 * 4))


def test_switch_refusals_by_name(tmp_path):
    """Every refusal comes before anything but params.json is read; switching it off leaves a dense FP8 model's `prefill_fp8` on."""
    base = dict(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512)
    moe, fp8 = dict(num_experts=4, num_experts_per_tok=2), dict(qformat_weight="fp8_e4m3")
    kinds = {"bf16": dict(base, moe=moe), "dense": dict(base, quantization=fp8), "mxfp4": dict(base, quantization=dict(qformat_weight="mxfp4")),
             "fp8moe": dict(base, moe=moe, quantization=dict(fp8, experts=True))}
    for name, params in kinds.items():
        os.makedirs(tmp_path / name)
        json.dump(params, open(tmp_path / name / "params.json", "w"))
    load = lambda n, **kw: Transformer.from_folder(tmp_path / n, device="cpu", **kw)  # noqa: E731
    for name, dtype, what in (("bf16", None, "a model without FP8 weights"), ("dense", None, "a dense model"), ("mxfp4", None, "MXFP4 weights"),
                              ("bf16", torch.float16, "a model with torch.float16 storage"), ("fp8moe", torch.float16, "torch.float16 storage")):
        with pytest.raises(NotImplementedError, match=f"prefill_fp8_experts=True on {what}"):
            load(name, prefill_fp8_experts=True, dtype=dtype)
    with pytest.raises(NotImplementedError, match="prefill_fp8=True on a MoE model with FP8 experts is not implemented .there is no token-grouped"):
        load("fp8moe", prefill_fp8=True)                          # today's message, word for word
    with torch.device("meta"):
        dense = Transformer(TransformerArgs.from_dict(kinds["dense"]))
    dense.prefill_fp8, dense.prefill_fp8_experts = True, False   # from_folder's order on every model
    assert dense.prefill_fp8 and all(m.prefill_fp8 for m in dense.modules() if isinstance(m, quant.Fp8Linear))
