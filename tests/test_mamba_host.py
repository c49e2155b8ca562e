"""Mamba2 without a GPU: the params.json schema and its named refusals, the model-class choice, the strict loader, and the
shape checks of the C ABI (which run before any launch)."""
import ctypes as C
import json

import pytest
import torch

import mamba_ref as mr
from mistral_inference import _hip
from mistral_inference.args import MambaArgs
from mistral_inference.mamba import Mamba, check_args, map_state_dict


def test_args_round_trip_and_named_refusals():
    p = mr.params(128, 2, 500, 1)
    a = MambaArgs.from_dict(p)
    assert a.to_dict() == p and MambaArgs.from_dict(a.to_dict()) == a
    with pytest.raises(AssertionError):
        MambaArgs.from_dict(dict(p, model_type="transformer"))
    check_args(a, torch.bfloat16, 1)
    for over, name in [({"rms_norm": False}, "rms_norm"), ({"residual_in_fp32": False}, "residual_in_fp32"),
                       ({"tie_embeddings": True}, "tie_embeddings"), ({"dim": 96}, "dim 96"), ({"n_groups": 3}, "n_groups 3")]:
        with pytest.raises(NotImplementedError, match=name):
            check_args(MambaArgs.from_dict(dict(p, **over)), torch.bfloat16, 1)
    with pytest.raises(NotImplementedError, match="float16"):
        check_args(a, torch.float16, 1)
    with pytest.raises(NotImplementedError, match="pipeline"):
        check_args(a, torch.bfloat16, 2)


def test_get_model_cls_picks_the_class_from_params_json(tmp_path):
    from mistral_inference.main import get_model_cls, refuse_transformer_flags
    from mistral_inference.transformer import Transformer
    for kind, cls in [("mamba", Mamba), ("transformer", Transformer), (None, Transformer)]:
        (tmp_path / "params.json").write_text(json.dumps({} if kind is None else {"model_type": kind}))
        assert get_model_cls(str(tmp_path)) is cls
    with pytest.raises(NotImplementedError, match="quantize"):
        refuse_transformer_flags(lora_path=None, quantize="fp8_e4m3", speculative=0)


def test_c_abi_names_the_offending_shape_before_any_launch():
    L = _hip.lib()
    assert hasattr(L, "mi_forward_mamba")  # the feature test of the additive ABI
    m = _hip.MiMambaModel(dim=96, n_layers=1, vocab_size=64, n_groups=1, eps=1e-5)
    bt = _hip.MiMambaBatch()
    assert L.mi_forward_mamba(C.byref(m), C.byref(bt), None) == _hip.MI_ERR_SHAPE and b"dim 96" in L.mi_last_error_detail()
    m.dim, m.n_groups = 128, 3
    assert L.mi_forward_mamba(C.byref(m), C.byref(bt), None) == _hip.MI_ERR_SHAPE and b"n_heads 4 % n_groups 3" in L.mi_last_error_detail()
    assert L.mi_workspace_bytes_mamba(C.byref(m), 1, 4) == 0
    assert L.mi_mamba_scan(1, 1, 1024, 1, 1, 1, 1, 1, 1, 1, 1, 4, 4, 3, None) == _hip.MI_ERR_SHAPE
    assert b"n_heads 4 % n_groups 3" in L.mi_last_error_detail()
    assert L.mi_mamba_scan(1, 1, 770, 1, 1, 1, 1, 1, 1, 1, 1, 4, 4, 1, None) == _hip.MI_ERR_SHAPE and b"ld = 770" in L.mi_last_error_detail()
    m.n_groups = 1
    assert L.mi_forward_mamba(C.byref(m), C.byref(bt), None) == -1  # a valid model, an empty batch: MI_ERR_ARG
    sizes = [L.mi_workspace_bytes_mamba(C.byref(m), 2, n) for n in (1, 2, 64, 65)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))  # grows with L


def test_strict_loader_names_missing_and_unexpected_keys():
    a = MambaArgs.from_dict(mr.params(64, 1, 64, 1))
    sd = mr.state_dict(mr.synth_weights(64, 1, 64, 1, seed=0))
    w = map_state_dict(sd, a)
    assert w["layers"][0]["A_log"].dtype == torch.float32 and w["layers"][0]["conv_w"].dtype == torch.bfloat16
    gone = "model.backbone.layers.0.mixer.dt_bias"
    with pytest.raises(RuntimeError, match=r"missing key\(s\) \['" + gone.replace(".", r"\.")):
        map_state_dict({k: v for k, v in sd.items() if k != gone}, a)
    with pytest.raises(RuntimeError, match=r"unexpected key\(s\) \['model\.extra'\]"):
        map_state_dict(dict(sd, **{"model.extra": torch.zeros(1)}), a)
    with pytest.raises(RuntimeError, match="shape"):
        map_state_dict(dict(sd, **{gone: torch.zeros(3)}), a)
