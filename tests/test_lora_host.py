"""Host side of un-merged LoRA (mistral_inference/lora.py, Transformer.load_lora on a model with `args.lora`, ABI v8 argument
checks).  No GPU: modules are built on the CPU, and the library validates before any device work."""
import ctypes as C

import pytest
import torch

from lora_util import BF, linear_dims, make_adapters

TINY = dict(dim=256, n_layers=2, head_dim=128, hidden_dim=512, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=64)


def _args(rank=8, **over):
    from mistral_inference.args import TransformerArgs
    a = TransformerArgs.from_dict(dict(TINY, lora=dict(rank=rank, scaling=2.0), **over))
    a.max_batch_size = 2
    return a


def _model(rank=8, **kw):
    from mistral_inference.transformer import Transformer
    return Transformer(_args(rank), **kw).to(BF)


def _base_state(prefix_linear: bool):
    g = torch.Generator().manual_seed(0)
    sd = {"tok_embeddings.weight": torch.randn(64, 256, generator=g).to(BF), "norm.weight": torch.ones(256, dtype=BF),
          "output.weight": torch.randn(64, 256, generator=g).to(BF)}
    for layer in range(2):
        sd[f"layers.{layer}.attention_norm.weight"] = torch.ones(256, dtype=BF)
        sd[f"layers.{layer}.ffn_norm.weight"] = torch.ones(256, dtype=BF)
        for name, (fin, fout) in linear_dims(TINY).items():
            key = f"layers.{layer}.{name}." + ("linear.weight" if prefix_linear else "weight")
            sd[key] = torch.randn(fout, fin, generator=g).to(BF)
    return sd


def test_module_path_and_parameter_names_are_the_references():
    from mistral_inference import args, lora
    assert lora.LoraArgs is args.LoraArgs
    m = lora.LoRALinear(256, 512, rank=16, scaling=2.0)
    assert sorted(n for n, _ in m.named_parameters()) == ["linear.weight", "lora_A.weight", "lora_B.weight"]
    assert m.lora_A.weight.shape == (16, 256) and m.lora_B.weight.shape == (512, 16) and m.linear.weight.shape == (512, 256)
    model = _model()
    n = sum(isinstance(x, lora.LoRALinear) for x in model.modules())
    assert n == 14 and not isinstance(model.output, lora.LoRALinear)     # the LM head has no adapter


@pytest.mark.parametrize("prefix_linear", [False, True])
def test_both_key_forms_load_and_absent_adapters_are_not_missing(prefix_linear):
    model = _model()
    sd = _base_state(prefix_linear)
    model.load_state_dict(sd, strict=True, assign=True)      # no "missing keys" error although no lora_* key is given
    wq = model.layers["0"].attention.wq
    src = sd["layers.0.attention.wq." + ("linear.weight" if prefix_linear else "weight")]
    assert torch.equal(wq.linear.weight, src) and torch.equal(wq.weight, src)
    if not prefix_linear:  # lora.py:76-89: the plain key form zero-initialises the adapters
        for mod in model.modules():
            if hasattr(mod, "lora_A"):
                assert not mod.lora_A.weight.any() and not mod.lora_B.weight.any()
                assert mod.lora_A.weight.dtype == BF
    with pytest.raises(ValueError, match="Unexpected key"):
        model.load_state_dict(dict(sd, bogus=torch.zeros(1)), strict=True, assign=True)


def test_load_lora_assigns_in_place_and_swaps():
    model = _model()
    model.load_state_dict(_base_state(False), strict=True, assign=True)
    params = dict(model.named_parameters())
    ptrs = {k: v.data_ptr() for k, v in params.items()}
    base = {k: v.clone() for k, v in params.items() if "lora" not in k}
    one, two = make_adapters(TINY, 8, seed=1), make_adapters(TINY, 8, seed=2)
    model._load_lora_state_dict(one, scaling=123.0)          # `scaling` is ignored in this branch, as in the reference
    assert all(torch.equal(params[k], v) for k, v in one.items())
    assert model.layers["1"].feed_forward.w2.scaling == 2.0
    model._load_lora_state_dict(two)
    assert all(torch.equal(params[k], v) for k, v in two.items())
    assert {k: v.data_ptr() for k, v in params.items()} == ptrs          # copy_, never a rebind
    assert all(torch.equal(params[k], v) for k, v in base.items())       # base weights untouched


def test_load_lora_keeps_the_three_assertions_and_names_a_misfit_key():
    model = _model()
    good = make_adapters(TINY, 8, seed=1)
    k0 = "layers.0.attention.wq.lora_A.weight"
    with pytest.raises(AssertionError, match="multiple different dtypes"):
        model._load_lora_state_dict(dict(good, **{k0: good[k0].float()}))
    with pytest.raises(AssertionError, match="dtype differs"):
        model._load_lora_state_dict({k: v.float() for k, v in good.items()})
    with pytest.raises(AssertionError):
        model._load_lora_state_dict({"layers.0.attention.wq.weight": torch.zeros(512, 256, dtype=BF)})   # not a lora key
    with pytest.raises(AssertionError, match="layers.0.attention.wq.lora_A.weight.*rank 8"):
        model._load_lora_state_dict(make_adapters(TINY, 16, seed=1))                                     # rank mismatch
    with pytest.raises(AssertionError, match="layers.1.feed_forward.w9.lora_B.weight"):
        model._load_lora_state_dict({"layers.1.feed_forward.w9.lora_B.weight": torch.zeros(256, 8, dtype=BF)})


def test_pipeline_rank_keeps_only_its_layers_adapter_keys():
    model = _model(pipeline_rank=1, num_pipeline_ranks=2)
    assert list(model.layers) == ["1"]
    sd = _base_state(True)
    sd.update(make_adapters(TINY, 8, seed=3))                # both layers' adapters, in the un-merged checkpoint form
    model.load_state_dict(sd, strict=True, assign=True)
    names = [n for n, _ in model.named_parameters()]
    assert any("layers.1.attention.wq.lora_A" in n for n in names) and not any(n.startswith("layers.0.") for n in names)
    assert torch.equal(model.layers["1"].attention.wv.lora_B.weight, sd["layers.1.attention.wv.lora_B.weight"])
    model._load_lora_state_dict(make_adapters(TINY, 8, seed=4))          # layer 0's keys are skipped, not an error
    assert torch.equal(model.layers["1"].attention.wv.lora_B.weight, make_adapters(TINY, 8, seed=4)["layers.1.attention.wv.lora_B.weight"])


def test_refused_combinations_say_which_one():
    from mistral_inference import _hip
    from mistral_inference.transformer import Transformer
    with pytest.raises(NotImplementedError, match="MoE"):
        Transformer(_args(moe=dict(num_experts=4, num_experts_per_tok=2)))
    with pytest.raises(NotImplementedError, match="rank 12"):
        Transformer(_args(rank=12))
    with pytest.raises(NotImplementedError, match="fp16 / fp32"):
        x = torch.zeros(2, 256)
        _hip.lora_linear(x, (torch.zeros(8, 256),), (None,), (None,), 2.0)
    # fp16 / fp32 storage is refused where the dtype becomes known: from_folder(dtype=...), before any file is read (a model
    # cast by hand afterwards is refused at its first forward, when the native layer table is built)
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(d + "/params.json", "w") as f:
            json.dump(dict(TINY, lora=dict(rank=8, scaling=2.0)), f)
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match="fp16 / fp32 storage") as e:
                Transformer.from_folder(d, device="cpu", dtype=dt)
            assert "MoE" not in str(e.value) and "shape" not in str(e.value)
    # the library itself: MoE, the generic (fp16 / fp32) entry and rank 12, before any device work
    L = _hip.lib()
    layers = (_hip.MiLayer * 1)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 256, 4, 2, 128, 512, 64, 1
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    bt = _hip.MiBatch()
    m.lora_rank, m.lora_scaling = 12, 2.0
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == _hip.MI_ERR_SHAPE and b"rank 12" in L.mi_last_error_detail()
    m.lora_rank = 72
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == _hip.MI_ERR_SHAPE and b"rank 72" in L.mi_last_error_detail()
    m.lora_rank = 16
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1             # a valid LoRA model, empty batch -> MI_ERR_ARG
    for dt in (0, 1, 2):
        assert L.mi_forward_generic(C.byref(m), C.byref(bt), dt, None) == -4
        d = L.mi_last_error_detail()
        assert b"fp16 / fp32" in d and b"MoE" not in d
    m.num_experts, m.top_k = 8, 2
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -4
    d = L.mi_last_error_detail()
    assert b"MoE" in d and b"fp16" not in d
    m.lora_rank = 0
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1 and L.mi_forward_generic(C.byref(m), C.byref(bt), 0, None) == -1


def _leaf(L, _hip, **over):
    kw = dict(out=1, ldo=384, x=1, ldx=256, M=4, K=256, w=(1, 1, 1), n_rows=(256, 64, 64), epi=0, residual=None, norm_w=None,
              A=(1, 1, 1), B=(1, 1, 1), rank=16, scaling=2.0, scratch=1, scratch_bytes=1 << 30)
    kw.update(over)
    vp = _hip._vp
    rc = L.mi_lora_linear(kw["out"], kw["ldo"], kw["x"], kw["ldx"], kw["M"], kw["K"], (vp * 3)(*kw["w"]), (C.c_int * 3)(*kw["n_rows"]),
                          kw["epi"], kw["residual"], kw["norm_w"], 1e-5, (vp * 3)(*kw["A"]), (vp * 3)(*kw["B"]), kw["rank"],
                          kw["scaling"], kw["scratch"], kw["scratch_bytes"], None)
    return rc, L.mi_last_error_detail().decode()


def test_leaf_entry_points_refuse_bad_arguments_before_any_device_work():
    from mistral_inference import _hip
    L = _hip.lib()
    assert _leaf(L, _hip, out=None) == (-1, "mi_lora_linear")
    assert _leaf(L, _hip, K=250)[0] == -1 and _leaf(L, _hip, ldx=250)[0] == -1 and _leaf(L, _hip, scratch=None)[0] == -1
    rc, d = _leaf(L, _hip, rank=12)
    assert rc == _hip.MI_ERR_SHAPE and "rank 12" in d
    rc, d = _leaf(L, _hip, rank=128)
    assert rc == _hip.MI_ERR_SHAPE and "rank 128" in d
    rc, d = _leaf(L, _hip, epi=3)
    assert rc == -1 and "LM head" in d
    rc, d = _leaf(L, _hip, epi=1)
    assert rc == -1 and "residual" in d
    rc, d = _leaf(L, _hip, epi=2, n_rows=(256, 64, 0))
    assert rc == -1 and "swiglu" in d
    rc, d = _leaf(L, _hip, A=(1, None, 1))
    assert rc == -1 and "adapter 1" in d
    rc, d = _leaf(L, _hip, scaling=0.0)
    assert rc == -1 and "scaling" in d
    rc, d = _leaf(L, _hip, M=9, norm_w=1)
    assert rc == -4 and "RMSNorm" in d
    rc, d = _leaf(L, _hip, scratch_bytes=64)
    assert rc == -3 and "scratch 64 < required" in d
    nr = (C.c_int * 3)(256, 64, 64)
    size = L.mi_lora_linear_scratch_bytes
    assert size(4, 256, nr, 0, 12, 0) == 0 and size(0, 256, nr, 0, 16, 0) == 0 and size(4, 256, None, 0, 16, 0) == 0
    need = size(4, 256, nr, 0, 16, 0)
    assert need >= 4 * 384 * 2 + 4 * 48 * 2
    assert size(4, 256, nr, 0, 16, 1) >= need + 4 * 256 * 2            # the normalised rows
    assert size(300, 256, nr, 0, 64, 0) > size(9, 256, nr, 0, 64, 0) > need
    assert _leaf(L, _hip, scratch_bytes=need - 1)[0] == -3


def test_workspace_grows_only_for_a_lora_model():
    from mistral_inference import _hip
    L = _hip.lib()
    layers = (_hip.MiLayer * 1)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 1
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    for T, B, W in ((1, 1, 64), (8, 8, 64), (9, 9, 4096), (300, 3, 4096)):
        m.lora_rank = 0
        plain = L.mi_workspace_bytes(C.byref(m), T, B, W)
        m.lora_rank = 64
        lora = L.mi_workspace_bytes(C.byref(m), T, B, W)
        assert lora >= plain + T * 3 * 64 * 2 + T * 2 * 1024 * 2, (T, plain, lora)
    assert C.sizeof(_hip.MiLoraLayer) == 14 * C.sizeof(C.c_void_p)
