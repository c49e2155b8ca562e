"""Host side of adapter banks (several LoRA adapters in one batch, ABI v9): what is decided before any launch.  No GPU: modules
are built on the CPU, and the library validates before any device work."""
import ctypes as C
import os
import re

import pytest
import torch

from lora_util import BF, make_adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(dim=256, n_layers=2, head_dim=128, hidden_dim=512, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=64)


def _model(lora=True, max_batch_size=3):
    from mistral_inference.args import TransformerArgs
    from mistral_inference.transformer import Transformer
    a = TransformerArgs.from_dict(dict(TINY, **(dict(lora=dict(rank=8, scaling=2.0)) if lora else {})))
    a.max_batch_size = max_batch_size
    return Transformer(a).to(BF)


def test_abi_version_is_9_on_both_sides():
    from mistral_inference import _hip
    header = open(os.path.join(ROOT, "include", "mistral_hip.h")).read()
    assert int(re.search(r"#define MI_ABI_VERSION (\d+)", header).group(1)) == 9
    assert _hip.MI_ABI_VERSION == 9 and _hip.lib().mi_abi_version() == 9
    assert "mi_lora_linear_slots" in _hip.EXPORTED_SYMBOLS
    assert _hip.MiModel._fields_[-1][0] == "lora_slots" and _hip.MiBatch._fields_[-1][0] == "seq_adapter"   # appended, not inserted


def test_set_lora_slots_keeps_names_shapes_and_slot_0():
    from mistral_inference.lora import LoRALinear
    model = _model()
    model._load_lora_state_dict(make_adapters(TINY, 8, seed=1))
    names = {k: tuple(v.shape) for k, v in model.named_parameters()}
    before = {k: v.clone() for k, v in model.state_dict().items()}
    base_ptrs = {k: v.data_ptr() for k, v in model.named_parameters() if "lora" not in k}
    model.set_lora_slots(3)
    assert model.lora_slots == 3
    assert {k: tuple(v.shape) for k, v in model.named_parameters()} == names
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
    assert {k: v.data_ptr() for k, v in model.named_parameters() if "lora" not in k} == base_ptrs   # base weights do not move
    mods = [m for m in model.modules() if isinstance(m, LoRALinear)]
    assert len(mods) == 14
    for m in mods:
        assert tuple(m.bank_A.shape) == (3, 8, m.in_features) and tuple(m.bank_B.shape) == (3, m.out_features, 8)
        assert m.bank_A.is_contiguous() and m.bank_B.is_contiguous()
        assert m.lora_A.weight.data_ptr() == m.bank_A.data_ptr() and m.lora_B.weight.data_ptr() == m.bank_B.data_ptr()   # views of slot 0
        assert not m.bank_A[1:].any() and not m.bank_B[1:].any()
    # slot 0 through the old door, slot 2 through the new one; neither disturbs the other
    two, three = make_adapters(TINY, 8, seed=2), make_adapters(TINY, 8, seed=3)
    model._load_lora_state_dict(two)
    model._load_lora_state_dict(three, slot=2)
    wq = model.layers["1"].attention.wq
    k = "layers.1.attention.wq.lora_"
    assert torch.equal(wq.bank_A[0], two[k + "A.weight"]) and torch.equal(wq.lora_B.weight, two[k + "B.weight"])
    assert torch.equal(wq.bank_A[2], three[k + "A.weight"]) and torch.equal(wq.bank_B[2], three[k + "B.weight"])
    assert not wq.bank_A[1].any()
    # a cast / move takes the bank along and keeps the parameters views of it
    model.to(torch.float32)
    assert wq.bank_A.dtype == torch.float32 and wq.lora_A.weight.data_ptr() == wq.bank_A.data_ptr()
    assert torch.equal(wq.bank_B[2], three[k + "B.weight"].float())


def test_set_lora_slots_again_keeps_the_slots_both_banks_have():
    model = _model()
    model.set_lora_slots(3)
    sets = [make_adapters(TINY, 8, seed=s) for s in (1, 2, 3)]
    for slot, sd in enumerate(sets):
        model._load_lora_state_dict(sd, slot=slot)
    wq, k = model.layers["1"].attention.wq, "layers.1.attention.wq.lora_"
    model.set_lora_slots(4)   # grow: 0..2 kept, 3 zero
    assert model.lora_slots == 4 and tuple(wq.bank_A.shape) == (4, 8, wq.in_features)
    for slot, sd in enumerate(sets):
        assert torch.equal(wq.bank_A[slot], sd[k + "A.weight"]) and torch.equal(wq.bank_B[slot], sd[k + "B.weight"]), slot
    assert not wq.bank_A[3].any() and not wq.bank_B[3].any()
    assert wq.lora_A.weight.data_ptr() == wq.bank_A.data_ptr()
    model.set_lora_slots(2)   # shrink: 0..1 kept
    assert tuple(wq.bank_B.shape) == (2, wq.out_features, 8)
    assert torch.equal(wq.bank_A[1], sets[1][k + "A.weight"]) and torch.equal(wq.lora_B.weight, sets[0][k + "B.weight"])


def test_slot_and_adapter_arguments_are_refused_before_any_launch(tmp_path):
    from safetensors.torch import save_file
    from mistral_inference.generate import generate
    path = tmp_path / "a.safetensors"
    save_file(make_adapters(TINY, 8, seed=1), str(path))
    ids = torch.tensor([1, 2, 3, 4, 5])
    plain = _model(lora=False)
    with pytest.raises(ValueError, match="slot"):
        plain.load_lora(path, slot=1)                       # the merge form has no slots
    with pytest.raises(ValueError, match="without `lora`"):
        plain.forward(ids, [2, 3], adapters=[0, 0])
    with pytest.raises(ValueError, match="without `lora`"):
        plain.set_lora_slots(2)
    model = _model()
    with pytest.raises(ValueError, match="slot"):
        model.load_lora(path, slot=1)                       # one slot until set_lora_slots
    with pytest.raises(ValueError, match="at least one"):
        model.set_lora_slots(0)
    model.set_lora_slots(3)
    for bad in (3, -1):
        with pytest.raises(ValueError, match="slot"):
            model.load_lora(path, slot=bad)
        with pytest.raises(ValueError, match="slot"):
            model._load_lora_state_dict(make_adapters(TINY, 8, seed=1), slot=bad)
    model.load_lora(path, slot=2)
    assert torch.equal(model.layers["0"].feed_forward.w2.bank_B[2], make_adapters(TINY, 8, seed=1)["layers.0.feed_forward.w2.lora_B.weight"])
    for call in (model.forward, model.forward_partial):
        with pytest.raises(AssertionError, match="3 entries for 2 sequences"):
            call(ids, [2, 3], adapters=[0, 1, 2])
        with pytest.raises(ValueError, match="slot 3 is outside"):
            call(ids, [2, 3], adapters=[0, 3])
        with pytest.raises(ValueError, match="slot -2 is outside"):
            call(ids, [2, 3], adapters=[-2, 0])
    with pytest.raises(ValueError, match="slot 5 is outside"):
        generate([[1, 2], [3, 4, 5]], model, max_tokens=2, temperature=0.0, adapters=[0, 5])
    with pytest.raises(AssertionError, match="1 entries for 2 sequences"):
        generate([[1, 2], [3, 4, 5]], model, max_tokens=2, temperature=0.0, adapters=[0])
    with pytest.raises(ValueError, match="without `lora`"):
        generate([[1, 2]], plain, max_tokens=2, temperature=0.0, adapters=[0])


def _tiny_native(**kw):
    from mistral_inference import _hip
    layers = (_hip.MiLayer * 1)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 256, 4, 2, 128, 512, 64, 1
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    m.final_norm = m.output = 1
    m._keep = layers
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _decode_batch():
    from mistral_inference import _hip
    bt = _hip.MiBatch()
    bt.T = bt.B = 1
    bt.branch, bt.max_q_len = 2, 1
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = bt.kv_seqlens = bt.h = bt.workspace = bt.logits = 1
    bt._keep = ((_hip._vp * 1)(), (_hip._vp * 1)(), (C.c_int32 * 1)(16))
    bt.cache_k, bt.cache_v, bt.cache_sizes = bt._keep[0], bt._keep[1], bt._keep[2]
    bt.workspace_bytes = 64     # too small: a batch that passes every argument check stops here, before any launch
    return bt


def test_native_entries_refuse_before_any_device_work():
    from mistral_inference import _hip
    L = _hip.lib()
    bt = _decode_batch()
    assert L.mi_forward(C.byref(_tiny_native()), C.byref(bt), None) == -3              # the batch itself is acceptable
    bt.seq_adapter = 1
    for entry in ("mi_forward", "mi_forward_generic"):
        m = _tiny_native()
        rc = L.mi_forward(C.byref(m), C.byref(bt), None) if entry == "mi_forward" else L.mi_forward_generic(C.byref(m), C.byref(bt), 0, None)
        assert rc == -1 and b"seq_adapter" in L.mi_last_error_detail(), (entry, rc)
    m = _tiny_native(lora_rank=16, lora_scaling=2.0, lora_slots=3)
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -3                           # a banked LoRA model takes seq_adapter
    m = _tiny_native(lora_slots=3)
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1 and b"lora_slots" in L.mi_last_error_detail()
    m = _tiny_native(lora_rank=16, lora_scaling=2.0, lora_slots=-1)
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1 and b"lora_slots" in L.mi_last_error_detail()
    m = _tiny_native(lora_rank=16, lora_scaling=2.0, lora_slots=3, num_experts=8, top_k=2)
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -4 and b"MoE" in L.mi_last_error_detail()
    m = _tiny_native(lora_rank=16, lora_scaling=2.0, lora_slots=3)
    assert L.mi_forward_generic(C.byref(m), C.byref(bt), 0, None) == -4                # fp16 / fp32 storage: still refused
    # the leaf
    vp = _hip._vp
    def leaf(slots=3, out=1):
        rc = L.mi_lora_linear_slots(out, 384, 1, 256, 4, 256, (vp * 3)(1, 1, 1), (C.c_int * 3)(256, 64, 64), 0, None, None, 1e-5,
                                    (vp * 3)(1, 1, 1), (vp * 3)(1, 1, 1), 16, 2.0, slots, 1, 1, 64, None)
        return rc, L.mi_last_error_detail().decode()
    assert leaf(out=None) == (-1, "mi_lora_linear_slots")
    rc, d = leaf(slots=0)
    assert rc == -1 and "slots 0" in d
    rc, d = leaf()
    assert rc == -3 and "mi_lora_linear_slots: scratch 64 < required" in d
