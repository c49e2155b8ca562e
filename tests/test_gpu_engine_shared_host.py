"""The engine's host side is compiled once (csrc/decode_engine_host.hip): what a debug setter stores is stored once and every
build's launch reads it.  One trace buffer, registered once, receives the timeline of a decode step that the default object
runs (engine variant 2) and of the next step, which the wide object runs (variant 1) - both keep their stamp sites - and both
steps compute the launch path's bits.  The holders knob is covered by test_gpu_engine.py::test_holder_waves_fingerprint.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TR_CONS, TR_EVENTS, ENG_MAXL = 18, 26, 32  # csrc/kernels.h: consumer events [0, TR_CONS), loader events [TR_CONS, TR_EVENTS)


def test_one_trace_buffer_set_once_serves_the_default_and_the_wide_object():
    import mistral_oracle as mo
    import test_engine_route as route
    import test_gpu_engine as g
    from mistral_inference import _hip
    L = _hip.lib()
    p = g.WIDE_SHAPES["gqa4_window_wraps"]  # the smallest shape that both objects take
    n_layers, steps, prompt_len = p["n_layers"], 2, 40
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    variants = (2, 1)
    assert [route._route(p, cus, v, 0) for v in variants] == ["default", "wide"]
    m, _ = g._model(mo.OracleArgs(**p), seed=17)
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(3)).cuda()
    ref, ref_rings, _ = g._run(m, ids, prompt_len, steps, engine=False)

    buf = torch.zeros(L.mi_debug_engine_trace_bytes() // 8, dtype=torch.int64, device="cuda")
    prev_engine = _hip.set_decode_engine(True)
    prev_variant = L.mi_debug_set_engine_variant(variants[0])
    try:
        c = g._cache(m, prompt_len + steps + 2)
        m.forward(ids[:prompt_len], [prompt_len], c)
        torch.cuda.synchronize()
        L.mi_debug_set_engine_trace(buf.data_ptr())  # once, for both steps
        for i, variant in enumerate(variants):
            L.mi_debug_set_engine_variant(variant)
            before = _hip.decode_engine_status(m._backend._workspace)["engine_launches"]
            out = m.forward(ids[prompt_len + i:prompt_len + i + 1], [1], c)[0].clone()
            torch.cuda.synchronize()
            st = _hip.decode_engine_status(m._backend._workspace)
            assert st["status"] == 0 and st["abort"] == 0 and st["engine_launches"] > before, (variant, st)
            t = buf.view(-1, ENG_MAXL, TR_EVENTS)
            for l in range(n_layers):
                assert bool(t[:, l, :TR_CONS].any()) and bool(t[:, l, TR_CONS:].any()), (variant, l)
            assert not bool(t[:, n_layers:].any()), variant
            buf.zero_()
            assert torch.equal(out, ref[i]), (variant, float((out - ref[i]).abs().max()))
        for l, (k0, v0) in enumerate(ref_rings):
            n = k0.shape[1]
            assert torch.equal(c.cache_k[l][:, :n], k0) and torch.equal(c.cache_v[l][:, :n], v0), l
    finally:
        L.mi_debug_set_engine_trace(None)
        L.mi_debug_set_engine_variant(prev_variant)
        _hip.set_decode_engine(prev_engine)
