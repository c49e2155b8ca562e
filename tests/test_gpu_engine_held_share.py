"""Round 7 of the headline engine build (decode_engine_next.o, build_native.ENGINE_NEXT_FLAGS): the holder waves fetch their W1|W3
units while the loader waits for a free ring slot or once the layer's Wo rows are issued (ENG_HOLD_GATE), and whatever the
loader does once ffn_norm(h1) stands in LDS.  The contract stays bit equality with the launch path, whatever the timing: at the
headline widths (28 units per CU, three whole units held), at 12 units per CU, at 8 units per CU (holder_units() declines:
no holders), and with a short ring right after a short prefill, where the loader may never wait for a ring slot and the holders
must still fetch before the hid values are due.  Every shape here is one decode_engine_next.o accepts (dim, n_heads * 128 and
hidden_dim multiples of 2048); each test also shows that it was that object which ran (_engine_object).
"""
import pytest
import torch

import mistral_oracle as mo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _model(args: mo.OracleArgs, seed: int):
    from mistral_inference.args import TransformerArgs
    from mistral_inference.transformer import Transformer
    w = mo.synth_weights(args, seed=seed)
    targs = TransformerArgs.from_dict(mo.params_json(args))
    targs.max_batch_size = 1
    with torch.device("meta"):
        m = Transformer(targs)
    m = m.to(BF).to_empty(device="cuda")
    m.load_state_dict({k: v.cuda() for k, v in w.items()}, assign=True)
    return m.eval()


def _engine_object(m, ids, prompt_len):
    """Which engine object runs a decode step of `m`: 'next' or 'other'.  A trace buffer is registered with every engine object;
    the default (frozen), wide and MoE objects keep their stamp sites (ENG_TRACE = 1) and write the step's timeline into it,
    decode_engine_next.o is compiled without them (ENG_TRACE = 0) and leaves it untouched."""
    from mistral_inference import _hip
    from mistral_inference.cache import BufferCache
    L = _hip.lib()
    prev = _hip.set_decode_engine(True)
    try:
        a = m.args
        c = BufferCache(m.n_local_layers, 1, prompt_len + 4, a.n_kv_heads, a.head_dim, a.sliding_window, device="cuda", dtype=BF)
        c.reset()
        m.forward(ids[:prompt_len], [prompt_len], c)
        torch.cuda.synchronize()
        before = _hip.decode_engine_status(m._backend._workspace)["engine_launches"]
        buf = torch.zeros(L.mi_debug_engine_trace_bytes() // 8, dtype=torch.int64, device="cuda")
        L.mi_debug_set_engine_trace(buf.data_ptr())
        try:
            m.forward(ids[prompt_len:prompt_len + 1], [1], c)
            torch.cuda.synchronize()
        finally:
            L.mi_debug_set_engine_trace(None)
        st = _hip.decode_engine_status(m._backend._workspace)
        assert st["status"] == 0 and st["engine_launches"] > before, st  # an engine object ran the step
        return "other" if bool(buf.any()) else "next"
    finally:
        _hip.set_decode_engine(prev)


def _run(m, ids, prompt_len, steps, engine: bool, graph: bool = False):
    """Prefill `prompt_len` tokens (launch path), then `steps` teacher-forced decode steps: logits, written K/V slots, status."""
    from mistral_inference import _hip
    from mistral_inference.cache import BufferCache
    prev = _hip.set_decode_engine(engine)
    try:
        a = m.args
        c = BufferCache(m.n_local_layers, 1, prompt_len + steps + 2, a.n_kv_heads, a.head_dim, a.sliding_window, device="cuda", dtype=BF)
        c.reset()
        m.forward(ids[:prompt_len], [prompt_len], c)
        outs = []
        if graph:
            with m.graphed_decode(c):
                for i in range(steps):
                    outs.append(m.forward(ids[prompt_len + i:prompt_len + i + 1], [1], c)[0].clone())
        else:
            for i in range(steps):
                outs.append(m.forward(ids[prompt_len + i:prompt_len + i + 1], [1], c)[0].clone())
        torch.cuda.synchronize()
        st = _hip.decode_engine_status(m._backend._workspace)
        rings = []
        for l in range(m.n_local_layers):
            n = min(c.cache_sizes[l], prompt_len + steps)
            rings.append((c.cache_k[l][:, :n].clone(), c.cache_v[l][:, :n].clone()))
        return outs, rings, st
    finally:
        _hip.set_decode_engine(prev)


def _check_equal(name, ref, ref_rings, got, got_rings):
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.isfinite(b).all(), (name, i)
        assert torch.equal(a, b), (name, i, float((a - b).abs().max()))
    for l, ((k0, v0), (k1, v1)) in enumerate(zip(ref_rings, got_rings)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1), (name, l)


# dense GQA-4 shapes with rows of 4-piece groups: routed to decode_engine_next.o.  W1|W3 units per CU = hidden_dim / 2 / 256.
HELD_SHAPES = {
    # the headline widths: 28 units per CU, three held, 25 from the ring
    "headline_widths": dict(dim=4096, n_layers=2, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5,
                            vocab_size=2048, sliding_window=64),
    # 12 units per CU, three held
    "units_12": dict(dim=2048, n_layers=3, head_dim=128, hidden_dim=6144, n_heads=16, n_kv_heads=4, norm_eps=1e-5,
                     vocab_size=1000, sliding_window=48),
    # 8 units per CU: fewer than holder_units() needs (11) - no holders, every unit from the ring
    "units_8_declined": dict(dim=2048, n_layers=2, head_dim=128, hidden_dim=4096, n_heads=16, n_kv_heads=4, norm_eps=1e-5,
                             vocab_size=514, sliding_window=48),
}


@pytest.mark.parametrize("name", sorted(HELD_SHAPES))
def test_held_share_bit_equal_launch_path_and_frozen_build(name):
    from mistral_inference import _hip
    p = HELD_SHAPES[name]
    m = _model(mo.OracleArgs(**p), seed=29)
    prompt_len, steps = 40, 14  # + 14 steps crosses the ring end
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(5)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    ref, ref_rings, st0 = _run(m, ids, prompt_len, steps, engine=False)
    got, got_rings, st1 = _run(m, ids, prompt_len, steps, engine=True)
    prev = _hip.lib().mi_debug_set_engine_variant(2)  # the frozen default object (round-3 holders)
    try:
        assert _engine_object(m, ids, prompt_len) == "other"  # (the probe tells the two objects apart)
        frozen, frozen_rings, st2 = _run(m, ids, prompt_len, steps, engine=True)
    finally:
        _hip.lib().mi_debug_set_engine_variant(prev)
    assert st1["status"] == 0 and st1["abort"] == 0 and st2["status"] == 0, (st1, st2)
    assert st1["engine_launches"] - st0["engine_launches"] >= steps
    _check_equal(name, ref, ref_rings, got, got_rings)
    _check_equal(name + "/frozen", ref, ref_rings, frozen, frozen_rings)


@pytest.mark.parametrize("prompt_len", [1, 5])
def test_short_ring_right_after_short_prefill(prompt_len):
    """A ring of prompt_len + steps + 2 slots (13 or 17) that starts nearly empty: the attention block is short, the loader may
    never find the ring full, and the holders' fetch must not depend on that signal (it falls back to the Wo stage / the hid
    deadline)."""
    p = dict(HELD_SHAPES["headline_widths"], sliding_window=4096)
    m = _model(mo.OracleArgs(**p), seed=31)
    steps = 10
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(6)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    ref, ref_rings, _ = _run(m, ids, prompt_len, steps, engine=False)
    got, got_rings, st = _run(m, ids, prompt_len, steps, engine=True)
    assert st["status"] == 0 and st["abort"] == 0 and st["engine_launches"] >= steps, st
    _check_equal(f"short_ring_{prompt_len}", ref, ref_rings, got, got_rings)


def test_status_word_clean_after_multi_step_graph_run():
    """60 graph-replayed steps across the ring end at the headline widths: no spin of any role timed out (status and abort
    words 0), every step ran on the engine, and the results are the launch path's."""
    p = HELD_SHAPES["headline_widths"]
    m = _model(mo.OracleArgs(**p), seed=37)
    prompt_len, steps = 20, 60
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(7)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    ref, ref_rings, st0 = _run(m, ids, prompt_len, steps, engine=False)
    got, got_rings, st = _run(m, ids, prompt_len, steps, engine=True, graph=True)
    assert st["status"] == 0 and st["abort"] == 0, st
    assert st["engine_launches"] - st0["engine_launches"] >= steps, (st0, st)
    _check_equal("graph_60_steps", ref, ref_rings, got, got_rings)
