"""Round 10 of the headline engine build (decode_engine_next.o, ENG_QKV_HOLD=3, ENG_QKV_WAVES=2): two of the three holder waves
carry two duties in turn.  They keep their W1|W3 unit of layer l as before, and from the FFN of layer l on two each of the last
four q|k|v row-pair units of layer l + 1, fetched while the loader waits for a ring slot (run_holder_both), reduced from
registers when attention_norm(h) stands in LDS.  Loader and consumers skip those units.  The contract stays bit equality with
the launch path and with the frozen default object, whatever the timing.

Shapes: the smallest dense GQA-4 ones at which BOTH duties are active (decode_engine.hip holder_units / qkv_held): dim 2048 (rows
of one 4-piece group), 32 / 8 heads = 12 q|k|v units per CU (>= 4 + 6, enough for three waves' worth too; the held ones are
the END of the list q.., k.., v..: ALL k and v units of a CU, so every K/V row a decode step writes comes from a holder wave),
hidden 6144 = 12 W1|W3 units per CU (>= 11).  Each test shows that it was decode_engine_next.o which ran."""
import re

import pytest
import torch

import mistral_oracle as mo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

BOTH = dict(dim=2048, head_dim=128, hidden_dim=6144, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=1000)


def _load(args: mo.OracleArgs, w):
    from mistral_inference.args import TransformerArgs
    from mistral_inference.transformer import Transformer
    targs = TransformerArgs.from_dict(mo.params_json(args))
    targs.max_batch_size = 1
    with torch.device("meta"):
        m = Transformer(targs)
    m = m.to(BF).to_empty(device="cuda")
    dev = {}  # one device copy per distinct host tensor (the 34-layer model repeats two layers' weights)
    m.load_state_dict({k: dev.setdefault(id(v), v.cuda()) for k, v in w.items()}, assign=True)
    return m.eval()


def _model(p, seed, distinct_layers=None):
    """distinct_layers = n: synthesise n layers' weights and repeat them cyclically over p['n_layers'] layers (the deep model
    needs 34 launches' worth of layers, not 34 different ones)."""
    args = mo.OracleArgs(**p)
    if distinct_layers is None:
        return _load(args, mo.synth_weights(args, seed=seed))
    few = mo.synth_weights(mo.OracleArgs(**dict(p, n_layers=distinct_layers)), seed=seed)
    w = {k: v for k, v in few.items() if not k.startswith("layers.")}
    for l in range(p["n_layers"]):
        for k, v in few.items():
            mt = re.match(r"layers\.(\d+)\.(.*)", k)
            if mt and int(mt.group(1)) == l % distinct_layers:
                w[f"layers.{l}.{mt.group(2)}"] = v
    return _load(args, w)


def _engine_object(m, ids, prompt_len):
    """'next' or 'other': decode_engine_next.o has no stamp sites and leaves a registered trace buffer untouched; the default
    (frozen), wide and MoE objects write the step's timeline into it."""
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
        assert st["status"] == 0 and st["engine_launches"] > before, st
        return "other" if bool(buf.any()) else "next"
    finally:
        _hip.set_decode_engine(prev)


def _run(m, ids, prompt_len, steps, engine: bool, graph: bool = False):
    """Prefill (launch path), then `steps` teacher-forced decode steps: logits of every step, the written K/V slots, status."""
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
    assert len(ref) == len(got) and len(ref_rings) == len(got_rings)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.isfinite(b).all(), (name, i)
        assert torch.equal(a, b), (name, i, float((a - b).abs().max()))
    for l, ((k0, v0), (k1, v1)) in enumerate(zip(ref_rings, got_rings)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1), (name, l)


# name: (n_layers, sliding_window, prompt_len, steps, distinct layers or None, launches per step)
CASES = {
    # first, middle and last role of a launch: layer 0 fetches at entry, layer 1 is prefetched and prefetches, layer 2 fetches nothing
    "three_layers": (3, 4096, 9, 8, None, 1),
    # a 48-slot ring: the position crosses the ring end inside the run (slots 40 .. 47, 0 .. 5)
    "ring_wraps": (3, 48, 40, 14, None, 1),
    # two splits of 128 slots: the current slot - whose k and v rows the holder waves write - moves from split 0 into split 1
    "slot_changes_split": (2, 256, 122, 12, None, 1),
    # more layers than one launch takes (32): two launches per step; layer 0 of the SECOND launch has nothing prefetched either,
    # and its holders fetch while that launch's consumers gather h
    "two_launches_34_layers": (34, 40, 30, 12, 2, 2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_duties_bit_equal_launch_path_and_frozen_build(name):
    from mistral_inference import _hip
    n_layers, window, prompt_len, steps, distinct, per_step = CASES[name]
    p = dict(BOTH, n_layers=n_layers, sliding_window=window)
    m = _model(p, seed=41, distinct_layers=distinct)
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(11)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    ref, ref_rings, st0 = _run(m, ids, prompt_len, steps, engine=False)
    got, got_rings, st1 = _run(m, ids, prompt_len, steps, engine=True)
    graph, graph_rings, st2 = _run(m, ids, prompt_len, steps, engine=True, graph=True)
    prev = _hip.lib().mi_debug_set_engine_variant(2)  # the frozen default object: no gate, no second duty
    try:
        assert _engine_object(m, ids, prompt_len) == "other"
        frozen, frozen_rings, st3 = _run(m, ids, prompt_len, steps, engine=True)
    finally:
        _hip.lib().mi_debug_set_engine_variant(prev)
    assert st1["status"] == 0 and st1["abort"] == 0 and st2["status"] == 0 and st2["abort"] == 0 and st3["status"] == 0, (st1, st2, st3)
    assert st1["engine_launches"] - st0["engine_launches"] == per_step * steps, (st0, st1)
    assert st2["engine_launches"] - st1["engine_launches"] >= per_step * steps, (st1, st2)
    _check_equal(name, ref, ref_rings, got, got_rings)
    _check_equal(name + "/graph", ref, ref_rings, graph, graph_rings)
    _check_equal(name + "/frozen", ref, ref_rings, frozen, frozen_rings)


def test_summation_order_fingerprint_through_the_held_units():
    """W[:, D/2:] = -W[:, :D/2] for Wq, Wk, Wv and an input whose halves are equal: every q, k and v value of layer 0 is
    mathematically zero, and what is computed is the rounding residue of the association order.  At this shape every k and v row
    of a decode step is reduced by a holder wave from its registers: the rows in the rings are the residues of THAT order, and
    they must be the launch path's bits (Cons::unit_dot<2>'s element order)."""
    p = dict(BOTH, n_layers=1, sliding_window=64, vocab_size=512)
    args = mo.OracleArgs(**p)
    w = mo.synth_weights(args, seed=43)
    half = p["dim"] // 2
    w["tok_embeddings.weight"][:, half:] = w["tok_embeddings.weight"][:, :half]
    w["layers.0.attention_norm.weight"][half:] = w["layers.0.attention_norm.weight"][:half]
    for n in ("wq", "wk", "wv"):
        t = w[f"layers.0.attention.{n}.weight"]
        t[:, half:] = -t[:, :half]
    m = _load(args, w)
    prompt_len, steps = 5, 6
    ids = torch.randint(0, p["vocab_size"], (prompt_len + steps,), generator=torch.Generator().manual_seed(12)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    ref, ref_rings, _ = _run(m, ids, prompt_len, steps, engine=False)
    got, got_rings, st = _run(m, ids, prompt_len, steps, engine=True)
    assert st["status"] == 0 and st["abort"] == 0
    (k0, v0), (k1, v1) = ref_rings[0], got_rings[0]
    dec_k, dec_v = k0[:, prompt_len:], v0[:, prompt_len:]           # rows written by the decode steps
    assert float(dec_k.float().abs().max()) < 1e-3 and float(dec_v.float().abs().max()) < 1e-3   # residues, not signal
    assert float((dec_v != 0).float().mean()) > 0.5                # ... and not trivially zero: the fingerprint is real
    _check_equal("fingerprint", ref, ref_rings, got, got_rings)


def test_failed_residency_gate_writes_nothing_with_rows_held_in_registers():
    """The holder waves have fetched layer 0's q|k|v rows by the time the residency gate is decided.  A launch that fails the
    gate (sabotaged: it waits for one workgroup too many) must leave position and rings untouched all the same - the holders'
    ring rows and granules come behind the gate - and report 0x700; the steps are then re-run on the launch path."""
    from mistral_inference import _hip
    from mistral_inference.cache import BufferCache
    p = dict(BOTH, n_layers=3, sliding_window=48)
    m = _model(p, seed=47)
    prompt_len, steps = 20, 7
    ids = torch.randint(0, p["vocab_size"], (prompt_len + 1,), generator=torch.Generator().manual_seed(13)).cuda()
    assert _engine_object(m, ids, prompt_len) == "next"
    a = m.args

    def prefill():
        c = BufferCache(m.n_local_layers, 1, prompt_len + steps + 6, a.n_kv_heads, a.head_dim, a.sliding_window, device="cuda", dtype=BF)
        c.reset()
        for l in range(c.n_layers):  # (the rings are torch.empty: a defined value in the slots nothing has written)
            c.cache_k[l].zero_()
            c.cache_v[l].zero_()
        return c, torch.argmax(m.forward(ids[:prompt_len], [prompt_len], c)[-1:], dim=-1)

    try:
        c0, first = prefill()
        ref = m.greedy_session(c0, first, graph=True)
        ref.run(steps + 4)
        ref_t, _ = ref.collect()
        c, first2 = prefill()
        assert torch.equal(first, first2)
        sess = m.greedy_session(c, first2, graph=True)
        sess.run(4)
        a_t, _ = sess.collect()
        kv_before = int(c.kv_seqlens[0])
        rings_before = [(c.cache_k[l].clone(), c.cache_v[l].clone()) for l in range(c.n_layers)]
        _hip.debug_engine_sabotage(m._backend._workspace, 1)
        sess.run(steps)                   # the first of these fails its gate; the others find the workspace poisoned
        torch.cuda.synchronize()
        st = _hip.decode_engine_status(m._backend._workspace)
        assert st["status"] == 0x700, st
        assert int(c.kv_seqlens[0]) == kv_before          # nothing advanced
        for l, (k, v) in enumerate(rings_before):         # no ring row written
            assert torch.equal(k, c.cache_k[l]) and torch.equal(v, c.cache_v[l]), l
        b_t, _ = sess.collect()           # notices, resets, re-runs the steps on the launch path
        st = _hip.decode_engine_status(m._backend._workspace)
        assert st["status"] == 0 and int(c.kv_seqlens[0]) == kv_before + steps
        assert torch.equal(torch.cat([a_t, b_t]), ref_t), (torch.cat([a_t, b_t])[:, 0].tolist(), ref_t[:, 0].tolist())
    finally:
        if m._backend._workspace is not None:
            _hip.debug_engine_sabotage(m._backend._workspace, 0)
        _hip.set_decode_engine(True)
