"""Which build of the persistent decode engine takes which model (csrc/api.hip: engine_route), checked without a GPU.

mi_debug_engine_route runs the routing function of mi_forward with a launch stub that always declines, so it lists the whole
chain of builds a batch-1 decode step would try; applicable() is host arithmetic and the library loads without a device.

RECORDED holds the answers of the PARENT of the commit that introduced engine_route - e99435d, whose mi_forward routed through
an if-chain over forty free functions: the same export was patched on top of that if-chain in a scratch checkout and the grid
below was dumped from it.  A change of routing has to change this table on purpose.

Grid: the model shapes of bench.PRESETS at the benchmark's context (Mixtral-8x22B as one pipeline stage), every shape of
tests/test_gpu_engine.py (SHAPES, WIDE_SHAPES, NEXT_SHAPES) and one odd-vocab shape that no build takes; engine variants 0-3;
MI_ENGINE_NEMO off / on; 256 CUs (MI355X) and 64 (a small device on which some shapes still find a build and others have more
attention work items or longer slabs than the CUs take; at 8 CUs no build takes any shape of the grid).  The K/V ring of every
layer of a test shape has `sliding_window` slots where the shape names one number, else 8192.
"""
import ctypes
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

CUS = (256, 64)
SETTINGS = list(itertools.product(range(4), (0, 1)))  # (engine variant, nemo opt-in): the order of a RECORDED row


def _shapes():
    import bench
    import test_gpu_engine as g
    # the benchmark's workloads: a 4096-token context; Mixtral-8x22B as ONE of its 8 pipeline stages (7 of 56 layers)
    shapes = {f"preset/{k}": dict(v[0], sliding_window=4096) for k, v in bench.PRESETS.items()}
    shapes["preset/mixtral-8x22b-stage"] = dict(shapes.pop("preset/mixtral-8x22b"), n_layers=7)
    for group, d in (("engine", g.SHAPES), ("wide", g.WIDE_SHAPES), ("next", g.NEXT_SHAPES)):
        shapes.update({f"{group}/{k}": v for k, v in d.items()})
    shapes["odd_vocab"] = dict(g.NEXT_SHAPES["headline_widths"], vocab_size=2049)
    return shapes


def _route(p, n_cus, variant, opt_in):
    from mistral_inference import _hip
    w, moe = p.get("sliding_window"), p.get("moe", p)  # (bench.PRESETS nest the MoE keys, the test shapes do not)
    out = ctypes.create_string_buffer(64)
    rc = _hip.lib().mi_debug_engine_route(p["dim"], p["n_heads"], p["n_kv_heads"], p["hidden_dim"], p["vocab_size"],
                                          moe.get("num_experts", 0), moe.get("num_experts_per_tok", 0), p["n_layers"],
                                          w if isinstance(w, int) else 8192, n_cus, variant, opt_in, out, len(out))
    assert rc == 0
    return out.value.decode()


def _row(p, n_cus):
    return [_route(p, n_cus, v, o) for v, o in SETTINGS]


# name: {CUs: routes for (variant, opt-in) = (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)}
RECORDED = {
    'engine/gqa2_long_ring': {
        256: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
    },
    'engine/gqa4_window_wraps': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'engine/holders_mid_size': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'engine/mha_no_window': {
        256: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'engine/moe_4_experts_mha': {
        256: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'engine/moe_8_experts_top2': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'engine/moe_qkv_holders': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'engine/nemo_rows_long_ring': {
        256: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'engine/nemo_rows_of_10_pieces': {
        256: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
        64: ['', '', 'wide', 'wide', '', '', '', ''],
    },
    'engine/ring_longer_than_lds': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'engine/rows_of_6_and_3_pieces': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'engine/two_launches_34_layers': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'engine/window_list': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'next/headline_widths': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'next/holders_window_wraps': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'next/no_holders_long_ring': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'odd_vocab': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'preset/mistral-7b': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'preset/mixtral-8x22b-stage': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'preset/mixtral-8x7b': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'preset/nemo-12b': {
        256: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'wide/gqa4_window_wraps': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'wide/gqa6_moe_rows_of_12': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'wide/gqa6_moe_rows_of_4': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'wide/gqa6_rows_of_5_and_3': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'wide/moe_8_experts_top2': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'wide/ring_longer_than_lds': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'wide/rows_of_10_pieces': {
        256: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
        64: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
    },
    'wide/rows_of_6_and_3_pieces': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
}


def test_grid_covers_every_shape():
    assert sorted(RECORDED) == sorted(_shapes())
    assert all(sorted(r) == sorted(CUS) and all(len(x) == len(SETTINGS) for x in r.values()) for r in RECORDED.values())


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_route_is_the_parents(name):
    p = _shapes()[name]
    assert {n: _row(p, n) for n in CUS} == RECORDED[name]


def test_rows_design_md_promises():
    """DESIGN.md section 3, independent of the table: the BASELINE models on an MI355X (256 CUs)."""
    s = _shapes()
    m7, nemo, x7, x22 = (s["preset/" + k] for k in ("mistral-7b", "nemo-12b", "mixtral-8x7b", "mixtral-8x22b-stage"))
    assert _route(m7, 256, 0, 0).split(",")[0] == "next"
    assert _route(m7, 256, 2, 0).split(",")[0] == "default"
    assert _route(nemo, 256, 0, 0) == ""                       # launch path
    assert _route(nemo, 256, 0, 1).split(",")[0] == "nemo"
    assert _route(nemo, 256, 3, 0).split(",")[0] == "nemo"
    assert _route(x7, 256, 0, 0) == "moe"
    assert _route(x22, 256, 0, 0) == "wide"
    assert _route(s["odd_vocab"], 256, 0, 0) == ""


def test_route_refuses_what_it_cannot_hold():
    from mistral_inference import _hip
    out = ctypes.create_string_buffer(4)
    L = _hip.lib()
    assert L.mi_debug_engine_route(4096, 32, 8, 14336, 32768, 0, 0, 32, 4096, 256, 0, 0, out, len(out)) == -1  # "next,default"
    assert L.mi_debug_engine_route(4096, 32, 8, 14336, 32768, 0, 0, 32, 4096, 0, 0, 0, out, len(out)) == -1    # no CUs


def test_shipped_slot_is_todays_headline_flags():
    """scripts/build_variants.py: the `shipped` experiment slot follows build_native.ENGINE_NEXT_FLAGS; as of this commit that
    is the round-7 winner typed by hand as `r7_gate`."""
    import build_variants as bv
    assert set(bv.ENGINE_SLOTS["shipped"]) == set(bv.ENGINE_SLOTS["r7_gate"])
