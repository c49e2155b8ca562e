"""Which build of the persistent decode engine takes which model (csrc/decode_engine_host.hip: engine_route), checked without a GPU.

mi_debug_engine_route runs the routing function of mi_forward with a launch stub that always declines, so it lists the whole
chain of builds a batch-1 decode step would try; decode_engine_applicable is host arithmetic and the library loads without a device.

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


# ---- shapes that straddle the build-dependent conditions of decode_engine_applicable --------------------------------------------
# The grid above was not chosen to hit them.  Each pair below sits on the two sides of ONE condition that reads a build's traits
# (EngineBuild: wide, headline_only, ring size), everything else equal; STRADDLE_RECORDED holds the answers of 97f0441, the last
# commit whose applicable() was a preprocessor ladder compiled once per build, dumped from its library with this file's _row.
# The activation region is LDS_TOTAL - RING_FILLS * 16 KiB - 1280: 31488 B on the 8-fill builds, 47872 B on the 7-fill wide build.
_DENSE = dict(dim=2048, n_layers=2, head_dim=128, hidden_dim=2048, n_heads=16, n_kv_heads=4, norm_eps=1e-5, vocab_size=2048,
              sliding_window=64)
_MOE = dict(_DENSE, n_heads=8, n_kv_heads=2, num_experts=8, num_experts_per_tok=2)
STRADDLE_SHAPES = {
    "nemo_rule/dim_3072": dict(_DENSE, dim=3072, n_heads=8, n_kv_heads=2),
    "nemo_rule/dim_5120": dict(_DENSE, dim=5120, n_heads=8, n_kv_heads=2),
    "odd_pieces/dim_4608": dict(_DENSE, dim=4608, n_heads=8, n_kv_heads=2),
    "headline_filter/hidden_4096": dict(_DENSE, dim=4096, n_heads=32, n_kv_heads=8, hidden_dim=4096),
    "headline_filter/hidden_4608": dict(_DENSE, dim=4096, n_heads=32, n_kv_heads=8, hidden_dim=4608),
    "kmax/hidden_15360": dict(_DENSE, hidden_dim=15360),   # 2 * 15360 = 30720 <= 31488
    "kmax/hidden_15872": dict(_DENSE, hidden_dim=15872),   # 31744 > 31488
    "kmax/hidden_23552": dict(_DENSE, hidden_dim=23552),   # 47104 <= 47872
    "kmax/hidden_24064": dict(_DENSE, hidden_dim=24064),   # 48128 > 47872
    "moe_vector/dim_4096": dict(_MOE, dim=4096),           # 6 * 4096 = 24576 <= 31488
    "moe_vector/dim_6144": dict(_MOE, dim=6144),           # 6 * 6144 = 36864: > 31488, <= 47872; 4 * 6144 = 24576 <= 31488
    "moe_vector/dim_8192": dict(_MOE, dim=8192),           # 6 * 8192 = 49152 > 47872; 4 * 8192 = 32768 > 31488
    # 2 * 2048 + 8 * ceil(V / 2 / 256) + 16 + 16 * 256 at 256 CUs: 31488 / 31496 and 47872 / 47880
    "lm_stash/vocab_1489920": dict(_DENSE, vocab_size=1489920),
    "lm_stash/vocab_1489922": dict(_DENSE, vocab_size=1489922),
    "lm_stash/vocab_2538496": dict(_DENSE, vocab_size=2538496),
    "lm_stash/vocab_2538498": dict(_DENSE, vocab_size=2538498),
    "gqa/ratio_2": dict(_DENSE, n_heads=4, n_kv_heads=2),
    "gqa/ratio_4": dict(_DENSE, n_heads=8, n_kv_heads=2),
    "gqa/ratio_6": dict(_DENSE, n_heads=12, n_kv_heads=2),
    "gqa/ratio_8": dict(_DENSE, n_heads=16, n_kv_heads=2),
    "gqa/moe_ratio_4": dict(_MOE),
    "gqa/moe_ratio_8": dict(_MOE, n_heads=16, n_kv_heads=2),
    # split-merge slab ne = 2 * ceil(n_heads * 64 / CUs).  8-fill ring, GQA 4: 4 * 4384 + 512 + 384 * ne <= 31488 up to ne = 34 (the
    # default build's formula), 4 * 2336 + 512 + 384 * ne <= 31488 up to ne = 56 (the wide formula on the MoE build): at 64 CUs
    "attn_scratch/heads_16": dict(_DENSE, n_heads=16, n_kv_heads=4),                 # ne = 32
    "attn_scratch/heads_20": dict(_DENSE, n_heads=20, n_kv_heads=5),                 # ne = 40
    "attn_scratch/moe_heads_28": dict(_MOE, n_heads=28, n_kv_heads=7),               # ne = 56
    "attn_scratch/moe_heads_32": dict(_MOE, n_heads=32, n_kv_heads=8),               # ne = 64
    # ratio 6: a split's K and V pieces, 2 * ceil(chunk / 4), against the 5 fills = 80 pieces that may hold them: chunk 160 / 176
    "ratio6_ring/window_5120": dict(_DENSE, n_heads=12, n_kv_heads=2, sliding_window=5120),
    "ratio6_ring/window_5136": dict(_DENSE, n_heads=12, n_kv_heads=2, sliding_window=5136),
}
# (condition, the shape on its accepting side, the shape on its declining side)
STRADDLE_PAIRS = [
    ("Nemo dims: the default build declines, the wide build takes them when forced only, the nemo build is exempt", "nemo_rule/dim_3072", "nemo_rule/dim_5120"),
    ("nemo build (HEADLINE_ONLY = 2): large dims only", "nemo_rule/dim_5120", "nemo_rule/dim_3072"),
    ("wide and nemo builds: odd piece count at a large dim", "nemo_rule/dim_5120", "odd_pieces/dim_4608"),
    ("next build (HEADLINE_ONLY = 1): every row a multiple of 4 pieces", "headline_filter/hidden_4096", "headline_filter/hidden_4608"),
    ("nemo build (HEADLINE_ONLY = 2): not every row a multiple of 4 pieces", "headline_filter/hidden_4608", "headline_filter/hidden_4096"),
    ("activation vector beside the 8-fill ring", "kmax/hidden_15360", "kmax/hidden_15872"),
    ("activation vector beside the 7-fill ring", "kmax/hidden_23552", "kmax/hidden_24064"),
    ("MoE, D * 6 on the 8-fill MoE build", "moe_vector/dim_4096", "moe_vector/dim_6144"),
    ("MoE, D * 6 on the 7-fill wide build and D * 4 on the default build", "moe_vector/dim_6144", "moe_vector/dim_8192"),
    ("LM-head stash beside the 8-fill ring", "lm_stash/vocab_1489920", "lm_stash/vocab_1489922"),
    ("LM-head stash beside the 7-fill ring", "lm_stash/vocab_2538496", "lm_stash/vocab_2538498"),
    ("R = 6: the wide build only", "gqa/ratio_4", "gqa/ratio_6"),
    ("R = 2: not the wide build", "gqa/ratio_4", "gqa/ratio_2"),
    ("R = 8: neither {4, 6} nor, for its attention scratch, the default build", "gqa/ratio_4", "gqa/ratio_8"),
    ("MoE build: R = 4 only", "gqa/moe_ratio_4", "gqa/moe_ratio_8"),
    ("attention scratch, the default build's formula", "attn_scratch/heads_16", "attn_scratch/heads_20"),
    ("attention scratch, the wide formula beside the 8-fill ring", "attn_scratch/moe_heads_28", "attn_scratch/moe_heads_32"),
    ("GQA ratio 6: ring length", "ratio6_ring/window_5120", "ratio6_ring/window_5136"),
]
STRADDLE_RECORDED = {
    'attn_scratch/heads_16': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'attn_scratch/heads_20': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'attn_scratch/moe_heads_28': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['moe', 'moe', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'attn_scratch/moe_heads_32': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'gqa/moe_ratio_4': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'gqa/moe_ratio_8': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'gqa/ratio_2': {
        256: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'default', 'default', 'default', 'default', 'default', 'default'],
    },
    'gqa/ratio_4': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'gqa/ratio_6': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'gqa/ratio_8': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'headline_filter/hidden_4096': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'headline_filter/hidden_4608': {
        256: ['default', 'nemo,default', 'wide', 'wide', 'default', 'default', 'nemo,default', 'nemo,default'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'kmax/hidden_15360': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'kmax/hidden_15872': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'kmax/hidden_23552': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'kmax/hidden_24064': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'lm_stash/vocab_1489920': {
        256: ['next,default', 'next,default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'lm_stash/vocab_1489922': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'lm_stash/vocab_2538496': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['', '', '', '', '', '', '', ''],
    },
    'lm_stash/vocab_2538498': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'moe_vector/dim_4096': {
        256: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['moe', 'moe', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'moe_vector/dim_6144': {
        256: ['wide', 'wide', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['wide', 'wide', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'moe_vector/dim_8192': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'nemo_rule/dim_3072': {
        256: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
        64: ['default', 'default', 'wide', 'wide', 'default', 'default', 'default', 'default'],
    },
    'nemo_rule/dim_5120': {
        256: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
        64: ['', 'nemo', 'wide', 'wide', '', '', 'nemo', 'nemo'],
    },
    'odd_pieces/dim_4608': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
    'ratio6_ring/window_5120': {
        256: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
        64: ['wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide', 'wide'],
    },
    'ratio6_ring/window_5136': {
        256: ['', '', '', '', '', '', '', ''],
        64: ['', '', '', '', '', '', '', ''],
    },
}


def test_straddle_pairs_differ_in_the_parent():
    """A pair counts only if the two recorded rows differ: then the condition between them decided a route.

    What routing cannot make visible, and why:
      * `the 8-fill MoE build takes MoE models only`: engine_route asks the moe build for MoE models alone.
      * R != 4 on the nemo build: its shape filter (n_heads == 4 * n_kv_heads) has already declined every other ratio.
      * the wide attention-scratch formula beside the 7-fill ring: 4 * 2336 + 512 + 384 * ne and 6 * 2336 + 512 + 384 * ne stay
        below 47872 for every ne <= 64, and a larger ne is declined one line earlier (split-merge slab)."""
    assert sorted(STRADDLE_RECORDED) == sorted(STRADDLE_SHAPES)
    for why, a, b in STRADDLE_PAIRS:
        assert STRADDLE_RECORDED[a] != STRADDLE_RECORDED[b], why


@pytest.mark.parametrize("name", sorted(STRADDLE_SHAPES))
def test_straddle_route_is_the_parents(name):
    assert {n: _row(STRADDLE_SHAPES[name], n) for n in CUS} == STRADDLE_RECORDED[name]


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
