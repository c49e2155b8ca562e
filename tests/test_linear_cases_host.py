"""CPU proof that the structured dense-linear cases (linear_cases.py) are exact and have teeth at the shapes
test_gpu_linear_structured.py runs: the generators' conditions hold on every case, the torch emulations of the GEMV unit loop
and of the tiled GEMMs equal the fp64 reference bit for bit inside the guarded buffer, every single-fault mutant changes
every case it applies to (the row substitutions except where the two rows' exact sums are equal for every token, the
W1 / W3 exchange except where bf16(silu(b)) == b makes the product commutative; both asserted), and the route mirror gives
the hand-written labels at 256 and at 64 compute units.

test_conditions_and_measured_ranges prints the figures quoted in linear_cases.py (max|y|, the range of a, the shares of inexact
sums, of ties and of visible double roundings); test_every_mutant_changes_every_case_it_applies_to prints the mutant table.
"""
import collections
import functools

import pytest
import torch

import linear_cases as lc

CUS = 256
CASES = lc.all_cases(CUS)
GROUPS = ["gemv", "qkv", "g128", "g256", "f16"]


@functools.lru_cache(maxsize=None)
def sweep():
    """One pass over every case (the inputs of a case are built once): conditions, emulation against the reference, mutants.
    Returns (figures {case: dict}, emulation mismatches, {group: {mutant: [(case, differing elements, provably invisible)]}})."""
    figs, bad = {}, []
    rep = {g: collections.OrderedDict() for g in GROUPS}
    for case in CASES:
        figs[case] = lc.conditions(case)
        want = lc.expected(case)
        got = lc.emulate(case)
        if lc.differing(got, want):
            bad.append((case, lc.describe(case, got, want)))
        sums = torch.cat(lc.exact_sums(lc.inputs(case)), dim=1) if case.epi != lc.SWIGLU else None
        for m in lc.mutants_of(case):
            out = lc.emulate(case, m)
            if out is None:
                continue
            n = lc.differing(out, want)
            same = False
            if n == 0 and m in lc.SUBSTITUTIONS:           # the substituted row computes the same sums for every token: invisible to any test
                a, b = {"odd_row_from_partner": (case.N - 1, case.N - 2), "seg_wrong_n0": (case.segs[0], 0),
                        "seg_wrong_n1": (sum(case.segs[:2]), case.segs[0])}[m]
                same = bool(torch.equal(sums[:, a], sums[:, b]))
            if n == 0 and m == "w1_w3_exchanged":            # bf16(silu(b)) == b everywhere (b = 8 or so): silu(a) b == silu(b) a, commutative
                b = lc.exact_sums(lc.inputs(case))[1]
                same = bool(torch.equal((b / (1.0 + torch.exp(-b))).to(lc.BF).double(), b))
            rep[case.group].setdefault(m, []).append((case, n, same))
    return figs, bad, rep


def test_emulations_are_bit_equal_to_the_reference():
    _, bad, _ = sweep()
    assert not bad, bad[:4]


def test_conditions_and_measured_ranges(capsys):
    figs, _, _ = sweep()
    rows = collections.defaultdict(list)
    for case, f in figs.items():
        fam = ("swiglu " if case.epi == lc.SWIGLU else "") + case.fam + (" f16" if case.dtype == "f16" else "")
        for k, v in f.items():
            rows[(fam, k)] += list(v) if isinstance(v, tuple) else [v]
    with capsys.disabled():
        for (fam, k), v in sorted(rows.items()):
            print(f"\n  {fam:18s} {k:8s} {min(v):10.4g} .. {max(v):10.4g}", end="")
    plain = [f for c, f in figs.items() if c.fam == "plain" and c.epi != lc.SWIGLU]
    assert max(f["maxy"] for f in plain) <= 256 and max(f["zeros"] for c, f in figs.items() if c.fam == "plain") < 0.15
    assert min(f["pairs"] for f in plain if "pairs" in f) >= 0.25
    assert all(24 <= f["a"][0] and f["a"][1] <= 256 for f in figs.values() if "a" in f)
    rnd = [f for c, f in figs.items() if c.fam == "round"]
    assert min(f["inexact"] for f in rnd) >= 0.25 and min(f["ties"] for f in rnd) >= 0.05
    assert min(f["double"] for f in rnd if "double" in f) >= 0.05
    assert max(f["bound"] for f in figs.values()) < 2 ** 24


def test_every_mutant_changes_every_case_it_applies_to(capsys):
    _, _, rep = sweep()
    missed = []
    with capsys.disabled():
        for g in GROUPS:
            for m, rows in rep[g].items():
                seen = [n for _, n, _ in rows if n]
                equal = sum(1 for _, n, same in rows if not n and same)
                print(f"\n  {g:5s} {m:26s} {len(seen)}/{len(rows) - equal}  max {max(seen, default=0)}" + (f"  ({equal} with equal rows)" if equal else ""), end="")
                missed += [(g, m, repr(c)) for c, n, same in rows if not n and not same]
    assert not missed, (len(missed), missed[:40])


def test_every_mutant_has_cases_on_its_paths():
    _, _, rep = sweep()
    for g, muts in (("gemv", lc.GEMV_MUTANTS), ("qkv", lc.QKV_MUTANTS), ("g128", [m for m in lc.GEMM_MUTANTS if m != "tail_c0_off"]),
                    ("g256", lc.GEMM_MUTANTS), ("f16", lc.OPERAND_MUTANTS + lc.TILE_MUTANTS[:8] + ["seg_wrong_n0", "seg_wrong_n1", "residual_before_rounding",
                                                                          "logits_not_rounded", "round_half_away"])):
        for m in muts:
            assert any(n for _, n, _ in rep[g].get(m, [])), (g, m, "changes no case")


def test_invisible_row_substitutions_are_tiny_cases_only():
    """Where a substituted row goes unseen its sums equal the right row's for every token: possible only at one token (a row is
    one number) or at K <= 16 (a sum has one or two +-1 terms)."""
    _, _, rep = sweep()
    for g in GROUPS:
        for m in lc.SUBSTITUTIONS:
            for case, n, same in rep[g].get(m, []):
                assert n or (same and (case.M == 1 or case.K <= 16)), (g, m, case)
        for case, n, same in rep[g].get("w1_w3_exchanged", []):
            assert n or (same and case.M * case.N <= 4), (g, case)


def test_single_faults_move_few_outputs():
    """What 1-ulp bounds on Gaussian data cannot see: one weight piece of one row moves at most M outputs, each by one product."""
    _, _, rep = sweep()
    for g in GROUPS:
        for m in ("piece_dropped_first", "piece_dropped_middle", "piece_dropped_last"):
            assert all(0 < n <= case.M * (2 if case.epi == lc.QKV else 1) * (3 if case.qkv and case.qkv[2] else 1) for case, n, _ in rep[g][m]), (g, m)


# ------------------------------------------------------------------------------------------------------------ route mirror
@pytest.mark.parametrize("cus", [256, 64, 304])
def test_cases_carry_the_label_the_mirror_gives(cus):
    for c in lc.all_cases(cus):
        assert lc.route(c.M, c.K, c.N, c.epi, cus, c.dtype, c.tail) == c.path, c
        assert c.blocks is None or lc.block_plan(c.M, c.K, c.N, c.epi, cus) == c.blocks, c


def test_route_mirror_against_the_launchers_comments():
    r, S, R, L, G, Q = lc.route, lc.STORE, lc.RESIDUAL, lc.LOGITS, lc.SWIGLU, lc.QKV
    # gemv_max_tokens: 144 KiB of rows, 5 -> 4 and 7 -> 6 (they would stage 6 / 8 rows)
    assert [lc.gemv_max_tokens(K) for K in (4096, 9216, 9224, 10240, 12288, 14336, 16384, 28672)] == [8, 8, 6, 6, 6, 4, 4, 2]
    assert lc.passes(8, 10240) == [(0, 6), (6, 2)] and lc.passes(8, 14336) == [(0, 4), (4, 4)] and lc.passes(7, 4096) == [(0, 7)]
    assert [lc.round_tt(T) for T in range(1, 9)] == [1, 2, 3, 4, 6, 6, 8, 8]
    # stage_by_dma: 8 x 256 pieces fit the registers of the plain modes, 4 x 256 those of the norm-style modes; never one row
    assert lc.dma_edge(S, 2) == (8192, 8200) and lc.dma_edge(S, 4) == (4096, 4104) and lc.dma_edge(R, 8) == (2048, 2056)
    assert lc.dma_edge(L, 2) == (4096, 4104) and lc.dma_edge(G, 4) == (2048, 2056) and lc.dma_edge(Q, 8) == (1024, 1032)
    assert not lc.stage_by_dma(S, 1, 28672)
    assert lc.lds_bytes(6, 10240) == 6 * 20480 + 96 > 80 * 1024 and lc.lds_bytes(3, 14336) == 86064
    # the grid (gemv_core.cuh): W1|W3 14336 units -> 512 blocks x 4 waves x 7 units; q|k|v 3072 units -> 768 blocks x 1
    assert lc.even_blocks(14336, 256) == (512, 7) and lc.even_blocks(3072, 256) == (768, 1) and lc.even_blocks(2560, 256) == (0, 0)
    assert lc.spread_blocks(2560, 512) == (320, 2)                   # Nemo's Wo / W2 on 4-wave blocks: 320 blocks
    assert r(1, 512, 5120, S, 256) == "gemv/nw=5" and lc.gemv_plan(1, 512, 5120, S, 256)["blocks"] == 512
    p = lc.gemv_plan(1, 512, 60 * 256, R, 256)                      # 7680 pairs > 16 cus: 768 five-wave blocks, two units per wave
    assert (p["nw"], p["k"], p["blocks"]) == (5, 2, 768) and lc.block_plan(1, 512, 60 * 64, S, 64) == "nw-k2-3-per-cu"
    assert r(1, 14336, 5120, R, 256) == "gemv/nw=5" and r(1, 28672, 5120, R, 256) == "gemv/TT=1"       # (a row above 48 KiB)
    assert r(2, 512, 5120, S, 256) == "gemv/TT=2" and r(1, 512, 5120, L, 256) == "gemv/TT=1"
    assert [r(1, 512, 2 * w * 256, R, 256) for w in (5, 6, 7)] == ["gemv/nw=5", "gemv/nw=6", "gemv/nw=7"]
    assert [r(1, 512, 2 * w * 64, S, 64) for w in (5, 6, 7)] == ["gemv/nw=5", "gemv/nw=6", "gemv/nw=7"]
    assert r(1, 512, 2 * 5 * 256, S, 64) == "gemv/TT=1"              # 1280 pairs on 64 CUs: 320 blocks = 5 per CU, even
    assert r(8, 10240, 64, S, 256) == "gemv/TT=6/dma/2-pass" and r(6, 10240, 2064, S, 256) == "gemv/TT=6/dma"
    assert lc.block_plan(6, 10240, 2064, S, 256) == "1-per-cu" and lc.block_plan(6, 10240, 2048, S, 256) == "even-k1"
    assert lc.block_plan(6, 10240, 528, S, 64) == "1-per-cu"
    assert r(5, 2048, 37, S, 256) == "gemv/TT=6" and r(7, 2048, 37, S, 256) == "gemv/TT=8" and r(7, 2056, 37, S, 256) == "gemv/TT=8/dma"
    assert r(8, 4096, 6144, Q, 256) == "gemv/TT=8/dma" and r(1, 4096, 6144, Q, 256) == "gemv/TT=1"
    # launch_gemm: the 256 kernel from 256 rows at K = 128, 192, ...; the 128 kernel by DMA at K % 64 == 0, else through registers
    assert r(9, 64, 8, S, 256) == "g128/dma" and r(9, 72, 8, S, 256) == "g128/regstage" and r(1030, 64, 8, S, 256) == "g128/dma"
    assert r(255, 128, 8, S, 256) == "g128/dma" and r(256, 128, 8, S, 256) == "g256" and r(300, 200, 8, S, 256) == "g128/regstage"
    # q|k|v of Mistral-7B at 4096 tokens: 16 x 24 = 384 tiles = 256 + 128 -> 256 + 256 half-height blocks
    assert r(4096, 4096, 6144, S, 256) == "g256+half" and lc.tail_split(4096, 6144, S, 256, 2) == (4096, "half")
    assert r(4096, 4096, 6144, S, 256, tail=1) == "g256+g128tail" and r(4096, 4096, 6144, S, 256, tail=0) == "g256"
    assert r(4096, 4096, 6144, L, 256) == "g256+g128tail"            # the half-height tiles take store and residual only
    assert r(4096, 4096, 4096, S, 256) == "g256" and r(4096, 4096, 14336, G, 256) == "g256"            # 256 and 1792 tiles: whole rounds
    assert r(4096, 128, 5 * 256, S, 64) == "g256+half" and lc.tail_split(4096, 1280, S, 64, 2) == (1024, "half")
    assert r(300, 128, 8, S, 256, dtype="f16") == "f16/g256" and r(300, 200, 8, S, 256, dtype="f16") == "f16/generic"
    assert r(9, 128, 8, S, 256, dtype="f16") == "f16/generic"


def test_cases_sit_on_the_edges_they_name():
    by = {c.name: c for c in CASES}
    gemv = [c for c in CASES if c.group == "gemv"]
    assert {c.M for c in gemv} == set(range(1, 9))
    assert {8, 16, 504, 512, 520, 2040, 2048, 2056, 4104, 14336, 28672, 10240} <= {c.K for c in gemv}
    for epi in lc.MODES:
        sub = [c for c in gemv if c.epi == epi]
        assert {c.M for c in sub} == set(range(1, 9)) and set(lc.GEMV_KS) <= {c.K for c in sub}, epi
    assert {(12, 13, 12), (12, 13, 13), (20, 21, 23), (30, 34), (1,), (2,), (3,), (37,), (64,)} <= {c.segs for c in gemv}
    for TT in (2, 4, 8):
        assert {c.path for c in gemv if c.M == TT and "lastreg" in c.name} == {f"gemv/TT={TT}"}
        assert {c.path for c in gemv if c.M == TT and "firstdma" in c.name} == {f"gemv/TT={TT}/dma"}
    assert {c.blocks for c in gemv if c.blocks} >= {"1-per-cu", "nw-k1-1-per-cu", "nw-k1-2-per-cu", "nw-k2-3-per-cu", "spread-k1", "spread-k2", "spread-k4", "even-k5"}
    k2 = [c for c in gemv if c.blocks == "nw-k2-3-per-cu"]                      # 5-wave blocks whose waves walk two units each
    assert {c.epi for c in k2} == {lc.STORE, lc.RESIDUAL} and all(lc.gemv_plan(1, c.K, c.N, c.epi, CUS)["k"] == 2 and c.N == 60 * CUS for c in k2)
    assert any(c.M == 2 and c.N == 60 * CUS and c.path == "gemv/TT=2" for c in gemv)
    big = by["m6k10240n2064-store"]
    assert lc.gemv_plan(6, 10240, 2064, lc.STORE, CUS)["lds"] > 80 * 1024 and lc.spread_blocks(1032, 2 * CUS)[0] > CUS and big.blocks == "1-per-cu"
    qkv = [c for c in CASES if c.group == "qkv"]
    assert {(c.qkv[0], c.qkv[1]) for c in qkv} == {(4, 2), (8, 8)} and {(c.K, c.M) for c in qkv} == {(D, T) for D in (512, 2560) for T in (1, 3, 8)} | {(10240, 8)}
    assert {(c.qkv[2], c.qkv[3]) for c in qkv} == {(l, s) for l in ("slot", "head", None) for s in (True, False)}
    assert any(c.K == 10240 and c.qkv[2] and not c.qkv[3] for c in qkv)       # two passes, a cache and no tok_seq: sequences 6, 7 in pass two
    g128 = [c for c in CASES if c.group == "g128"]
    assert {9, 127, 128, 129, 255, 1030} <= {c.M for c in g128} and {64, 128, 192, 8, 72, 200, 520} == {c.K for c in g128}
    assert {8, 120, 128, 136, 1160} <= {c.N for c in g128 if c.epi != lc.SWIGLU} and {64, 72, 200} == {c.N for c in g128 if c.epi == lc.SWIGLU}
    assert any(c.M >= 256 and c.K == 200 for c in g128) and {c.epi for c in g128} == set(lc.MODES)
    g256 = [c for c in CASES if c.group == "g256" and "tail" not in c.name]
    assert {c.M for c in g256} == {256, 257, 300, 1030} and {c.K for c in g256} == {128, 192, 448, 4096}
    assert {8, 256, 264, 640} <= {c.N for c in g256 if c.epi != lc.SWIGLU} and {128, 136} == {c.N for c in g256 if c.epi == lc.SWIGLU}
    tail = [c for c in CASES if "tail" in c.name]
    assert [(c.M, c.N, c.tail, c.path) for c in tail[:3]] == [(4096, 6144, 2, "g256+half"), (4096, 6144, 1, "g256+g128tail"), (4096, 6144, 0, "g256")]
    assert tail[3].M == 4000 and all(e % 256 and e % 128 for e in (tail[0].segs[0], sum(tail[0].segs[:2])))
    f16 = [c for c in CASES if c.group == "f16"]
    assert {c.path for c in f16} == {"f16/g256", "f16/generic"} and {c.M for c in f16 if c.path == "f16/generic"} == {9, 300}
    assert {(c.epi, len(c.segs)) for c in f16 if c.path == "f16/g256"} >= {(lc.STORE, 1), (lc.STORE, 3), (lc.RESIDUAL, 1), (lc.LOGITS, 1)}
