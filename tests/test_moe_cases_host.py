"""CPU proof that the structured MoE cases (moe_cases.py) are exact and have teeth at the shapes test_gpu_moe_structured.py
runs: the generator's two conditions hold on every case, the torch emulation of each pipeline equals the fp64-chain reference
bit for bit, every single-fault mutant changes the output of at least one case of each path it belongs to, the routing
builder hits its counts with distinct picks, and the Gaussian family's tolerance constant is three times what the honest
emulation reaches.

Mutants (what each one breaks heads moe_cases.py): the cases that see it, each with its number of differing output rows,
from this file's own run (test_every_mutant_is_seen_on_its_path prints the counts).  Cases by letter - 128-row tiles:
A e8k2t300-edges, B e4k2t520-wrap, C e8k2t516-16tiles, D e16k4t100-order, E e2k1t200-empty0, F e2k2t520-k264,
G e2k2t511-switch; 256-row tiles: P e3k2t768-ragged255, Q e2k1t1024-empty0, R e4k4t512-order, S e2k2t512-switch; decode: the 27
cases k in {1, 2, 4} x T in {1, 3, 8} x F in {264, 520, 1544} (the two LDS-edge cases carry no mutants).  A case missing from a
line has nothing for that mutant to break (no ragged tile followed by another row, no empty expert in front of a row, k = 1).

  mutant                  128-row tiles                                  256-row tiles               decode (rows per case)
  last_row_dropped        A B C D E F G: 1 each                          P: 1                        -
  row_past_written        A B C D F G: 1 each                            P: 1                        -
  next_expert_weights     A B F G: 128, C: 1, D: 8                       P R S: 256                  -
  empty_expert_tile       A E: 1                                         Q: 1                        -
  w1_w3_exchanged         every row of A .. G (300 .. 520)               every row of P .. S         all 27: every token
  tok_of_off_by_one       A .. G: 1 each                                 P Q R S: 1 each             -
  combine_slot_order      D: 66                                          R: 341                      the 9 k = 4 cases: 1 .. 6
  slot_weights_exchanged  A B C D F G: 1 each                            P R S: 1 each               the 18 k >= 2 cases: 1
  slot_of_identity        -                                              -                           the 18 k >= 2 cases: 1 .. 6
  hid_fp32                every row of A .. G                            every row of P .. S         all 27: every token
  w13_kskip_first/middle/last   A B C F G: 128, D: 8, E: 72              P Q R S: 256                all 27: every token
  w2_kskip_first/middle/last    A B C F G: 128, D: 8, E: 72              P Q R S: 256                all 27: every token
  table128_tiles256       -                                              P: 384, Q S: 256, R: 512    -

The order mutant (combine_slot_order) is visible only at k = 4: at k = 2 the bf16 sum of two addends from zero is commutative,
so of the cases it applies to (every case) exactly D, R and the nine k = 4 decode cases see it, which
test_order_mutant_needs_k4 asserts in both directions.
"""
import functools

import pytest
import torch

import moe_cases as mc

PATH_CASES = {"g128": mc.G128_CASES + [mc.SWITCH_511], "g256": mc.G256_CASES, "decode": mc.DECODE_CASES}
PATH_MUTANTS = {"g128": [m for m in mc.GROUPED_MUTANTS if m != "table128_tiles256"], "g256": mc.GROUPED_MUTANTS,
                "decode": mc.DECODE_MUTANTS}


@pytest.mark.parametrize("case", mc.EXACT_CASES, ids=repr)
def test_conditions_hold_and_emulation_is_bit_equal(case):
    lo, hi, bound = mc.conditions(case)
    assert 24 <= lo <= hi <= 256 and max(bound) < 2 ** 24
    ref, _ = mc.reference(case)
    got = mc.emulate(case)
    bad = torch.nonzero((got != ref).any(dim=1))[:, 0].tolist()
    assert not bad, (case, mc.describe_rows(case, bad))


@functools.lru_cache(maxsize=None)
def mutant_report(path):
    """{mutant: [(case, differing rows)]} over the cases of one path where the mutant applies."""
    rep = {m: [] for m in PATH_MUTANTS[path]}
    for case in PATH_CASES[path]:
        assert case.path == path and case.mutants
        ref, _ = mc.reference(case)
        for m in PATH_MUTANTS[path]:
            out = mc.emulate(case, m)
            if out is not None:
                rep[m].append((case, int((out != ref).any(dim=1).sum())))
    return rep


@pytest.mark.parametrize("path", list(PATH_CASES))
def test_every_mutant_is_seen_on_its_path(path, capsys):
    rep = mutant_report(path)
    with capsys.disabled():
        for m, rows in rep.items():
            seen = [(repr(c), n) for c, n in rows if n]
            print(f"\n  {path:7s} {m:24s} {len(seen)}/{len(rows)}  max rows {max((n for _, n in seen), default=0)}", end="")
    for m, rows in rep.items():
        assert any(n > 0 for _, n in rows), (path, m, "changes no case", [repr(c) for c, _ in rows])


@pytest.mark.parametrize("path", list(PATH_CASES))
def test_order_mutant_needs_k4(path):
    """Combining in slot order changes the output at k = 4 and cannot at k <= 2 (commutative)."""
    for case, n in mutant_report(path)["combine_slot_order"]:
        assert (n > 0) == (case.k == 4), (case, n)


def test_single_fault_mutants_move_few_rows():
    """What the gross bound of the operator tests cannot see: one row of hundreds."""
    for path in ("g128", "g256"):
        rep = mutant_report(path)
        for m in ("last_row_dropped", "row_past_written", "empty_expert_tile", "tok_of_off_by_one", "slot_weights_exchanged"):
            assert rep[m] and all(n == 1 for _, n in rep[m]), (path, m, rep[m])


@pytest.mark.parametrize("case", [c for c in mc.EXACT_CASES + mc.GAUSS_CASES if c.prefix_of is None], ids=repr)
def test_routing_hits_its_counts_with_distinct_picks(case):
    inp = mc.inputs(case)
    idx = inp.sel_idx
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (case.T, case.k) and inp.sel_w.dtype == torch.float32
    assert int(idx.min()) >= 0 and int(idx.max()) < case.E
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    if case.counts is not None:
        assert torch.bincount(idx.reshape(-1).long(), minlength=case.E).tolist() == list(case.counts)
    assert torch.equal(inp.sel_w.sum(dim=1), torch.ones(case.T))
    assert torch.equal(inp.sel_w.to(torch.bfloat16).float(), inp.sel_w)
    if case.k > 1:
        assert bool((torch.sort(inp.sel_w, dim=1).values.diff(dim=1) > 0).all())       # a token's weights all differ
    if case.order == "mixed" and case.T >= 3 and case.k > 1:                                # all three slot orders occur
        asc = (idx[:, 1:] > idx[:, :-1]).all(dim=1)
        desc = (idx[:, 1:] < idx[:, :-1]).all(dim=1)
        assert bool(asc.any()) and bool(desc.any()) and (case.k == 2 or bool((~asc & ~desc).any()))


def test_routing_builder_orders_and_edges():
    for order in ("asc", "desc", "rot"):
        idx = mc.route_from_counts(7, 4, (7, 0, 7, 3, 4, 7), order)
        assert torch.bincount(idx.reshape(-1).long(), minlength=6).tolist() == [7, 0, 7, 3, 4, 7]
        assert all(len(set(r)) == 4 for r in idx.tolist())
        asc = (idx[:, 1:] > idx[:, :-1]).all(dim=1)
        assert bool(asc.all()) == (order == "asc")
    with pytest.raises(AssertionError):
        mc.route_from_counts(4, 2, (5, 3))          # a count above T would give a token the same expert twice
    with pytest.raises(AssertionError):
        mc.route_from_counts(4, 2, (4, 3))          # counts must sum to T k


def test_decode_routing_shares_all_and_none():
    for case in mc.DECODE_CASES:
        if case.T < 3:
            continue
        idx = mc.inputs(case).sel_idx
        assert set(idx[0].tolist()) == set(idx[1].tolist())
        assert case.k == 1 or idx[0].tolist() != idx[1].tolist()
        assert not set(idx[0].tolist()) & set(idx[2].tolist())


def test_cases_sit_on_the_edges_they_name():
    """Tile size per case, n_tiles against max_m_tiles, the lists kernel's stride wrap, the LDS limit."""
    tiles = {}
    for case in PATH_CASES["g128"] + PATH_CASES["g256"]:
        tr = mc.tile_rows_for(case.T, case.k, case.E, case.D, case.F)
        assert tr == (256 if case.path == "g256" else 128)
        _, _, tl = mc.moe_lists(mc.inputs(case).sel_idx, case.E, tr)
        tiles[case.name] = (len(tl), mc.max_m_tiles(case.T, case.k, case.E, tr), sorted({rv for _, _, rv in tl}))
    assert tiles["e8k2t300-edges"][2] == [1, 87, 127, 128] and tiles["e8k2t516-16tiles"][:2] == (16, 17)
    assert tiles["e4k2t520-wrap"][0] == 5 + 3 + 2 + 1 and 520 * 2 > 1024
    assert tiles["e3k2t768-ragged255"][2] == [1, 255, 256]
    big = mc.Case("k264", 2, 2, 520, (520, 520), D=264, F=520)
    assert big.T * big.k >= 512 * big.E and big.path == "g128"
    assert mc.SWITCH_511.T * 2 < 512 * 2 <= mc.SWITCH_512.T * 2
    assert all(c.k * c.F * 2 == 65536 for c in mc.LDS_EDGE_CASES)
    assert {c.F % 512 for c in mc.DECODE_CASES} == {264, 8} and {(c.F + 511) // 512 for c in mc.DECODE_CASES} == {1, 2, 4}


def test_gaussian_tolerance_is_three_times_the_honest_emulation():
    worst = 0.0
    for case in mc.GAUSS_CASES:
        ref, S = mc.reference(case)
        worst = max(worst, mc.gauss_ratio(mc.emulate(case), ref, S))
    assert 0.9 * mc.GAUSS_HONEST <= worst <= mc.GAUSS_HONEST, worst
    assert mc.GAUSS_C == 3 * mc.GAUSS_HONEST
