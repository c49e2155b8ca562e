"""CPU proof that the structured row-kernel cases (row_cases.py) are sharp and have teeth at the shapes test_gpu_rows_structured.py
runs: every construction's conditions hold (sums exact, codes representable, ties only where they were placed), every torch
emulation of a kernel's index logic agrees with its high-precision reference, and every single-fault mutant fails the very
comparison the GPU test applies (row_cases.*_mismatch, tolerance included) on every case it applies to - or is provably invisible
there, for a reason that is stated in row_cases.*_invisible and asserted here from both sides: a mutant with a reason must leave
the case unchanged, a mutant without one must change it.

test_every_mutant_is_caught_or_provably_invisible prints the mutant table; test_caps_hold_for_the_reference_alone prints how far
the references themselves sit from the bounds."""
import collections
import functools

import pytest
import torch

import row_cases as rc

NAMES = list(rc.GROUPS)


def family(m):
    return m.split("@")[0]


@functools.lru_cache(maxsize=None)
def sweep(name):
    """One pass over a group's cases: (figures {case: dict}, emulation mismatches, {mutant family: [(case, mutant, caught, reason)]})."""
    g = rc.GROUPS[name]
    figs, bad, rep = {}, [], collections.OrderedDict()
    for case in g.cases():
        figs[case] = g.conditions(case)
        want = g.expected(case)
        d = g.mismatch(case, g.emulate(case), want)
        if d:
            bad.append((case, d))
        for m in g.mutants_of(case):
            got = g.emulate(case, m)
            rep.setdefault(family(m), []).append((case, m, g.mismatch(case, got, want), g.invisible(case, m)))
    return figs, bad, rep


@pytest.mark.parametrize("name", NAMES)
def test_conditions_hold_and_emulations_equal_the_reference(name):
    _, bad, _ = sweep(name)
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_is_caught_or_provably_invisible(name, capsys):
    _, _, rep = sweep(name)
    missed, phantom = [], []
    with capsys.disabled():
        for fam, rows in rep.items():
            caught = sum(1 for _, _, d, _ in rows if d)
            reasons = collections.Counter(r for _, _, d, r in rows if r)
            print(f"\n  {name:8s} {fam:18s} caught {caught}/{len(rows) - sum(reasons.values())}"
                  + "".join(f"  [{n} invisible: {r}]" for r, n in reasons.items()), end="")
            missed += [(c, m) for c, m, d, r in rows if not d and not r]
            phantom += [(c, m, r) for c, m, d, r in rows if d and r]
    assert not missed, (len(missed), missed[:20])
    assert not phantom, (len(phantom), phantom[:20])


def test_every_listed_mutant_has_a_case_that_shows_it():
    want = {"greedy": rc.GREEDY_MUTANTS, "rms": ["drop", "dup", "div_padded", "eps_dropped", "neighbour_inv", "w_shift"], "rope": rc.ROPE_MUTANTS,
            "router": rc.ROUTER_MUTANTS + ["norm_skipped"], "kv": rc.KV_MUTANTS, "logprob": rc.LOGPROB_MUTANTS}
    for name, fams in want.items():
        rep = sweep(name)[2]
        for fam in fams:
            assert any(d for _, _, d, _ in rep.get(fam, [])), (name, fam, "changes no case")


def test_cases_sit_on_the_edges_they_name():
    gc = rc.greedy_cases()
    assert {c.V for c in gc if c.V % 4 == 0} == set(rc.GREEDY_VEC_V) and {c.V for c in gc if c.V % 4} == set(rc.GREEDY_SCALAR_V)
    for c in gc:
        labels, buf = rc.greedy_inputs(c)
        vec = rc.greedy_row_is_vector(c, buf.shape[0])
        assert rc.greedy_ld(c) >= c.V and (c.layout == "dense") == (rc.greedy_ld(c) == c.V)
        assert int(vec.sum()) == {"dense": len(vec), "pad": len(vec), "odd": len(vec) // 2}[c.layout] * (c.V % 4 == 0)
        if c.V == 16388:
            assert sum(l.startswith("t0/trip1/slot") for l in labels) == 4 * (2 if c.layout == "odd" else 1)
        if c.V % 4 == 0 and c.V >= 32768:          # every slot of three threads' trips, and every kind of tie
            assert sum(l.startswith(("t0/slot", "t1023/slot", "t5/trip1/slot")) for l in labels) >= 48 * (2 if c.layout == "odd" else 1)
            assert all(any(l.startswith(t) for l in labels) for t in ("same float4", "two float4", "trip 0 / trip 1", "neighbours,", "waves,", "all equal"))
        assert all(any(l.startswith(t) for l in labels) for t in ("all equal", "lp peaked", "lp +-80"))
        assert c.V - 1 in rc.greedy_expected(c)[0].tolist() and 0 in rc.greedy_expected(c)[0].tolist()
        assert c.V == 1 or all(any(l.startswith(t) for l in labels) for t in ("-inf low", "-inf trip", "-inf tail"))
    big = rc.greedy_rows(16384)[1]
    trip = big[rc.greedy_rows(16384)[0].index("-inf trip")]
    assert bool(torch.isinf(trip[[rc.vec_index(2, 0, e) for e in range(16)]]).all()) and int(torch.isinf(trip).sum()) == 16
    rms = rc.rms_cases()
    assert {c.D for c in rms} == set(rc.RMS_DS) and {c.T for c in rms} == {1, 4, 5}
    assert [rc.rms_template(D) for D in (4096, 4104, 6144, 6152, 8192, 8200, 16384)] == [8, 12, 12, 16, 16, 32, 32]
    for D in rc.RMS_DS:
        np_ = D >> 3
        hot = {int(k[4:]) for c in rms if c.D == D for k in c.kinds if k.startswith("hot@")}
        assert hot == {p for p in {0, 63, 64, np_ - 1} | {64 * j - 1 for j in range(1, 40)} if p < np_}
    rope = rc.rope_cases()
    assert {(c.Dh, c.H, c.Hkv, c.pad, c.T) for c in rope} == {(d, h, k, p, t) for d in (64, 80, 128, 256) for h, k in ((4, 2), (3, 1)) for p in (0, 8)
                                                              for t in (1, 37, 300)}
    assert 300 * (4 + 2) * 64 // 8 > 256 and (300 * (3 + 1) * 80 // 8) % 256       # several blocks, a ragged last one
    router = rc.router_cases()
    assert {(c.E, c.k) for c in router} == {(2, 1), (2, 2), (8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (16, 4)}
    assert {c.D for c in router} == {8, 504, 512, 520, 4096} and {c.T for c in router} == {1, 5}
    assert {p for c in router if c.T == 1 for p in rc.router_patterns(c)} == set(rc.ROUTER_PATTERNS)
    assert {c.W for c in rc.kv_cases()} == {1, 7, 300} and {c.head_major for c in rc.kv_cases()} == {False, True}
    assert {(c.V, c.M) for c in rc.logprob_cases()} == {(V, M) for V in (1000, 4096) for M in (3, 256)}


def test_caps_hold_for_the_reference_alone(capsys):
    """The bounds the GPU test applies, against what the references and emulations themselves need: the greedy emulation (an fp64
    online softmax in the kernel's order) sits 1e-9 from fp64 log_softmax against the 2e-5 allowed; the router's fp32 softmax puts no
    weight more than one bf16 ulp from bf16(fp64 softmax) (the share that is not bit-equal is printed); rmsnorm, rope and the ring
    writes are bit-equal, no cap."""
    worst = 0.0
    for c in rc.greedy_cases():
        if c.V > 32773:
            continue
        tok, lp = rc.greedy_emulate(c)
        wtok, wlp = rc.greedy_expected(c)
        assert torch.equal(tok, wtok)
        worst = max(worst, float((lp - wlp).abs().max()))
    off = n = 0
    for c in rc.router_cases():
        idx, wt = rc.router_emulate(c)
        widx, wwt, exact = rc.router_expected(c)
        assert torch.equal(idx, widx) and torch.equal(wt[exact], wwt[exact])
        off += int((wt != wwt).sum())
        n += wt.numel()
    with capsys.disabled():
        print(f"\n  greedy emulation against fp64 log_softmax: worst {worst:.3g} (allowed {rc.LP_TOL})"
              f"\n  router weights one bf16 ulp from bf16(fp64 softmax): {off} of {n}", end="")
    assert worst < 1e-9 and off <= n // 20
