"""CPU proof that the structured generic-linear cases (generic_linear_cases.py) are exact and have teeth at the shapes
test_gpu_generic_linear_structured.py runs, in fp32, fp16 and bf16: the constructions' conditions hold on every case and the
route mirror gives the intended label; the torch emulations of g_gemv_kernel, g_gemm_mfma_kernel and g_gemm_kernel equal the fp64
reference bit for bit inside the guarded buffer; every single-fault mutant fails the very comparison the GPU test applies
(glc.mismatch) on every case it applies to - or is invisible there for a reason that glc.invisible states and that is asserted
here from both sides: a mutant with a reason must leave the buffer unchanged, a mutant without one must change it.

test_every_mutant_is_caught_or_provably_invisible prints the mutant table, test_conditions_and_measured_figures how far the
references sit from each cap (the figures quoted in generic_linear_cases.py)."""
import collections
import functools

import pytest

import generic_linear_cases as glc

CASES = glc.all_cases()
KERNELS = ["gemv", "mfma", "fma"]


@functools.lru_cache(maxsize=None)
def sweep():
    """One pass over every case: (figures {case: dict}, emulation mismatches, {kernel: {family: [(case, mutant, caught, reason)]}})."""
    figs, bad = {}, []
    rep = {k: collections.OrderedDict() for k in KERNELS}
    for case in CASES:
        figs[case] = glc.conditions(case)
        want = glc.expected(case)
        d = glc.mismatch(case, glc.emulate(case), want)
        if d:
            bad.append(d)
        for m in glc.mutants_of(case):
            caught = glc.mismatch(case, glc.emulate(case, m), want)
            rep[case.kernel].setdefault(glc.family(m), []).append((case, m, caught, glc.invisible(case, m)))
    return figs, bad, rep


def test_conditions_hold_and_emulations_equal_the_reference():
    _, bad, _ = sweep()
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_mutant_is_caught_or_provably_invisible(kernel, capsys):
    rep = sweep()[2][kernel]
    missed, phantom = [], []
    with capsys.disabled():
        for fam, rows in rep.items():
            caught = sum(1 for _, _, d, _ in rows if d)
            reasons = collections.Counter(r for _, _, d, r in rows if r)
            print(f"\n  {kernel:5s} {fam:26s} caught {caught}/{len(rows) - sum(reasons.values())}"
                  + "".join(f"  [{n} invisible: {r}]" for r, n in reasons.items()), end="")
            missed += [(c, m) for c, m, d, r in rows if not d and not r]
            phantom += [(c, m, r) for c, m, d, r in rows if d and r]
    assert not missed, (len(missed), missed[:20])
    assert not phantom, (len(phantom), phantom[:20])


def test_every_listed_mutant_family_has_a_case_that_shows_it():
    """... in each of the three types where the family exists there (the rounding faults: fp16 and bf16).  The four faults that no
    exact case can show (glc.NEVER_VISIBLE) must be invisible on every case instead."""
    rep = sweep()[2]
    never = {glc.family(m) for m in glc.NEVER_VISIBLE} - {"swiglu_round"}
    rounding = {"swiglu_round", "residual_single_rounding", "logits_not_rounded"}
    for kernel, mutants in glc.MUTANTS.items():
        for fam in dict.fromkeys(glc.family(m) for m in mutants):
            rows = rep[kernel].get(fam, [])
            assert rows, (kernel, fam, "applies to no case")
            if fam in never:
                assert not any(d for _, _, d, _ in rows), (kernel, fam)
                continue
            for t in ("f16", "bf16") if fam in rounding else ("f32", "f16", "bf16"):
                assert any(d for c, _, d, _ in rows if c.dtype == t), (kernel, fam, t, "changes no case")
    for m in glc.NEVER_VISIBLE:
        assert any(m in glc.mutants_of(c) for c in CASES), m


def test_cases_sit_on_the_edges_they_name():
    for t in ("f32", "f16", "bf16"):
        cs = [c for c in CASES if c.dtype == t]
        gv = [c for c in cs if c.kernel == "gemv"]
        assert {c.M for c in gv} == {1, 2, 3, 4, 5, 8} and {1, 2, 7, 9, 40} <= {c.N for c in gv}
        assert {glc.case_route(c) for c in gv} == {"gemv/MR=1", "gemv/MR=2", "gemv/MR=4", "gemv/MR=8"}
        for K in glc.GEMV_KS[t]:                       # every K of the chunk ladder at both UNR values
            assert {glc.gemv_unr(c.M) for c in gv if c.K == K and c.fam == "plain" and c.epi != glc.SWIGLU and not c.norm} == {2, 4}, (t, K)
        for unr in (2, 4):                             # below a chunk, exactly one, one + a piece, one + a partial second round
            rem = {(c.K // c.EPP) // (64 * unr) * 1000 + (c.K // c.EPP) % (64 * unr) for c in gv if glc.gemv_unr(c.M) == unr}
            one = 2 if t == "f32" else 1               # (fp32: K % 8 == 0 admits one chunk + TWO pieces at the least)
            assert {one, 25 * one, 1000, 1000 + one} <= rem and any(r // 1000 >= 1 and 1 < r % 1000 < 64 * unr for r in rem), (t, unr, sorted(rem))
        assert any(len(c.segs) == 3 and c.segs[0] % 2 == 1 and c.segs[1] % 2 == 0 for c in gv)
        assert {c.N for c in gv if c.epi == glc.SWIGLU and c.fam == "plain"} == {1, 5, 40}
        assert any(c.norm and len(c.segs) == 3 for c in gv) and any(c.norm and len(c.segs) == 1 and c.epi == glc.STORE for c in gv)
        assert {c.active for c in gv if c.active} == {"none", "one"}
        mf = [c for c in cs if c.kernel == "mfma"]
        assert {9, 127, 128, 129, 300} == {c.M for c in mf} and {1, 127, 129, 200} <= {c.N for c in mf}
        assert {8, 24, 32, 40, 72, 200} <= {c.K for c in mf} and any(c.active for c in mf)
        fm = [c for c in cs if c.kernel == "fma"]
        assert {1, 3, 15, 16, 17, 100} <= {c.K for c in fm} and {1, 9, 64, 65} <= {c.M for c in fm} and {1, 63, 65} <= {c.N for c in fm}
        assert any(c.misalign and c.K % 8 == 0 and c.ldx % 8 == 0 for c in fm) and any(c.active for c in fm)
        assert any(c.own_ldr for c in gv) and any(c.own_ldr for c in mf) and any(c.own_ldr for c in fm)
    for c in CASES:
        inp = glc.inputs(c)
        assert c.ldx > c.K and (c.epi != glc.RESIDUAL or (c.ldr != c.N + 8) == c.own_ldr)
        xv = glc.x_view(inp.xbuf, c)                    # the view, mis-aligned or not, lies inside its own allocation
        assert xv.storage_offset() + (c.M - 1) * c.ldx + c.K <= inp.xbuf.numel() and (xv.storage_offset() * c.R.itemsize == 8) == c.misalign


def test_conditions_and_measured_figures(capsys):
    figs = sweep()[0]
    with capsys.disabled():
        count = collections.Counter((c.dtype, c.path) for c in CASES)
        print("\n  cases per (type, route): " + ", ".join(f"{t} {p}: {n}" for (t, p), n in sorted(count.items())) + f"; {len(CASES)} in all")
        plain = [(c, f) for c, f in figs.items() if c.fam == "plain"]
        print(f"  plain: max|y| {max(f['maxy'] for _, f in plain):.0f}, sum|w x| <= {max(f['bound'] for _, f in figs.items()):.0f}, zeros at most "
              f"{100 * max(f['zeros'] for _, f in plain):.1f} % (norm cases aside: {100 * max(f['zeros'] for c, f in plain if not c.norm):.1f} %)")
        sw = [f for c, f in figs.items() if c.epi == glc.SWIGLU]
        print(f"  SwiGLU: a in [{min(f['a'][0] for f in sw):.0f}, {max(f['a'][1] for f in sw):.0f}], b == 0 in at most {100 * max(f['bzeros'] for f in sw):.1f} %")
        for t in ("bf16", "f16"):
            rf = [f for c, f in figs.items() if c.fam == "round" and c.dtype == t]
            dbl = [f["double"] for f in rf if "double" in f]
            print(f"  rounding family {t}: {min(f['miny'] for f in rf):.0f} <= |y| <= {max(f['maxy'] for f in rf):.0f}, not values of T "
                  f"{100 * min(f['inexact'] for f in rf):.1f} .. {100 * max(f['inexact'] for f in rf):.1f} %, ties {100 * min(f['ties'] for f in rf):.1f} .. "
                  f"{100 * max(f['ties'] for f in rf):.1f} %, double rounding visible {100 * min(dbl):.1f} .. {100 * max(dbl):.1f} %", end="\n" if t == "bf16" else "")
    assert len(CASES) >= 100
