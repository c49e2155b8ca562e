"""Sampled verify steps (speculative decoding at temperature > 0), host side (no GPU): the rule of include/mistral_hip.h
`mi_verify_sample` as tests/spec_sampling_util.py restates it preserves the sampler's distribution - by exact enumeration, no
Monte Carlo -; the variate grids of the GPU test leave enough variates counted; the refusal surface; generate() on a CPU stand-in
whose verify_step is the util's rule; the new symbol and what it refuses before any launch."""
import ctypes as C
import itertools

import pytest
import torch

import spec_sampling_util as su
from mistral_inference import _hip
from mistral_inference.generate import SpeculativeArgs, generate, refuse_speculative
from test_generate_decoders_host import Standin, _case, _standin
from test_speculative_host import _stub

NINF = -float("inf")
ARG = -1  # MI_ERR_ARG
# (row, temperature, top_p): V = 5 .. 40, ties, -inf entries, a tie across the cut, a one-token nucleus
SMALL = {
    "plain5": (torch.tensor([1.0, 0.5, -0.25, 2.0, 0.0]), 0.7, 0.8),
    "ties_across_the_cut": (torch.tensor([2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0]), 1.0, 0.6),
    "neg_inf": (torch.tensor([0.5, NINF, 1.5, NINF, 0.25, 1.5, NINF, -1.0, 0.0]), 0.7, 0.8),
    "sole_survivor": (torch.tensor([0.0, 9.0, 0.5, 1.0, -2.0, 0.25]), 0.05, 0.8),
    "all_equal": (torch.full((12,), -1.25), 0.7, 0.8),
    "p1_everything_kept": (torch.tensor([0.3, NINF, 0.1, 0.2, 0.3, -0.4]), 1.0, 1.0),
    "wide40": (torch.randn(40, generator=torch.Generator().manual_seed(40)) * 2.0, 0.7, 0.8),
}


def _nuc(name):
    row, t, p = SMALL[name]
    return su.Nucleus(row, t, p), row


def test_the_small_rows_hold_the_required_drafts():
    """Outside the nucleus; tied at the cut, kept and not kept; the sole nucleus token."""
    nuc, row = _nuc("ties_across_the_cut")
    d = su.drafts_for(nuc, row)
    assert {"first_outside", "tied_kept", "tied_left_out"} <= set(d)
    assert row[d["tied_kept"]] == row[d["tied_left_out"]] and nuc.prob(d["tied_kept"]) > 0 and nuc.prob(d["tied_left_out"]) == 0
    assert d["tied_kept"] < d["tied_left_out"]                      # ascending id decides among the ties
    sole, _ = _nuc("sole_survivor")
    assert sole.prob(1) == 1.0 and int((sole.mass > 0).sum()) == 1
    inf, row = _nuc("neg_inf")
    assert inf.prob(su.drafts_for(inf, row)["neg_inf"]) == 0
    full, _ = _nuc("p1_everything_kept")
    assert full.prob(1) == 0 and int((full.mass > 0).sum()) == 5    # top_p = 1: all of the finite ones


@pytest.mark.parametrize("name", sorted(SMALL))
def test_accept_or_residual_is_the_sampler_distribution_for_every_draft(name):
    """P(d) * delta_d + (1 - P(d)) * R_d == P to 1e-12, for every possible draft id of the row."""
    nuc, _ = _nuc(name)
    P = nuc.P()
    assert abs(float(P.sum()) - 1) < 1e-12
    for d in range(nuc.V):
        pd = nuc.prob(d)
        assert pd == float(P[d])
        mix = torch.zeros_like(P)
        mix[d] = pd
        if pd < 1.0:
            R = nuc.residual(d)
            assert float(R[d]) == 0 and abs(float(R.sum()) - 1) < 1e-12
            mix += (1 - pd) * R
        assert float((mix - P).abs().max()) < 1e-12, (name, d)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_rule_with_variates_draws_those_distributions(name):
    """`decide` / `draw` at the midpoint of every interval of the variates realise exactly P(d), R_d and P: the accept interval is
    [0, P(d)), and the inverse CDF gives token k on an interval of length R_d(k) (plain draw: P(k)), in the kept order."""
    nuc, _ = _nuc(name)
    P = nuc.P()
    for d in list(range(nuc.V)) + [None]:
        dist = P if d is None else (nuc.residual(d) if nuc.prob(d) < 1.0 else None)
        if d is not None:
            pd = nuc.prob(d)
            if pd > 0:
                assert nuc.decide(d, 0.5 * pd, 0.3)[:2] == (True, d) and nuc.decide(d, 0.0, 0.3)[:2] == (True, d)
            if pd < 1:
                assert nuc.decide(d, 0.5 * (1 + pd), 0.3)[0] is False and nuc.decide(d, pd, 0.3)[0] is False
        if dist is None:
            continue
        by_pos = dist[nuc.order]
        cdf = torch.cumsum(by_pos, 0)
        for k in (by_pos > 0).nonzero()[:, 0].tolist():
            mid = float(cdf[k] - 0.5 * by_pos[k])
            got = nuc.draw(d, mid)[0] if d is None else nuc.decide(d, 0.999999999, mid)[1]
            if d is not None and nuc.prob(d) > 0.999999999:
                continue
            assert got == int(nuc.order[k]), (name, d, k)


def test_the_law_of_n_accept_over_a_three_row_sequence():
    """Rows 0, 1, 2 with drafts d1, d2: n_accept is 0 / 1 / 2 with probability 1 - P0(d1) / P0(d1)(1 - P1(d2)) / P0(d1) P1(d2), and
    every emitted token is distributed as its row's P - integrated exactly over the variates: the rule is piecewise constant in
    them, so one point per piece, weighted by the piece's length."""
    names = ["wide40", "ties_across_the_cut", "plain5"]
    rows = [_nuc(n)[0] for n in names]
    for d1, d2 in [(int(rows[0].order[1]), int(rows[1].order[2])), (int(rows[0].order[0]), su.drafts_for(rows[1], SMALL[names[1]][0])["tied_left_out"])]:
        p1, p2 = rows[0].prob(d1), rows[1].prob(d2)

        def pieces(cuts):
            """(midpoint, length) of the intervals of [0, 1) that the sorted `cuts` bound."""
            edges = [0.0] + [c for c in cuts if 0 < c < 1] + [1.0]
            return [(0.5 * (a + b), b - a) for a, b in zip(edges, edges[1:]) if b > a]

        def draw_pieces(nuc, d):
            dist = (nuc.P() if d is None else nuc.residual(d))[nuc.order]
            return pieces(torch.cumsum(dist[dist > 0], 0).tolist()[:-1])

        law = {0: 0.0, 1: 0.0, 2: 0.0}
        emitted = [torch.zeros(r.V, dtype=torch.float64) for r in rows]
        reach = [0.0, 0.0, 0.0]
        acc = [pieces([p1]), pieces([p2]), [(0.5, 1.0)]]
        for (a0, w0), (a1, w1) in itertools.product(acc[0], acc[1]):
            # the draw variate matters only where a row draws: rejecting rows and the last row
            first = su.verify_sample_reference(rows, [0, d1, d2], [0, 3], None, None, [[a0, 0.5], [a1, 0.5], [0.5, 0.5]])[2][0]
            drawing = rows[first]
            removed = [d1, d2, None][first]
            for ud, wd in draw_pieces(drawing, removed):
                u = [[a0, 0.5], [a1, 0.5], [0.5, 0.5]]
                u[first][1] = ud
                tok, lp, n_acc, _ = su.verify_sample_reference(rows, [0, d1, d2], [0, 3], None, None, u)
                w = w0 * w1 * wd
                assert n_acc == [first]
                law[first] += w
                for i in range(first + 1):
                    emitted[i][tok[i]] += w
                    assert float(lp[i]) == float(rows[i].lsm[tok[i]])
                assert tok[first + 1:].tolist() == [-1] * (2 - first) and lp[first + 1:].tolist() == [0.0] * (2 - first)
        assert abs(law[0] - (1 - p1)) < 1e-12 and abs(law[1] - p1 * (1 - p2)) < 1e-12 and abs(law[2] - p1 * p2) < 1e-12
        reach = [1.0, p1, p1 * p2]
        for i in range(3):   # row i's token, given that the scan reached it, is distributed as P_i
            if reach[i] > 0:
                assert float((emitted[i] / reach[i] - rows[i].P()).abs().max()) < 1e-12, (d1, d2, i)


@pytest.mark.parametrize("name", sorted(su.gpu_rows()))
def test_the_gpu_grid_leaves_nine_variates_in_ten_counted(name):
    """The GPU leaf test does not count a sequence whose variate sat within min(2e-6, step / 4) of a decision point; its grid
    is chosen so that the rule alone leaves at least 90 % of them counted on every row and draft kind, checked here."""
    row, t, p, nuclei, ids, q_start, u, kinds = su.two_row_problem(name, su.n_variates(name))
    tok, lp, n_acc, near = su.verify_sample_reference(nuclei, ids, q_start, t, p, u)
    counted = su.counted_sequences(q_start, near)
    assert abs(nuclei[0].oracle_kept - int((nuclei[0].mass > 0).sum())) <= max(2, nuclei[0].oracle_kept // 2000)
    for kind in set(kinds):
        sel = torch.tensor([k == kind for k in kinds])
        assert float(counted[sel].double().mean()) >= 0.9, (name, kind)
    need = {"mode", "last_kept", "first_outside"}
    assert need <= set(kinds) or name == "v32773_fp32_cold"
    # both outcomes occur where both can
    acc = torch.tensor(n_acc)
    assert int(acc.max()) == 1 and int(acc.min()) == 0


@pytest.mark.parametrize("split", sorted(su.SPLITS))
def test_the_eight_row_launches_run_deep_and_stay_counted(split):
    q_start = su.SPLITS[split]
    rows, nucs, t, p, launches = su.eight_row_launches(split)
    depth, counted = [], 0
    for which, ids, u in launches:
        tok, lp, n_acc, near = su.verify_sample_reference([nucs[w] for w in which], ids, q_start, t, p, u)
        ok = su.counted_sequences(q_start, near)
        depth += [a for a, c in zip(n_acc, ok.tolist()) if c]
        counted += int(ok.sum())
    assert counted >= 0.9 * len(launches) * (len(q_start) - 1)
    assert max(depth) == max(b - a for a, b in zip(q_start, q_start[1:])) - 1 and min(depth) == 0


def test_the_frequency_problem_has_a_draft_of_probability_three_tenths():
    row, t, p, d = su.frequency_problem()
    nuc = su.Nucleus(row, t, p)
    assert abs(nuc.prob(d) - 0.3) < 1e-3 and int((nuc.P() * 4096 >= 25).sum()) >= 5   # well-populated tokens for the histogram


# ------------------------------------------------------------------------------------------------ the refusal surface
def test_refusals_at_temperature_above_zero():
    ok = _stub()
    refuse_speculative(ok, 1, 0.7, None, SpeculativeArgs(sample=True))
    refuse_speculative(ok, 1, 0.0, None, SpeculativeArgs(sample=True))        # (the greedy path)
    for spec in (None, SpeculativeArgs()):
        with pytest.raises(NotImplementedError, match=r"temperature 0\.7 > 0.*sample=True"):
            refuse_speculative(ok, 1, 0.7, None, spec)
    with pytest.raises(NotImplementedError, match=r"sample=True"):
        refuse_speculative(ok, 1, 0.7, None)
    # the other refusals do not move with sample=True
    s = SpeculativeArgs(sample=True)
    with pytest.raises(NotImplementedError, match="2 prompts"):
        refuse_speculative(ok, 2, 0.7, None, s)
    with pytest.raises(NotImplementedError, match="FP8 K/V cache"):
        refuse_speculative(ok, 1, 0.7, torch.float8_e4m3fn, s)
    import types
    with pytest.raises(NotImplementedError, match="un-merged LoRA"):
        refuse_speculative(_stub(args=types.SimpleNamespace(lora=object())), 1, 0.7, None, s)
    with pytest.raises(NotImplementedError, match="pipeline ranks"):
        refuse_speculative(_stub(num_pipeline_ranks=2), 1, 0.7, None, s)
    a = SpeculativeArgs()
    assert a.sample is False and SpeculativeArgs(3, 3, 1, None, True).sample is True   # after the existing fields


def test_the_cli_opts_in_when_it_is_given_a_temperature():
    import inspect
    from mistral_inference import main
    assert main.speculative_arg(3).sample is False                    # (speculative_arg itself is unchanged)
    for fn in (main.interactive, main.demo):
        src = inspect.getsource(fn)
        assert "dataclasses.replace(spec, sample=True)" in src and "temperature > 0" in src
    assert inspect.signature(main.interactive).parameters["temperature"].default == 0.7   # mistral-chat --speculative 3 samples


# ------------------------------------------------------------------------------------------------ generate() on a CPU stand-in
def _variates(seed, offset, row):
    g = torch.Generator().manual_seed((seed * 1000003 + offset * 8 + row) % (2 ** 62))
    return torch.rand(2, generator=g, dtype=torch.float64).tolist()


class SamplingStandin(Standin):
    """verify_step at temperature > 0 is the util's rule, one forward per reached row (rows behind a rejection are never run,
    so exactly n_accept + 1 rows enter the cache); the variates are a function of (seed, offset, row)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls, self.seen = [], []

    def verify_step(self, ids, seqlens, cache, *, temperature=0.0, top_p=0.8, seed=0, offset=0):
        self.calls.append((temperature, top_p, seed, offset))
        if temperature == 0:
            return super().verify_step(ids, seqlens, cache)
        m = seqlens[0]
        tok, lp, a = torch.full((m,), -1, dtype=torch.long), torch.zeros(m), 0
        for i in range(m):
            logits = self.forward(ids[i: i + 1], [1], cache)
            nuc = su.Nucleus(logits[0], temperature, top_p)
            u = [_variates(seed, offset, i)]
            sub_ids = [int(ids[i])] + ([int(ids[i + 1])] if i + 1 < m else [])
            t, l, n, _ = su.verify_sample_reference([nuc] * len(sub_ids), sub_ids, [0, len(sub_ids)], temperature, top_p,
                                                    u * len(sub_ids))
            tok[i], lp[i] = t[0], l[0]
            self.seen.append((nuc, int(t[0]), float(l[0])))
            if n[0] == 0:
                break
            a += 1
        return tok, lp, [a]


def _first_sample(logits, temperature, top_p, seed=0, offset=0):
    """The native nucleus draw's CPU stand-in for token 0 (generate() asks `_hip.sample_top_p` for it at offset 2^63)."""
    assert offset == 1 << 63 and logits.shape[0] == 1
    nuc = su.Nucleus(logits[0], temperature, top_p)
    tok = nuc.draw(None, _variates(seed, 7, 7)[1])[0]
    return torch.tensor([tok]), nuc.lsm[tok].float().reshape(1)


@pytest.fixture(scope="module")
def standin():
    import functools
    import mistral_oracle as mo
    mp = pytest.MonkeyPatch()
    mp.setattr(_hip, "sample_top_p", _first_sample)
    mp.setattr(mo, "rope_angles", functools.lru_cache(maxsize=None)(mo.rope_angles))   # (as test_generate_decoders_host.py does)
    yield _standin(SamplingStandin)
    mp.undo()


def _gen(m, seed, max_tokens=10, eos_id=None, drafter=None, temperature=0.7):
    V = _case()[0].args.vocab_size
    prompt = [5, 9, 2, 7, 9, 2]
    drafter = drafter or (lambda h: [(h[-1] * 7 + 1) % V, (h[-1] * 3 + 2) % V, 4])
    m.calls.clear(), m.seen.clear()
    torch.manual_seed(seed)
    toks, lps = generate([prompt], m, max_tokens=max_tokens, temperature=temperature, eos_id=eos_id,
                         speculative=SpeculativeArgs(k=3, drafter=drafter, sample=True))
    return (toks[0] if toks else []), lps[0][len(prompt) - 1:]


def test_generate_on_the_standin_is_reproducible_per_seed(standin):
    a, lpa = _gen(standin, 2025)
    calls = list(standin.calls)
    seen = list(standin.seen)
    b, lpb = _gen(standin, 2025)
    c, _ = _gen(standin, 7)
    assert a == b and lpa == lpb and a != c and len(a) == 10
    # one seed per generation, the step index as the offset, top-p 0.8 as the plain loop
    assert len({s for _, _, s, _ in calls}) == 1 and [o for _, _, _, o in calls] == list(range(len(calls)))
    assert all(t == 0.7 and abs(p - 0.8) < 1e-12 for t, p, _, _ in calls)
    # every emitted token inside the stand-in's nucleus; log-probs are the unscaled log-softmax
    emitted = [(n, t, l) for n, t, l in seen]
    assert len(emitted) >= len(a) - 1
    for (nuc, t, l), tok, lp in zip(emitted, a[1:], lpa[1:]):
        assert t == tok and nuc.prob(tok) > 0 and abs(lp - float(nuc.lsm[tok])) < 1e-6 and abs(l - lp) < 1e-6


def test_generate_on_the_standin_truncates_and_stops_as_the_plain_loop(standin):
    full, lps = _gen(standin, 11, max_tokens=10)
    for n in (1, 2, 5):
        short, lp_short = _gen(standin, 11, max_tokens=n)
        # exactly max_tokens tokens; the drafts are cut to what may still be emitted, so only the steps before the cut repeat
        assert len(short) == n == len(lp_short) and short[0] == full[0]
    eos = full[4]
    first = full.index(eos)
    stopped, lp_stopped = _gen(standin, 11, max_tokens=10, eos_id=eos)
    assert stopped == full[:first] and lp_stopped == lps[:first]   # the EOS token itself is not returned
    # temperature 0 with sample=True is the greedy path: verify_step is called without a new keyword
    greedy, _ = _gen(standin, 11, temperature=0.0)
    assert all(c == (0.0, 0.8, 0, 0) for c in standin.calls)
    torch.manual_seed(11)
    V = _case()[0].args.vocab_size
    plain, _ = generate([[5, 9, 2, 7, 9, 2]], standin, max_tokens=10, temperature=0.0,
                        speculative=SpeculativeArgs(k=3, drafter=lambda h: [(h[-1] * 7 + 1) % V]))
    assert greedy == plain[0]


# ------------------------------------------------------------------------------------------------ the library, before any launch
def test_mi_verify_sample_is_exported_and_declared():
    import os
    import re
    L = _hip.lib()
    assert "mi_verify_sample" in _hip.EXPORTED_SYMBOLS and hasattr(L, "mi_verify_sample") and L.mi_abi_version() == 9
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert re.search(r"\bmi_verify_sample\(", open(os.path.join(root, "include", "mistral_hip.h")).read())
    assert "mi_verify_sample" in open(os.path.join(root, "examples", "abi_probe.c")).read()


def test_mi_verify_sample_argument_checks():
    L = _hip.lib()

    def call(T=8, B=2, vocab=16, ld=16, t=0.7, p=0.8, logits=1, ids=1, q_start=1, tokens=1, logprobs=1, n_accept=1):
        rc = L.mi_verify_sample(logits, ld, T, B, vocab, ids, q_start, t, p, 0, 0, None, tokens, logprobs, n_accept, None)
        return rc, L.mi_last_error_detail().decode()

    for t in (0.0, -1.0):
        rc, why = call(t=t)
        assert rc == ARG and "temperature" in why and "mi_verify_sample" in why
    for p in (1.5, -0.1, float("nan")):
        rc, why = call(p=p)
        assert rc == ARG and "top_p" in why
    for kw in (dict(tokens=None), dict(logprobs=None), dict(n_accept=None), dict(logits=None), dict(ids=None), dict(q_start=None)):
        assert call(**kw)[0] == ARG, kw
    rc, why = call(T=2, B=3)
    assert rc == ARG and "B 3" in why
    assert call(T=0, B=0)[0] == ARG and call(ld=8)[0] == ARG and call(vocab=0)[0] == ARG


def test_mi_forward_verify_checks_top_p_of_a_sampled_step():
    from test_abi import _tiny_model
    from test_speculative_host import _out, _verify_batch
    L = _hip.lib()
    m = _tiny_model()
    m.tok_embeddings = 1
    for p in (1.5, -0.25):
        bt, vo = _verify_batch(sample_temperature=0.7, sample_top_p=p), _out()
        assert L.mi_forward_verify(C.byref(m), None, None, C.byref(bt), C.byref(vo), None) == ARG
        assert "sample_top_p" in L.mi_last_error_detail().decode()
    bt, vo = _verify_batch(sample_temperature=-1.0, sample_top_p=0.8, workspace_bytes=1 << 30), _out()
    assert L.mi_forward_verify(C.byref(m), None, None, C.byref(bt), C.byref(vo), None) == ARG
    assert "sample_temperature" in L.mi_last_error_detail().decode()
