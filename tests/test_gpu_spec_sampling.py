"""Sampled verify steps on the GPU (csrc/sampling.hip `verify_sample_kernel` + its scan, `mi_verify_sample`, and behind the LM head
of `mi_forward_verify` at sample_temperature > 0) against the float64 restatement of the rule in tests/spec_sampling_util.py:
  * the leaf with pinned variates: every draft kind on every row, sequences of 2 rows and launches of T = 8 rows as 1, 2 and 3
    sequences.  A sequence one of whose variates sat within min(2e-6, step / 4) of a decision point (a CDF step; P(d) for u_acc)
    is not counted (fp32 exp / 2^-40 fixed point, as tests/test_gpu_sampling.py); at least 90 % must stay counted - the grid
    is checked for that on the CPU, tests/test_spec_sampling_host.py - and none of the counted may differ;
  * its own Philox variates: deterministic per (seed, offset), and 4096 sequences reproduce P and the acceptance probability;
  * the verify step on the tiny fixture of tests/verify_util.py with the ring wrapped, on bf16, FP8 and MXFP4 weights;
  * generate(): reproducible per torch.manual_seed, inside the nucleus, equal to the greedy loop where every nucleus is one token."""
import pytest
import torch

import spec_sampling_util as su
import verify_util as vu
from test_gpu_sampling import _rescore
from test_gpu_speculative import CORRUPT, N, PROMPT, V, folder, garbage_drafter, oracle_drafter, run  # noqa: F401  (fixtures)
from test_gpu_verify_step import STEP_BOUND, W, _snapshot

pytestmark = pytest.mark.gpu
LP_TOL = 2e-5     # the leaf test of the plain sampler's: log_softmax in fp32 against float64
T_SAMPLE, TOP_P = 0.7, 0.8
T_ONE_TOKEN = 0.01  # every nucleus of the confident-head fixture is one token: its top-2 margin is above 4 x STEP_BOUND = 0.25 on
#                     the plain run and so above 0.125 on any route; 511 * exp(-0.125 / 0.01) = 2e-3 of the mode's mass, far below 0.25


def _leaf(nuclei_row, T, ids, q_start, t, p, **kw):
    from mistral_inference import _hip
    logits = nuclei_row.cuda()[None, :].expand(T, nuclei_row.numel()).contiguous()
    tok, lp, n_acc = _hip.verify_sample(logits, ids, torch.tensor(q_start, dtype=torch.int32), t, p, **kw)
    return tok.cpu(), lp.cpu(), n_acc.cpu().tolist()


def _compare(name, got, want, q_start):
    """Counted sequences: equal tokens (the -1 behind a rejection included), equal n_accept, log-probs within LP_TOL."""
    tok, lp, n_acc = got
    w_tok, w_lp, w_acc, near = want
    counted = su.counted_sequences(q_start, near)
    misses = 0
    for b in range(len(q_start) - 1):
        if counted[b]:
            s = slice(q_start[b], q_start[b + 1])
            ok = tok[s].tolist() == w_tok[s].tolist() and n_acc[b] == w_acc[b]
            misses += not ok
            if ok:
                assert float((lp[s].double() - w_lp[s]).abs().max()) < LP_TOL, (name, b)
    share = float(counted.double().mean())
    print(f"{name}: {int(counted.sum())} of {len(counted)} sequences counted, {misses} misses")
    assert share >= 0.9, (name, share)
    assert misses == 0, (name, misses)
    # whatever the variate: an emitted token is a number's, never one of mass 0 unless it is the accepted draft's own
    assert bool(torch.isfinite(lp).all())
    return counted


@pytest.mark.parametrize("name", sorted(su.gpu_rows()))
def test_leaf_matches_the_rule_for_every_draft_kind(name):
    row, t, p, nuclei, ids, q_start, u, kinds = su.two_row_problem(name, su.n_variates(name))
    want = su.verify_sample_reference(nuclei, ids, q_start, t, p, u)
    got = _leaf(row, len(ids), ids, q_start, t, p, uniforms=u)
    _compare(name, got, want, q_start)
    # a draft of mass 0 is never accepted, the sole token of a nucleus always
    nuc = nuclei[0]
    for b, kind in enumerate(kinds):
        pd = nuc.prob(int(ids[2 * b + 1]))
        if pd == 0.0:
            assert got[2][b] == 0, (name, kind)
        if pd == 1.0:
            assert got[2][b] == 1 and int(got[0][2 * b]) == int(ids[2 * b + 1]), (name, kind)


@pytest.mark.parametrize("split", sorted(su.SPLITS))
def test_launches_of_eight_rows_as_one_two_and_three_sequences(split):
    """Rows after the first rejection emit nothing; a row that opens a sequence is nobody's draft (spec_sampling_util.
    eight_row_launches: two logits rows alternating, scans that run deep)."""
    from mistral_inference import _hip
    q_start = su.SPLITS[split]
    rows, nucs, t, p, launches = su.eight_row_launches(split)
    depth, all_counted = [], 0
    for n, (which, ids, u) in enumerate(launches):
        want = su.verify_sample_reference([nucs[w] for w in which], ids, q_start, t, p, u)
        logits = torch.stack([rows[w] for w in which]).cuda()
        tok, lp, n_acc = _hip.verify_sample(logits, torch.tensor(ids), torch.tensor(q_start, dtype=torch.int32), t, p, uniforms=u)
        tok, lp, n_acc = tok.cpu(), lp.cpu(), n_acc.cpu().tolist()
        counted = su.counted_sequences(q_start, want[3])
        for b in range(len(q_start) - 1):
            if counted[b]:
                s = slice(q_start[b], q_start[b + 1])
                assert tok[s].tolist() == want[0][s].tolist() and n_acc[b] == want[2][b], (n, b, tok, want[0], n_acc, want[2])
                assert float((lp[s].double() - want[1][s]).abs().max()) < LP_TOL
                behind = s.stop - s.start - n_acc[b] - 1
                assert tok[s][n_acc[b] + 1:].tolist() == [-1] * behind and lp[s][n_acc[b] + 1:].tolist() == [0.0] * behind
                depth.append(n_acc[b])
        all_counted += int(counted.sum())
    assert all_counted >= 0.9 * len(launches) * (len(q_start) - 1)
    longest = max(b - a for a, b in zip(q_start, q_start[1:]))
    assert max(depth) == longest - 1 and min(depth) == 0, depth     # all accepted somewhere, rejected at once somewhere


def test_philox_variates_are_deterministic_and_reproduce_the_law():
    """4096 two-row sequences with one draft of P(d) near 0.3 and one fixed seed: the first emitted token follows P (the bounds of
    the plain sampler's frequency test), the accepted share P(d) within 5 sigma."""
    row, t, p, d = su.frequency_problem()
    nuc = su.Nucleus(row, t, p)
    pd = nuc.prob(d)
    B = 4096
    ids, q_start = [0, d] * B, list(range(0, 2 * B + 1, 2))
    a = _leaf(row, 2 * B, ids, q_start, t, p, seed=1234, offset=5)
    b = _leaf(row, 2 * B, ids, q_start, t, p, seed=1234, offset=5)
    c = _leaf(row, 2 * B, ids, q_start, t, p, seed=1234, offset=6)
    e = _leaf(row, 2 * B, ids, q_start, t, p, seed=1235, offset=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], e[0]) and a[2] != c[2] and a[2] != e[2]
    tok, _, n_acc = a
    first, second = tok[0::2], tok[1::2]
    acc = torch.tensor(n_acc)
    assert bool((first[acc == 1] == d).all()) and bool((second[acc == 0] == -1).all()) and bool((second[acc == 1] >= 0).all())
    assert bool((first[acc == 0] != d).all())                          # an accepting row emits the draft, a rejecting one never
    share = float(acc.double().mean())
    sigma = (pd * (1 - pd) / B) ** 0.5
    print(f"accepted share {share:.4f}, P(d) {pd:.4f}, sigma {sigma:.4f}")
    assert abs(share - pd) < 5 * sigma
    for emitted in (first, second[acc == 1]):                          # row 0 of every sequence; row 1 where it was reached
        n = emitted.numel()
        exp = nuc.P() * n
        obs = torch.bincount(emitted, minlength=nuc.V).double()
        assert float(obs[exp == 0].sum()) == 0                         # nothing outside the nucleus, ever
        big = exp >= 25
        z = (obs[big] - exp[big]) / exp[big].sqrt()
        assert float(z.abs().max()) < 5.0, float(z.abs().max())        # 5 sigma over the well-populated tokens
        k = int(big.sum())
        assert float((z ** 2).sum()) < k + 6 * (2 * k) ** 0.5, (float((z ** 2).sum()), k)


# ------------------------------------------------------------------------------------------------ the verify step
def _succ():
    """The confident head's favourite successor of every token (verify_util.weights: output[v] leans on the embedding of perm[v])."""
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(vu.SEED + 1000))
    succ = torch.empty(V, dtype=torch.long)
    succ[perm] = torch.arange(V)
    return succ.tolist()


def test_sampled_step_on_a_wrapped_ring(run):
    """Position 75 of 32-slot rings.  ids = the step's own greedy chain, so the greedy step on a twin commits every row; the sampled
    step commits rows 0 .. n_accept of the same stash."""
    from mistral_inference import _hip
    model = run[0]
    prompt = vu.prompt(75, 3)
    cache = vu.new_cache(1)
    m = 5
    with torch.inference_mode():
        t0 = int(model.forward(torch.tensor(prompt, device="cuda"), [75], cache)[-1].argmax())
        ids = [t0]
        while len(ids) < m:                       # grow the chain: row i depends on rows <= i only
            tok, _, n_acc = model.verify_step(torch.tensor(ids, device="cuda"), [len(ids)], vu.clone_cache(cache))
            assert n_acc == [len(ids) - 1]
            ids.append(int(tok[len(ids) - 1]))
        ids_t = torch.tensor(ids, device="cuda")
        twin = vu.clone_cache(cache)
        g_tok, g_lp, g_acc, g_logits = model.verify_step(ids_t, [m], twin, return_logits=True)
        assert g_acc == [m - 1]
        before = _snapshot(cache)
        seen_accepts = set()
        for seed, offset in [(11, 0), (11, 1), (12, 0), (99, 7), (5, 3), (77, 2)]:
            c = vu.clone_cache(cache)
            tok, lp, n_acc, logits = model.verify_step(ids_t, [m], c, return_logits=True, temperature=T_SAMPLE, top_p=TOP_P,
                                                       seed=seed, offset=offset)
            assert torch.equal(logits, g_logits)                                     # the same launches up to the LM head
            l_tok, l_lp, l_acc = _hip.verify_sample(logits, ids_t, torch.tensor([0, m], dtype=torch.int32), T_SAMPLE, TOP_P,
                                                    seed=seed, offset=offset)
            assert torch.equal(tok, l_tok) and torch.equal(lp, l_lp) and n_acc == l_acc.tolist()
            a = n_acc[0]
            seen_accepts.add(a)
            assert tok[:a].tolist() == ids[1:a + 1] and int(tok[a]) >= 0 and tok[a + 1:].tolist() == [-1] * (m - 1 - a)
            assert c._seen == [75 + a + 1] and c.kv_seqlens.tolist() == c._seen
            for l in range(c.n_layers):
                for which, (ring, ring_g, old) in enumerate(zip((c.cache_k[l], c.cache_v[l]), (twin.cache_k[l], twin.cache_v[l]), before[l])):
                    now = vu.bits(ring)
                    accepted = torch.zeros(now.shape[:2], dtype=torch.bool, device=now.device)
                    for i in range(a + 1):
                        accepted[0, (75 + i) % W] = True
                    keep = ~accepted[:, :, None, None].expand_as(now)
                    take = accepted[:, :, None, None].expand_as(now)
                    assert torch.equal(now[keep], old[keep]), ("a ring byte outside the accepted slots changed", l, "kv"[which])
                    assert torch.equal(now[take], vu.bits(ring_g)[take]), ("accepted rows differ from the greedy step's", l, "kv"[which])
        print(f"n_accept over the seeds: {sorted(seen_accepts)}")
        assert len(seen_accepts) > 1, seen_accepts      # the seeds do decide
        # temperature 0 with the new keywords is the greedy step
        tok, lp, n_acc = model.verify_step(ids_t, [m], vu.clone_cache(cache), temperature=0.0, seed=3, offset=9)
        assert torch.equal(tok, g_tok) and torch.equal(lp, g_lp) and n_acc == g_acc
        with pytest.raises((RuntimeError, ValueError)):
            model.verify_step(ids_t, [m], vu.clone_cache(cache), temperature=0.7, top_p=1.5)


# ------------------------------------------------------------------------------------------------ generate()
def _sampled(model, seed, spec, temperature=T_SAMPLE, **kw):
    from mistral_inference.generate import generate
    torch.manual_seed(seed)
    kw.setdefault("max_tokens", N)
    toks, lps = generate([PROMPT], model, temperature=temperature, speculative=spec, **kw)
    return (toks[0] if toks else []), lps[0]


def test_generate_is_reproducible_and_inside_the_nucleus(run):
    from mistral_inference.generate import SpeculativeArgs, generate
    model = run[0]
    succ = _succ()
    steps = []
    orig = model.verify_step

    def counting(ids, seqlens, cache, **kw):
        out = orig(ids, seqlens, cache, **kw)
        steps.append((seqlens[0], out[2][0], kw.get("offset")))
        return out

    def chain(history, k=3):
        out = [succ[history[-1]]]
        while len(out) < k:
            out.append(succ[out[-1]])
        return out
    spec = SpeculativeArgs(k=3, drafter=chain, sample=True)
    model.verify_step = counting
    try:
        toks, lps = _sampled(model, 2025, spec)
    finally:
        del model.verify_step
    assert len(toks) == N and len(lps) == len(PROMPT) - 1 + N
    assert [o for _, _, o in steps] == list(range(len(steps)))                 # offset = the step's index
    accepted = sum(a for _, a, _ in steps)
    print(f"{len(steps)} verify steps for {N} tokens, {accepted} drafts accepted")
    assert 0 < accepted < 3 * len(steps)                                        # drafts are accepted and rejected
    again, lp_again = _sampled(model, 2025, spec)
    assert again == toks and lp_again == lps                                    # torch.manual_seed makes it reproducible
    assert _sampled(model, 7, spec)[0] != toks                                  # ... and another seed another generation
    assert toks != run[1]                                                       # not the greedy tokens
    ref_lp, inside = _rescore(model, [PROMPT], [toks], T_SAMPLE)
    assert inside
    got = torch.tensor(lps[len(PROMPT) - 1:])
    d = float((got - ref_lp[0]).abs().max())
    print(f"max |dlogprob| against the teacher-forced re-score = {d:.6f}")
    assert d < 6e-2                                                             # (_rescore's bound in test_gpu_sampling.py)
    # truncation, the EOS stop, and the refusals that remain
    assert len(_sampled(model, 2025, spec, max_tokens=5)[0]) == 5 and len(_sampled(model, 2025, spec, max_tokens=1)[0]) == 1
    eos = toks[20]
    assert _sampled(model, 2025, spec, eos_id=eos)[0] == toks[:toks.index(eos)]
    with pytest.raises(NotImplementedError, match="sample=True"):
        generate([PROMPT], model, max_tokens=4, temperature=T_SAMPLE, speculative=SpeculativeArgs(k=3))
    with pytest.raises(NotImplementedError, match="one prompt per call"):
        generate([PROMPT, PROMPT], model, max_tokens=4, temperature=T_SAMPLE, speculative=spec)
    with pytest.raises(NotImplementedError, match="FP8 K/V cache"):
        generate([PROMPT], model, max_tokens=4, temperature=T_SAMPLE, speculative=spec, kv_dtype=torch.float8_e4m3fn)


@pytest.mark.parametrize("drafter", ["corrupted_oracle", "garbage"])
def test_one_token_nuclei_give_the_greedy_tokens(run, drafter):
    """At T_ONE_TOKEN every nucleus holds the argmax alone: a right draft is always accepted, a wrong one has mass 0, every draw
    returns the argmax - the plain greedy loop's tokens exactly, and its log-probs within the step bound."""
    from mistral_inference.generate import SpeculativeArgs
    model, ref_t, ref_lp = run
    d = oracle_drafter(ref_t, 3, CORRUPT) if drafter == "corrupted_oracle" else garbage_drafter(3)
    toks, lps = _sampled(model, 1, SpeculativeArgs(k=3, drafter=d, sample=True), temperature=T_ONE_TOKEN)
    assert toks == ref_t
    assert max(abs(a - b) for a, b in zip(lps, ref_lp)) <= STEP_BOUND


def test_the_cache_continues_like_one_that_never_speculated(run):
    """Sampled verify steps by hand on a cache of our own, a twin that takes the same tokens through plain decode steps, then one
    plain decode step on both."""
    model = run[0]
    succ = _succ()
    cache, twin = vu.new_cache(1), vu.new_cache(1)
    with torch.inference_mode():
        for c in (cache, twin):
            last = model.forward(torch.tensor(PROMPT, device="cuda"), [len(PROMPT)], c)
        out = [int(last[-1].argmax())]
        step = 0
        while len(out) < N:
            drafts = [succ[out[-1]], succ[succ[out[-1]]], (out[-1] + 5) % V][:N - len(out) - 1]
            tok, _, n_acc = model.verify_step(torch.tensor([out[-1]] + drafts, device="cuda"), [1 + len(drafts)], cache,
                                              temperature=T_SAMPLE, top_p=TOP_P, seed=31, offset=step)
            out += tok[:n_acc[0] + 1].tolist()
            step += 1
        assert all(0 <= t < V for t in out)
        for t in out[:-1]:
            model.forward(torch.tensor([t], device="cuda"), [1], twin)
        assert cache._seen == twin._seen == [len(PROMPT) + len(out) - 1]
        assert cache.kv_seqlens.tolist() == twin.kv_seqlens.tolist()
        nxt = torch.tensor([out[-1]], device="cuda")
        a, b = model.forward(nxt, [1], cache), model.forward(nxt, [1], twin)
    d = float((a - b).abs().max())
    print(f"decode step after {len(out)} sampled speculative tokens against the twin: max |dlogit| = {d:.6f} (bound {STEP_BOUND})")
    assert d <= STEP_BOUND, d
