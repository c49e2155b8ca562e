"""Transformer.verify_step (mi_forward_verify): rejected drafts leave no trace in the rings, accepted rows enter them as a prefill
chunk would have written them, and the step's logits are the chunked route's up to one summation order.

Models (verify_util.py): dim 512, 4 heads, 2 kv heads, head_dim 128, hidden 1024, vocab 512, 2 layers, rings of 32 slots; a dense
one and a 4-expert top-2 one.  Cached positions before the step: 9 (the ring does not wrap under the step) and 75 (wrapped
twice: every slot the step could touch holds a position that some row of the step still sees).

Step parity bound.  MEASURED on the commit before this feature, on these models and at these
positions (four prompts each): max |dlogit| between a decode step and a one-token prefill chunk at the same position - two routes
that differ in the attention kernel and its summation order, as the verify step differs from either - is
    ROUTE_SPREAD = 0.03125      (one bf16 ulp of a logit in [4, 8); 14 of the 16 samples show 0.0078125)
and a verify step may differ from the chunked route by 2 x that: one more attention summation order, one more spread.
    STEP_BOUND = 0.0625
test_parent_routes_spread re-measures the spread on every run and fails if the recorded figure no longer holds."""
import pytest
import torch

import verify_util as vu

pytestmark = pytest.mark.gpu

ROUTE_SPREAD = 0.03125
STEP_BOUND = 2 * ROUTE_SPREAD
POSITIONS = [9, 75]
W = vu.W


@pytest.fixture(scope="module", params=["dense", "moe"])
def model(request, tmp_path_factory):
    return vu.load(vu.make_folder(request.param, tmp_path_factory), B=2)


def _prefilled(model, lens, seed=0):
    """A cache holding one prompt per sequence, and each sequence's first greedy token (not yet cached)."""
    prompts = [vu.prompt(n, seed + b) for b, n in enumerate(lens)]
    cache = vu.new_cache(len(lens))
    with torch.inference_mode():
        logits = model.forward(torch.tensor(sum(prompts, []), device="cuda"), list(lens), cache)
    ends = torch.tensor(lens).cumsum(0) - 1
    return cache, [int(t) for t in logits[ends].argmax(-1)]


def _chains(model, cache, t0, n_drafts):
    """The step's own argmaxes: sequence b's chain t0, g_0, g_1, ..., g_n with n = n_drafts[b] (2 + n tokens: the first 1 + n are
    the ids of an all-right step, the last one is the argmax of its last row), grown one draft at a time by verify steps on
    clones of the cache - row i of a step depends on rows <= i only."""
    chains = [[t] for t in t0]
    with torch.inference_mode():
        while any(len(c) < 2 + n for c, n in zip(chains, n_drafts)):
            ids = [c[:1 + n] for c, n in zip(chains, n_drafts)]
            lens = [len(c) for c in ids]
            tok, _, n_acc = model.verify_step(torch.tensor(sum(ids, []), device="cuda"), lens, vu.clone_cache(cache))
            assert n_acc == [n - 1 for n in lens], (n_acc, lens)          # every draft so far is the step's own argmax
            ends = torch.tensor(lens).cumsum(0) - 1
            for b, c in enumerate(chains):
                if len(c) < 2 + n_drafts[b]:
                    c.append(int(tok[ends[b]]))
    return chains


def _snapshot(cache):
    return [(vu.bits(cache.cache_k[l]).clone(), vu.bits(cache.cache_v[l]).clone()) for l in range(cache.n_layers)]


def _check_step(model, cache, ids_per_seq, chains, want_accept):
    """One verify step: acceptance, emitted tokens, positions, and every ring byte."""
    B = len(ids_per_seq)
    lens = [len(x) for x in ids_per_seq]
    seen = list(cache._seen)
    before = _snapshot(cache)
    twin = vu.clone_cache(cache)
    with torch.inference_mode():
        tok, lp, n_acc = model.verify_step(torch.tensor(sum(ids_per_seq, []), device="cuda"), lens, cache)
    assert n_acc == want_accept, (n_acc, want_accept)
    tok, lp = tok.tolist(), lp.tolist()
    off = 0
    for b in range(B):
        a = want_accept[b]
        assert tok[off:off + a + 1] == chains[b][1:a + 2], (b, tok[off:off + a + 1], chains[b])   # argmaxes of rows 0 .. a
        assert all(x <= 0.0 for x in lp[off:off + lens[b]])
        off += lens[b]
    assert cache._seen == [p + a + 1 for p, a in zip(seen, want_accept)]
    assert cache.kv_seqlens.tolist() == cache._seen
    # what a prefill chunk of the accepted rows writes into layer 0 (the same GEMV kernels): bit-equal in the accepted slots
    with torch.inference_mode():
        model.forward(torch.tensor(sum((x[:a + 1] for x, a in zip(ids_per_seq, want_accept)), []), device="cuda"),
                      [a + 1 for a in want_accept], twin)
    for l in range(cache.n_layers):
        for which, (ring, old) in enumerate(zip((cache.cache_k[l], cache.cache_v[l]), before[l])):
            now = vu.bits(ring)
            accepted = torch.zeros(now.shape[:2], dtype=torch.bool, device=now.device)      # [sequence, slot]
            for b in range(B):
                for i in range(want_accept[b] + 1):
                    accepted[b, (seen[b] + i) % W] = True
            keep = ~accepted[:, :, None, None].expand_as(now)
            assert torch.equal(now[keep], old[keep]), ("a ring byte outside the accepted slots changed", l, "kv"[which])
            if l == 0:
                ref = vu.bits((twin.cache_k[0], twin.cache_v[0])[which])
                take = accepted[:, :, None, None].expand_as(now)
                assert torch.equal(now[take], ref[take]), ("accepted rows differ from the chunk's", "kv"[which])
                assert not torch.equal(now[take], old[take])


@pytest.mark.parametrize("p", POSITIONS)
def test_rejected_drafts_leave_no_trace(model, p):
    V = vu.DENSE.vocab_size
    cache, t0 = _prefilled(model, [p])
    chain = _chains(model, cache, t0, [7])[0]                    # t0, g_0 .. g_7; drafts d_i = g_(i-1)
    right = chain[1:8]
    cases = [(right, 7)]                                         # all right
    for j in range(7):                                           # wrong at draft j (the later ones stay the chain's)
        cases.append((right[:j] + [(right[j] + 1) % V] + right[j + 1:], j))
    cases.append(([(t + 1) % V for t in right], 0))              # all wrong
    cases.append(([], 0))                                        # no drafts
    for drafts, want in cases:
        _check_step(model, vu.clone_cache(cache), [[chain[0]] + drafts], [chain], [want])


def test_two_sequences_with_different_rows_and_accept_counts(model):
    V = vu.DENSE.vocab_size
    cache, t0 = _prefilled(model, [9, 75])
    chains = _chains(model, cache, t0, [2, 4])
    ids0 = chains[0][:3]                                          # m = 3: both drafts right
    ids1 = chains[1][:2] + [(chains[1][2] + 1) % V] + chains[1][3:5]   # m = 5: the second draft wrong
    _check_step(model, cache, [ids0, ids1], chains, [2, 1])
    # the cache goes on: a plain decode step on it matches a twin that took the accepted tokens through the chunked route
    twin, _ = _prefilled(model, [9, 75])
    with torch.inference_mode():
        model.forward(torch.tensor(ids0 + ids1[:2], device="cuda"), [3, 2], twin)
        nxt = torch.tensor([chains[0][3], chains[1][2]], device="cuda")                 # the last token each sequence emitted
        a, b = model.forward(nxt, [1, 1], cache), model.forward(nxt, [1, 1], twin)
    assert float((a - b).abs().max()) <= STEP_BOUND, float((a - b).abs().max())


@pytest.mark.parametrize("p", POSITIONS)
def test_step_logits_match_the_chunked_route(model, p):
    cache, t0 = _prefilled(model, [p])
    worst = 0.0
    for m in (1, 2, 5, 8):
        chain = _chains(model, cache, t0, [m - 1])[0]
        ids = torch.tensor(chain[:m], device="cuda")
        with torch.inference_mode():
            _, lp, _, got = model.verify_step(ids, [m], vu.clone_cache(cache), return_logits=True)
            ref = model.forward(ids, [m], vu.clone_cache(cache))
        d = float((got - ref).abs().max())
        print(f"p={p} m={m}: verify step to chunked route max |dlogit| = {d:.6f} (bound {STEP_BOUND})")
        worst = max(worst, d)
        assert float((lp - torch.log_softmax(got, -1).max(-1).values).abs().max()) <= 1e-5
    assert worst <= STEP_BOUND, worst


def test_parent_routes_spread(model):
    """The figure the bound stands on: a decode step against a one-token prefill chunk at the same position (sequence 0 of a
    two-sequence batch whose other sequence brings two rows, which selects the prefill branch)."""
    worst = 0.0
    for p in POSITIONS:
        for seed in range(4):
            pr = vu.prompt(p, seed)
            cache = vu.new_cache(2)
            with torch.inference_mode():
                lg = model.forward(torch.tensor(pr + pr, device="cuda"), [p, p], cache)
                t = int(lg[p - 1].argmax())
                twin = vu.clone_cache(cache)
                a = model.forward(torch.tensor([t, t], device="cuda"), [1, 1], cache)
                b = model.forward(torch.tensor([t, t, 5], device="cuda"), [1, 2], twin)
            worst = max(worst, float((a[0] - b[0]).abs().max()))
    print(f"decode step to one-token prefill chunk: max |dlogit| = {worst:.6f} (recorded {ROUTE_SPREAD})")
    assert worst <= ROUTE_SPREAD, worst


def test_verify_step_refusals(model):
    cache, t0 = _prefilled(model, [9])
    with pytest.raises(ValueError, match="1 .. 8 rows"):
        model.verify_step(torch.zeros(9, dtype=torch.long, device="cuda"), [9], cache)
    with pytest.raises(ValueError, match="at least one per sequence"):
        model.verify_step(torch.zeros(0, dtype=torch.long, device="cuda"), [0], cache)
    with pytest.raises(ValueError, match="needs a cache"):
        model.verify_step(torch.zeros(1, dtype=torch.long, device="cuda"), [1], None)
    from mistral_inference.cache import BufferCache
    c8 = BufferCache(2, 1, 160, 2, 128, W, device="cuda", dtype=torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="FP8 K/V cache"):
        model.verify_step(torch.zeros(1, dtype=torch.long, device="cuda"), [1], c8)
    assert cache._seen == [9]
