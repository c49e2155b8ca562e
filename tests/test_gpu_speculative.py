"""generate(speculative=SpeculativeArgs(...)) returns what plain greedy generate() returns: the same 48 tokens across the wrap of
the 32-slot rings (positions 9 .. 56), log-probabilities within the step bound of test_gpu_verify_step.py, whatever the drafter
proposes - an oracle drafter (the plain run's own tokens) corrupted at chosen indices, a garbage drafter - at k = 1, 3 and 7, on
bf16, FP8 and MXFP4 weights; and the cache a speculative run leaves behind continues like one that never speculated.

Fixture (verify_util.weights: the synthetic weights with a confident LM head; prompt = verify_util.prompt(9, 0)), chosen with the
CPU oracle (oracle/mistral_oracle.py, bf16): over the 48 greedy steps the smallest top-2 logit margin is 1.546875 and the largest
|logit| 5.90625, against 4 x STEP_BOUND = 0.25.  Every test re-checks the condition on the plain run of the model it uses - at
EVERY step, none excluded - and FAILS as a bad fixture where a margin is not above 4 x STEP_BOUND: two summation orders could
then legitimately pick different tokens and token equality would test nothing."""
import pytest
import torch

import verify_util as vu
from test_gpu_verify_step import STEP_BOUND

pytestmark = pytest.mark.gpu

N = 48
PROMPT = vu.prompt(9, 0)
V = vu.DENSE.vocab_size
CORRUPT = {0, 3, 4, 10, 17, 22, 23, 24, 31, 32, 33, 40, 47}     # indices into the generated tokens whose draft is wrong


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return vu.make_folder("dense", tmp_path_factory)


@pytest.fixture(scope="module", params=[None, "fp8_e4m3", "mxfp4"], ids=["bf16", "fp8", "mxfp4"])
def run(request, folder):
    """(model, plain tokens, plain log-probs) with the fixture condition checked on this model's plain run."""
    from mistral_inference.generate import generate
    model = vu.load(folder, B=1, **({"quantize": request.param} if request.param else {}))
    from mistral_inference.quant import QuantLinear
    assert isinstance(model.layers["0"].attention.wq, QuantLinear) == (request.param is not None)
    toks, lps = generate([PROMPT], model, max_tokens=N, temperature=0.0)
    assert len(toks[0]) == N
    # the plain run again, step by step, for its logits: the margin of EVERY step
    cache = vu.new_cache(1)
    margins = []
    with torch.inference_mode():
        last = model.forward(torch.tensor(PROMPT, device="cuda"), [len(PROMPT)], cache)[-1:]
        for i in range(N):
            top2 = torch.topk(last[0], 2).values
            margins.append(float(top2[0] - top2[1]))
            assert int(last.argmax(-1)) == toks[0][i], i
            last = model.forward(last.argmax(-1), [1], cache)
    print(f"{request.param or 'bf16'}: smallest top-2 margin over {N} steps = {min(margins)} (needs > {4 * STEP_BOUND})")
    assert min(margins) > 4 * STEP_BOUND, ("bad fixture: a greedy step of the plain run is too close to call", min(margins))
    return model, toks[0], lps[0]


def oracle_drafter(ref, k, corrupt=frozenset()):
    def draft(history):
        n = len(history) - len(PROMPT)          # tokens emitted so far: the next one is ref[n]
        return [(ref[i] + 1) % V if i in corrupt else ref[i] for i in range(n, min(n + k, len(ref)))]
    return draft


def garbage_drafter(k):
    return lambda history: [(history[-1] * 7 + 13 * (i + 1) + len(history)) % V for i in range(k)]


def _check(run, spec):
    from mistral_inference.generate import generate
    model, ref_t, ref_lp = run
    toks, lps = generate([PROMPT], model, max_tokens=N, temperature=0.0, speculative=spec)
    assert toks == [ref_t]
    assert len(lps[0]) == len(ref_lp) == len(PROMPT) - 1 + N
    assert lps[0][:len(PROMPT) - 1] == ref_lp[:len(PROMPT) - 1]         # the prompt is scored by the same launches
    d = max(abs(a - b) for a, b in zip(lps[0], ref_lp))
    print(f"k={spec.k}: max |dlogprob| = {d:.6f} (bound {STEP_BOUND})")
    assert d <= STEP_BOUND, d


@pytest.mark.parametrize("k", [1, 3, 7])
def test_same_tokens_with_a_corrupted_oracle_drafter(run, k):
    from mistral_inference.generate import SpeculativeArgs
    _check(run, SpeculativeArgs(k=k, drafter=oracle_drafter(run[1], k, CORRUPT)))


@pytest.mark.parametrize("k", [1, 3, 7])
def test_same_tokens_with_a_garbage_drafter(run, k):
    from mistral_inference.generate import SpeculativeArgs
    _check(run, SpeculativeArgs(k=k, drafter=garbage_drafter(k)))


def test_perfect_drafts_are_all_accepted_and_the_default_drafter_runs(run):
    from mistral_inference.generate import SpeculativeArgs, generate
    model, ref_t, _ = run
    steps = []
    orig = model.verify_step

    def counting(ids, seqlens, cache, **kw):
        out = orig(ids, seqlens, cache, **kw)
        steps.append((seqlens[0], out[2][0]))
        return out
    model.verify_step = counting
    try:
        _check(run, SpeculativeArgs(k=7, drafter=oracle_drafter(ref_t, 7)))
        assert all(a == m - 1 for m, a in steps) and len(steps) == 6, steps     # 1 + 5 x 8 + 7: every draft accepted
        del steps[:]
        _check(run, SpeculativeArgs(k=3))                                        # prompt lookup: few matches here; same tokens
        assert steps and all(1 <= m <= 4 for m, _ in steps)
    finally:
        del model.verify_step
    # truncation and the EOS stop follow the plain loop
    for kw in ({"max_tokens": 5}, {"max_tokens": N, "eos_id": ref_t[20]}, {"max_tokens": 1}, {"max_tokens": N, "eos_id": ref_t[0]}):
        want = generate([PROMPT], model, temperature=0.0, **kw)
        got = generate([PROMPT], model, temperature=0.0, speculative=SpeculativeArgs(k=3, drafter=oracle_drafter(ref_t, 3, CORRUPT)), **kw)
        assert got[0] == want[0] and len(got[1][0]) == len(want[1][0]), kw


def test_the_cache_continues_like_one_that_never_speculated(run):
    """The speculative loop by hand on a cache of our own (generate() keeps its cache to itself), a twin that takes the same
    tokens through plain decode steps, then one plain decode step on both."""
    model, ref_t, _ = run
    draft = oracle_drafter(ref_t, 3, CORRUPT)
    cache, twin = vu.new_cache(1), vu.new_cache(1)
    with torch.inference_mode():
        for c in (cache, twin):
            model.forward(torch.tensor(PROMPT, device="cuda"), [len(PROMPT)], c)
        out = [ref_t[0]]
        while len(out) < N:
            drafts = draft(PROMPT + out)[:N - len(out) - 1]
            tok, _, n_acc = model.verify_step(torch.tensor([out[-1]] + drafts, device="cuda"), [1 + len(drafts)], cache)
            out += tok[:n_acc[0] + 1].tolist()
        assert out[:N] == ref_t
        for t in out[:-1]:
            model.forward(torch.tensor([t], device="cuda"), [1], twin)
        assert cache._seen == twin._seen == [len(PROMPT) + len(out) - 1]
        assert cache.kv_seqlens.tolist() == twin.kv_seqlens.tolist()
        nxt = torch.tensor([out[-1]], device="cuda")
        a, b = model.forward(nxt, [1], cache), model.forward(nxt, [1], twin)
    d = float((a - b).abs().max())
    print(f"decode step after 48 speculated tokens against the twin: max |dlogit| = {d:.6f} (bound {STEP_BOUND})")
    assert d <= STEP_BOUND, d
