"""generate()'s three decoders and the one place that chooses between them, on the CPU (no GPU): the choice table, the three
decoders against each other and the reference's outputs, the draws each path takes from torch's default generator, the
collectives it issues, and that only the host loop enters `graphed_decode` - and leaves it, whichever way the call ends."""
import contextlib
import functools
import types

import pytest
import torch

import mistral_oracle as mo
from golden_util import Case
from mistral_inference import _hip
from mistral_inference import generate as gen_mod
from mistral_inference.args import TransformerArgs
from mistral_inference.cache import BufferCache
from mistral_inference.generate import SpeculativeArgs, _pick_decoder, generate, sample
from mistral_inference.transformer import Transformer
from oracle_backend import OracleStackBackend

PATHS = ("speculative", "session", "loop")
TOL = 2e-5  # test_host_logic.py's: fp32 accumulation-order noise


# ------------------------------------------------------------------------------------------------ the choice table
def _caps(**kw):
    """A model as the chooser sees it: a greedy_session and the attributes' defaults, unless a row says otherwise."""
    base = dict(greedy_session=lambda cache, first: None)
    base.update(kw)
    return types.SimpleNamespace(**{k: v for k, v in base.items() if v is not _ABSENT})


_ABSENT = object()
SPEC = SpeculativeArgs()
#        name                                    model attributes                                  device  temp  max  spec   expected
CHOICES = [
    ("max_tokens 0",                             {},                                               "cuda", 0.0,  0,   None,  "none"),
    ("max_tokens 0 with speculation",            {},                                               "cuda", 0.0,  0,   SPEC,  "none"),
    ("speculative",                              {},                                               "cuda", 0.0,  4,   SPEC,  "speculative"),
    ("speculative on the cpu",                   {"greedy_session": _ABSENT},                      "cpu",  0.0,  1,   SPEC,  "speculative"),
    ("cuda with a session",                      {},                                               "cuda", 0.0,  4,   None,  "session"),
    ("cuda with a session, sampling",            {},                                               "cuda", 0.7,  4,   None,  "session"),
    ("cuda, one token",                          {},                                               "cuda", 0.0,  1,   None,  "session"),
    ("cpu without any_device",                   {},                                               "cpu",  0.0,  4,   None,  "loop"),
    ("cpu, temperature 0, any_device",           {"greedy_session_any_device": True},              "cpu",  0.0,  4,   None,  "session"),
    ("cpu, temperature > 0, any_device",         {"greedy_session_any_device": True},              "cpu",  0.7,  4,   None,  "loop"),
    ("2 ranks without greedy_session_pp",        {"num_pipeline_ranks": 2},                        "cuda", 0.0,  4,   None,  "loop"),
    ("2 ranks, greedy_session_pp False",         {"num_pipeline_ranks": 2, "greedy_session_pp": False}, "cuda", 0.0, 4, None, "loop"),
    ("2 ranks with greedy_session_pp",           {"num_pipeline_ranks": 2, "greedy_session_pp": True},  "cuda", 0.7, 4, None, "session"),
    ("softmax_fp32 False",                       {"softmax_fp32": False},                          "cuda", 0.0,  4,   None,  "loop"),
    ("fused_greedy False",                       {"fused_greedy": False},                          "cuda", 0.0,  4,   None,  "loop"),
    ("no greedy_session attribute",              {"greedy_session": _ABSENT},                      "cuda", 0.0,  4,   None,  "loop"),
]


@pytest.mark.parametrize("name,attrs,device_type,temperature,max_tokens,spec,expected", CHOICES, ids=[c[0] for c in CHOICES])
def test_pick_decoder(name, attrs, device_type, temperature, max_tokens, spec, expected):
    assert _pick_decoder(_caps(**attrs), device_type, temperature, max_tokens, spec) == expected


def test_pick_decoder_reads_the_product_model_as_generate_does():
    m = _standin()
    assert _pick_decoder(m, "cpu", 0.0, 4, None) == "session" and _pick_decoder(m, "cpu", 0.7, 4, None) == "loop"
    m.fused_greedy = False
    assert _pick_decoder(m, "cpu", 0.0, 4, None) == "loop" and _pick_decoder(m, "cuda", 0.0, 4, None) == "loop"


# ------------------------------------------------------------------------------------------------ CPU stand-ins
class CpuSession:
    """GreedySession's surface (run / collect / HIST) with one forward per step; greedy whatever the temperature."""
    HIST = 1024

    def __init__(self, model, cache, first):
        self.m, self.cache, self.tok, self.out = model, cache, first.clone(), []

    def run(self, n):
        for _ in range(n):
            logits = self.m.forward(self.tok, [1] * self.tok.numel(), self.cache)
            self.tok = torch.argmax(logits, dim=-1)
            lp = torch.log_softmax(logits, dim=-1).gather(1, self.tok[:, None])[:, 0]
            self.out.append((self.tok.clone(), lp))

    def collect(self, n):
        got, self.out = self.out[:n], self.out[n:]
        assert len(got) == n
        return torch.stack([t for t, _ in got]), torch.stack([l for _, l in got])


def _verify_rows(model, ids, seqlens, cache):
    """verify_step's contract with one forward per row: the argmax and log-prob of every scored row, n_accept = how many
    drafts the argmaxes confirm, and exactly n_accept + 1 rows in the cache (rows behind a refuted draft are never run)."""
    assert len(seqlens) == 1 and ids.shape == (seqlens[0],) and 1 <= seqlens[0] <= 8
    tok, lp, n_accept = torch.zeros_like(ids), torch.zeros(ids.numel()), 0
    for i in range(ids.numel()):
        logits = model.forward(ids[i: i + 1], [1], cache)
        tok[i] = torch.argmax(logits, dim=-1)[0]
        lp[i] = torch.log_softmax(logits, dim=-1)[0, tok[i]]
        if i + 1 == ids.numel() or int(ids[i + 1]) != int(tok[i]):
            break
        n_accept += 1
    return tok, lp, [n_accept]


class Standin(Transformer):
    """The product's Transformer over the oracle, with a CPU session, a CPU verify step and a `graphed_decode` that counts."""
    greedy_session_any_device = True

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.entries, self.sessions, self.fail_after_steps = 0, 0, None

    def greedy_session(self, cache, first_tokens, graph=True):
        self.sessions += 1
        return CpuSession(self, cache, first_tokens)

    def refuse_verify(self, cache, model_only=False):  # (the product refuses fp32 storage: the stand-in below does not need bf16)
        pass

    def verify_step(self, ids, seqlens, cache):
        return _verify_rows(self, ids, seqlens, cache)

    @contextlib.contextmanager
    def graphed_decode(self, cache):
        self.entries += 1
        self._graphed = {"cache": None}  # (no cache is this one: forward() stays on its plain route)
        try:
            yield self
        finally:
            self._graphed = None

    def forward(self, input_ids, seqlens, cache=None, images=None, **kw):
        if self.fail_after_steps is not None and all(s == 1 for s in seqlens):
            if self.fail_after_steps == 0:
                raise RuntimeError("the stand-in's forward fails here")
            self.fail_after_steps -= 1
        return super().forward(input_ids, seqlens, cache, images, **kw)


@pytest.fixture(autouse=True, scope="module")
def _rope_table_once():
    """The oracle backend builds its rotary table anew in every forward, most of a forward's time at this size: the same
    table, built once for this module's few hundred generations."""
    mp = pytest.MonkeyPatch()
    mp.setattr(mo, "rope_angles", functools.lru_cache(maxsize=None)(mo.rope_angles))
    yield
    mp.undo()


@functools.lru_cache(maxsize=None)
def _case():
    case = Case("dense_fp32")
    return case, case.weights()


def _standin(cls=Standin):
    case, w = _case()
    a = TransformerArgs.from_dict(case.params)
    a.max_batch_size = case.max_batch_size
    m = cls(a, backend=OracleStackBackend())
    m.load_state_dict(w, assign=True)
    return m


def _drafter(prompt, ref):
    """Two right drafts and a wrong one per step: every verify step accepts some rows and rejects one."""
    V = _case()[0].args.vocab_size

    def draft(history):
        at = len(history) - len(prompt)
        return ref[at: at + 2] + [(ref[at + 2] + 1) % V if at + 2 < len(ref) else 0]
    return draft


def _run(m, path, prompts, ref, **kw):
    """One generation on the named path; the model's counters say that it was that path."""
    m.fused_greedy = path == "session"
    spec = SpeculativeArgs(k=3, drafter=_drafter(prompts[0], ref)) if path == "speculative" else None
    before = (m.sessions, m.entries)
    out = generate(prompts, m, speculative=spec, **kw)
    if kw["max_tokens"] > 0:
        assert (m.sessions > before[0], m.entries > before[1]) == (path == "session", path == "loop") or (
            path == "session" and out[0] == [])  # (first token EOS: no session is made)
    return out


# ------------------------------------------------------------------------------------------------ three decoders, one answer
@pytest.mark.parametrize("max_tokens", [0, 1, 2, None], ids=["0", "1", "2", "all"])
def test_three_decoders_one_answer(max_tokens):
    """One prompt at temperature 0 through each decoder, without an eos_id and with every token of the reference run as one:
    the reference's tokens (up to the first eos, which is not returned) and log-probs from all three."""
    case, _ = _case()
    m = _standin()
    prompts, ref, ref_lp = case.prompts[:1], case.tokens()[0], case.logprobs()[0]
    n_prompt = len(prompts[0]) - 1
    assert len(ref) == case.max_tokens and case.max_tokens > 2
    max_tokens = case.max_tokens if max_tokens is None else max_tokens
    for eos in [None] + ref:
        want = ref[:max_tokens]
        if eos in want:
            want = want[: want.index(eos)]   # generate.py:128-132
        got = {p: _run(m, p, prompts, ref, max_tokens=max_tokens, temperature=0.0, chunk_size=case.chunk_size, eos_id=eos)
               for p in PATHS}
        for p, (toks, lps) in got.items():
            assert toks == ([want] if want else []), (p, eos, toks)
            assert len(lps) == 1 and len(lps[0]) == n_prompt + len(want), (p, eos)
            assert max(abs(x - y) for x, y in zip(lps[0], ref_lp)) < TOL, (p, eos)
            assert max(abs(x - y) for x, y in zip(lps[0], got["loop"][1][0])) < TOL, (p, eos)


def test_one_token_makes_a_session_and_never_steps_it():
    case, _ = _case()
    m = _standin()
    m.fail_after_steps = 0           # any decode forward raises
    toks, _ = generate(case.prompts, m, max_tokens=1, temperature=0.0, chunk_size=case.chunk_size)
    assert m.sessions == 1 and toks == [r[:1] for r in case.tokens()]


# ------------------------------------------------------------------------------------------------ draws from the default generator
@pytest.mark.parametrize("path", PATHS)
def test_no_draws_at_temperature_0(path):
    case, _ = _case()
    m = _standin()
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    for eos in (None, case.tokens()[0][2]):
        _run(m, path, case.prompts[:1], case.tokens()[0], max_tokens=case.max_tokens, temperature=0.0, eos_id=eos)
        assert torch.equal(torch.get_rng_state(), state)


def test_host_loop_draws_once_per_step_in_step_order():
    """temperature > 0, one rank: the draws are sample()'s own.  The reference is the loop of the reference's generate.py:120-140
    written out here - forward, sample, append - after the same manual_seed."""
    case, _ = _case()
    m = _standin()
    n_new = 5
    torch.manual_seed(77)
    toks, lps = generate(case.prompts, m, max_tokens=n_new, temperature=0.7)
    after = torch.get_rng_state()
    assert m.entries == 1 and m.sessions == 0

    torch.manual_seed(77)
    B, a = len(case.prompts), m.args
    with torch.inference_mode():
        cache = BufferCache(m.n_local_layers, a.max_batch_size, max(map(len, case.prompts)) + n_new, a.n_kv_heads, a.head_dim,
                            a.sliding_window, device=m.device, dtype=m.dtype)
        cache.reset()
        seqlens = [len(p) for p in case.prompts]
        prelogits = m.forward(torch.tensor(sum(case.prompts, [])), seqlens=seqlens, cache=cache)
        last = prelogits.index_select(0, torch.tensor(seqlens).cumsum(0) - 1)
        want_t, want_lp = [[] for _ in range(B)], [[] for _ in range(B)]
        for _ in range(n_new):
            next_token = sample(last, temperature=0.7, top_p=0.8)
            lsm = torch.log_softmax(last, dim=-1)
            for b in range(B):
                want_t[b].append(int(next_token[b]))
                want_lp[b].append(float(lsm[b, next_token[b]]))
            last = m.forward(next_token, seqlens=[1] * B, cache=cache)
    assert toks == want_t
    assert torch.equal(torch.get_rng_state(), after)   # the same number of draws, too
    for b in range(B):
        assert max(abs(x - y) for x, y in zip(lps[b][len(case.prompts[b]) - 1:], want_lp[b])) < TOL
    torch.manual_seed(78)
    assert generate(case.prompts, m, max_tokens=n_new, temperature=0.7)[0] != toks   # (the seed is what decides)


def _cpu_sample_top_p(events):
    def sample_top_p(logits, temperature, top_p, seed=0, offset=0):
        events.append(("first_sample", temperature, top_p, seed, offset))
        tok = torch.argmax(logits, dim=-1)
        return tok, torch.log_softmax(logits, dim=-1).gather(1, tok[:, None])[:, 0]
    return sample_top_p


def _count_randint(monkeypatch, events):
    real = torch.randint

    def randint(*a, **k):
        out = real(*a, **k)
        events.append(("randint", a, int(out[0])))
        return out
    monkeypatch.setattr(torch, "randint", randint)


def test_session_path_draws_one_seed_before_the_session_is_made(monkeypatch):
    """temperature > 0 on the session path (a GPU's; here the chooser is told to take it and the native draw has a CPU
    stand-in): one randint per generation, after the prompt and before the first sample, and that value is the session's seed."""
    events = []

    class Sampled(Standin):
        def greedy_session(self, cache, first_tokens, graph=True, temperature=0.0, top_p=0.8, seed=0):
            events.append(("session", temperature, top_p, seed))
            return CpuSession(self, cache, first_tokens)

        def forward(self, input_ids, seqlens, cache=None, images=None, **kw):
            events.append(("forward", sum(seqlens)))
            return super().forward(input_ids, seqlens, cache, images, **kw)

    case, _ = _case()
    m = _standin(Sampled)
    monkeypatch.setattr(gen_mod, "_pick_decoder", lambda *a: "session")
    monkeypatch.setattr(_hip, "sample_top_p", _cpu_sample_top_p(events))
    _count_randint(monkeypatch, events)
    torch.manual_seed(5)
    drawn = int(torch.randint(0, 2 ** 62, (1,))[0])
    del events[:]
    torch.manual_seed(5)
    toks, _ = generate(case.prompts, m, max_tokens=4, temperature=0.7)
    assert [len(t) for t in toks] == [4] * len(case.prompts)
    kinds = [e[0] for e in events]
    assert kinds.count("randint") == 1 and kinds.count("session") == 1 and kinds.count("first_sample") == 1
    assert kinds[:4] == ["forward", "randint", "first_sample", "session"], kinds
    assert events[1] == ("randint", (0, 2 ** 62, (1,)), drawn)
    assert events[2] == ("first_sample", 0.7, 0.8, drawn, 1 << 63)
    assert events[3] == ("session", 0.7, 0.8, drawn)
    assert m.entries == 0 and m._graphed is None


# ------------------------------------------------------------------------------------------------ the graphed_decode context
@pytest.mark.parametrize("path", PATHS)
def test_only_the_host_loop_enters_graphed_decode(path):
    case, _ = _case()
    m = _standin()
    _run(m, path, case.prompts[:1], case.tokens()[0], max_tokens=case.max_tokens, temperature=0.0)
    assert m.entries == (1 if path == "loop" else 0)
    assert getattr(m, "_graphed", None) is None
    m.entries, m.fail_after_steps = 0, 2   # forward raises in the middle of the decode steps
    with pytest.raises(RuntimeError, match="stand-in's forward fails"):
        _run(m, path, case.prompts[:1], case.tokens()[0], max_tokens=case.max_tokens, temperature=0.0)
    assert m.entries == (1 if path == "loop" else 0)
    assert getattr(m, "_graphed", None) is None


def test_no_tokens_no_decoder():
    case, _ = _case()
    m = _standin()
    for path in PATHS:
        toks, lps = _run(m, path, case.prompts[:1], case.tokens()[0], max_tokens=0, temperature=0.0)
        assert toks == [] and len(lps[0]) == len(case.prompts[0]) - 1
    assert m.entries == 0 and m.sessions == 0 and m._graphed is None


# ------------------------------------------------------------------------------------------------ collectives
class PipelineStage:
    """One stage of a 2-rank pipeline as generate() sees it: `forward` returns the logits every rank holds (a fixed table of
    the last token; the model's own transfers are not generate()'s), `pp_comm` records what generate() itself issues."""
    num_pipeline_ranks = 2
    greedy_session_pp = True
    greedy_session_any_device = True
    dtype = torch.float32
    device = torch.device("cpu")
    n_local_layers = 1
    V = 48

    def __init__(self):
        self.table = torch.randn(self.V, self.V, generator=torch.Generator().manual_seed(3))   # (no draw from the default generator)
        self.args = types.SimpleNamespace(vocab_size=self.V, max_batch_size=1, n_kv_heads=1, head_dim=8, sliding_window=None)
        self.broadcasts = []
        self.pp_comm = types.SimpleNamespace(broadcast=lambda t, src: self.broadcasts.append((tuple(t.shape), src)))

    def eval(self):
        return self

    def forward(self, input_ids, seqlens, cache=None, images=None):
        return self.table[input_ids]

    def greedy_session(self, cache, first_tokens, graph=True, temperature=0.0, top_p=0.8, seed=0):
        return CpuSession(self, cache, first_tokens)

    def verify_step(self, ids, seqlens, cache):
        return _verify_rows(self, ids, seqlens, cache)


@pytest.mark.parametrize("path,temperature,n_broadcasts", [
    ("speculative", 0.0, 0), ("session", 0.0, 0), ("loop", 0.0, 0), ("session", 0.7, 1), ("loop", 0.7, 1)])
def test_collectives_generate_issues_on_two_ranks(monkeypatch, path, temperature, n_broadcasts):
    m = PipelineStage()
    m.fused_greedy = path == "session"
    if path == "session" and temperature > 0:   # (a GPU's path: the chooser is told, the native draw has a CPU stand-in)
        monkeypatch.setattr(gen_mod, "_pick_decoder", lambda *a: "session")
        monkeypatch.setattr(_hip, "sample_top_p", _cpu_sample_top_p([]))
    spec = SpeculativeArgs(k=2, drafter=lambda history: [1, 2]) if path == "speculative" else None
    events = []
    _count_randint(monkeypatch, events)
    torch.manual_seed(9)
    toks, _ = generate([[5, 7, 11]], m, max_tokens=6, temperature=temperature, speculative=spec)
    assert len(toks[0]) == 6
    assert m.broadcasts == [((1,), 0)] * n_broadcasts     # the seed, from rank 0
    assert len(events) == n_broadcasts                    # ... drawn once, and nothing else drawn: sample() gets (seed, step)
