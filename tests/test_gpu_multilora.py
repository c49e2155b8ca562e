"""Several LoRA adapters in one batch, one per sequence (adapter banks, the bank mode of csrc/lora.hip's kernels, ABI v9).

The reference has one adapter set per model, so the meaning is defined through it: the rows of sequence b are what the reference
computes for that sequence with adapter adapters[b] loaded.  Sequences interact only inside attention, which is per sequence, and
the bank mode of a kernel runs for one (row, column) the loop of its single-adapter mode, the same fp32 operations in the same
order - so every comparison of a mixed batch with uniform batches here is torch.equal; only the anchors to the reference (the
leaf's STORE output at the odd K, the model's stored logits) carry a tolerance."""
import ctypes as C
import itertools

import pytest
import torch

import mistral_oracle as mo
from lora_util import BF, LoraCase, make_adapters, write_lora_checkpoint
from test_gpu_lora import _parts, _widened_store

pytestmark = pytest.mark.gpu
LOGIT_ATOL = 4e-2   # tests/test_gpu_model.py
ENGINE_DIMS = dict(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                   sliding_window=16)   # tests/test_gpu_lora.py
RANK = 16
SEEDS = (5, 6, 7)   # adapters of slots 0, 1, 2
N_STEPS = 12


def _hip():
    from mistral_inference import _hip
    return _hip


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ 1. leaf
def _row_slots(M):
    return list(itertools.islice(itertools.cycle([1, -1, 0, 2, 2, 0]), M))


def _mixed_vs_uniform(h, x, ws, banks_a, banks_b, s, epi, slots, **kw):
    """mi_lora_linear_slots on the banks, and row by row the rows of mi_lora_linear on the row's slot (-1: B = 0)."""
    M = x.shape[0]
    got = h.lora_linear(x, ws, banks_a, banks_b, s, epi, banked=True, row_slot=torch.tensor(slots, dtype=torch.int32, device="cuda"), **kw)
    uniform = {}
    for sl in (-1, 0, 1, 2):
        a = tuple(None if t is None else t[max(sl, 0)] for t in banks_a)
        b = tuple(None if t is None else (torch.zeros_like(t[0]) if sl < 0 else t[sl]) for t in banks_b)
        uniform[sl] = h.lora_linear(x, ws, a, b, s, epi, **kw)
    want = torch.stack([uniform[slots[m]][m] for m in range(M)])
    assert torch.equal(got, want), (epi, M, [m for m in range(M) if not torch.equal(got[m], want[m])])
    assert not torch.equal(uniform[0], uniform[1]) and not torch.equal(uniform[1], uniform[2]) and not torch.equal(uniform[0], uniform[-1])
    # row_slot = NULL: slot 0 on the kernels' single-adapter mode
    assert torch.equal(h.lora_linear(x, ws, banks_a, banks_b, s, epi, banked=True, **kw), uniform[0])
    return got


def _store_against_the_reference(h, x, K, r, s):
    """STORE of mi_lora_linear (136 | 64 | 64 rows, three adapters) against lora_util.lora_linear_ref, every element inside
    test_gpu_lora's widened bound, in its unconditional form: one of the element's two addends on the neighbouring bf16 value,
    plus what one flipped element of t moves d by - granted everywhere, not only behind an observed flip (see the caller)."""
    rows = (136, 64, 64)
    ws = [rnd(n, K, seed=70 + i, scale=K ** -0.5) for i, n in enumerate(rows)]
    As = [rnd(r, K, seed=73 + i, scale=K ** -0.5) for i in range(3)]
    Bs = [rnd(n, r, seed=76 + i, scale=0.25 * r ** -0.5) for i, n in enumerate(rows)]
    cuda = lambda ts: tuple(t.cuda() for t in ts)  # noqa: E731
    y, base, d, _, tflip = _parts(x.cpu(), ws, As, Bs, s)
    wide = _widened_store(y, base, d) + tflip
    err = (h.lora_linear(x, cuda(ws), cuda(As), cuda(Bs), s).cpu().float() - y).abs()
    print(f"M={x.shape[0]} K={K} r={r}: store against the reference, worst err/bound {float((err / wide).max()):.3f}")
    assert bool((err <= wide).all()), float((err / wide).max())
    # teeth, on the CPU reference
    assert bool(((_parts(x.cpu(), ws, As, Bs, 2 * s)[0] - y).abs() > wide).any()), "doubling s stays inside the bound"
    ysw = _parts(x.cpu(), ws, [As[0], As[2], As[1]], [Bs[0], Bs[2], Bs[1]], s)[0]
    assert bool(((ysw - y).abs() > wide).any()), "exchanged adapters stay inside the bound"


# (the K = 256 cases keep the ids they had before K became a parameter)
LEAF_CASES = [pytest.param(M, K, id=str(M) if K == 256 else f"{M}-K{K}") for K in (256, 264, 2312) for M in (1, 3, 5, 8, 9, 40)]


@pytest.mark.parametrize("r", [8, 64])
@pytest.mark.parametrize("M,K", LEAF_CASES)
def test_leaf_mixed_rows_equal_uniform_calls(M, K, r):
    """mi_lora_linear_slots with 3 slots and row_slot cycling through [1, -1, 0, 2, 2, 0]: neighbouring rows differ, the 16-row MFMA
    tiles (M = 40) and the 8-row blocks of lora_up straddle slots.  Row m equals row m of mi_lora_linear with slot row_slot[m]'s
    A / B, bit for bit.  STORE with three unequal segments, the middle one without adapter; RESIDUAL; SWIGLU; the fused norm at
    M <= 8.  M = 1, 3, 5, 8 take the row-streaming lora_down (M = 5: lora_down_rows_kernel<8> on fewer tokens than it holds, and
    five per-token blocks with a bank), 9 and 40 the MFMA form.  K = 264 is a multiple of 8 and not of 32: the dead quarter-waves
    of the MFMA K loop and the dead pieces of the row loop; K = 2312 is 289 pieces: a second, ragged trip of the row loop's 256.
    Both modes of a kernel are one source, so at the new K values (M = 5, 40) the STORE output of mi_lora_linear is also compared
    with the reference (_store_against_the_reference) - a coarse anchor: its bound admits one flipped element of t on EVERY
    element, so it sees a wrong slot, segment or scale, not an error below s * max|B| * |t| * 2^-7 such as one dropped piece of
    the A dot.  The fine-grained contract is test_gpu_lora.test_lora_linear_leaf's."""
    h = _hip()
    s, S = 1.5, 3
    slots = _row_slots(M)
    x = rnd(M, K, seed=20).cuda()
    bank = lambda n, m, seed, scale: rnd(S, n, m, seed=seed, scale=scale).cuda()  # noqa: E731
    # STORE: 136 | 64 | 40 rows, adapters on the first and the last segment
    rows = (136, 64, 40)
    ws = tuple(rnd(n, K, seed=30 + i, scale=K ** -0.5).cuda() for i, n in enumerate(rows))
    A = (bank(r, K, 33, K ** -0.5), None, bank(r, K, 35, K ** -0.5))
    B = (bank(rows[0], r, 36, 0.25 * r ** -0.5), None, bank(rows[2], r, 38, 0.25 * r ** -0.5))
    got = _mixed_vs_uniform(h, x, ws, A, B, s, h.EPI_STORE, slots)
    assert torch.equal(got[:, 136:200], h.linear(x, ws, h.EPI_STORE)[:, 136:200])   # the segment without adapter: mi_linear's
    # RESIDUAL: one segment of 130 rows
    w = (rnd(130, K, seed=40, scale=K ** -0.5).cuda(),)
    A1, B1 = (bank(r, K, 41, K ** -0.5),), (bank(130, r, 42, 0.25 * r ** -0.5),)
    res = rnd(M, 130, seed=43).cuda()
    _mixed_vs_uniform(h, x, w, A1, B1, s, h.EPI_RESIDUAL, slots, residual=res)
    # SWIGLU: W1 | W3 of 130 rows each, two adapters
    w13 = (rnd(130, K, seed=50, scale=0.06).cuda(), rnd(130, K, seed=51, scale=0.06).cuda())
    A2 = (bank(r, K, 52, K ** -0.5), bank(r, K, 53, K ** -0.5))
    B2 = (bank(130, r, 54, 0.25 * r ** -0.5), bank(130, r, 55, 0.25 * r ** -0.5))
    _mixed_vs_uniform(h, x, w13, A2, B2, s, h.EPI_SWIGLU, slots)
    if M <= 8:   # RMSNorm fused in front of W and of A
        nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(61))).to(BF).cuda()
        _mixed_vs_uniform(h, x, ws, A, B, s, h.EPI_STORE, slots, norm_w=nw, eps=1e-5)
        _mixed_vs_uniform(h, x, w13, A2, B2, s, h.EPI_SWIGLU, slots, norm_w=nw, eps=1e-5)
    if K != 256 and M in (5, 40):
        _store_against_the_reference(h, x, K, r, s)


# ------------------------------------------------------------------------------------------------ models
def _load(folder, max_batch_size):
    from mistral_inference.transformer import Transformer
    return Transformer.from_folder(folder, max_batch_size=max_batch_size, device="cuda", dtype=BF)


def _adapter_sets(params=ENGINE_DIMS, rank=RANK):
    return [make_adapters(params, rank, seed=s) for s in SEEDS]


def _bank_model(folder, max_batch_size=9):
    model = _load(folder, max_batch_size)
    model.set_lora_slots(3)
    for slot, sd in enumerate(_adapter_sets()):
        model._load_lora_state_dict(sd, slot=slot)
    return model


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """The same synthetic weights three times: with a bank of three adapter sets, with ONE set (seed 5, never saw set_lora_slots),
    and without `lora`."""
    d = tmp_path_factory.mktemp("multilora")
    w = mo.synth_weights(mo.OracleArgs.from_params(ENGINE_DIMS), seed=9)
    lora_dir = write_lora_checkpoint(d / "lora", dict(ENGINE_DIMS, lora=dict(rank=RANK, scaling=2.0)), w)
    plain_dir = write_lora_checkpoint(d / "plain", dict(ENGINE_DIMS), w)
    bank = _bank_model(lora_dir)
    one = _load(lora_dir, 9)
    one._load_lora_state_dict(_adapter_sets()[0])
    return dict(bank=bank, one=one, plain=_load(plain_dir, 9), lora_dir=lora_dir)


def _forwards(model, prompts, force, adapters="absent"):
    """Logits of the prefill and of len(force) teacher-forced decode steps."""
    from mistral_inference.cache import BufferCache
    a = model.args
    kw = {} if adapters == "absent" else dict(adapters=adapters)
    lens = [len(p) for p in prompts]
    cache = BufferCache(model.n_local_layers, a.max_batch_size, max(lens) + len(force) + 1, a.n_kv_heads, a.head_dim, a.sliding_window,
                        device="cuda", dtype=BF)
    cache.reset()
    out = [model.forward(torch.tensor(sum(prompts, []), device="cuda"), lens, cache, **kw).clone()]
    for tok in force:
        out.append(model.forward(tok.cuda(), [1] * len(prompts), cache, **kw).clone())
    return out


def _seq_rows(outs, lens, b):
    """The rows of sequence b: its prompt rows of the prefill, then its row of every decode step."""
    start = sum(lens[:b])
    return [outs[0][start:start + lens[b]]] + [o[b:b + 1] for o in outs[1:]]


def _prompts(lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, ENGINE_DIMS["vocab_size"], (n,), generator=g).tolist() for n in lens]


MIXES = {
    "15rows_one_tile": ((7, 3, 5), [1, -1, 0]),            # one MFMA tile across three sequences
    "7rows_prefill_gemv": ((3, 2, 2), [2, 0, 1]),          # the T <= 8 kernels on the PREFILL branch: token != sequence
    "seams_at_40_49": ((40, 9, 30), [1, -1, 0]),
    "decode_T9_mfma": (tuple(range(2, 11)), [0, 1, 2, -1, 0, 1, 2, -1, 0]),   # decode with T = 9: the MFMA forms on the DECODE branch
}


@pytest.mark.parametrize("mix", list(MIXES))
def test_model_mixed_batch_equals_uniform_batches(mix, models):
    """Prefill + 12 teacher-forced decode steps of a 3-slot model with one adapter per sequence: for every sequence b, its logits
    rows of every forward equal those of the same schedule run with adapters = [a_b] * B; the rows of a -1 sequence equal those
    of the same weights loaded without `lora`; uniform runs of two different slots differ (a kernel that ignores the slot fails)."""
    lens, adapters = MIXES[mix]
    bank, plain = models["bank"], models["plain"]
    prompts = _prompts(lens)
    B = len(lens)
    g = torch.Generator().manual_seed(11)
    force = [torch.randint(1, ENGINE_DIMS["vocab_size"], (B,), generator=g) for _ in range(N_STEPS)]
    mixed = _forwards(bank, prompts, force, adapters)
    assert len(mixed) == N_STEPS + 1
    uniform = {a: _forwards(bank, prompts, force, [a] * B) for a in sorted(set(adapters))}
    for b, a in enumerate(adapters):
        for f, (got, want) in enumerate(zip(_seq_rows(mixed, lens, b), _seq_rows(uniform[a], lens, b))):
            assert torch.equal(got, want), (mix, "sequence", b, "slot", a, "forward", f, float((got - want).abs().max()))
    if -1 in uniform:
        base = _forwards(plain, prompts, force)
        for f, (got, want) in enumerate(zip(uniform[-1], base)):
            assert torch.equal(got, want), (mix, "slot -1 against the plain model, forward", f)
    keys = sorted(uniform)
    for a, c in zip(keys, keys[1:]):
        assert not torch.equal(uniform[a][0], uniform[c][0]) and not torch.equal(uniform[a][-1], uniform[c][-1]), (a, c)


@pytest.mark.parametrize("lens", [(12,), (7, 3, 5)], ids=["batch1", "batch3"])
def test_none_and_all_zero_equal_the_one_slot_model(lens, models):
    """Existing behaviour: on the 3-slot model adapters=None (the kernels' single-adapter mode) and adapters=[0] * B (their bank mode)
    both give the logits, tokens and log-probabilities of a one-slot model that never saw set_lora_slots and carries slot 0's set."""
    from mistral_inference.generate import generate
    bank, one = models["bank"], models["one"]
    prompts, B = _prompts(lens, seed=4), len(lens)
    g = torch.Generator().manual_seed(12)
    force = [torch.randint(1, ENGINE_DIMS["vocab_size"], (B,), generator=g) for _ in range(N_STEPS)]
    ref = _forwards(one, prompts, force)
    for adapters in ("absent", None, [0] * B):
        got = _forwards(bank, prompts, force, adapters)
        for f, (x, y) in enumerate(zip(got, ref)):
            assert torch.equal(x, y), (adapters, f, float((x - y).abs().max()))
    t_ref, lp_ref = generate(prompts, one, max_tokens=N_STEPS, temperature=0.0)
    assert generate(prompts, bank, max_tokens=N_STEPS, temperature=0.0) == (t_ref, lp_ref)
    assert generate(prompts, bank, max_tokens=N_STEPS, temperature=0.0, adapters=None) == (t_ref, lp_ref)
    assert generate(prompts, bank, max_tokens=N_STEPS, temperature=0.0, adapters=[0] * B) == (t_ref, lp_ref)


def test_sequence_on_the_references_adapter_matches_the_stored_reference(tmp_path):
    """Anchor to the unmodified reference: golden case lora_dense_bf16, its adapters in slot 1 (seeds 6 and 7 in slots 0 and 2),
    sequence 0 on slot 1 and the others cycling through 0, 2, -1.  Teacher-forced replay of the case's schedule: sequence 0's rows
    of every forward within LOGIT_ATOL of the reference's stored logits, its first greedy token the reference's."""
    from mistral_inference.cache import BufferCache
    case = LoraCase("lora_dense_bf16")
    rank = case.params["lora"]["rank"]
    model = _load(write_lora_checkpoint(tmp_path / "ckpt", case.params, case.weights()), case.max_batch_size)
    model.set_lora_slots(3)
    model._load_lora_state_dict(make_adapters(case.params, rank, seed=6), slot=0)
    model._load_lora_state_dict(case.adapters, slot=1)
    model._load_lora_state_dict(make_adapters(case.params, rank, seed=7), slot=2)
    B = len(case.prompts)
    adapters = [1] + list(itertools.islice(itertools.cycle([0, 2, -1]), B - 1))
    a = model.args
    lens = [len(p) for p in case.prompts]
    cache = BufferCache(model.n_local_layers, a.max_batch_size, max(lens) + case.max_tokens, a.n_kv_heads, a.head_dim, a.sliding_window,
                        device="cuda", dtype=BF)
    cache.reset()
    chunk = case.chunk_size or max(lens)
    toks = case.tokens()
    worst, last0 = 0.0, None
    for c, s in enumerate(range(0, max(lens), chunk)):
        parts = [p[s:s + chunk] for p in case.prompts]
        out = model.forward(torch.tensor(sum(parts, []), device="cuda"), [len(p) for p in parts], cache, adapters=adapters).cpu()
        n0 = len(parts[0])
        ref = case.t[f"prefill_logits.{c}"][:n0]
        d = float((out[:n0] - ref).abs().max())
        print(f"prefill chunk {c}: sequence 0 max |d| {d:.4f}")
        assert d <= LOGIT_ATOL, ("prefill", c, d)
        worst, last0 = max(worst, d), out[n0 - 1]
    assert int(last0.argmax()) == toks[0][0]
    for step in range(len(toks[0])):
        out = model.forward(torch.tensor([t[step] for t in toks], device="cuda"), [1] * B, cache, adapters=adapters).cpu()
        d = float((out[0] - case.t[f"decode_logits.{step}"][0]).abs().max())
        assert d <= LOGIT_ATOL, ("decode", step, d)
        worst = max(worst, d)
    print(f"sequence 0 against the reference over {len(toks[0]) + 1} forwards: max |d| {worst:.4f} (bound {LOGIT_ATOL})")


GEN_PROMPTS = [[1, 5, 9, 200, 17, 3, 44], [7, 300, 2], [11, 12, 13, 14, 15]]
GEN_ADAPTERS = [1, -1, 0]


def _generate_mixed_and_uniform(model):
    from mistral_inference.generate import generate
    mixed = generate(GEN_PROMPTS, model, max_tokens=N_STEPS, temperature=0.0, adapters=GEN_ADAPTERS)
    uniform = {a: generate(GEN_PROMPTS, model, max_tokens=N_STEPS, temperature=0.0, adapters=[a] * 3) for a in GEN_ADAPTERS}
    return mixed, uniform


def test_generate_with_one_adapter_per_sequence(models):
    """generate(adapters=[1, -1, 0]), 12 tokens at temperature 0: each sequence's tokens and log-probabilities are those of the
    uniform call for its slot."""
    (toks, lps), uniform = _generate_mixed_and_uniform(models["bank"])
    assert len(toks) == 3 and all(len(t) == N_STEPS for t in toks)
    for b, a in enumerate(GEN_ADAPTERS):
        assert toks[b] == uniform[a][0][b] and lps[b] == uniform[a][1][b], (b, a)
    assert uniform[1] != uniform[0] and uniform[0] != uniform[-1]


def test_swapping_one_slot_on_a_live_model(models, tmp_path):
    """load_lora(path, slot=1) on a live 3-slot model: the sequences on slots 0 and -1 come out bit for bit as before, the one on
    slot 1 changes, and loading the old set back restores it bit for bit.  Base weights never move (pointers and values)."""
    from safetensors.torch import save_file
    from mistral_inference.generate import generate
    model = _bank_model(models["lora_dir"], max_batch_size=3)
    base_ptrs = {k: v.data_ptr() for k, v in model.named_parameters() if "lora" not in k}
    base_vals = {k: v.clone() for k, v in model.named_parameters() if "lora" not in k}
    old, new = tmp_path / "old.safetensors", tmp_path / "new.safetensors"
    save_file(_adapter_sets()[1], str(old))
    save_file(make_adapters(ENGINE_DIMS, RANK, seed=77), str(new))
    run = lambda: generate(GEN_PROMPTS, model, max_tokens=N_STEPS, temperature=0.0, adapters=GEN_ADAPTERS)  # noqa: E731
    t1, lp1 = run()
    model.load_lora(new, slot=1)
    t2, lp2 = run()
    model.load_lora(old, slot=1)
    t3, lp3 = run()
    for b in (1, 2):   # slots -1 and 0
        assert t2[b] == t1[b] and lp2[b] == lp1[b], b
    assert (t2[0], lp2[0]) != (t1[0], lp1[0])
    assert (t3, lp3) == (t1, lp1)
    now = dict(model.named_parameters())
    assert all(now[k].data_ptr() == p for k, p in base_ptrs.items())
    assert all(torch.equal(now[k], v) for k, v in base_vals.items())


@pytest.mark.parametrize("lens", [(3, 2, 2), (7, 3, 5)], ids=["7rows_gemv", "15rows_mfma"])
def test_forward_without_a_cache_reads_each_rows_own_sequence(lens, models):
    """cache=None (NOCACHE branch) with adapters.  Attention there is ONE unmasked segment over all rows, so a sequence's rows
    depend on its neighbours' adapters and cannot be compared with uniform runs; what must hold instead:
    * [0, 0, 0] through the bank mode equals the one-slot model's cache-less forward (tok_seq 0, 1, 2 all on slot 0);
    * [2, 0, 1] equals [0, 1, 2] on a bank whose slots carry the sets (2, 0, 1) - the same set per sequence, other slot numbers;
    * [2, 0, 1] differs from [2, 2, 2], which is what it would give if every row were taken for sequence 0."""
    one = models["one"]
    bank = _bank_model(models["lora_dir"], max_batch_size=3)
    ids = torch.tensor(sum(_prompts(lens, seed=8), []), device="cuda")
    assert torch.equal(bank.forward(ids, list(lens), adapters=[0, 0, 0]), one.forward(ids, list(lens)))
    mixed = bank.forward(ids, list(lens), adapters=[2, 0, 1]).clone()
    assert not torch.equal(mixed, bank.forward(ids, list(lens), adapters=[2, 2, 2]))
    sets = _adapter_sets()
    for slot, src in enumerate((2, 0, 1)):
        bank._load_lora_state_dict(sets[src], slot=slot)
    assert torch.equal(bank.forward(ids, list(lens), adapters=[0, 1, 2]), mixed)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_a_session_keeps_the_adapters_it_was_made_with(graph, models):
    """A hand-driven GreedySession latches the adapter choice at construction (the pointer or NULL; the VALUES stay those of the
    shared tensor): a forward(adapters=None) on the same model between its steps moves neither its eager nor its replayed steps."""
    from mistral_inference.cache import BufferCache
    bank = models["bank"]
    a = bank.args
    lens = [len(p) for p in GEN_PROMPTS]
    ids = torch.tensor(sum(GEN_PROMPTS, []), device="cuda")
    other = torch.tensor([5, 6, 7], device="cuda")

    def run(disturb):
        cache = BufferCache(bank.n_local_layers, a.max_batch_size, max(lens) + N_STEPS + 1, a.n_kv_heads, a.head_dim,
                            a.sliding_window, device="cuda", dtype=BF)
        cache.reset()
        logits = bank.forward(ids, lens, cache, adapters=GEN_ADAPTERS)
        ends = torch.tensor(lens, device="cuda").cumsum(0) - 1
        sess = bank.greedy_session(cache, logits[ends].argmax(-1), graph=graph)
        for _ in range(4):
            if disturb:   # (before the session's first step too: its eager warm-up step and its capture come after a None)
                bank.forward(other, [3], adapters=None)
            sess.run(3)
        toks, lps = sess.collect()
        return toks.clone(), lps.clone()

    t0, lp0 = run(False)
    t1, lp1 = run(True)
    assert torch.equal(t0, t1) and torch.equal(lp0, lp1)
    # and the latched choice is the mixed one: slot 0 for every sequence (what a session that followed the last forward would run)
    cache = BufferCache(bank.n_local_layers, a.max_batch_size, max(lens) + N_STEPS + 1, a.n_kv_heads, a.head_dim, a.sliding_window,
                        device="cuda", dtype=BF)
    cache.reset()
    logits = bank.forward(ids, lens, cache, adapters=GEN_ADAPTERS)
    first = logits[torch.tensor(lens, device="cuda").cumsum(0) - 1].argmax(-1)
    bank.forward(other, [3], adapters=None)
    sess = bank.greedy_session(cache, first, graph=graph)   # made AFTER the choice went back to None: slot 0 on its steps
    sess.run(N_STEPS)
    uniform0 = sess.collect()[1]
    assert not torch.equal(uniform0, lp0)


def test_refusals_through_the_c_abi():
    """seq_adapter on a model without un-merged LoRA: MI_ERR_ARG; a MoE model with lora_slots = 3: still MI_ERR_UNSUPPORTED.
    Both before any launch."""
    h = _hip()
    L = h.lib()
    layers = (h.MiLayer * 1)()
    m = h.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 256, 4, 2, 128, 512, 64, 1
    m.layers = C.cast(layers, C.POINTER(h.MiLayer))
    m.final_norm = m.output = 1
    bt = h.MiBatch()
    bt.T = bt.B = 1
    bt.branch, bt.max_q_len = 2, 1
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = bt.kv_seqlens = bt.h = bt.workspace = bt.logits = 1
    keep = ((h._vp * 1)(), (h._vp * 1)(), (C.c_int32 * 1)(16))
    bt.cache_k, bt.cache_v, bt.cache_sizes = keep
    bt.workspace_bytes = 64
    bt.seq_adapter = 1
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1 and b"seq_adapter" in L.mi_last_error_detail()
    m.lora_rank, m.lora_scaling, m.lora_slots = 16, 2.0, 3
    m.num_experts, m.top_k = 8, 2
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -4 and b"MoE" in L.mi_last_error_detail()
