"""Un-merged LoRA adapters on the GPU (csrc/lora.hip, ABI v8): the leaf against the numerics contract, whole models against the
unmodified reference's stored outputs (tests/golden/lora_*), adapter swapping, routing."""
import math

import pytest
import torch
import torch.nn.functional as F

import mistral_oracle as mo
from lora_util import BF, LoraCase, lora_linear_ref, make_adapters, write_lora_checkpoint

pytestmark = pytest.mark.gpu
LOGIT_ATOL = 4e-2   # tests/test_gpu_model.py
ENGINE_DIMS = dict(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                   sliding_window=16)   # dims the persistent decode engine takes (the second model of smoke())


def _hip():
    from mistral_inference import _hip
    return _hip


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ 1. leaf
def _parts(x, ws, As, Bs, s, t_fp32=False, single_round_d=False):
    """Per segment (y, base, d, t, tflip) of the contract on the CPU; y / base / d / tflip concatenated over the segments, t
    stacked [nseg, M, r].  tflip[m, n] = what ONE element of t landing one bf16 ulp away moves d[m, n] by:
    s * max_j |B[n, j]| * |t[m, j]| * 2^-7.  single_round_d (a mutant): d = bf16((B t) * s), the inner rounding dropped."""
    ys, bases, ds, ts, tf = [], [], [], [], []
    for w, a, b in zip(ws, As, Bs):
        y, base, d = lora_linear_ref(x, w, a, b, s, t_fp32=t_fp32, parts=True)
        t = F.linear(x.float(), a.float()).to(BF).float()
        if single_round_d:
            d = (F.linear(t, b.float()) * float(s)).to(BF)
            y = (base.float() + d.float()).to(BF)
        ys.append(y), bases.append(base), ds.append(d), ts.append(t)
        tf.append(abs(s) * (b.float().abs()[None, :, :] * t.abs()[:, None, :]).amax(-1) * 2.0 ** -7)
    return torch.cat(ys, 1).float(), torch.cat(bases, 1).float(), torch.cat(ds, 1).float(), torch.stack(ts), torch.cat(tf, 1)


def _strict_store(ref):
    """tests/test_gpu_ops.py, mi_linear STORE: bf16_ulp_close(got, ref, ulps=1.0) = 1 bf16 ulp at |ref| (floor 1e-3) + 1e-6."""
    return ref.abs().clamp(min=1e-3) * 2.0 ** -7 + 1e-6


def _strict_residual(out, res, y):
    """tests/test_gpu_ops.py, mi_linear RESIDUAL: 1.5 ulp at the largest of |res|, |y|, |out|, + 1e-6."""
    return 1.5 * torch.stack([res.abs(), y.abs(), out.abs()]).amax(0) * 2.0 ** -7 + 1e-6


def _flip_budget(n, k):
    """How many of n bf16-rounded fp32 dot products of length k may legitimately land on the neighbouring bf16 value when the
    summation order differs (CPU sgemm against lanes + wave reduction / MFMA).  Two fp32 sums of k random-sign terms differ by
    about sqrt(k) * 2^-24 relative to the result (random walk of k roundings of partial sums of size sqrt(k) * term); taken four
    times larger, d_rel = 4 * sqrt(k) * 2^-24.  A result flips when it lies within d_rel of a rounding boundary, and boundaries
    are at least 2^-8 apart relative to the value: p <= 2 * d_rel / 2^-8 = 8 * sqrt(k) * 2^-16 (2.8e-3 at k = 512, 1e-3 at 64).
    The budget is ceil(p * n) + 2."""
    return math.ceil(8.0 * k ** 0.5 * 2.0 ** -16 * n) + 2


def _widened_store(y, base, d):
    """What an element may reach when ONE of its two addends landed on the neighbouring bf16 value: one ulp of that addend (not of
    a y that cancellation made small - test_gpu_ops' reasoning for its residual sum) plus y's own rounding."""
    return (torch.maximum(base.abs(), d.abs()) + y.abs().clamp(min=1e-3)) * 2.0 ** -7 + 1e-6


def _swiglu(y1, y3):
    return (F.silu(y1) * y3).float()   # bf16 tensors: silu and the product are each rounded (transformer_layers.py:105-106)


def _bound_swiglu(ref):
    return 4 * ref.abs() * 2.0 ** -7 + 8e-3   # test_gpu_ops.test_linear_residual_swiglu_logits, unchanged


@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("M", [1, 2, 3, 8, 9, 300])
def test_lora_linear_leaf(M, K, r):
    """mi_lora_linear against lora_util.lora_linear_ref: three segments 256|64|64 with three different adapters (s = 1.5) and one
    segment of 130 rows (s = 0.7: not powers of two, so the inner rounding of d = bf16(bf16(B t) * s) matters), epilogues STORE /
    RESIDUAL / SWIGLU.

    Every element is held to the bound tests/test_gpu_ops.py applies to mi_linear for the epilogue.  An element may leave it
    only where one of its bf16-rounded inputs provably landed on the neighbouring value on the GPU, and those are observed, not
    assumed - through the public entry itself: base = mi_linear; d = mi_lora_linear with W = 0; t = mi_lora_linear with W = 0,
    B = I, s = 1:
      * t against bf16(A x): test_gpu_ops' 1-ulp bound on every element, at most _flip_budget elements off by their last bit;
      * d against bf16(bf16(B t) s): the 1-ulp bound on every element of every (row, segment) slice whose t is bit-equal - no
        exception - and at most _flip_budget bit mismatches there; in a slice with a flipped t element, what that flip moves d
        by plus one ulp for each of d's two roundings;
      * y == bf16(base + d) and out == bf16(residual + y) BIT FOR BIT on the GPU's own base, d, y;
      * y, and residual + y, against the reference: the epilogue's bound, except at elements whose base or d differs from the
        reference's in the last bit, which stay inside _widened_store.
    With B = 0 the output is mi_linear's, bit for bit; with adapters on q and v only (k: NULL pair) the k columns are
    mi_linear's and the q, v columns those of the full set, bit for bit.
    Teeth, asserted on the CPU reference: adapters of two segments exchanged, or s doubled, leave even the widened bound; t
    kept in fp32 (r = 64) leaves the 1-ulp bound on d - where no exception is admitted - and mismatches more bits of d than the
    budget; the inner rounding of d dropped mismatches more bits of d than the budget."""
    h = _hip()
    x = rnd(M, K, seed=20)
    cuda = lambda ts: tuple(t.cuda() for t in ts)  # noqa: E731
    for rows, seed, s in (((256, 64, 64), 30, 1.5), ((130,), 40, 0.7)):
        nseg, N = len(rows), sum(rows)
        ws = [rnd(n, K, seed=seed + i, scale=K ** -0.5) for i, n in enumerate(rows)]
        As = [rnd(r, K, seed=seed + 3 + i, scale=K ** -0.5) for i in range(nseg)]
        Bs = [rnd(n, r, seed=seed + 6 + i, scale=0.25 * r ** -0.5) for i, n in enumerate(rows)]
        res = rnd(M, N, seed=seed + 9)
        y, base, d, t, tflip = _parts(x, ws, As, Bs, s)
        xg, wg, ag, bg = x.cuda(), cuda(ws), cuda(As), cuda(Bs)
        zw = tuple(torch.zeros_like(w) for w in wg)
        # --- what the GPU's rounded intermediates are
        eye, zr = torch.eye(r, dtype=BF, device="cuda"), torch.zeros(r, K, dtype=BF, device="cuda")
        t_g = torch.stack([h.lora_linear(xg, (zr,), (a,), (eye,), 1.0).cpu().float() for a in ag])
        d_g = h.lora_linear(xg, zw, ag, bg, s).cpu().float()
        base_g = h.linear(xg, wg, h.EPI_STORE).cpu().float()
        y_g = h.lora_linear(xg, wg, ag, bg, s).cpu().float()
        out_g = h.lora_linear(xg, wg, ag, bg, s, h.EPI_RESIDUAL, residual=res.cuda()).cpu().float()
        # --- t
        assert bool(((t_g - t).abs() <= _strict_store(t)).all())
        t_flip = t_g != t
        assert int(t_flip.sum()) <= _flip_budget(t.numel(), K), (int(t_flip.sum()), _flip_budget(t.numel(), K))
        col_flip = torch.cat([t_flip[i].any(-1, keepdim=True).expand(M, n) for i, n in enumerate(rows)], 1)   # [M, N]
        # --- d
        err_d = (d_g - d).abs()
        in_flip = (err_d / (2 * _strict_store(d) + tflip))[col_flip]
        print(f"   d: worst err/bound {float((err_d / _strict_store(d))[~col_flip].max()):.2f} where t is bit-equal, "
              f"{float(in_flip.max()) if in_flip.numel() else 0.0:.2f} in the {int(col_flip.sum())} elements behind a flipped t")
        assert bool((err_d[~col_flip] <= _strict_store(d)[~col_flip]).all())
        assert bool((in_flip <= 1.0).all())   # the flip itself, and one spacing for each of d's two roundings
        d_diff = (d_g != d)
        n_d = int((d_diff & ~col_flip).sum())
        assert n_d <= _flip_budget(d.numel(), r), (n_d, _flip_budget(d.numel(), r))
        # --- the last rounding and the epilogue, on the GPU's own inputs
        assert torch.equal(y_g, (base_g + d_g).to(BF).float())
        assert torch.equal(out_g, (res.float() + y_g).to(BF).float())
        # --- against the reference
        base_diff = base_g != base
        assert bool(((base_g - base).abs() <= _strict_store(base)).all()) and int(base_diff.sum()) <= _flip_budget(base.numel(), K)
        excused = base_diff | d_diff
        wide = _widened_store(y, base, d) + tflip * col_flip
        err = (y_g - y).abs()
        over = err > _strict_store(y)
        print(f"M={M} K={K} r={r} N={N} s={s}: t flips {int(t_flip.sum())}, d bit mismatches {n_d}, base flips {int(base_diff.sum())}; "
              f"store worst err/bound {float((err / _strict_store(y)).max()):.2f}, over the bound {int(over.sum())} "
              f"(worst err/widened {float((err / wide).max()):.2f})")
        assert bool((~over | excused).all()) and bool((err <= wide).all())
        ref_res = (res.float() + y).to(BF).float()
        strict_r = _strict_residual(ref_res, res.float(), y)
        err = (out_g - ref_res).abs()
        over = err > strict_r
        print(f"   residual worst err/bound {float((err / strict_r).max()):.2f}, over the bound {int(over.sum())}")
        assert bool((~over | excused).all()) and bool((err <= strict_r + wide).all())
        # --- teeth on the CPU reference
        y2 = _parts(x, ws, As, Bs, 2 * s)[0]
        assert bool(((y2 - y).abs() > wide).any()), "doubling s stays inside the bound"
        if nseg == 3:
            ysw = _parts(x, ws, [As[0], As[2], As[1]], [Bs[0], Bs[2], Bs[1]], s)[0]
            assert bool(((ysw - y).abs() > wide).any()), "exchanged adapters stay inside the bound"
        d1 = _parts(x, ws, As, Bs, s, single_round_d=True)[2]
        if M * N >= 384:   # (one row of 130 values holds ~25 such mismatches: too close to the budget's constant to call)
            assert int((d1 != d).sum()) > 4 * _flip_budget(d.numel(), r), ("inner rounding of d", int((d1 != d).sum()))
        if r == 64:
            dt = _parts(x, ws, As, Bs, s, t_fp32=True)[2]
            n_over, n_bits = int(((dt - d).abs() > _strict_store(d)).sum()), int((dt != d).sum())
            print(f"   t in fp32: {n_over} elements of d over the 1-ulp bound, {n_bits} bit mismatches (budget {_flip_budget(d.numel(), r)})")
            assert n_over > 0 and n_bits > _flip_budget(d.numel(), r), "t kept in fp32 is not visible"
        # --- B = 0 and partial adapter sets: bit-equal to mi_linear where there is no adapter
        zeros = tuple(torch.zeros_like(b) for b in bg)
        assert torch.equal(h.lora_linear(xg, wg, ag, zeros, s), h.linear(xg, wg, h.EPI_STORE))
        plain = h.linear(xg, wg, h.EPI_RESIDUAL, residual=res.cuda())
        assert torch.equal(h.lora_linear(xg, wg, ag, zeros, s, h.EPI_RESIDUAL, residual=res.cuda()), plain)
        assert torch.equal(h.lora_linear(xg, wg, (None,) * nseg, (None,) * nseg, s), h.linear(xg, wg, h.EPI_STORE))
        if nseg == 3:   # q and v carry adapters, k does not
            part = h.lora_linear(xg, wg, (ag[0], None, ag[2]), (bg[0], None, bg[2]), s).cpu().float()
            assert torch.equal(part[:, 256:320], base_g[:, 256:320])
            assert torch.equal(part[:, :256], y_g[:, :256]) and torch.equal(part[:, 320:], y_g[:, 320:])
            part = h.lora_linear(xg, wg, (None, ag[1], None), (None, bg[1], None), s, h.EPI_RESIDUAL, residual=res.cuda()).cpu().float()
            assert torch.equal(part[:, 256:320], out_g[:, 256:320])
            assert torch.equal(part[:, :256], plain.cpu().float()[:, :256]) and torch.equal(part[:, 320:], plain.cpu().float()[:, 320:])
    # SWIGLU: W1 | W3 of 130 rows each, two different adapters (test_gpu_ops' weight scale and bound for this epilogue)
    n, s = 130, 1.5
    w1, w3 = rnd(n, K, seed=50, scale=0.06), rnd(n, K, seed=51, scale=0.06)
    As = [rnd(r, K, seed=52 + i, scale=K ** -0.5) for i in range(2)]
    Bs = [rnd(n, r, seed=54 + i, scale=0.25 * r ** -0.5) for i in range(2)]
    y1, y3 = lora_linear_ref(x, w1, As[0], Bs[0], s), lora_linear_ref(x, w3, As[1], Bs[1], s)
    ref = _swiglu(y1, y3)
    got = h.lora_linear(x.cuda(), cuda((w1, w3)), cuda(As), cuda(Bs), s, h.EPI_SWIGLU).cpu().float()
    err = (got - ref).abs()
    print(f"   swiglu: max err {float(err.max()):.3e}, worst err/bound {float((err / _bound_swiglu(ref)).max()):.3f}")
    assert got.shape == (M, n) and bool((err <= _bound_swiglu(ref)).all())
    ref2 = _swiglu(lora_linear_ref(x, w1, As[0], Bs[0], 2 * s), lora_linear_ref(x, w3, As[1], Bs[1], 2 * s))
    assert bool(((ref2 - ref).abs() > _bound_swiglu(ref)).any()), "doubling s stays inside the bound"
    refsw = _swiglu(lora_linear_ref(x, w1, As[1], Bs[1], s), lora_linear_ref(x, w3, As[0], Bs[0], s))
    assert bool(((refsw - ref).abs() > _bound_swiglu(ref)).any()), "exchanged adapters stay inside the bound"
    zeros = tuple(torch.zeros_like(b).cuda() for b in Bs)
    assert torch.equal(h.lora_linear(x.cuda(), cuda((w1, w3)), cuda(As), zeros, s, h.EPI_SWIGLU),
                       h.linear(x.cuda(), cuda((w1, w3)), h.EPI_SWIGLU))
    # W1 with an adapter, W3 without: the same as W3's adapter with B = 0
    one = h.lora_linear(x.cuda(), cuda((w1, w3)), (As[0].cuda(), None), (Bs[0].cuda(), None), s, h.EPI_SWIGLU)
    assert torch.equal(one, h.lora_linear(x.cuda(), cuda((w1, w3)), cuda(As), (Bs[0].cuda(), zeros[1]), s, h.EPI_SWIGLU))


def test_lora_linear_leaf_fused_norm_with_zero_b_is_mi_linear():
    """norm_w on the M <= 8 path: RMSNorm in front of W and of A; with B = 0 bit-equal to mi_linear with the same norm_w."""
    h = _hip()
    K, n, r = 512, 256, 16
    x = rnd(3, K, seed=60, scale=2.0).cuda()
    nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(61))).to(BF).cuda()
    w1, w3 = rnd(n, K, seed=62, scale=0.05).cuda(), rnd(n, K, seed=63, scale=0.05).cuda()
    a, zero = rnd(r, K, seed=64, scale=K ** -0.5).cuda(), torch.zeros(n, r, dtype=BF, device="cuda")
    for epi, ws in ((h.EPI_STORE, (w1,)), (h.EPI_SWIGLU, (w1, w3))):
        got = h.lora_linear(x, ws, (a,) * len(ws), (zero,) * len(ws), 2.0, epi, norm_w=nw, eps=1e-5)
        assert torch.equal(got, h.linear(x, ws, epi, norm_w=nw, eps=1e-5)), epi


# ------------------------------------------------------------------------------------------------ models
def _folder(tmp_path, params, weights, name="ckpt"):
    return write_lora_checkpoint(tmp_path / name, params, weights)


def _load(folder, max_batch_size=4):
    from mistral_inference.transformer import Transformer
    return Transformer.from_folder(folder, max_batch_size=max_batch_size, device="cuda", dtype=BF)


def _engine_pair(tmp_path, rank=16):
    """The same synthetic weights as a LoRA model (base checkpoint in the plain key form: zero adapters) and as a plain model."""
    oargs = mo.OracleArgs.from_params(ENGINE_DIMS)
    w = mo.synth_weights(oargs, seed=9)
    lora = _load(_folder(tmp_path, dict(ENGINE_DIMS, lora=dict(rank=rank, scaling=2.0)), w, "lora"))
    plain = _load(_folder(tmp_path, dict(ENGINE_DIMS), w, "plain"))
    return lora, plain


def _forwards(model, prompts, n_steps, force=None):
    """Prefill logits and n_steps decode logits; the decode inputs are `force` or the model's own argmax."""
    from mistral_inference.cache import BufferCache
    a = model.args
    lens = [len(p) for p in prompts]
    cache = BufferCache(model.n_local_layers, a.max_batch_size, max(lens) + n_steps + 1, a.n_kv_heads, a.head_dim, a.sliding_window,
                        device="cuda", dtype=BF)
    cache.reset()
    out = [model.forward(torch.tensor(sum(prompts, []), device="cuda"), lens, cache).clone()]
    ends = torch.tensor(lens).cumsum(0) - 1
    nxt = out[0][ends.cuda()].argmax(-1)
    toks = []
    for step in range(n_steps):
        if force is not None:
            nxt = force[step].cuda()
        toks.append(nxt.cpu())
        out.append(model.forward(nxt, [1] * len(prompts), cache).clone())
        nxt = out[-1].argmax(-1)
    return out, toks


@pytest.mark.parametrize("prompts", [[[3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]], [[1, 5, 9, 200, 17, 3, 44], [7, 300, 2], [11, 12, 13, 14, 15]]],
                         ids=["batch1", "batch3"])
def test_zero_adapters_reproduce_the_plain_model_bit_for_bit(prompts, tmp_path):
    """bf16(y + 0) = y: a LoRA model whose B matrices are zero (A random, so lora_down and lora_up do run) gives the logits and
    the greedy tokens of the same weights loaded without `lora` - prefill and 12 decode steps; the plain model's batch-1 steps run
    on the persistent engine, the LoRA model's on the launch path."""
    from mistral_inference.generate import generate
    lora, plain = _engine_pair(tmp_path)
    ad = make_adapters(ENGINE_DIMS, 16, seed=5)
    lora._load_lora_state_dict({k: (torch.zeros_like(v) if "lora_B" in k else v) for k, v in ad.items()})
    ref, toks = _forwards(plain, prompts, 12)
    got, toks2 = _forwards(lora, prompts, 12)
    assert len(got) == 13
    for f, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), (f, float((g - r).abs().max()))
    assert all(torch.equal(a, b) for a, b in zip(toks, toks2))
    t1, lp1 = generate(prompts, plain, max_tokens=12, temperature=0.0)
    t2, lp2 = generate(prompts, lora, max_tokens=12, temperature=0.0)
    assert t1 == t2
    # log-probabilities: the persistent engine's fused sample (plain model, batch 1) and the launch path's sample kernel reduce the
    # same logits in different orders - tests/test_gpu_engine.py holds them to 1e-4; on the launch path both sides are bit-equal
    worst = max(abs(x - y) for a, b in zip(lp1, lp2) for x, y in zip(a, b))
    assert worst < 1e-4 and (len(prompts) == 1 or lp1 == lp2), worst


def _replay(model, case: LoraCase):
    from mistral_inference.cache import BufferCache
    a = model.args
    lens = [len(p) for p in case.prompts]
    cache = BufferCache(model.n_local_layers, a.max_batch_size, max(lens) + case.max_tokens, a.n_kv_heads, a.head_dim, a.sliding_window,
                        device="cuda", dtype=BF)
    cache.reset()
    chunk = case.chunk_size or max(lens)
    toks = case.tokens()
    outs = []
    for s in range(0, max(lens), chunk):
        parts = [p[s:s + chunk] for p in case.prompts]
        outs.append(model.forward(torch.tensor(sum(parts, []), device="cuda"), [len(p) for p in parts], cache).cpu())
    for step in range(len(toks[0])):
        outs.append(model.forward(torch.tensor([t[step] for t in toks], device="cuda"), [1] * len(toks), cache).cpu())
    return outs


@pytest.mark.parametrize("name", ["lora_dense_bf16", "lora_swa_chunk_bf16", "lora_r64_bf16"])
def test_golden_replay_vs_the_reference(name, tmp_path):
    """Teacher-forced replay of the reference's schedule and generate(), measured as tests/test_gpu_model.py measures dense_bf16 /
    swa_chunk_bf16 against the reference's stored outputs (same statistics, same thresholds)."""
    from mistral_inference.generate import generate
    case = LoraCase(name)
    model = _load(_folder(tmp_path, case.params, case.weights()))
    from safetensors.torch import save_file
    path = tmp_path / "adapter.safetensors"
    save_file(case.adapters, str(path))
    model.load_lora(path)
    outs = _replay(model, case)
    pre, n_dec = case.schedule()
    refs = [case.t[f"prefill_logits.{c}"] for c in range(len(pre))] + [case.t[f"decode_logits.{s}"] for s in range(n_dec)]
    assert len(outs) == len(refs)
    within = elems = exact = in2 = in3 = 0
    abs_sum = 0.0
    for f, (got, ref) in enumerate(zip(outs, refs)):
        assert got.shape == ref.shape and got.dtype == torch.float32
        d = (got - ref).abs()
        assert d.max().item() <= LOGIT_ATOL, (name, "vs reference", f, d.max().item())
        ulp = ref.abs().clamp(min=1.0) * 2.0 ** -7
        within += int((d <= 1e-2).sum()); elems += d.numel(); abs_sum += float(d.sum()); exact += int((d == 0).sum())
        in2 += int((d <= 2.0 * ulp + 1e-7).sum()); in3 += int((d <= 3.0 * ulp + 1e-7).sum())
    print(f"\n{name}: bit-exact {exact / elems:.3f}, within 2 / 3 bf16 ulp(ref) {in2 / elems:.4f} / {in3 / elems:.4f}, "
          f"within 1e-2 {within / elems:.4f}, mean |d| {abs_sum / elems:.5f}")
    assert in2 >= 0.999 * elems, (name, in2 / elems)
    assert in3 == elems, (name, in3 / elems)
    assert exact >= 0.25 * elems, (name, exact / elems)
    assert within >= 0.97 * elems, (name, within / elems)
    assert abs_sum / elems <= 2.5e-3, (name, abs_sum / elems)
    # generate(): test_generate_vs_reference's measure
    toks, lps = generate(case.prompts, model, max_tokens=case.max_tokens, temperature=0.0, chunk_size=case.chunk_size)
    ref_toks, ref_lps = case.tokens(), case.logprobs()
    agree = 0
    for b, (mine, ref) in enumerate(zip(toks, ref_toks)):
        n = next((i for i, (x, y) in enumerate(zip(mine, ref)) if x != y), len(ref))
        agree += n
        assert n >= 1, (name, b, mine, ref)
        npl = len(case.prompts[b]) - 1 + n
        assert len(lps[b]) == len(ref_lps[b])
        assert max(abs(x - y) for x, y in zip(lps[b][:npl], ref_lps[b][:npl])) <= 6e-2, (name, b)
    assert agree >= 0.6 * sum(len(t) for t in ref_toks), (name, agree)


def test_swapping_adapters_on_a_live_model(tmp_path):
    """One model object, a GreedySession used before the first swap: set 1, set 2, set 1 again.  The third generation equals the
    first bit for bit (tokens and log-probabilities), the second differs, the base weights never move."""
    from mistral_inference.generate import generate
    case = LoraCase("lora_dense_bf16")
    model = _load(_folder(tmp_path, case.params, case.weights()))
    base_ptrs = {k: v.data_ptr() for k, v in model.named_parameters() if "lora" not in k}
    base_vals = {k: v.clone() for k, v in model.named_parameters() if "lora" not in k}
    t0, lp0 = generate(case.prompts, model, max_tokens=6, temperature=0.0)       # zero adapters; runs a GreedySession
    set1, set2 = case.adapters, make_adapters(case.params, 16, seed=77)
    model._load_lora_state_dict(set1)
    t1, lp1 = generate(case.prompts, model, max_tokens=6, temperature=0.0)
    model._load_lora_state_dict(set2)
    t2, lp2 = generate(case.prompts, model, max_tokens=6, temperature=0.0)
    model._load_lora_state_dict(set1)
    t3, lp3 = generate(case.prompts, model, max_tokens=6, temperature=0.0)
    assert t3 == t1 and lp3 == lp1
    assert (t2, lp2) != (t1, lp1) and (t0, lp0) != (t1, lp1)
    assert t1[0][0] == case.tokens()[0][0]                                       # and set 1 is the reference's fine-tune
    now = dict(model.named_parameters())
    assert all(now[k].data_ptr() == p for k, p in base_ptrs.items())
    assert all(torch.equal(now[k], v) for k, v in base_vals.items())


def test_module_level_block_equals_the_runner(tmp_path):
    """TransformerBlock.forward with adapters (module by module: mi_lora_linear leaves) == the same layer inside mi_forward.  15
    rows: both sides take the RMSNorm kernel and the MFMA GEMM, so the comparison is bit for bit (at T <= 8 the runner's GEMV
    fuses the RMSNorm and sums its squares in another order: the 2-ulp bound of the bf16 / FP8 / MXFP4 block tests at 4 rows)."""
    case = LoraCase("lora_dense_bf16")
    p = dict(case.params, n_layers=1)
    w = {k: v for k, v in case.weights().items() if not k.startswith("layers.1.")}
    model = _load(_folder(tmp_path, p, w))
    model._load_lora_state_dict({k: v for k, v in case.adapters.items() if k.startswith("layers.0.")})
    lens = [len(x) for x in case.prompts]
    ids = torch.tensor(sum(case.prompts, []), device="cuda")
    h, _ = model._run(ids, lens, None, want_logits=True)        # with logits requested, h stays the block stack's output
    pos = torch.cat([torch.arange(n) for n in lens]).cuda()
    out = model.layers["0"](model.tok_embeddings.weight[ids], model.freqs_cis[pos])
    assert torch.equal(out, h), float((out.float() - h.float()).abs().max())
    assert not torch.equal(out, torch.zeros_like(out))


def test_lora_decode_steps_stay_off_the_persistent_engine(tmp_path):
    """The routing function declines a model with adapters: status word 4 (engine launches) does not move over a batch-1
    generation, while the same weights without `lora` run every decode step on the engine."""
    from mistral_inference.generate import generate
    h = _hip()
    lora, plain = _engine_pair(tmp_path)
    lora._load_lora_state_dict(make_adapters(ENGINE_DIMS, 16, seed=6))
    prompt = [[3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]]
    generate(prompt, plain, max_tokens=8, temperature=0.0)
    st = h.decode_engine_status(plain._backend._workspace)
    assert st["engine_launches"] >= 7 and st["status"] == 0, st
    generate(prompt, lora, max_tokens=8, temperature=0.0)
    st = h.decode_engine_status(lora._backend._workspace)
    assert st["engine_launches"] == 0 and st["steps"] >= 7 and st["status"] == 0, st
