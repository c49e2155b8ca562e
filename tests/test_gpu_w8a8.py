"""FP8 prefill GEMMs (W8A8) on the device: the activation quantiser bit for bit against quant.quantize_rows, the GEMM
(csrc/gemm256_w8a8.hip) on the exact structured cases of tests/w8a8_cases.py and on Gaussian operands inside the envelopes of
tests/test_gpu_fp8.py, the fallbacks below the applicability limit bit for bit, and a model with `prefill_fp8=True`."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

import linear_cases as lc
import quant_util as qu
import w8a8_cases as wc
from quant_util import BF, _cache, _hip, _quant, bf, deltas_of, inside_envelope, rnd

pytestmark = pytest.mark.gpu

CASES = wc.all_cases()


# ------------------------------------------------------------------------------------------------ 1. exact structured cases
def _run_case(h, case):
    """The case through its leaf, into a guarded buffer on the device; returns the whole buffer on the CPU."""
    inp = wc.inputs(case)
    buf, view = lc.guard(case.M, case.N, BF)
    buf = buf.cuda()
    view = buf[2:2 + case.M, :case.N]
    wq = [w.view(torch.uint8).cuda() for w in inp.wq]
    ws = [s.cuda() for s in inp.ws]
    x = inp.x.cuda()
    if case.epi == lc.QKV:
        H, Hkv = case.qkv[:2]
        h.qkv_rope_w8a8(x, wq, ws, H, Hkv, inp.rope_cs.cuda(), inp.tok_pos.cuda(), out=view)
    else:
        res = None
        if case.epi == lc.RESIDUAL:   # in a buffer of the output's geometry: the epilogue reads it at the output's row stride
            rbuf = torch.zeros_like(buf)
            res = rbuf[2:2 + case.M, :case.N]
            res.copy_(inp.res.cuda())
        h.linear_w8a8(x, wq, ws, lc.EPI_CODE[case.epi], residual=res, out=view)
    return buf.cpu()


@pytest.mark.parametrize("group", [lc.STORE, lc.RESIDUAL, lc.SWIGLU, lc.QKV])
def test_structured_cases_are_bit_equal_to_the_fp64_chain_reference(group):
    """Activation and weight quantisation are lossless on these inputs and every contraction is an exact integer sum: the guarded
    output buffer equals the fp64-chain reference bit for bit, twice in a row (test_w8a8_host.py: the single faults that
    cannot pass - a fragment from the neighbouring k group, a dropped K slice, a scale of the row beside or of another segment,
    W1 / W3 exchanged, the scale applied after the rounding, a store past a ragged edge)."""
    h = _hip()
    bad = []
    for case in (c for c in CASES if c.epi == group):
        want = wc.expected(case)
        first, second = _run_case(h, case), _run_case(h, case)
        if not torch.equal(first, want):
            bad.append((case.name, lc.describe(case, first, want)))
        assert torch.equal(first, second), case
    assert not bad, bad[:3]


# ------------------------------------------------------------------------------------------------ 2. the quantiser, bit for bit
def _same_as_cpu(h, x, **kw):
    q, s = h.act_quant_e4m3(x.cuda(), **kw)
    return q.view(torch.uint8).cpu(), s.cpu()


@pytest.mark.parametrize("K", [128, 4096, 14336])
def test_act_quant_is_quantize_rows_bit_for_bit(K):
    h, quant = _hip(), _quant()
    g = torch.Generator().manual_seed(K)
    rows = [torch.randn(K, generator=g) * m for m in (1e-30, 1e-6, 0.02, 1.0, 37.0, 3e4, 1e30)]
    for e in (-20, -9, 0, 7, 100):                      # amax exactly 448 * 2^e, and one bf16 ulp either side
        for step in (-1, 0, 1):
            r = torch.randn(K, generator=g).clamp_(-3, 3) * 2.0 ** e
            top = torch.tensor(448.0 * 2.0 ** e).to(BF)
            r[5] = (top.view(torch.int16) + step).view(BF).float()
            rows.append(r)
    rows.append(torch.zeros(K))                          # scale 1, codes 0
    big = torch.randn(K, generator=g) * 1e37
    big[K // 2] = -float(torch.finfo(BF).max)            # the row that holds bf16 max: its code steps down instead of reaching inf
    rows.append(big)
    ld = K + 24
    buf = torch.zeros(len(rows), ld).to(BF)
    buf[:, :K] = torch.stack(rows).to(BF)
    x = buf[:, :K]                                       # ldx > K
    want_q, want_s = quant.quantize_rows(x)
    xd = buf.cuda()[:, :K]
    q, s = h.act_quant_e4m3(xd)
    q, s = q.view(torch.uint8).cpu(), s.cpu()
    assert torch.equal(s, want_s), (s, want_s)
    assert torch.equal(q, want_q.view(torch.uint8)), int((q != want_q.view(torch.uint8)).sum())
    assert not bool(((q & 0x7F) == 0x7F).any()) and float(want_s[-2]) == 1.0
    assert bool(torch.isfinite(quant.dequantize(q, s).float()).all())
    # with the fused norm: the row quantised is the bf16 row the RMSNorm kernel writes
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    xs = rnd(9, K, seed=K + 1, scale=2.0)
    xn = h.rmsnorm(xs.cuda(), nw.cuda(), 1e-5).cpu()
    want_q, want_s = quant.quantize_rows(xn)
    q, s = _same_as_cpu(h, xs, norm_w=nw.cuda(), eps=1e-5)
    assert torch.equal(s, want_s) and torch.equal(q, want_q.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ 3. Gaussian leaf
class QW:
    """tests/test_gpu_fp8.py's QW: a random matrix quantised by the project's quantiser."""

    def __init__(self, n, k, seed):
        self.q, s = _quant().quantize_rows(rnd(n, k, seed=seed, scale=k ** -0.5))
        self.s = s.float().contiguous()
        self.vals = self.q.double()
        self.qd, self.sd = self.q.view(torch.uint8).cuda(), self.s.cuda()

    def sums(self, x):
        xd = x.double()
        return (xd @ self.vals.T) * self.s.double(), (xd.abs() @ self.vals.abs().T) * self.s.double()


@pytest.mark.parametrize("M,K,N", [(300, 1152, 200), (513, 4096, 264)])
def test_gaussian_leaf_inside_the_envelopes_of_the_fp8_tests(M, K, N):
    """N(0, 1) x and N(0, 1/K) weights.  The reference is fp64 on the CPU-quantised operands - dequantize(quantize_rows(.)) of both -
    with the bf16 rounding chain; only the summation order differs from it, so the bounds are test_gpu_fp8.py's: STORE
    |y - ref| <= 2^-8 |ref| + K 2^-23 sum|w x|, RESIDUAL and SWIGLU inside the envelope of their chains.  mi_linear_w8 on the same
    dequantised activations must pass the identical bound."""
    h, quant = _hip(), _quant()
    x = rnd(M, K, seed=5)
    xd = quant.dequantize(*quant.quantize_rows(x))           # the activations the route contracts, as bf16 rows (exact)
    w1, w3 = QW(N, K, seed=6), QW(N, K, seed=7)
    res = rnd(M, N, seed=8)
    ref, mag = w1.sums(xd)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    for name, got in (("w8a8", h.linear_w8a8(x.cuda(), [w1.qd], [w1.sd])), ("w8 on dequantised x", h.linear_w8(xd.cuda(), [w1.qd], [w1.sd]))):
        err = (got.double().cpu() - ref).abs()
        print(f"{name} store M={M} K={K}: worst |err| / bound = {float((err / bound.clamp_min(1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), name
    f = lambda y: bf(res.float() + bf(y))  # noqa: E731
    for name, got in (("w8a8", h.linear_w8a8(x.cuda(), [w1.qd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda())),
                      ("w8 on dequantised x", h.linear_w8(xd.cuda(), [w1.qd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda()))):
        ok, over = inside_envelope(got.cpu(), f, [ref], [deltas_of(ref, mag, K)])
        assert ok, ("residual", name, over)
    r3, m3 = w3.sums(xd)
    g = lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3))  # noqa: E731
    for name, got in (("w8a8", h.linear_w8a8(x.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU)),
                      ("w8 on dequantised x", h.linear_w8(xd.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU))):
        ok, over = inside_envelope(got.cpu(), g, [ref, r3], [deltas_of(ref, mag, K), deltas_of(r3, m3, K)])
        assert ok, ("swiglu", name, over)


# ------------------------------------------------------------------------------------------------ 4. fallbacks unchanged
@pytest.mark.parametrize("M,K", [(8, 256), (9, 256), (255, 256), (300, 192), (512, 1040), (300, 16512)])
def test_below_the_limit_the_leaf_is_mi_linear_w8(M, K):
    """Few rows, K % 128 != 0, and K = 16512 - a multiple of 128 above the 16384 elements the quantiser holds in registers (the w2
    group of a model with hidden_dim > 16384): the weight-only route, bit for bit, not an error."""
    h = _hip()
    x, res = rnd(M, K, seed=M), rnd(M, 72, seed=M + 1)
    w1, w3 = QW(72, K, seed=11), QW(72, K, seed=12)
    for epi, ws, kw in ((h.EPI_STORE, [w1, w3], {}), (h.EPI_RESIDUAL, [w1], dict(residual=res.cuda())), (h.EPI_SWIGLU, [w1, w3], {})):
        a = h.linear_w8a8(x.cuda(), [w.qd for w in ws], [w.sd for w in ws], epi, **kw)
        b = h.linear_w8(x.cuda(), [w.qd for w in ws], [w.sd for w in ws], epi, **kw)
        assert torch.equal(a, b), (M, K, epi)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return qu.make_folders(qu.FP8, tmp_path_factory)


def test_short_prompts_decode_steps_and_speculative_decoding_are_unchanged(folders):
    """12 prompt tokens, then decode steps from identical caches: prefill_fp8 on and off give the same bits (fewer than 256 rows is
    launch for launch mi_forward_w8); generate(speculative=...) on the flagged model returns the plain greedy loop's tokens."""
    from mistral_inference.generate import SpeculativeArgs, generate
    off, on = qu._load(folders[1], B=1), qu._load(folders[1], B=1, prefill_fp8=True)
    assert on.prefill_fp8 and not off.prefill_fp8
    prompt = qu.PROMPTS[1][0]
    ca, cb = _cache(1), _cache(1)
    with torch.inference_mode():
        la = off.forward(torch.tensor(prompt, device="cuda"), [len(prompt)], ca)
        lb = on.forward(torch.tensor(prompt, device="cuda"), [len(prompt)], cb)
        assert torch.equal(la, lb)
        tok = la[-1:].argmax(-1)
        for _ in range(6):
            la, lb = off.forward(tok, [1], ca), on.forward(tok, [1], cb)
            assert torch.equal(la, lb)
            tok = la.argmax(-1)
    plain, _ = generate([prompt], off, max_tokens=12, temperature=0.0)
    spec, _ = generate([prompt], on, max_tokens=12, temperature=0.0, speculative=SpeculativeArgs(k=4))
    assert spec == plain


# ------------------------------------------------------------------------------------------------ 5. model level
T_LONG = 300


def _one_layer(folders, tmp_path, **kw):
    import safetensors
    from safetensors.torch import save_file
    src = folders[1]
    one = tmp_path / "one"
    one.mkdir()
    p = json.load(open(src + "/params.json"))
    json.dump(dict(p, n_layers=1), open(one / "params.json", "w"))
    with safetensors.safe_open(src + "/consolidated.safetensors", framework="pt", device="cpu") as f:
        save_file({k: f.get_tensor(k) for k in f.keys() if not k.startswith("layers.1.")}, str(one / "consolidated.safetensors"))
    return qu._load(str(one), B=1, **kw)


def _long_ids():
    g = torch.Generator().manual_seed(300)
    return torch.randint(0, qu.MODEL.vocab_size, (T_LONG,), generator=g).cuda()


def test_module_level_block_against_the_runner_at_300_rows(folders, tmp_path):
    """quant_util.check_module_level_block's comparison with prefill_fp8=True: TransformerBlock.forward module by module
    (mi_rmsnorm, mi_linear_w8a8, mi_rope_inplace leaves) against the same layer inside mi_forward_w8a8, at most 2 bf16 ulps at the
    block output's largest magnitude; and the route is really taken: the output differs from the flag-off runner's."""
    model = _one_layer(folders, tmp_path, prefill_fp8=True)
    ids = _long_ids()
    with torch.inference_mode():
        h, _ = model._run(ids, [T_LONG], None, want_logits=True)
        out = model.layers["0"](model.tok_embeddings.weight[ids], model.freqs_cis[torch.arange(T_LONG, device="cuda")])
        model.prefill_fp8 = False
        h_off, _ = model._run(ids, [T_LONG], None, want_logits=True)
    assert bool(torch.isfinite(h.float()).all()) and not torch.equal(out, torch.zeros_like(out))
    tol = 2.0 * float(qu.ulp_bf16(h.float().abs().max().cpu()))
    worst = float((out.float() - h.float()).abs().max())
    print(f"module-level block to runner: max |d| = {worst:.4e} (bound {tol:.4e}); runner on to off: {float((h.float() - h_off.float()).abs().max()):.4e}")
    assert worst <= tol, (worst, tol)
    assert not torch.equal(h, h_off)


@pytest.mark.parametrize("kv", [None, torch.float8_e4m3fn], ids=["bf16_rings", "e4m3_rings"])
def test_long_prompt_logits_with_either_ring_dtype_and_prompt_logprobs(folders, kv):
    from mistral_inference.cache import BufferCache
    model = qu._load(folders[1], B=1, prefill_fp8=True)
    ids = _long_ids()
    mk = lambda: BufferCache(qu.MODEL.n_layers, 1, 512, qu.MODEL.n_kv_heads, qu.MODEL.head_dim, qu.MODEL.sliding_window,  # noqa: E731
                             device="cuda", dtype=kv or BF)
    tgt = torch.cat([ids[1:], ids[:1]]).to(torch.int32)
    with torch.inference_mode():
        on = model.forward(ids, [T_LONG], mk())
        on_bf16 = model.forward(ids, [T_LONG], _cache(1))
        lp_on, last_on = model.prompt_logprobs(ids, [T_LONG], mk(), tgt)
        model.prefill_fp8 = False
        off = model.forward(ids, [T_LONG], mk())
        lp_off, _ = model.prompt_logprobs(ids, [T_LONG], mk(), tgt)
    assert bool(torch.isfinite(on).all()) and not torch.equal(on, off)
    assert float((on - on_bf16).abs().max()) <= qu.LOGIT_ATOL          # an empty ring of either dtype: the chunk reads its own rows
    want = torch.log_softmax(on, dim=-1)[torch.arange(T_LONG), tgt.long()]
    assert float((lp_on - want).abs().max()) <= 1e-3 and not torch.equal(lp_on, lp_off)
    assert float((last_on - on[-1:]).abs().max()) <= qu.LOGIT_ATOL
    print(f"logits on to off: max |d| = {float((on - off).abs().max()):.4e}")


def test_workspace_query_and_a_workspace_one_byte_short(folders):
    h = _hip()
    model = qu._load(folders[1], B=1, prefill_fp8=True)
    ids = _long_ids()
    with torch.inference_mode():
        model.forward(ids, [T_LONG], None)                      # builds the plan and a workspace of the route's size
    be = model._backend
    m, qm = be.plan(model), be._quant[0]
    L = h.lib()
    for lay in (0, 1, h.KV_E4M3):
        need = L.mi_workspace_bytes_w8a8(C.byref(m), C.byref(qm), T_LONG, 1, 16, lay)
        assert need >= L.mi_workspace_bytes_kv(C.byref(m), 1, T_LONG, 1, 16, lay) + T_LONG * 1024 + T_LONG * 4
    need = L.mi_workspace_bytes_w8a8(C.byref(m), C.byref(qm), T_LONG, 1, 1, 0)
    assert be._workspace.numel() >= need
    i32 = torch.zeros(T_LONG + 2, dtype=torch.int32, device="cuda")
    hbuf = torch.zeros(T_LONG, qu.MODEL.dim, dtype=BF, device="cuda")
    bt = h.MiBatch()
    bt.T, bt.B, bt.branch, bt.max_q_len = T_LONG, 1, h.BRANCH_NOCACHE, T_LONG
    bt.input_ids = ids.data_ptr()
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = i32.data_ptr()
    bt.h, bt.workspace, bt.workspace_bytes = hbuf.data_ptr(), be._workspace.data_ptr(), need - 1
    assert L.mi_forward_w8a8(C.byref(m), C.byref(qm), C.byref(bt), None) == -3     # MI_ERR_WORKSPACE, before any launch
    assert "workspace" in L.mi_last_error_detail().decode()
