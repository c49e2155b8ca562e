"""MXFP4 x FP8 prefill GEMMs (W4A8) on the device: the GEMM (csrc/gemm256_w4a8.hip) behind the activation quantiser on the exact
structured cases of tests/w4a8_cases.py and on Gaussian operands inside the envelopes of tests/test_gpu_w8a8.py, the fallbacks below
the applicability limit bit for bit, and a model with `prefill_w4a8=True`."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

import linear_cases as lc
import mxfp4_cases as mc
import quant_util as qu
import w4a8_cases as wc
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
    codes = [c.cuda() for c in inp.codes]
    scales = [s.cuda() for s in inp.scales]
    x = inp.x.cuda()
    if case.epi == lc.QKV:
        H, Hkv = case.qkv[:2]
        h.qkv_rope_w4a8(x, codes, scales, H, Hkv, inp.rope_cs.cuda(), inp.tok_pos.cuda(), out=view)
    else:
        res = None
        if case.epi == lc.RESIDUAL:   # in a buffer of the output's geometry: the epilogue reads it at the output's row stride
            rbuf = torch.zeros_like(buf)
            res = rbuf[2:2 + case.M, :case.N]
            res.copy_(inp.res.cuda())
        h.linear_w4a8(x, codes, scales, lc.EPI_CODE[case.epi], residual=res, out=view)
    return buf.cpu()


@pytest.mark.parametrize("group", [lc.STORE, lc.RESIDUAL, lc.SWIGLU, lc.QKV])
def test_structured_cases_are_bit_equal_to_the_fp64_chain_reference(group):
    """The activation quantisation is lossless on these inputs and every contraction an exact fp32 sum in any order: the guarded
    output buffer equals the fp64-chain reference bit for bit, twice in a row, no case left out (test_w4a8_host.py: the single
    faults that cannot pass - the nibbles of a byte exchanged, the scale of the next block, of the next K tile, of the row beside,
    of another segment, every scale 127, s_x of the row beside, a dropped K slice, W1 / W3 exchanged, a store past a ragged edge)."""
    h = _hip()
    bad = []
    for case in (c for c in CASES if c.epi == group):
        want = wc.expected(case)
        first, second = _run_case(h, case), _run_case(h, case)
        if not torch.equal(first, want):
            bad.append((case.name, lc.describe(case, first, want)))
        assert torch.equal(first, second), case
    assert not bad, (len(bad), bad[:3])


# ------------------------------------------------------------------------------------------------ 2. Gaussian leaf
class QW:
    """A random matrix quantised by the project's MXFP4 quantiser; its real values by mxfp4_cases' independent dequantiser."""

    def __init__(self, n, k, seed):
        self.q, self.s = _quant().quantize_blocks(rnd(n, k, seed=seed, scale=k ** -0.5))
        self.vals = mc.dequant_f64(self.q, self.s)
        self.qd, self.sd = self.q.cuda(), self.s.cuda()

    def sums(self, x):
        xd = x.double()
        return xd @ self.vals.T, xd.abs() @ self.vals.abs().T


@pytest.mark.parametrize("M,K,N", [(300, 1152, 200), (513, 4096, 264)])
def test_gaussian_leaf_inside_the_envelopes_of_the_w8a8_tests(M, K, N):
    """N(0, 1) x and N(0, 1/K) weights.  The reference is fp64 on the CPU-quantised operands - dequantize(quantize_rows(x)) and the
    dequantised MXFP4 weights - with the bf16 rounding chain; only the summation order differs from it, so the bounds are
    test_gpu_w8a8.py's, unchanged: STORE |y - ref| <= 2^-8 |ref| + K 2^-23 sum|w x|, RESIDUAL and SWIGLU inside the envelope of
    their chains.  mi_linear_w4 on the same dequantised activations must pass the identical bound."""
    h, quant = _hip(), _quant()
    x = rnd(M, K, seed=5)
    xd = quant.dequantize(*quant.quantize_rows(x))           # the activations the route contracts, as bf16 rows (exact)
    w1, w3 = QW(N, K, seed=6), QW(N, K, seed=7)
    res = rnd(M, N, seed=8)
    ref, mag = w1.sums(xd)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    for name, got in (("w4a8", h.linear_w4a8(x.cuda(), [w1.qd], [w1.sd])), ("w4 on dequantised x", h.linear_w4(xd.cuda(), [w1.qd], [w1.sd]))):
        err = (got.double().cpu() - ref).abs()
        print(f"{name} store M={M} K={K}: worst |err| / bound = {float((err / bound.clamp_min(1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), name
    f = lambda y: bf(res.float() + bf(y))  # noqa: E731
    for name, got in (("w4a8", h.linear_w4a8(x.cuda(), [w1.qd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda())),
                      ("w4 on dequantised x", h.linear_w4(xd.cuda(), [w1.qd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda()))):
        ok, over = inside_envelope(got.cpu(), f, [ref], [deltas_of(ref, mag, K)])
        assert ok, ("residual", name, over)
    r3, m3 = w3.sums(xd)
    g = lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3))  # noqa: E731
    for name, got in (("w4a8", h.linear_w4a8(x.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU)),
                      ("w4 on dequantised x", h.linear_w4(xd.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU))):
        ok, over = inside_envelope(got.cpu(), g, [ref, r3], [deltas_of(ref, mag, K), deltas_of(r3, m3, K)])
        assert ok, ("swiglu", name, over)


# ------------------------------------------------------------------------------------------------ 3. fallbacks unchanged
@pytest.mark.parametrize("M,K", [(8, 256), (9, 256), (255, 256), (300, 192), (512, 1056), (300, 16512)])
def test_below_the_limit_the_leaf_is_mi_linear_w4(M, K):
    """Few rows, K % 128 != 0, and K = 16512 - a multiple of 128 above the 16384 elements the quantiser holds in registers: the
    weight-only route, bit for bit, not an error."""
    h = _hip()
    x, res = rnd(M, K, seed=M), rnd(M, 72, seed=M + 1)
    w1, w3 = QW(72, K, seed=11), QW(72, K, seed=12)
    for epi, ws, kw in ((h.EPI_STORE, [w1, w3], {}), (h.EPI_RESIDUAL, [w1], dict(residual=res.cuda())), (h.EPI_SWIGLU, [w1, w3], {})):
        a = h.linear_w4a8(x.cuda(), [w.qd for w in ws], [w.sd for w in ws], epi, **kw)
        b = h.linear_w4(x.cuda(), [w.qd for w in ws], [w.sd for w in ws], epi, **kw)
        assert torch.equal(a, b), (M, K, epi)


def test_operands_the_wide_accesses_cannot_read_take_the_weight_only_route():
    """Inside the route's shape, a code matrix that is not 16-byte aligned or a scale matrix that is not 4-byte aligned is no error:
    mi_linear_w4's routes, bit for bit."""
    h = _hip()
    M, K, N = 300, 256, 72
    x, w = rnd(M, K, seed=3).cuda(), QW(N, K, seed=13)
    qoff = torch.zeros(N * K // 2 + 8, dtype=torch.uint8, device="cuda")[8:].view(N, K // 2)
    qoff.copy_(w.qd)
    soff = torch.zeros(N * K // 32 + 2, dtype=torch.uint8, device="cuda")[2:].view(N, K // 32)
    soff.copy_(w.sd)
    assert qoff.data_ptr() % 16 == 8 and soff.data_ptr() % 4 == 2
    want = h.linear_w4(x, [w.qd], [w.sd])
    assert torch.equal(h.linear_w4a8(x, [qoff], [w.sd]), want)
    assert torch.equal(h.linear_w4a8(x, [w.qd], [soff]), want)
    assert not torch.equal(h.linear_w4a8(x, [w.qd], [w.sd]), want)      # (aligned, the route is taken: Gaussian x is not lossless)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return qu.make_folders(qu.MXFP4, tmp_path_factory)


def test_short_prompts_decode_steps_and_speculative_decoding_are_unchanged(folders):
    """12 prompt tokens, then decode steps from identical caches: prefill_w4a8 on and off give the same bits (fewer than 256 rows is
    launch for launch mi_forward_w4); generate(speculative=...) on the flagged model returns the plain greedy loop's tokens."""
    from mistral_inference.generate import SpeculativeArgs, generate
    off, on = qu._load(folders[1], B=1), qu._load(folders[1], B=1, prefill_w4a8=True)
    assert on.prefill_w4a8 and not off.prefill_w4a8
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


# ------------------------------------------------------------------------------------------------ 4. model level
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
    """quant_util.check_module_level_block's comparison with prefill_w4a8=True at 300 rows: TransformerBlock.forward module by module
    (mi_rmsnorm, mi_linear_w4a8, mi_rope_inplace leaves) against the same layer inside mi_forward_w4a8, under that helper's bound for
    more than 8 rows - bit-equal: the fused norm quantises the bf16 row mi_rmsnorm writes, the GEMM's RoPE epilogue is
    mi_rope_inplace's arithmetic on the same bf16 values.  And the route is really taken: the output differs from the flag-off
    runner's."""
    model = _one_layer(folders, tmp_path, prefill_w4a8=True)
    ids = _long_ids()
    with torch.inference_mode():
        h, _ = model._run(ids, [T_LONG], None, want_logits=True)
        out = model.layers["0"](model.tok_embeddings.weight[ids], model.freqs_cis[torch.arange(T_LONG, device="cuda")])
        model.prefill_w4a8 = False
        h_off, _ = model._run(ids, [T_LONG], None, want_logits=True)
    assert bool(torch.isfinite(h.float()).all()) and not torch.equal(out, torch.zeros_like(out))
    worst = float((out.float() - h.float()).abs().max())
    print(f"module-level block to runner: max |d| = {worst:.4e}; runner on to off: {float((h.float() - h_off.float()).abs().max()):.4e}")
    assert torch.equal(out, h), worst
    assert not torch.equal(h, h_off)


@pytest.mark.parametrize("kv", [None, torch.float8_e4m3fn], ids=["bf16_rings", "e4m3_rings"])
def test_long_prompt_logits_with_either_ring_dtype_and_prompt_logprobs(folders, kv):
    from mistral_inference.cache import BufferCache
    model = qu._load(folders[1], B=1, prefill_w4a8=True)
    ids = _long_ids()
    mk = lambda: BufferCache(qu.MODEL.n_layers, 1, 512, qu.MODEL.n_kv_heads, qu.MODEL.head_dim, qu.MODEL.sliding_window,  # noqa: E731
                             device="cuda", dtype=kv or BF)
    tgt = torch.cat([ids[1:], ids[:1]]).to(torch.int32)
    with torch.inference_mode():
        on = model.forward(ids, [T_LONG], mk())
        on_bf16 = model.forward(ids, [T_LONG], _cache(1))
        lp_on, last_on = model.prompt_logprobs(ids, [T_LONG], mk(), tgt)
        model.prefill_w4a8 = False
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
    model = qu._load(folders[1], B=1, prefill_w4a8=True)
    ids = _long_ids()
    with torch.inference_mode():
        model.forward(ids, [T_LONG], None)                      # builds the plan and a workspace of the route's size
    be = model._backend
    m, qm = be.plan(model), be._quant[0]
    L = h.lib()
    for lay in (0, 1, h.KV_E4M3):
        need = L.mi_workspace_bytes_w4a8(C.byref(m), C.byref(qm), T_LONG, 1, 16, lay)
        assert need >= L.mi_workspace_bytes_kv(C.byref(m), 1, T_LONG, 1, 16, lay) + T_LONG * 1024 + T_LONG * 4
    need = L.mi_workspace_bytes_w4a8(C.byref(m), C.byref(qm), T_LONG, 1, 1, 0)
    assert be._workspace.numel() >= need
    i32 = torch.zeros(T_LONG + 2, dtype=torch.int32, device="cuda")
    hbuf = torch.zeros(T_LONG, qu.MODEL.dim, dtype=BF, device="cuda")
    bt = h.MiBatch()
    bt.T, bt.B, bt.branch, bt.max_q_len = T_LONG, 1, h.BRANCH_NOCACHE, T_LONG
    bt.input_ids = ids.data_ptr()
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = i32.data_ptr()
    bt.h, bt.workspace, bt.workspace_bytes = hbuf.data_ptr(), be._workspace.data_ptr(), need - 1
    assert L.mi_forward_w4a8(C.byref(m), C.byref(qm), C.byref(bt), None) == -3     # MI_ERR_WORKSPACE, before any launch
    assert "workspace" in L.mi_last_error_detail().decode()
