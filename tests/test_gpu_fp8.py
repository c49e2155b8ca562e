"""Weight-only FP8 (OCP e4m3) on the device: the e4m3 GEMV family and the dequantise + GEMM route (csrc/gemv_w8.hip) through the
new leaves, the layer-stack runner on a quantised model, the loader paths, generate() and the module-level block.

The numerics contract (quant.py): acc = sum_k e4m3(W[r, k]) x[k] in fp32, y = acc * scale[r] in fp32, and y enters the bf16
kernels' epilogues where acc enters them; above 8 rows the MFMA GEMM runs on bf16(scale * e4m3(W)).  With power-of-two scales
both are the bf16 model on the dequantised weights up to fp32 summation order, which is what the tolerances below state."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import mistral_oracle as mo
import quant_util as qu
from quant_util import BF, _cache, _hip, _quant, bf, deltas_of, inside_envelope, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(512, 96), (1040, 33), (4096, 512), (14336, 64)]   # (1040, 33): a 16-weight tail in the second chunk, an odd row
MS = [1, 3, 8]                                               # count and fewer units than waves


class QW:
    """A random weight matrix quantised by the project's quantiser: bytes, scales, exact values, its bf16 dequantisation."""

    def __init__(self, n, k, seed, arbitrary=False):
        q, s = _quant().quantize_rows(rnd(n, k, seed=seed, scale=k ** -0.5))
        if arbitrary:  # scales as another quantiser might make them: positive, finite, not powers of two
            s = s * (1.0 + 0.37 * torch.rand(n, generator=torch.Generator().manual_seed(seed + 1000)))
        self.q, self.s = q, s.float().contiguous()
        self.vals = q.double()                       # e4m3(W), exact
        self.deq = _quant().dequantize(q, self.s)    # exact iff the scales are powers of two
        self.qd, self.sd, self.deqd = q.view(torch.uint8).cuda(), self.s.cuda(), self.deq.cuda()

    def sums(self, x):
        """fp64: s * sum_k w x  and  s * sum_k |w x|, [M, n]."""
        xd = x.double()
        return (xd @ self.vals.T) * self.s.double(), (xd.abs() @ self.vals.abs().T) * self.s.double()


# ------------------------------------------------------------------------------------------------ 1. the decode of every code
def test_every_e4m3_code_decodes_as_ocp_e4m3fn():
    """All 254 finite codes (both zeros included) at K = 16, the smallest the kernels take; scales 1 and 2^-3; one-hot bf16
    rows.  Every output is ONE exact product, so it equals W[r, c] * scale[r] bit for bit (as values: the kernels' +0 start makes
    the product with the code 0x80 a +0) - on the GEMV (8 rows) and on the dequantise + GEMM route (16 rows).  An fnuz decode, a
    dropped subnormal or a swapped byte within the dword cannot pass."""
    h = _hip()
    codes = [c for c in range(256) if c & 0x7F != 0x7F]
    assert len(codes) == 254
    wb = torch.tensor(codes + [0x00, 0x80], dtype=torch.uint8).reshape(16, 16)
    w = wb.view(torch.float8_e4m3fn).float()
    assert bool(torch.isfinite(w).all()) and float(w.abs().max()) == 448.0 and float(w.abs()[w != 0].min()) == 2.0 ** -9
    scale = torch.tensor([1.0, 0.125] * 8)
    ref = (w * scale[:, None]).T.contiguous()          # ref[c, r]: the row of the one-hot input e_c
    eye = torch.eye(16, dtype=BF).cuda()
    wd, sd = wb.cuda(), scale.cuda()
    for rows in (slice(0, 8), slice(8, 16)):           # M = 8: the e4m3 GEMV
        got = h.linear_w8(eye[rows].contiguous(), [wd], [sd]).float().cpu()
        assert torch.equal(got, ref[rows]), (got - ref[rows]).abs().max()
    got = h.linear_w8(eye, [wd], [sd]).float().cpu()   # M = 16: dequantise + MFMA GEMM
    assert torch.equal(got, ref), (got - ref).abs().max()
    one = h.linear_w8(eye[3:4].contiguous(), [wd], [sd]).float().cpu()   # one token: the four-row-unit instantiations' sibling
    assert torch.equal(one, ref[3:4])


# ------------------------------------------------------------------------------------------------ 2. STORE against fp64
@pytest.fixture(scope="module")
def store_cases():
    """Per (K, N): the quantised matrix, the inputs of the largest M, a norm weight - made once, shared, never changed."""
    out = {}
    for i, (K, N) in enumerate(SHAPES):
        out[(K, N)] = (QW(N, K, seed=20 + i), QW(N, K, seed=20 + i, arbitrary=True), rnd(8, K, seed=30 + i, scale=2.0),
                       (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(40 + i))).to(BF))
    return out


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "fused_norm"])
@pytest.mark.parametrize("K,N", SHAPES)
def test_linear_w8_store_against_fp64(store_cases, K, N, norm):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 s sum|w x|: one bf16 rounding of the result plus fp32 accumulation in any order (the
    standard bound gamma_K ~ K 2^-24, doubled).  ref is the fp64 product on the rows the kernel contracts (the RMS-normalised
    bf16 rows when the norm is fused).  mi_linear on the dequantised weights must pass the identical bound - the tolerance's own
    check - where dequantisation is exact (power-of-two scales; with arbitrary scales the bf16 image of a weight is rounded,
    which is the documented difference between the two forms and outside this bound)."""
    h = _hip()
    pow2, arb, x8, nw = store_cases[(K, N)]
    for M, qw in itertools.chain(((m, pow2) for m in MS), [(3, arb)]):
        x = x8[:M].contiguous()
        xn = mo.rms_norm(x, nw, 1e-5) if norm else x
        ref, mag = qw.sums(xn)
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
        kw = dict(norm_w=nw.cuda(), eps=1e-5) if norm else {}
        got = h.linear_w8(x.cuda(), [qw.qd], [qw.sd], **kw).double().cpu()
        worst = float(((got - ref).abs() / bound.clamp_min(1e-30)).max())
        print(f"w8 store K={K} N={N} M={M} norm={norm} arbitrary={qw is arb}: worst |err| / bound = {worst:.3f}")
        assert bool(((got - ref).abs() <= bound).all()), (M, worst)
        if qw is pow2:
            base = h.linear(x.cuda(), (qw.deqd,), **kw).double().cpu()
            worst_b = float(((base - ref).abs() / bound.clamp_min(1e-30)).max())
            print(f"   bf16 mi_linear on the dequantised weights: worst |err| / bound = {worst_b:.3f}")
            assert bool(((base - ref).abs() <= bound).all()), (M, worst_b)


# ------------------------------------------------------------------------------------------------ 3. the fused epilogues
@pytest.mark.parametrize("K,N", SHAPES)
def test_linear_w8_residual_and_swiglu_envelopes(store_cases, K, N):
    h = _hip()
    w1, _, x8, nw = store_cases[(K, N)]
    w3 = QW(N, K, seed=77)
    res8 = rnd(8, N, seed=78)
    for M in MS:
        x, res = x8[:M].contiguous(), res8[:M].contiguous()
        # residual: out = bf16(res + bf16(y))
        ref, mag = w1.sums(x)
        f = lambda y: bf(res.float() + bf(y))  # noqa: E731
        for name, got in (("w8", h.linear_w8(x.cuda(), [w1.qd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda())),
                          ("bf16 on dequantised", h.linear(x.cuda(), (w1.deqd,), h.EPI_RESIDUAL, residual=res.cuda()))):
            ok, over = inside_envelope(got.cpu(), f, [ref], [deltas_of(ref, mag, K)])
            assert ok, ("residual", name, M, over)
        # swiglu with the fused norm: out = bf16(bf16(silu(bf16(y1))) * bf16(y3)) on the RMS-normalised rows
        xn = mo.rms_norm(x, nw, 1e-5)
        (r1, m1), (r3, m3) = w1.sums(xn), w3.sums(xn)
        g = lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3))  # noqa: E731
        kw = dict(norm_w=nw.cuda(), eps=1e-5)
        for name, got in (("w8", h.linear_w8(x.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU, **kw)),
                          ("bf16 on dequantised", h.linear(x.cuda(), (w1.deqd, w3.deqd), h.EPI_SWIGLU, **kw))):
            assert tuple(got.shape) == (M, N)
            ok, over = inside_envelope(got.cpu(), g, [r1, r3], [deltas_of(r1, m1, K), deltas_of(r3, m3, K)])
            assert ok, ("swiglu", name, M, over)


def test_four_row_units_at_one_token():
    """One token and at least 32 row pairs per CU: launch_gemv_w8 switches to units of four rows (the W1|W3 shape of a 7B
    model).  The smallest such matrices on a 256-CU device, with an odd pair count so that the last unit is half empty: STORE
    against the fp64 bound of test_linear_w8_store_against_fp64, SWIGLU inside its envelope."""
    h = _hip()
    K = 512
    x = rnd(1, K, seed=90, scale=2.0)
    w = QW(16390, K, seed=91)
    ref, mag = w.sums(x)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    got = h.linear_w8(x.cuda(), [w.qd], [w.sd]).double().cpu()
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound.clamp_min(1e-30)).max())
    w1, w3 = QW(8195, K, seed=92), QW(8195, K, seed=93)
    (r1, m1), (r3, m3) = w1.sums(x), w3.sums(x)
    got = h.linear_w8(x.cuda(), [w1.qd, w3.qd], [w1.sd, w3.sd], h.EPI_SWIGLU).cpu()
    ok, over = inside_envelope(got, lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3)), [r1, r3],
                               [deltas_of(r1, m1, K), deltas_of(r3, m3, K)])
    assert ok, over


@pytest.mark.parametrize("head_major", [False, True], ids=["slot_major", "head_major"])
@pytest.mark.parametrize("D", [512, 1040, 4096, 14336])
def test_qkv_rope_kvwrite_w8_envelope_and_ring(D, head_major):
    """q|k|v + RoPE + ring write on e4m3 weights: every output inside the envelope of `bf16(rope(bf16(y0), bf16(y1)))`; the ring
    rows are the k | v columns of the same call's output bit for bit, in both ring layouts, at positions past the ring's length
    (slot = pos % W wraps) and with tok_seq a permutation."""
    h = _hip()
    H, Hkv, Dh, W = 2, 1, 128, 24
    nq, nkv = H * Dh, Hkv * Dh
    wq, wk, wv = QW(nq, D, seed=50), QW(nkv, D, seed=51), QW(nkv, D, seed=52)
    nw = (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(53))).to(BF)
    cs = mo.rope_angles(Dh, 4000, 1e6)
    x8 = rnd(8, D, seed=54, scale=2.0)
    for T in MS:
        x = x8[:T].contiguous()
        pos = torch.tensor([W + 5, 3, 4 * W - 1, 977, 2 * W, 31, 7, 1500][:T], dtype=torch.int32)   # the first: wraps to slot 5
        seq = torch.arange(T, dtype=torch.int32).flip(0).contiguous()
        mk = (lambda: torch.zeros(T, Hkv, W, Dh, dtype=BF, device="cuda").permute(0, 2, 1, 3)) if head_major else \
             (lambda: torch.zeros(T, W, Hkv, Dh, dtype=BF, device="cuda"))
        xn = mo.rms_norm(x, nw, 1e-5)
        sums = [w.sums(xn) for w in (wq, wk, wv)]
        ref = torch.cat([s[0] for s in sums], dim=1)
        dl = deltas_of(ref, torch.cat([s[1] for s in sums], dim=1), D)
        c = cs[pos.long()]                                   # [T, Dh / 2, 2] = (cos, sin)
        cos = torch.cat([c[..., 0].repeat(1, H + Hkv), torch.ones(T, nkv // 2)], dim=1)    # v pairs: the identity turn
        sin = torch.cat([c[..., 1].repeat(1, H + Hkv), torch.zeros(T, nkv // 2)], dim=1)
        rot = (torch.arange(ref.shape[1] // 2) < (nq + nkv) // 2)[None, :]
        re = lambda y0, y1: bf(torch.where(rot, bf(y0) * cos - bf(y1) * sin, bf(y0)))  # noqa: E731
        im = lambda y0, y1: bf(torch.where(rot, bf(y0) * sin + bf(y1) * cos, bf(y1)))  # noqa: E731
        ev, od = ref[:, 0::2], ref[:, 1::2]
        for name in ("w8", "bf16 on dequantised"):
            ck, cv = mk(), mk()
            if name == "w8":
                got = h.qkv_rope_kvwrite_w8(x.cuda(), wq.qd, wk.qd, wv.qd, wq.sd, wk.sd, wv.sd, Dh, cs.cuda(), pos.cuda(), norm_w=nw.cuda(),
                                            eps=1e-5, cache_k=ck, cache_v=cv, tok_seq=seq.cuda()).cpu()
            else:
                got = h.qkv_rope_kvwrite(x.cuda(), wq.deqd, wk.deqd, wv.deqd, Dh, cs.cuda(), pos.cuda(), norm_w=nw.cuda(), eps=1e-5,
                                         cache_k=ck, cache_v=cv, tok_seq=seq.cuda()).cpu()
            for part, f in ((got[:, 0::2], re), (got[:, 1::2], im)):
                ok, over = inside_envelope(part, f, [ev, od], [dl[:, 0::2], dl[:, 1::2]])
                assert ok, (name, T, over)
            ckc, cvc = ck.cpu(), cv.cpu()
            for t in range(T):
                slot = int(pos[t]) % W
                assert torch.equal(ckc[int(seq[t]), slot].reshape(-1), got[t, nq:nq + nkv]), (name, t)
                assert torch.equal(cvc[int(seq[t]), slot].reshape(-1), got[t, nq + nkv:]), (name, t)
            assert int((ckc.float().abs().amax(dim=(1, 2, 3)) > 0).sum()) == T and int((ckc.float().abs().amax(dim=(0, 2, 3)) > 0).sum()) <= T


# ------------------------------------------------------------------------------------------------ 4-7. model level
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return qu.make_folders(qu.FP8, tmp_path_factory)


@pytest.fixture(scope="module")
def oracle_runs(folders):
    return qu.make_oracle_runs(folders)


def test_quantised_model_against_the_oracle_on_the_dequantised_weights(folders, oracle_runs):
    """A 12-token prefill (dequantise + GEMM), a prefill in chunks of 5 (the GEMV without the ring epilogue), 24 decode steps at
    B = 1 and B = 3 across the ring wrap: the logits of every forward stay within the project's bf16 tolerance of the oracle on
    the dequantised weights - with power-of-two scales the quantised model IS that bf16 model up to summation order.  The bf16
    HIP path on the dequantised weights is run beside it; both distances are printed."""
    qu.check_model_against_the_oracle(qu.FP8, folders, oracle_runs)


def test_quantise_while_loading_equals_the_quantised_checkpoint(folders):
    qu.check_quantise_while_loading(qu.FP8, folders)


def test_generate_on_the_quantised_model(folders):
    """24 greedy steps with the session and the graph on equal step-by-step forward + argmax on the same model - the same
    kernels, so tokens and log-probabilities are bit-equal; every step ran on the launch path; prompt_logprobs runs."""
    def last_logits(model, prompt, cache, lps):
        ids = torch.tensor(prompt, device="cuda")
        tgt = torch.tensor(prompt[1:] + [-1], dtype=torch.int32, device="cuda")
        lp_rows, last = model.prompt_logprobs(ids, [len(prompt)], cache, tgt)
        full = torch.log_softmax(model.forward(ids, [len(prompt)], _cache(1)), dim=-1)
        want = full[torch.arange(len(prompt) - 1), torch.tensor(prompt[1:])]
        assert float((lp_rows[:-1] - want).abs().max()) <= 1e-3
        assert lps[0][:len(prompt) - 1] == lp_rows[:-1].tolist()
        return last
    qu.check_generate(folders, last_logits)


@pytest.mark.parametrize("T", [4, 12])
def test_module_level_block_on_fp8_linears_against_the_runner(folders, tmp_path, T):
    """TransformerBlock.forward on Fp8Linear layers (module by module: mi_linear_w8 / mi_qkv_rope_kvwrite_w8 leaves) against the
    same layer inside mi_forward_w8.  12 rows: both sides take the RMSNorm kernel, the dequantisation and the MFMA GEMM, so the
    comparison is bit for bit, as tests/test_gpu_lora.py compares its block.  4 rows: the runner's GEMV fuses the RMSNorm and sums
    its squares in another order (the note of that test), which can move a normalised element by one bf16 ulp; the residual
    stream then differs by rounding: at most 2 bf16 ulps at the block output's largest magnitude."""
    qu.check_module_level_block(folders, tmp_path, T)
