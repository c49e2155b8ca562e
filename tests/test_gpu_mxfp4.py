"""Weight-only MXFP4 (OCP e2m1 codes in blocks of 32, e8m0 block scales) on the device: the MXFP4 GEMV family and the dequantise +
GEMM route (csrc/gemv_w4.hip) through the new leaves, the layer-stack runner on a quantised model, the loader paths, generate() and
the module-level block.

The numerics contract (quant.py, include/mistral_hip.h): every weight 2^(b - 127) * e2m1(code) is exact in bf16, so at any number of
rows a quantised linear is the bf16 linear on the dequantised weights up to the order of the fp32 summation.  Nothing here is a
tolerance to the unquantised model."""

import pytest
import torch
import torch.nn.functional as F

import mistral_oracle as mo
import quant_util as qu
from mxfp4_cases import EXACT_SHAPES, UNIT, dequant_f64, exact_case, exact_reference, exact_sum_of_magnitudes_units
from quant_util import BF, MODEL, _hip, _quant, bf, deltas_of, inside_envelope, rnd

pytestmark = pytest.mark.gpu

MS = [1, 3, 8]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


class QW:
    """A random weight matrix quantised by the project's quantiser: code bytes, block scales, its exact bf16 dequantisation."""

    def __init__(self, n, k, seed):
        self.packed, self.scale = _quant().quantize_blocks(rnd(n, k, seed=seed, scale=k ** -0.5))
        self.vals = dequant_f64(self.packed, self.scale)
        self.deq = _quant().dequantize_mxfp4(self.packed, self.scale)
        assert torch.equal(self.deq.double(), self.vals)
        self.pd, self.sd, self.deqd = self.packed.cuda(), self.scale.cuda(), self.deq.cuda()

    def sums(self, x):
        """fp64: sum_k w x and sum_k |w x|, [M, n]."""
        xd = x.double()
        return xd @ self.vals.T, xd.abs() @ self.vals.abs().T


# ------------------------------------------------------------------------------------------------ 1. every code, both nibbles
def test_every_e2m1_code_in_both_nibbles_and_the_scale_byte():
    """K = 32, the smallest the kernels take.  W is 32 x 32 with code (r + c) % 16 at row r, column c: every code at even and at odd
    k, i.e. in both nibbles; scale bytes cycle 127, 124, 130 by row; one-hot bf16 inputs.  Every output is ONE exact product and
    equals +-e2m1 * 2^(b - 127) bit for bit as values (the kernels' +0 start makes the product with the code 8 a +0).  A swapped
    nibble, a wrong code table or a scale read as a full float cannot pass."""
    h = _hip()
    r, c = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    codes = ((r + c) % 16).to(torch.uint8)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    scale = torch.tensor([127, 124, 130] * 11, dtype=torch.uint8)[:32].reshape(32, 1).contiguous()
    tab = torch.tensor(E2M1 + [-v for v in E2M1])
    w = tab[codes.long()] * torch.tensor([1.0, 0.125, 8.0] * 11)[:32, None]
    assert torch.equal(_quant().dequantize_mxfp4(packed, scale).float(), w)
    ref = w.T.contiguous()                         # ref[c, r]: the row of the one-hot input e_c
    eye = torch.eye(32, dtype=BF).cuda()
    pd, sd = packed.cuda(), scale.cuda()
    for s in range(0, 32, 8):                      # M = 8: the MXFP4 GEMV
        got = h.linear_w4(eye[s:s + 8].contiguous(), [pd], [sd]).float().cpu()
        assert torch.equal(got, ref[s:s + 8]), (s, (got - ref[s:s + 8]).abs().max())
    one = h.linear_w4(eye[5:6].contiguous(), [pd], [sd]).float().cpu()      # one token: the one-token instantiations
    assert torch.equal(one, ref[5:6])
    got = h.linear_w4(eye, [pd], [sd]).float().cpu()                         # M = 32: dequantise + MFMA GEMM
    assert torch.equal(got, ref), (got - ref).abs().max()


# ------------------------------------------------------------------------------------------------ 2. the exact family
@pytest.fixture(scope="module")
def exact_cases():
    """Per (K, N): codes, scales, 16 integer input rows, residual rows in multiples of 8, the fp64 result - made once, never changed."""
    out = {}
    for K, N in EXACT_SHAPES:
        packed, scale, x = exact_case(K, N, M=16)
        g = torch.Generator().manual_seed(K + N)
        res = (8 * torch.randint(-4, 5, (16, N), generator=g)).to(BF)
        units = exact_sum_of_magnitudes_units(packed, scale, x)
        out[(K, N)] = (packed, scale, x, res, exact_reference(packed, scale, x), units)
    return out


@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("K,N", EXACT_SHAPES)
def test_exact_family_against_the_fp64_chain(exact_cases, K, N, M):
    """Every term is a multiple of 2^-4 and sum |term| < 2^24 such units: y is the same fp32 in any summation order, so the
    outputs are compared with torch.equal.  STORE: bf16(y).  RESIDUAL: bf16(res + bf16(y)).  Both also equal mi_linear on the
    dequantised bf16 weights bit for bit.  M = 16 takes the dequantise + GEMM route."""
    h, q = _hip(), _quant()
    packed, scale, x16, res16, y16, units = exact_cases[(K, N)]
    print(f"K={K} N={N}: max sum|term| = {units:.3e} units of 2^-4")
    assert units < 2 ** 24
    x, res, y = x16[:M].contiguous(), res16[:M].contiguous(), y16[:M]
    assert torch.equal(y.float().double(), y) and bool((y / UNIT == (y / UNIT).round()).all())
    pd, sd = packed.cuda(), scale.cuda()
    deq = q.dequantize_mxfp4(packed, scale).cuda()
    want = y.float().to(BF)
    got = h.linear_w4(x.cuda(), [pd], [sd])
    assert torch.equal(got.cpu(), want), float((got.cpu().float() - want.float()).abs().max())
    assert torch.equal(got, h.linear(x.cuda(), (deq,)))
    want_r = (res.float() + want.float()).to(BF)
    got_r = h.linear_w4(x.cuda(), [pd], [sd], h.EPI_RESIDUAL, residual=res.cuda())
    assert torch.equal(got_r.cpu(), want_r), float((got_r.cpu().float() - want_r.float()).abs().max())
    assert torch.equal(got_r, h.linear(x.cuda(), (deq,), h.EPI_RESIDUAL, residual=res.cuda()))
    if M <= 8:  # with the fused RMSNorm the normalised rows are not integers: the bound of test 3
        nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(K))).to(BF)
        xn = mo.rms_norm(x, nw, 1e-5).double()
        vals = dequant_f64(packed, scale)
        ref, mag = xn @ vals.T, xn.abs() @ vals.abs().T
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
        got_n = h.linear_w4(x.cuda(), [pd], [sd], norm_w=nw.cuda(), eps=1e-5).double().cpu()
        assert bool(((got_n - ref).abs() <= bound).all()), float(((got_n - ref).abs() / bound.clamp_min(1e-30)).max())


# ------------------------------------------------------------------------------------------------ 3. the fused epilogues
@pytest.fixture(scope="module")
def gauss_cases():
    out = {}
    for i, (K, N) in enumerate(EXACT_SHAPES):
        out[(K, N)] = (QW(N, K, seed=20 + i), QW(N, K, seed=60 + i), rnd(8, K, seed=30 + i, scale=2.0), rnd(8, N, seed=78 + i),
                       (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(40 + i))).to(BF))
    return out


@pytest.mark.parametrize("K,N", EXACT_SHAPES)
def test_fused_epilogues_on_gaussian_inputs(gauss_cases, K, N):
    """Output between the epilogue restated in torch at acc +- (ulp_bf16(ref) + K 2^-23 sum|w x|), widened by one bf16 ulp (the
    envelope of tests/test_gpu_fp8.py); the bf16 kernel on the dequantised weights must pass the same envelope.  RESIDUAL; SWIGLU
    with the fused norm; STORE with the fused norm against 2^-8 |ref| + K 2^-23 sum|w x|."""
    h = _hip()
    w1, w3, x8, res8, nw = gauss_cases[(K, N)]
    kw = dict(norm_w=nw.cuda(), eps=1e-5)
    for M in MS:
        x, res = x8[:M].contiguous(), res8[:M].contiguous()
        ref, mag = w1.sums(x)
        f = lambda y: bf(res.float() + bf(y))  # noqa: E731
        for name, got in (("w4", h.linear_w4(x.cuda(), [w1.pd], [w1.sd], h.EPI_RESIDUAL, residual=res.cuda())),
                          ("bf16 on dequantised", h.linear(x.cuda(), (w1.deqd,), h.EPI_RESIDUAL, residual=res.cuda()))):
            ok, over = inside_envelope(got.cpu(), f, [ref], [deltas_of(ref, mag, K)])
            assert ok, ("residual", name, M, over)
        xn = mo.rms_norm(x, nw, 1e-5)
        (r1, m1), (r3, m3) = w1.sums(xn), w3.sums(xn)
        g = lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3))  # noqa: E731
        for name, got in (("w4", h.linear_w4(x.cuda(), [w1.pd, w3.pd], [w1.sd, w3.sd], h.EPI_SWIGLU, **kw)),
                          ("bf16 on dequantised", h.linear(x.cuda(), (w1.deqd, w3.deqd), h.EPI_SWIGLU, **kw))):
            assert tuple(got.shape) == (M, N)
            ok, over = inside_envelope(got.cpu(), g, [r1, r3], [deltas_of(r1, m1, K), deltas_of(r3, m3, K)])
            assert ok, ("swiglu", name, M, over)
        bound = 2.0 ** -8 * r1.abs() + K * 2.0 ** -23 * m1
        for name, got in (("w4", h.linear_w4(x.cuda(), [w1.pd], [w1.sd], **kw)), ("bf16 on dequantised", h.linear(x.cuda(), (w1.deqd,), **kw))):
            err = (got.double().cpu() - r1).abs()
            assert bool((err <= bound).all()), ("store + norm", name, M, float((err / bound.clamp_min(1e-30)).max()))


# ------------------------------------------------------------------------------------------------ 4. every unit size
def _unit_threshold():
    """(cus, the smallest row-pair count at which the launcher takes two row pairs per unit at one token) - asked of the launcher's
    own rule, so that a change of the rule moves these tests with it."""
    h = _hip()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rule = lambda n: int(h.lib().mi_debug_gemv_w4_row_pairs(n, cus))  # noqa: E731
    assert rule(1) == 1
    first = next(n for n in range(1, 128 * cus + 1) if rule(n) == 2)
    assert {rule(n) for n in (1, first - 1, first, 4 * first, 1 << 20)} == {1, 2}, "the unit sizes the launcher picks: 1 and 2 row pairs"
    return cus, first


def test_every_unit_size_the_launcher_picks_at_one_token():
    """One token: units of one row pair below the launcher's threshold, of two from there on, in every mode.  The smallest matrices
    that reach the larger unit on this device, with an odd pair count so that the last unit is part empty, and their neighbours just
    below the threshold: STORE and RESIDUAL are exact on the integer family (the residual pair of the unit's second row pair, the
    clamp of a missing second pair, an odd last row), SWIGLU inside its envelope."""
    h = _hip()
    _, first = _unit_threshold()
    K = 64
    for npairs in (first + 3 - first % 2, first - 1):   # an odd pair count at or above the threshold; one below it
        assert npairs % 2 == 1 or npairs < first
        N = 2 * npairs                     # STORE / RESIDUAL: output rows (2 q, 2 q + 1)
        packed, scale, x = exact_case(K, N, M=1, seed=npairs)
        res = (8 * torch.randint(-4, 5, (1, N), generator=torch.Generator().manual_seed(npairs))).to(BF)
        want = exact_reference(packed, scale, x).float().to(BF)
        want_r = (res.float() + want.float()).to(BF)
        assert exact_sum_of_magnitudes_units(packed, scale, x) < 2 ** 24
        for n in (N, N - 1):               # N - 1: an odd last row inside the last pair
            pd, sd = packed[:n].contiguous().cuda(), scale[:n].contiguous().cuda()
            got = h.linear_w4(x.cuda(), [pd], [sd]).cpu()
            assert torch.equal(got, want[:, :n]), ("store", npairs, n, float((got.float() - want[:, :n].float()).abs().max()))
            got = h.linear_w4(x.cuda(), [pd], [sd], h.EPI_RESIDUAL, residual=res[:, :n].contiguous().cuda()).cpu()
            assert torch.equal(got, want_r[:, :n]), ("residual", npairs, n, float((got.float() - want_r[:, :n].float()).abs().max()))
        # three segments with an odd pair count in the first: a four-row unit straddles the segment boundary
        n0 = 2 * ((npairs // 3) | 1)
        n1 = n0 + 2 * (npairs // 3)
        ws = [packed[:n0], packed[n0:n1], packed[n1:]]
        ss = [scale[:n0], scale[n0:n1], scale[n1:]]
        assert (n0 // 2) % 2 == 1 and all(w.shape[0] > 0 for w in ws)
        got = h.linear_w4(x.cuda(), [w.contiguous().cuda() for w in ws], [s.contiguous().cuda() for s in ss], h.EPI_RESIDUAL,
                          residual=res.cuda()).cpu()
        assert torch.equal(got, want_r), ("residual, three segments", npairs)
        w1, w3 = QW(npairs, K, seed=92), QW(npairs, K, seed=93)        # SWIGLU: a pair is (W1 row q, W3 row q)
        xg = rnd(1, K, seed=90, scale=2.0)
        (r1, m1), (r3, m3) = w1.sums(xg), w3.sums(xg)
        got = h.linear_w4(xg.cuda(), [w1.pd, w3.pd], [w1.sd, w3.sd], h.EPI_SWIGLU).cpu()
        ok, over = inside_envelope(got, lambda y1, y3: bf(bf(F.silu(bf(y1))) * bf(y3)), [r1, r3],
                                   [deltas_of(r1, m1, K), deltas_of(r3, m3, K)])
        assert ok, (npairs, over)


# ------------------------------------------------------------------------------------------------ 5. q|k|v + RoPE + ring
def _qkv_rope_ring_case(D, H, Hkv, Ts, head_major):
    """q|k|v + RoPE + ring write on MXFP4 weights: every output inside the envelope of `bf16(rope(bf16(y0), bf16(y1)))`; the ring
    rows are the k | v columns of the same call's output bit for bit, at positions past the ring's length (slot = pos % W wraps)
    and with tok_seq a permutation.  The bf16 kernel on the dequantised weights goes through the same checks."""
    h = _hip()
    Dh, W = 128, 24
    nq, nkv = H * Dh, Hkv * Dh
    wq, wk, wv = QW(nq, D, seed=50), QW(nkv, D, seed=51), QW(nkv, D, seed=52)
    nw = (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(53))).to(BF)
    cs = mo.rope_angles(Dh, 4000, 1e6)
    x8 = rnd(8, D, seed=54, scale=2.0)
    for T in Ts:
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
        for name in ("w4", "bf16 on dequantised"):
            ck, cv = mk(), mk()
            if name == "w4":
                got = h.qkv_rope_kvwrite_w4(x.cuda(), wq.pd, wk.pd, wv.pd, wq.sd, wk.sd, wv.sd, Dh, cs.cuda(), pos.cuda(), norm_w=nw.cuda(),
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


@pytest.mark.parametrize("head_major", [False, True], ids=["slot_major", "head_major"])
@pytest.mark.parametrize("D", [512, 1056, 4096])
def test_qkv_rope_kvwrite_w4_envelope_and_ring(D, head_major):
    """T = 1, 3, 8 at 2 + 1 heads (two-row units at one token on any device), both ring layouts."""
    _qkv_rope_ring_case(D, 2, 1, MS, head_major)


@pytest.mark.parametrize("head_major", [False, True], ids=["slot_major", "head_major"])
def test_qkv_rope_kvwrite_w4_in_four_row_units(head_major):
    """One token and enough heads that the launcher takes two row pairs per unit (the q|k|v launch of every decode step at the 7B
    dims): the RoPE entry of each of the unit's pairs, the ring write from a four-row unit, q / k / v segment ends inside the
    grid.  The smallest head count above the launcher's threshold on this device, at D = 64; with a GQA ratio of 6 when it fits."""
    h = _hip()
    cus, first = _unit_threshold()
    heads = -(-first // 64)                 # a head is 64 row pairs; q + k + v heads needed
    Hkv = max(1, heads // 8)
    H = max(heads - 2 * Hkv, Hkv)
    H += (-H) % Hkv
    assert (H + 2 * Hkv) * 64 >= first and int(h.lib().mi_debug_gemv_w4_row_pairs((H + 2 * Hkv) * 64, cus)) == 2
    _qkv_rope_ring_case(64, H, Hkv, [1], head_major)


# ------------------------------------------------------------------------------------------------ 6-9. model level
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return qu.make_folders(qu.MXFP4, tmp_path_factory)


@pytest.fixture(scope="module")
def oracle_runs(folders):
    return qu.make_oracle_runs(folders)


def test_quantised_model_against_the_oracle_on_the_dequantised_weights(folders, oracle_runs):
    """A 12-token prefill (dequantise + GEMM), a prefill in chunks of 5 (the GEMV without the ring epilogue), 24 decode steps at
    B = 1 and B = 3 across the ring wrap: the logits of every forward stay within the project's bf16 tolerance of the oracle on
    the dequantised weights - the quantised model IS that bf16 model up to summation order.  The bf16 HIP path on the dequantised
    weights is run beside it; both distances are printed."""
    qu.check_model_against_the_oracle(qu.MXFP4, folders, oracle_runs)


def test_quantise_while_loading_equals_the_quantised_checkpoint(folders):
    qu.check_quantise_while_loading(qu.MXFP4, folders)
    # the quantiser on the device gives the CPU's bytes
    w = mo.synth_weights(MODEL, seed=21)["layers.1.feed_forward.w2.weight"]
    pc, sc = _quant().quantize_blocks(w)
    pg, sg = _quant().quantize_blocks(w.cuda())
    assert torch.equal(pg.cpu(), pc) and torch.equal(sg.cpu(), sc)
    ties = torch.tensor([[6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0] * 4, [3e38, -1e-30, 0.0, 1.0] * 8])
    for t in (ties, ties.to(BF)):
        (pc, sc), (pg, sg) = _quant().quantize_blocks(t), _quant().quantize_blocks(t.cuda())
        assert torch.equal(pg.cpu(), pc) and torch.equal(sg.cpu(), sc)


def test_generate_on_the_quantised_model(folders):
    """24 greedy steps with the session and the graph on equal step-by-step forward + argmax on the same model - the same
    kernels, so tokens and log-probabilities are bit-equal; every step ran on the launch path."""
    qu.check_generate(folders)


@pytest.mark.parametrize("T", [4, 12])
def test_module_level_block_on_mxfp4_linears_against_the_runner(folders, tmp_path, T):
    """TransformerBlock.forward on Mxfp4Linear layers (module by module: mi_linear_w4 / mi_qkv_rope_kvwrite_w4 leaves) against the
    same layer inside mi_forward_w4.  12 rows: both sides take the RMSNorm kernel, the dequantisation and the MFMA GEMM: bit for
    bit.  4 rows: the runner's GEMV fuses the RMSNorm and sums its squares in another order, which can move a normalised element
    by one bf16 ulp (test_module_level_block_on_fp8_linears_against_the_runner): at most 2 bf16 ulps at the block output's largest
    magnitude."""
    qu.check_module_level_block(folders, tmp_path, T)
