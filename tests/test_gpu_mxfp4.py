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
from hip_util import write_checkpoint
from mxfp4_cases import EXACT_SHAPES, UNIT, dequant_f64, exact_case, exact_reference, exact_sum_of_magnitudes_units
from test_gpu_fp8 import LOGIT_ATOL, MODEL, N_DECODE, PROMPTS, _cache, _replay, _schedule, bf, deltas_of, inside_envelope, rnd, ulp_bf16

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
MS = [1, 3, 8]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _hip():
    from mistral_inference import _hip
    return _hip


def _quant():
    from mistral_inference import quant
    return quant


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
def _load(folder, B=3, **kw):
    from mistral_inference.transformer import Transformer
    return Transformer.from_folder(folder, max_batch_size=B, device="cuda", dtype=BF, **kw)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """bf16 checkpoint -> quantize_checkpoint(qformat="mxfp4") -> (bf16 folder, MXFP4 folder, folder of the dequantised bf16
    weights, those weights)."""
    import safetensors
    q = _quant()
    d = tmp_path_factory.mktemp("mxfp4")
    w = mo.synth_weights(MODEL, seed=21)
    src = write_checkpoint(d / "bf16", MODEL, w)
    dst = q.quantize_checkpoint(src, d / "mxfp4", qformat="mxfp4")
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys()}
    deq = {}
    for k, v in sd.items():
        if k.endswith(q.QSCALE_KEY):
            continue
        deq[k] = q.dequantize_mxfp4(v, sd[k[:-len("weight")] + q.QSCALE_KEY]) if v.dtype == torch.uint8 else v
    assert set(deq) == set(w) and sum(v.dtype == torch.uint8 for v in sd.values()) == 2 * 7 * MODEL.n_layers
    return src, str(dst), write_checkpoint(d / "deq", MODEL, deq), deq


@pytest.fixture(scope="module")
def oracle_runs(folders):
    """The bf16 oracle on the dequantised weights, once per schedule: logits of every forward and the greedy tokens that every
    model under test is then fed (teacher forcing)."""
    om = mo.OracleModel(MODEL, folders[3])
    runs = {}
    for B, chunk in ((1, None), (1, 5), (3, None)):
        oc = mo.OracleCache(MODEL.n_layers, B, 64, MODEL.n_kv_heads, MODEL.head_dim, MODEL.sliding_window, dtype=BF)
        logits, fed = [], []
        for ids, lens in _schedule(B, chunk):
            logits.append(om.forward(torch.tensor(ids), lens, oc))
        ends = torch.tensor(_schedule(B, chunk)[-1][1]).cumsum(0) - 1
        tok = logits[-1][ends].argmax(-1)
        for _ in range(N_DECODE if chunk is None else 3):
            fed.append(tok)
            logits.append(om.forward(tok, [1] * B, oc))
            tok = logits[-1].argmax(-1)
        runs[(B, chunk)] = (logits, fed)
    return runs


def test_quantised_model_against_the_oracle_on_the_dequantised_weights(folders, oracle_runs):
    """A 12-token prefill (dequantise + GEMM), a prefill in chunks of 5 (the GEMV without the ring epilogue), 24 decode steps at
    B = 1 and B = 3 across the ring wrap: the logits of every forward stay within the project's bf16 tolerance of the oracle on
    the dequantised weights - the quantised model IS that bf16 model up to summation order.  The bf16 HIP path on the dequantised
    weights is run beside it; both distances are printed."""
    _, q_dir, deq_dir, _ = folders
    fp4, plain = _load(q_dir), _load(deq_dir)
    from mistral_inference.quant import Mxfp4Linear
    assert isinstance(fp4.layers["0"].attention.wq, Mxfp4Linear) and fp4.dtype == BF
    worst = {"mxfp4": 0.0, "bf16": 0.0}
    for (B, chunk), (ref, fed) in oracle_runs.items():
        for name, model in (("mxfp4", fp4), ("bf16", plain)):
            got = _replay(model, B, chunk, fed)
            assert len(got) == len(ref)
            d = max(float((g - r).abs().max()) for g, r in zip(got, ref))
            print(f"B={B} chunk={chunk}: {name}-HIP to oracle max |dlogit| = {d:.4e} over {len(ref)} forwards")
            worst[name] = max(worst[name], d)
    print(f"mxfp4-HIP to oracle {worst['mxfp4']:.4e}; bf16-HIP on dequantised weights to oracle {worst['bf16']:.4e}")
    assert worst["mxfp4"] <= LOGIT_ATOL, worst
    st = _hip().decode_engine_status(fp4._backend._workspace)
    assert st["engine_launches"] == 0 and st["status"] == 0 and st["bad_id"] == 0, st


def test_quantise_while_loading_equals_the_quantised_checkpoint(folders):
    src, q_dir, _, deq = folders
    a, b = _load(q_dir), _load(src, quantize="mxfp4")
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert set(pa) == set(pb)
    for k in pa:
        assert pa[k].dtype == pb[k].dtype and torch.equal(pa[k], pb[k]), k
    assert sum(p.dtype == torch.uint8 for p in pa.values()) == 2 * 7 * MODEL.n_layers
    ids, lens = _schedule(3, None)[0]
    ca, cb = _cache(3), _cache(3)
    with torch.inference_mode():
        la, lb = a.forward(torch.tensor(ids, device="cuda"), lens, ca), b.forward(torch.tensor(ids, device="cuda"), lens, cb)
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
        tok = torch.tensor([5, 6, 7], device="cuda")
        assert torch.equal(a.forward(tok, [1, 1, 1], ca), b.forward(tok, [1, 1, 1], cb))
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
    from mistral_inference.generate import generate
    h = _hip()
    model = _load(folders[1], B=1)
    prompt = PROMPTS[1][0]
    toks, lps = generate([prompt], model, max_tokens=N_DECODE, temperature=0.0)
    st = h.decode_engine_status(model._backend._workspace)
    assert st["engine_launches"] == 0 and st["steps"] >= N_DECODE - 1 and st["status"] == 0, st
    assert len(toks[0]) == N_DECODE and len(lps[0]) == len(prompt) - 1 + N_DECODE
    with torch.inference_mode():
        cache = _cache(1)
        ids = torch.tensor(prompt, device="cuda")
        last = model.forward(ids, [len(prompt)], cache)[-1:]
        tok = last.argmax(-1)
        lp = torch.log_softmax(last, dim=-1).gather(1, tok[:, None])[:, 0]   # the first sample is drawn by torch in generate()
        ref_t, ref_lp = [int(tok)], [float(lp)]
        for _ in range(N_DECODE - 1):
            tok, lp = h.greedy_sample(model.forward(tok, [1], cache))
            ref_t.append(int(tok))
            ref_lp.append(float(lp))
    assert toks[0] == ref_t
    assert lps[0][len(prompt) - 1:] == ref_lp


@pytest.mark.parametrize("T", [4, 12])
def test_module_level_block_on_mxfp4_linears_against_the_runner(folders, tmp_path, T):
    """TransformerBlock.forward on Mxfp4Linear layers (module by module: mi_linear_w4 / mi_qkv_rope_kvwrite_w4 leaves) against the
    same layer inside mi_forward_w4.  12 rows: both sides take the RMSNorm kernel, the dequantisation and the MFMA GEMM: bit for
    bit.  4 rows: the runner's GEMV fuses the RMSNorm and sums its squares in another order, which can move a normalised element
    by one bf16 ulp (test_module_level_block_on_fp8_linears_against_the_runner): at most 2 bf16 ulps at the block output's largest
    magnitude."""
    import json
    import safetensors
    from safetensors.torch import save_file
    src = folders[1]
    one = tmp_path / "one"
    one.mkdir()
    p = json.load(open(src + "/params.json"))
    json.dump(dict(p, n_layers=1), open(one / "params.json", "w"))
    with safetensors.safe_open(src + "/consolidated.safetensors", framework="pt", device="cpu") as f:
        save_file({k: f.get_tensor(k) for k in f.keys() if not k.startswith("layers.1.")}, str(one / "consolidated.safetensors"))
    model = _load(str(one), B=1)
    ids = torch.tensor((PROMPTS[1][0] * 2)[:T], device="cuda")
    with torch.inference_mode():
        h, _ = model._run(ids, [T], None, want_logits=True)        # with logits requested, h stays the block stack's output
        out = model.layers["0"](model.tok_embeddings.weight[ids], model.freqs_cis[torch.arange(T, device="cuda")])
    assert not torch.equal(out, torch.zeros_like(out))
    if T > 8:
        assert torch.equal(out, h), float((out.float() - h.float()).abs().max())
    else:
        tol = 2.0 * float(ulp_bf16(h.float().abs().max().cpu()))
        assert float((out.float() - h.float()).abs().max()) <= tol, (float((out.float() - h.float()).abs().max()), tol)
