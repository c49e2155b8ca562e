"""The weight-streaming MFMA GEMM of 9 .. 64 rows on quantised weight rows (csrc/gemm_skinny_q.hip) behind `_hip.linear_w8`,
`_hip.linear_w4` and `Transformer.forward`.  Integer-valued codes and activations: every partial sum is an integer (a multiple of
2^-4 at MXFP4) below 2^24 units, so any summation order is exact and the outputs are compared bit for bit."""
import pytest
import torch

import quant_util as qu
from linear_cases import SENT
from mxfp4_cases import dequant_f64, exact_case, exact_sum_of_magnitudes_units

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

MS = [9, 16, 17, 64]                                     # group boundaries and a ragged last group
KS = {"w8": [128, 640, 8320], "w4": [256, 1280, 16640]}  # one chunk (fewer than waves), 5 chunks (uneven split), 65 (the ring wraps)
NS = [(8,), (12, 13, 12), (40, 50, 46)]                  # below one unit, segment boundaries inside a unit, ragged multi-unit
CASES = [(M, ki, NS[(mi + ki) % 3]) for mi, M in enumerate(MS) for ki in range(3)]


def _hip():
    from mistral_inference import _hip
    return _hip


@pytest.fixture
def skinny_on():
    h = _hip()
    prev = h.debug_set_gemm_skinny(64)        # every format up to 64 rows, whatever bound the route ships with
    yield h
    h.debug_set_gemm_skinny(prev)


def _threshold_cases():
    """One N on each side of the launcher's switch to two units per block (ceil(N / 32) >= CUs), the last pair part empty."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [(17, 0, (32 * cus - 24,)), (17, 0, (32 * cus - 40,))]


def _w8(K, segs, seed, pow2=False):
    """(e4m3 bytes per segment, fp32 scales per segment, fp64 values [N, K]): integer codes in -4 .. 4, scales k / 3 (or 2^-k)."""
    g = torch.Generator().manual_seed(seed)
    N = sum(segs)
    vals = torch.randint(-4, 5, (N, K), generator=g).float()
    r = torch.arange(N)
    scale = (0.5 ** (r % 4).float()) if pow2 else ((1 + r % 7).float() / 3.0)
    ws = [w.contiguous().cuda() for w in vals.to(torch.float8_e4m3fn).split(segs)]
    return ws, [s.contiguous().cuda() for s in scale.split(segs)], vals.double(), scale


def _w4(K, segs, seed):
    packed, scale, _ = exact_case(K, sum(segs), 1, seed=seed)   # scale bytes vary along a row and between rows
    return ([w.contiguous().cuda() for w in packed.split(segs)], [s.contiguous().cuda() for s in scale.split(segs)],
            dequant_f64(packed, scale), packed, scale)


def _x(M, K, seed):
    return torch.randint(-2, 3, (M, K), generator=torch.Generator().manual_seed(seed)).to(BF)


def _run(fn, x, ws, ss, epi, M, N, res=None):
    """The call on a guarded output view (ldo = N + 8; the residual in a view of the same stride); returns the whole buffer."""
    buf = torch.full((M + 4, N + 8), SENT, dtype=BF, device="cuda")
    rv = None
    if res is not None:
        rv = torch.full((M + 4, N + 8), SENT, dtype=BF, device="cuda")[2:2 + M, :N]
        rv.copy_(res)
    fn(x.cuda(), ws, ss, epi, residual=rv, out=buf[2:2 + M, :N])
    return buf.cpu()


def _check(h, fn, x, ws, ss, y, M, N):
    """y: the bf16 STORE result.  STORE and RESIDUAL bit-equal, the sentinels untouched."""
    res = (8 * torch.randint(-4, 5, (M, N), generator=torch.Generator().manual_seed(N))).to(BF)
    for epi, want in ((h.EPI_STORE, y), (h.EPI_RESIDUAL, (res.float() + y.float()).to(BF))):
        exp = torch.full((M + 4, N + 8), SENT, dtype=BF)
        exp[2:2 + M, :N] = want
        got = _run(fn, x, ws, ss, epi, M, N, res if epi == h.EPI_RESIDUAL else None)
        assert torch.equal(got, exp), (epi, float((got.float() - exp.float()).abs().max()))


@pytest.mark.parametrize("M,ki,segs", CASES + [pytest.param(None, 0, None, id="two-unit-threshold")])
def test_fp8_exact_with_arbitrary_scales(M, ki, segs, skinny_on):
    """y = bf16(scale_f32 * S) with S the exact integer sum: one fp32 multiply behind the accumulation, the rule of the e4m3 GEMV.
    The dequantise-first route rounds bf16(scale * w) per weight and cannot produce these values (scales k / 3)."""
    for M, ki, segs in (_threshold_cases() if M is None else [(M, ki, segs)]):
        K, N = KS["w8"][ki], sum(segs)
        ws, ss, vals, scale = _w8(K, segs, seed=M + K)
        x = _x(M, K, seed=K)
        S = x.double() @ vals.T
        assert float((x.double().abs() @ vals.abs().T).max()) < 2 ** 24
        _check(skinny_on, skinny_on.linear_w8, x, ws, ss, (S.float() * scale[None, :]).to(BF), M, N)


@pytest.mark.parametrize("M,ki,segs", CASES + [pytest.param(None, 0, None, id="two-unit-threshold")])
def test_mxfp4_exact(M, ki, segs, skinny_on):
    """The fp64 product on the dequantised values, rounded once."""
    for M, ki, segs in (_threshold_cases() if M is None else [(M, ki, segs)]):
        K, N = KS["w4"][ki], sum(segs)
        ws, ss, vals, packed, scale = _w4(K, segs, seed=M + K)
        x = _x(M, K, seed=K)
        assert exact_sum_of_magnitudes_units(packed, scale, x) < 2 ** 24
        _check(skinny_on, skinny_on.linear_w4, x, ws, ss, (x.double() @ vals.T).float().to(BF), M, N)


@pytest.mark.parametrize("fmt,M,K,epi", [("w8", 17, 640, "swiglu"), ("w8", 64, 128, "swiglu"), ("w4", 17, 1280, "swiglu"),
                                         ("w4", 64, 256, "swiglu"), ("w8", 17, 192, "store"), ("w4", 17, 288, "store")])
def test_switch_on_equals_switch_off(fmt, M, K, epi, skinny_on):
    """SWIGLU on integer inputs (power-of-two FP8 scales: the image of the dequantisation route is exact): the same accumulators
    and the same epilogue arithmetic, so bit-equal; and a K the kernel declines (192, 288) is the route of before."""
    h = skinny_on
    fn = h.linear_w8 if fmt == "w8" else h.linear_w4
    nseg = 2 if epi == "swiglu" else 1
    ws, ss = (_w8(K, (72,) * nseg, seed=K, pow2=True) if fmt == "w8" else _w4(K, (72,) * nseg, seed=K))[:2]
    code = h.EPI_SWIGLU if epi == "swiglu" else h.EPI_STORE
    on = _run(fn, _x(M, K, seed=M), ws, ss, code, M, 72)
    h.debug_set_gemm_skinny(0)
    assert torch.equal(on, _run(fn, _x(M, K, seed=M), ws, ss, code, M, 72))
    assert bool((on[2:2 + M, :72] != SENT).any()) and bool((on[:2] == SENT).all()) and bool((on[:, 72:] == SENT).all())


@pytest.mark.parametrize("fmt", [qu.FP8, qu.MXFP4], ids=lambda f: f.name)
def test_model_prefill_chunk_and_decode_step(fmt, tmp_path_factory, skinny_on):
    """16 sequences through the 2-layer quantised model: a prefill chunk of 24 rows and a decode step of 16 rows (RoPE epilogue, the
    ring write behind it, residual, SwiGLU), switch on against switch off under test_gpu_gemm_skinny.py's logit bound."""
    h = skinny_on
    model = qu._load(qu.make_folders(fmt, tmp_path_factory)[1], B=16)
    lens = [1 + (b % 2) for b in range(16)]  # 24 rows
    prompt = torch.tensor([(3 * i + 7 * b + 1) % 512 for b in range(16) for i in range(lens[b])], device="cuda")
    nxt = torch.tensor([(5 * b + 2) % 512 for b in range(16)], device="cuda")
    logits = []
    for mode in (1, 0):
        h.debug_set_gemm_skinny(mode)
        cache = qu._cache(16)
        logits.append([model.forward(prompt, lens, cache).cpu(), model.forward(nxt, [1] * 16, cache).cpu()])
    for on, off in zip(*logits):
        assert on.shape == off.shape and bool(torch.isfinite(on).all()) and float((on - off).abs().max()) <= 4e-2
