"""The weight-streaming MFMA GEMM of 9 .. 64 rows (csrc/gemm_skinny.hip) behind `_hip.linear` and `Transformer.forward`:
exact against the fp64 reference of linear_cases.py on integer inputs, and against the tile kernels (switch off: the routes of
before) on Gaussian ones."""
import math

import pytest
import torch

import linear_cases as lc
import mistral_oracle as mo
from hip_util import bf16_ulp_close, write_checkpoint

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

MS = [9, 16, 17, 48, 64]                    # group boundaries and a ragged last group
KS = [64, 192, 576, 4160]                   # fewer chunks than waves, an uneven split, a long ring
NS = [(8,), (24,), (12, 13, 12), (40, 50, 46), (300, 500, 360)]     # below one unit, ragged, segment boundaries inside a unit
EPIS = [lc.STORE, lc.RESIDUAL, lc.LOGITS]


def _cases():
    out, i = [], 0
    for M in MS:
        for K in KS:                          # (20 shapes: every N spec meets every epilogue)
            segs, epi = NS[i % 5], EPIS[(i // 5 + i % 5) % 3]
            fams = ["plain"] + (["round"] if epi != lc.STORE and M * sum(segs) >= 64 else [])
            out += [lc.Case(lc._nm(M, K, segs, epi, f), M, K, segs, epi, "skinny", fam=f) for f in fams]
            i += 1
    for M, K in ((9, 64), (17, 576), (48, 192), (64, 4160)):
        out += [lc.Case(lc._nm(M, K, (72,), lc.SWIGLU, f), M, K, (72,), lc.SWIGLU, "skinny", fam=f) for f in ("plain", "round")]
    return out


def _hip():
    from mistral_inference import _hip
    return _hip


@pytest.fixture
def skinny_on():
    h = _hip()
    prev = h.debug_set_gemm_skinny(64)        # every epilogue up to 64 rows (mode 1, the shipped route, stops the LM head at 48)
    yield h
    h.debug_set_gemm_skinny(prev)


def _guarded(M, N, dtype, fill=None):
    buf = torch.full((M + 4, N + 8), lc.SENT, dtype=dtype, device="cuda")
    view = buf[2:2 + M, :N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _exact(h, case, pad=0):
    inp = lc.inputs(case)
    x = inp.x.cuda()
    if pad:                                   # lda > K: the rows inside a wider buffer of the sentinel
        wide = torch.full((case.M, case.K + pad), lc.SENT, dtype=BF, device="cuda")
        wide[:, :case.K] = x
        x = wide[:, :case.K]
    buf, out = _guarded(case.M, case.N, case.odt)
    res = _guarded(case.M, case.N, BF, inp.res)[1] if case.epi == lc.RESIDUAL else None
    h.linear(x, [w.cuda() for w in inp.w], lc.EPI_CODE[case.epi], residual=res, out=out)
    got, want = [buf.cpu()], lc.expected(case)
    assert torch.equal(got[0], want[0]), (case, lc.describe(case, got, want))


@pytest.mark.parametrize("case", _cases(), ids=repr)
def test_exact_against_fp64(case, skinny_on):
    """Integer inputs: bit-equal to the fp64 reference, the sentinel rows and columns around the view (ldo = N + 8) untouched."""
    _exact(skinny_on, case)


def test_exact_with_padded_input_rows(skinny_on):
    _exact(skinny_on, lc.Case("m17k576n12+13+12-lda", 17, 576, (12, 13, 12), lc.STORE, "skinny"), pad=24)


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF).cuda()


@pytest.mark.parametrize("M,K,N", [(16, 4096, 1024), (64, 512, 640)])
def test_agrees_with_the_tile_kernel(M, K, N, skinny_on):
    """Gaussian inputs, switch on against switch off (the 128-tile kernel): within 1 bf16 ulp (the bound the 128- and 256-tile
    kernels are granted against each other); logits widen the stored values; ten launches bit-equal."""
    h = skinny_on
    x, w = _rnd(M, K, seed=70), (_rnd(N // 2, K, seed=71, scale=1 / math.sqrt(K)), _rnd(N // 2, K, seed=72, scale=1 / math.sqrt(K)))
    on = h.linear(x, w, h.EPI_STORE)
    logits = h.linear(x, w, h.EPI_LOGITS)
    assert logits.dtype == torch.float32 and torch.equal(logits.to(BF), on)
    for _ in range(10):
        assert torch.equal(h.linear(x, w, h.EPI_STORE), on)
    h.debug_set_gemm_skinny(0)
    ok, err = bf16_ulp_close(on, h.linear(x, w, h.EPI_STORE), ulps=1.0)
    assert ok, err


@pytest.mark.parametrize("M,K", [(65, 512), (16, 200)])
def test_shapes_it_does_not_take(M, K, skinny_on):
    h = skinny_on
    x, w = _rnd(M, K, seed=80), (_rnd(136, K, seed=81, scale=1 / math.sqrt(K)),)
    on = h.linear(x, w, h.EPI_STORE)
    h.debug_set_gemm_skinny(0)
    assert torch.equal(h.linear(x, w, h.EPI_STORE), on)


def test_model_prefill_chunk_and_decode_step(tmp_path, skinny_on):
    """16 sequences of different lengths through a 2-layer model: a prefill chunk of 24 rows and a decode step of 16 rows (RoPE
    epilogue, the ring write behind it, the LM head), switch on against switch off under test_gpu_model.py's logit bound."""
    from mistral_inference.cache import BufferCache
    from mistral_inference.transformer import Transformer
    h = skinny_on
    args = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                         sliding_window=16)
    model = Transformer.from_folder(write_checkpoint(tmp_path / "ckpt", args, mo.synth_weights(args, seed=12)), max_batch_size=16,
                                    device="cuda", dtype=BF)
    lens = [1 + (b % 2) for b in range(16)]  # 24 rows
    prompt = torch.tensor([(3 * i + 7 * b + 1) % 512 for b in range(16) for i in range(lens[b])], device="cuda")
    nxt = torch.tensor([(5 * b + 2) % 512 for b in range(16)], device="cuda")
    logits = []
    for mode in (1, 0):
        h.debug_set_gemm_skinny(mode)
        cache = BufferCache(2, 16, 32, 2, 128, 16, device="cuda", dtype=BF)
        logits.append([model.forward(prompt, lens, cache).cpu(), model.forward(nxt, [1] * 16, cache).cpu()])
    for on, off in zip(*logits):
        assert on.shape == off.shape and float((on - off).abs().max()) <= 4e-2
