"""A quantised LM head on the device (opt-in `quantize_lm_head`): the GEMV_LOGITS instantiations of gemv_w8.hip / gemv_w4.hip
through `mi_lm_head_q` on lm_head_cases' exact inputs, the sliced dequantise + GEMM route and the log-prob leaf against the bf16
kernels on the dequantised head, and the model level - mi_forward_q under forward, prompt_logprobs, generate and verify steps.

The numerics contract (include/mistral_hip.h): at M <= 8 the logit is float(bf16(acc * scale[r])) (MXFP4: float(bf16(acc))), one
rounding where the bf16 head rounds; above, the bf16 GEMM on the head's bf16 image, slice by slice, bit-equal to one launch."""
import pytest
import torch

import lm_head_cases as lc
import mistral_oracle as mo
import quant_util as qu
import verify_util as vu
from hip_util import write_checkpoint
from quant_util import BF, _cache, _hip, _quant, bf, deltas_of, inside_envelope, rnd
from test_gpu_verify_step import STEP_BOUND

pytestmark = pytest.mark.gpu

MS = [1, 3, 5, 8]                       # 5 runs on the 6-row instantiation
SENT = -0.3125                          # guard value: no logit of these inputs


def _fmt(kind):
    return _hip().W8 if lc.is_fp8(kind) else _hip().W4


# ------------------------------------------------------------------------------------------------ 1. the leaf at M <= 8
LEAF = [(kind, K, N) for kind in lc.ISSUE_KINDS for K in (288, 2080, 5120) for N in (521, 20000)] + \
       [(lc.FP8_HAND, 288, 521), (lc.FP8_HAND, 2080, 20000), (lc.MXFP4_SHIFT, 288, 521), (lc.MXFP4_SHIFT, 2080, 20000)]


@pytest.mark.parametrize("kind,K,N", LEAF)
def test_logits_leaf_is_the_fp64_chain_bit_for_bit(kind, K, N):
    """torch.equal against float(bf16(exact product)) at M = 1, 3, 5, 8: K = 288 (one chunk, partly filled), 2080 (one full MXFP4
    chunk plus one piece; two FP8 chunks plus a piece), 5120; N = 521 (an odd last row, fewer units than waves) and 20000 (every
    wave walks several units); written into a guarded buffer whose row stride is not N.  Then the same launches with the fused
    RMSNorm: the rows are no integers any more, so every logit must lie inside the envelope of bf16(y) over the fp32 summation
    error (quant_util.inside_envelope, as test_gpu_fp8.py checks its fused forms)."""
    h = _hip()
    hd = lc.Head(kind, N, K, device="cuda")          # the project's quantiser, on the device: the same bytes as on the CPU
    assert hd.round_trip
    x8 = lc.x_rows(kind, 8, K)
    y, mag = lc.exact_products(hd, x8)
    assert float(mag.max()) < 2 ** 24
    ref = y.to(BF).float()
    assert float((ref.double() != y).double().mean()) >= 0.25        # the rounding is visible in a quarter of the logits
    for M in MS:
        buf = torch.full((M + 4, N + 8), SENT, dtype=torch.float32, device="cuda")
        h.lm_head_q(_fmt(kind), x8[:M].cuda(), hd.weight, hd.scale, out=buf[2:2 + M, :N])
        want = torch.full((M + 4, N + 8), SENT, dtype=torch.float32)
        want[2:2 + M, :N] = ref[:M]
        got = buf.cpu()
        assert torch.equal(got, want), (kind, K, N, M, int((got != want).sum()), (got - want).abs().max())
    nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(K))).to(BF)
    xn = mo.rms_norm(x8, nw, 1e-5)
    yn, magn = lc.exact_products(hd, xn)
    for M in MS:
        got = h.lm_head_q(_fmt(kind), x8[:M].cuda(), hd.weight, hd.scale, norm_w=nw.cuda(), eps=1e-5).cpu()
        ok, over = inside_envelope(got, bf, [yn[:M]], [deltas_of(yn[:M], magn[:M], K)])
        assert ok, ("fused norm", kind, K, N, M, over)
        assert bool((got == got.to(BF).float()).all())               # every logit is a bf16 value, widened


# ------------------------------------------------------------------------------------------------ 2. more than 8 rows
class RandomHead:
    """A random head quantised by the project's quantiser, and its bf16 image."""

    def __init__(self, fmt, N, K, seed):
        q = _quant()
        w = rnd(N, K, seed=seed, scale=K ** -0.5).cuda()
        if fmt == "fp8":
            codes, self.scale = q.quantize_rows(w)
            self.weight, self.hip = codes.view(torch.uint8), _hip().W8
            self.deq = q.dequantize(codes, self.scale)
        else:
            self.weight, self.scale = q.quantize_blocks(w)
            self.hip = _hip().W4
            self.deq = q.dequantize_mxfp4(self.weight, self.scale)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("M,K,N", [(9, 288, 8492), (300, 288, 8492), (9, 512, 8492), (300, 512, 8492), (300, 512, 40000)])
def test_sliced_route_equals_the_bf16_kernels_on_the_dequantised_head(fmt, M, K, N):
    """M = 9 and 300 (the 128-tile and, at K = 512, the 256-tile GEMM; at N = 40000 on 256 CUs the launch on the whole image splits
    its columns between the two kernels): the logits are mi_linear(EPI_LOGITS) on the dequantised head and the log-probabilities
    mi_lm_head_logprobs on it, bit for bit - the same GEMM on the same image.  8492 vocabulary rows are two dequantisation slices,
    the second of 300 rows; 40000 are five.  K = 288 takes the unfused log-prob route, K = 512 at 300 rows the fused one, whose
    per-tile partials are reduced over the whole vocabulary."""
    h = _hip()
    assert N > h.MI_LM_HEAD_SLICE_ROWS and N % h.MI_LM_HEAD_SLICE_ROWS != 0
    hd = RandomHead(fmt, N, K, seed=N + K)
    x = rnd(M, K, seed=M + K, scale=2.0).cuda()
    want = h.linear(x, (hd.deq,), h.EPI_LOGITS)
    got = h.lm_head_q(hd.hip, x, hd.weight, hd.scale)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1.0
    assert torch.equal(got, want), (int((got != want).sum()), float((got - want).abs().max()))
    tgt = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(5)).to(torch.int32)
    tgt[0], tgt[-1] = N - 1, h.MI_LM_HEAD_SLICE_ROWS              # the last row of the last slice, the first row of the second
    lp_want = h.lm_head_logprobs(x, hd.deq, tgt.cuda())
    lp_got = h.lm_head_logprobs_q(hd.hip, x, hd.weight, hd.scale, tgt.cuda())
    assert bool(torch.isfinite(lp_want).all()) and torch.equal(lp_got, lp_want), float((lp_got - lp_want).abs().max())
    full = torch.log_softmax(want, dim=-1).gather(1, tgt.cuda().long()[:, None])[:, 0]
    assert float((lp_got - full).abs().max()) <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. model level
FORMATS = {"fp8": qu.FP8, "mxfp4": qu.MXFP4}


def make_folders(fmt, tmp_path_factory):
    """quant_util.make_folders with the head quantised too: (bf16 folder, quantised folder, folder of the dequantised bf16 weights
    - head included - and those weights), and beside them the folder that quantises the layers only."""
    import safetensors
    q = _quant()
    d = tmp_path_factory.mktemp("lm_head_" + fmt.name)
    w = mo.synth_weights(qu.MODEL, seed=21)
    src = write_checkpoint(d / "bf16", qu.MODEL, w)
    dst = q.quantize_checkpoint(src, d / fmt.name, qformat=fmt.qformat, lm_head=True)
    layers_only = q.quantize_checkpoint(src, d / (fmt.name + "_layers"), qformat=fmt.qformat)
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys()}
    deq = {}
    for k, v in sd.items():
        if k.endswith(q.QSCALE_KEY):
            continue
        sk = k[:-len("weight")] + q.QSCALE_KEY
        deq[k] = getattr(q, fmt.dequantize)(v, sd[sk]) if sk in sd else v
    n_quant = sum(k[:-len("weight")] + q.QSCALE_KEY in sd for k in sd)
    assert set(deq) == set(w) and n_quant == 7 * qu.MODEL.n_layers + 1
    assert deq["output.weight"].dtype == BF and not torch.equal(deq["output.weight"], w["output.weight"])
    return (src, str(dst), write_checkpoint(d / "deq", qu.MODEL, deq), deq), str(layers_only)


@pytest.fixture(scope="module", params=list(FORMATS), ids=list(FORMATS))
def setup(request, tmp_path_factory):
    fmt = FORMATS[request.param]
    folders, layers_only = make_folders(fmt, tmp_path_factory)
    return fmt, folders, layers_only, qu.make_oracle_runs(folders)


def test_model_against_the_oracle_on_the_dequantised_weights_head_included(setup):
    """quant_util's schedule - a 12-token prefill, chunks of 5, 24 decode steps at B = 1 and B = 3 across the ring wrap - within
    LOGIT_ATOL of the oracle on the dequantised weights, head included; the bf16 HIP path on the same weights is printed beside
    it; every step on the launch path (engine_launches == 0)."""
    fmt, folders, _, runs = setup
    model = qu._load(folders[1])
    assert isinstance(model.output, getattr(_quant(), fmt.linear)) and model.args.quantization.lm_head
    assert model.tok_embeddings.weight.dtype == BF
    qu.check_model_against_the_oracle(fmt, folders, runs)


def test_hidden_state_in_front_of_the_head_does_not_depend_on_the_flag(setup):
    """The same layers with quantize_lm_head on and off: the block stack's output is bit-equal (a 12-row prefill and a decode
    step at B = 3), the logits are not."""
    fmt, folders, layers_only, _ = setup
    on, off = qu._load(folders[1]), qu._load(layers_only)
    assert type(off.output) is torch.nn.Linear
    ids, lens = qu._schedule(3, None)[0]
    ca, cb = _cache(3), _cache(3)
    with torch.inference_mode():
        for t, ln in ((torch.tensor(ids, device="cuda"), lens), (torch.tensor([5, 6, 7], device="cuda"), [1, 1, 1])):
            (ha, la), (hb, lb) = on._run(t, ln, ca, want_logits=True), off._run(t, ln, cb, want_logits=True)
            assert torch.equal(ha, hb) and bool(torch.isfinite(la).all()) and not torch.equal(la, lb)


def test_quantise_while_loading_equals_the_written_checkpoint(setup):
    fmt, folders, layers_only, _ = setup
    a = qu._load(folders[1])
    pa = dict(a.named_parameters())
    assert sum(p.dtype == torch.uint8 for p in pa.values()) == fmt.u8_per_linear * (7 * qu.MODEL.n_layers + 1)
    ids, lens = qu._schedule(3, None)[0]
    for src, kw in ((folders[0], dict(quantize=fmt.qformat, quantize_lm_head=True)), (layers_only, dict(quantize_lm_head=True))):
        b = qu._load(src, **kw)
        pb = dict(b.named_parameters())
        assert set(pa) == set(pb)
        for k in pa:
            assert pa[k].dtype == pb[k].dtype and torch.equal(pa[k], pb[k]), k
        ca, cb = _cache(3), _cache(3)
        with torch.inference_mode():
            la, lb = a.forward(torch.tensor(ids, device="cuda"), lens, ca), b.forward(torch.tensor(ids, device="cuda"), lens, cb)
            assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
            tok = torch.tensor([5, 6, 7], device="cuda")
            assert torch.equal(a.forward(tok, [1, 1, 1], ca), b.forward(tok, [1, 1, 1], cb))


def test_generate_and_prompt_logprobs_on_a_quantised_head(setup):
    """generate() at temperature 0 (the session, the graph) equals step-by-step forward + greedy_sample on the same model bit for
    bit, every step on the launch path; prompt_logprobs (mi_lm_head_logprobs_q) is within 1e-3 of log_softmax(forward), the bound
    of test_gpu_fp8.py, and is what generate() reports for the prompt."""
    fmt, folders, _, _ = setup

    def last_logits(model, prompt, cache, lps):
        assert isinstance(model.output, getattr(_quant(), fmt.linear))
        ids = torch.tensor(prompt, device="cuda")
        tgt = torch.tensor(prompt[1:] + [-1], dtype=torch.int32, device="cuda")
        lp_rows, last = model.prompt_logprobs(ids, [len(prompt)], cache, tgt)
        logits = model.forward(ids, [len(prompt)], _cache(1))
        want = torch.log_softmax(logits, dim=-1)[torch.arange(len(prompt) - 1), torch.tensor(prompt[1:])]
        assert float((lp_rows[:-1] - want).abs().max()) <= 1e-3
        assert lps[0][:len(prompt) - 1] == lp_rows[:-1].tolist()
        assert float((last - logits[-1:]).abs().max()) <= qu.LOGIT_ATOL      # (one row: the GEMV; twelve: the GEMM on the image)
        return last
    qu.check_generate(folders, last_logits)


def test_speculative_generation_equals_the_plain_loop(tmp_path_factory, setup):
    """verify_util's confident head, quantised with the layers while loading: 48 greedy tokens across the ring wrap, then the same
    through verify steps (a corrupted oracle drafter at k = 3 and k = 7: the 4-, 6- and 8-row head launches)."""
    from mistral_inference.generate import SpeculativeArgs, generate
    fmt = setup[0]
    model = vu.load(vu.make_folder("dense", tmp_path_factory), B=1, quantize=fmt.qformat, quantize_lm_head=True)
    assert isinstance(model.output, getattr(_quant(), fmt.linear))
    prompt, n, V = vu.prompt(9, 0), 48, vu.DENSE.vocab_size
    toks, lps = generate([prompt], model, max_tokens=n, temperature=0.0)
    cache, margins = vu.new_cache(1), []
    with torch.inference_mode():
        last = model.forward(torch.tensor(prompt, device="cuda"), [len(prompt)], cache)[-1:]
        for i in range(n):
            top2 = torch.topk(last[0], 2).values
            margins.append(float(top2[0] - top2[1]))
            assert int(last.argmax(-1)) == toks[0][i], i
            last = model.forward(last.argmax(-1), [1], cache)
    print(f"{fmt.name} head: smallest top-2 margin over {n} steps = {min(margins)} (needs > {4 * STEP_BOUND})")
    assert min(margins) > 4 * STEP_BOUND, ("bad fixture: a greedy step of the plain run is too close to call", min(margins))
    corrupt = {0, 3, 4, 10, 17, 22, 23, 24, 31, 32, 33, 40, 47}
    for k in (3, 7):
        def draft(history, k=k):
            m = len(history) - len(prompt)
            return [(toks[0][i] + 1) % V if i in corrupt else toks[0][i] for i in range(m, min(m + k, n))]
        got, glp = generate([prompt], model, max_tokens=n, temperature=0.0, speculative=SpeculativeArgs(k=k, drafter=draft))
        assert got == toks, k
        assert max(abs(a - b) for a, b in zip(glp[0], lps[0])) <= STEP_BOUND
    st = _hip().decode_engine_status(model._backend._workspace)
    assert st["engine_launches"] == 0 and st["status"] == 0, st
