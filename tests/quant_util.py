"""Shared by tests/test_gpu_fp8.py and tests/test_gpu_mxfp4.py: the numeric helpers of the kernel-level tests, the two-layer
model with its schedule of forwards, and the bodies of the four model-level tests as functions of the weight format."""
import itertools
import json
from typing import NamedTuple

import torch

import mistral_oracle as mo
from hip_util import write_checkpoint

BF = torch.bfloat16
LOGIT_ATOL = 4e-2   # tests/test_gpu_model.py: the project's bf16 tolerance on logits at these dims
MODEL = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                      sliding_window=16)


class Format(NamedTuple):
    name: str            # in printed lines and temporary folders
    qformat: str         # params.json `quantization.qformat_weight`, from_folder(quantize=...)
    linear: str          # the class of mistral_inference.quant that stands for nn.Linear
    dequantize: str      # the function of mistral_inference.quant: (weight, scale) -> bf16 [out, in]
    weight_dtype: torch.dtype  # of a quantised `<linear>.weight` in the checkpoint
    u8_per_linear: int   # uint8 tensors per linear, in the checkpoint and as parameters (MXFP4: codes and scales)


FP8 = Format("fp8", "fp8_e4m3", "Fp8Linear", "dequantize", torch.float8_e4m3fn, 1)
MXFP4 = Format("mxfp4", "mxfp4", "Mxfp4Linear", "dequantize_mxfp4", torch.uint8, 2)


def _hip():
    from mistral_inference import _hip
    return _hip


def _quant():
    from mistral_inference import quant
    return quant


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |v| (0 at 0)."""
    _, ex = torch.frexp(v.abs().double())
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - 8))


def bf(v: torch.Tensor) -> torch.Tensor:
    """A bf16 rounding point, carried on in fp32."""
    return v.float().to(BF).float()


def inside_envelope(got, f, accs, deltas):
    """The epilogue restated in torch (f, on fp32 tensors) at acc - d, acc, acc + d per accumulator; the output must lie between
    the smallest and the largest of those values, widened by one bf16 ulp of the output."""
    vals = []
    for signs in itertools.product((-1.0, 0.0, 1.0), repeat=len(accs)):
        vals.append(f(*[(a + sg * d).float() for a, d, sg in zip(accs, deltas, signs)]).double())
    lo, hi = torch.stack(vals).amin(0), torch.stack(vals).amax(0)
    slack = ulp_bf16(torch.maximum(lo.abs(), hi.abs()))
    g = got.double()
    ok = (g >= lo - slack) & (g <= hi + slack)
    return bool(ok.all()), float(torch.maximum(lo - slack - g, g - hi - slack).max())


def deltas_of(ref, mag, K):
    return ulp_bf16(ref) + K * 2.0 ** -23 * mag


# ------------------------------------------------------------------------------------------------ model level
def _load(folder, B=3, **kw):
    from mistral_inference.transformer import Transformer
    return Transformer.from_folder(folder, max_batch_size=B, device="cuda", dtype=BF, **kw)


def make_folders(fmt: Format, tmp_path_factory):
    """bf16 checkpoint -> quantize_checkpoint -> (bf16 folder, quantised folder, folder of the dequantised bf16 weights, those weights)."""
    import safetensors
    q = _quant()
    d = tmp_path_factory.mktemp(fmt.name)
    w = mo.synth_weights(MODEL, seed=21)
    src = write_checkpoint(d / "bf16", MODEL, w)
    dst = q.quantize_checkpoint(src, d / fmt.name, qformat=fmt.qformat)
    with safetensors.safe_open(str(dst / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys()}
    deq = {}
    for k, v in sd.items():
        if k.endswith(q.QSCALE_KEY):
            continue
        deq[k] = getattr(q, fmt.dequantize)(v, sd[k[:-len("weight")] + q.QSCALE_KEY]) if v.dtype == fmt.weight_dtype else v
    n_quant = sum(v.dtype == fmt.weight_dtype for v in sd.values())
    assert set(deq) == set(w) and n_quant == fmt.u8_per_linear * 7 * MODEL.n_layers
    return src, str(dst), write_checkpoint(d / "deq", MODEL, deq), deq


def _cache(B, dev="cuda"):
    from mistral_inference.cache import BufferCache
    return BufferCache(MODEL.n_layers, B, 64, MODEL.n_kv_heads, MODEL.head_dim, MODEL.sliding_window, device=dev, dtype=BF)


PROMPTS = {1: [[3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]], 3: [[3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8], [7, 300, 2, 44, 8, 90, 11], [11, 12, 13, 14, 15, 16, 17, 18, 19]]}
N_DECODE = 24   # positions 12 .. 35 of the longest sequence: the 16-slot ring wraps


def _schedule(B, chunk):
    """[(flat ids, seqlens)] of the prompt forwards: the whole prompts at once, or chunks of `chunk` tokens (B = 1)."""
    ps = PROMPTS[B]
    if chunk is None:
        return [(sum(ps, []), [len(p) for p in ps])]
    assert B == 1
    return [(ps[0][s:s + chunk], [len(ps[0][s:s + chunk])]) for s in range(0, len(ps[0]), chunk)]


def make_oracle_runs(folders):
    """The bf16 oracle on the dequantised weights, once per schedule: logits of every forward and the greedy tokens that every
    model under test is then fed (teacher forcing: all three see the same inputs)."""
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


def _replay(model, B, chunk, fed):
    cache = _cache(B)
    out = []
    with torch.inference_mode():
        for ids, lens in _schedule(B, chunk):
            out.append(model.forward(torch.tensor(ids, device="cuda"), lens, cache).cpu())
        for tok in fed:
            out.append(model.forward(tok.cuda(), [1] * B, cache).cpu())
    return out


def check_model_against_the_oracle(fmt: Format, folders, oracle_runs):
    _, q_dir, deq_dir, _ = folders
    quantised, plain = _load(q_dir), _load(deq_dir)
    assert isinstance(quantised.layers["0"].attention.wq, getattr(_quant(), fmt.linear)) and quantised.dtype == BF
    worst = {fmt.name: 0.0, "bf16": 0.0}
    for (B, chunk), (ref, fed) in oracle_runs.items():
        for name, model in ((fmt.name, quantised), ("bf16", plain)):
            got = _replay(model, B, chunk, fed)
            assert len(got) == len(ref)
            d = max(float((g - r).abs().max()) for g, r in zip(got, ref))
            print(f"B={B} chunk={chunk}: {name}-HIP to oracle max |dlogit| = {d:.4e} over {len(ref)} forwards")
            worst[name] = max(worst[name], d)
    print(f"{fmt.name}-HIP to oracle {worst[fmt.name]:.4e}; bf16-HIP on dequantised weights to oracle {worst['bf16']:.4e}")
    assert worst[fmt.name] <= LOGIT_ATOL, worst
    st = _hip().decode_engine_status(quantised._backend._workspace)
    assert st["engine_launches"] == 0 and st["status"] == 0 and st["bad_id"] == 0, st


def check_quantise_while_loading(fmt: Format, folders):
    src, q_dir, _, _ = folders
    a, b = _load(q_dir), _load(src, quantize=fmt.qformat)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert set(pa) == set(pb)
    for k in pa:
        assert pa[k].dtype == pb[k].dtype and torch.equal(pa[k], pb[k]), k
    assert sum(p.dtype == torch.uint8 for p in pa.values()) == fmt.u8_per_linear * 7 * MODEL.n_layers
    ids, lens = _schedule(3, None)[0]
    ca, cb = _cache(3), _cache(3)
    with torch.inference_mode():
        la, lb = a.forward(torch.tensor(ids, device="cuda"), lens, ca), b.forward(torch.tensor(ids, device="cuda"), lens, cb)
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
        tok = torch.tensor([5, 6, 7], device="cuda")
        assert torch.equal(a.forward(tok, [1, 1, 1], ca), b.forward(tok, [1, 1, 1], cb))


def last_prompt_logits(model, prompt, cache, lps):
    """Logits [1, V] of the prompt's last token, the prompt written into `cache`: by the forward."""
    return model.forward(torch.tensor(prompt, device="cuda"), [len(prompt)], cache)[-1:]


def check_generate(folders, last_logits=last_prompt_logits):
    """last_logits(model, prompt, cache, lps): see last_prompt_logits; lps are generate()'s log-probabilities, for a format's own
    checks of the prompt's."""
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
        last = last_logits(model, prompt, cache, lps)
        tok = last.argmax(-1)
        lp = torch.log_softmax(last, dim=-1).gather(1, tok[:, None])[:, 0]   # the first sample is drawn by torch in generate()
        ref_t, ref_lp = [int(tok)], [float(lp)]
        for _ in range(N_DECODE - 1):
            tok, lp = h.greedy_sample(model.forward(tok, [1], cache))
            ref_t.append(int(tok))
            ref_lp.append(float(lp))
    assert toks[0] == ref_t
    assert lps[0][len(prompt) - 1:] == ref_lp


def check_module_level_block(folders, tmp_path, T):
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
