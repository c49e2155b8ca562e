#!/usr/bin/env python3
"""What FP8 prefill GEMMs (W8A8, `prefill_fp8`) buy at the Mistral-7B dims, one process on one box:

    python scripts/w8a8_probe.py [--layers 32] [--reps 5]

Times (HIP events on the launch stream; warm-up first, same discipline as bench.py and scripts/fp8_probe.py):
  (a) a prefill of 4096 and of 2048 tokens on three routes - the bf16 model, the FP8 model on the weight-only route (one
      dequantisation pass per linear group in front of the bf16 GEMM) and the same FP8 model with `prefill_fp8` - each measured
      twice, interleaved (bf16, fp8, w8a8, bf16, fp8, w8a8), so that a drifting clock or power state shows as a spread;
  (b) per linear group of a layer (q|k|v, wo, w1|w3, w2) at 4096 rows: the W8A8 leaf (quantiser + GEMM), the quantiser alone, their
      difference as the GEMM alone, and the bf16 GEMM route (gemm256) on the same shape, in microseconds and TF/s;
  (c) the four quantiser passes of a layer (two with the RMSNorm fused), their sum and the GB/s each stands for.
Weights are random (timing only).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from fp8_probe import DEV, DIMS, build, event_ms  # noqa: E402
from mistral_inference import _hip  # noqa: E402
from mistral_inference.cache import BufferCache  # noqa: E402
from mistral_inference.quant import quantize_rows  # noqa: E402


def prefill_runner(model, T: int):
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, T, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    ids = torch.randint(0, a.vocab_size, (T,), generator=torch.Generator().manual_seed(0)).to(DEV)

    def run():
        cache.reset()
        model.forward_partial(ids, [T], cache)
    return run


def leaf_us(fn, reps: int, inner: int = 10) -> float:
    def many():
        for _ in range(inner):
            fn()
    many()
    torch.cuda.synchronize()
    return event_ms(many, reps) * 1000.0 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    o = ap.parse_args()
    out = {"layers": o.layers, "reps": o.reps}
    D, F = DIMS["dim"], DIMS["hidden_dim"]
    nq, nkv = DIMS["n_heads"] * DIMS["head_dim"], DIMS["n_kv_heads"] * DIMS["head_dim"]
    with torch.inference_mode():
        plain, fp8 = build(o.layers, False), build(o.layers, True)
        for T in (4096, 2048):
            runs = {"bf16": (plain, False), "fp8": (fp8, False), "w8a8": (fp8, True)}
            ms = {k: [] for k in runs}
            for _ in range(2):
                for name, (model, flag) in runs.items():
                    if model is fp8:
                        model.prefill_fp8 = flag
                    run = prefill_runner(model, T)
                    run()
                    torch.cuda.synchronize()
                    ms[name].append(event_ms(run, o.reps))
            for name, v in ms.items():
                out[f"{name}_prefill{T}_ms"] = [round(x, 2) for x in v]
                out[f"{name}_prefill{T}_tok_s"] = round(T / min(v) * 1e3)
        fp8.prefill_fp8 = False
        del plain, fp8
        torch.cuda.empty_cache()

        # ---- the leaves at 4096 rows: (name, K, segment rows, epilogue, fused norm)
        M = 4096
        g = torch.Generator(device=DEV).manual_seed(2)
        groups = [("qkv", D, (nq, nkv, nkv), _hip.EPI_STORE, True), ("wo", nq, (D,), _hip.EPI_RESIDUAL, False),
                  ("w13", D, (F, F), _hip.EPI_SWIGLU, True), ("w2", F, (D,), _hip.EPI_RESIDUAL, False)]
        quant_total = 0.0
        for name, K, segs, epi, norm in groups:
            x = torch.empty((M, K), device=DEV, dtype=torch.bfloat16).normal_(0.0, 1.0, generator=g)
            ws = [torch.empty((n, K), device=DEV, dtype=torch.bfloat16).normal_(0.0, K ** -0.5, generator=g) for n in segs]
            qs = [quantize_rows(w) for w in ws]
            wq, sc = [q.view(torch.uint8) for q, _ in qs], [s for _, s in qs]
            nw = torch.ones(K, device=DEV, dtype=torch.bfloat16) if norm else None
            N = segs[0] if epi == _hip.EPI_SWIGLU else sum(segs)
            res = torch.zeros((M, N), device=DEV, dtype=torch.bfloat16) if epi == _hip.EPI_RESIDUAL else None
            o8 = torch.empty((M, N), device=DEV, dtype=torch.bfloat16)
            flops = 2.0 * M * K * sum(segs)
            t_leaf = leaf_us(lambda: _hip.linear_w8a8(x, wq, sc, epi, residual=res, norm_w=nw, eps=1e-5, out=o8), o.reps)
            t_q = leaf_us(lambda: _hip.act_quant_e4m3(x, norm_w=nw, eps=1e-5), o.reps)
            t_bf = leaf_us(lambda: _hip.linear(x, ws, epi, residual=res, out=o8), o.reps)   # (bf16: the norm is a launch of its own, not timed)
            t_deq = leaf_us(lambda: _hip.linear_w8(x, wq, sc, epi, residual=res, out=o8), o.reps)
            t_gemm = t_leaf - t_q
            quant_total += t_q
            out[name] = {"w8a8_leaf_us": round(t_leaf, 1), "act_quant_us": round(t_q, 1), "w8a8_gemm_us": round(t_gemm, 1),
                         "bf16_gemm256_us": round(t_bf, 1), "w8_dequant_gemm_us": round(t_deq, 1),
                         "w8a8_gemm_tfs": round(flops / t_gemm / 1e6, 1), "bf16_gemm256_tfs": round(flops / t_bf / 1e6, 1),
                         "act_quant_gbs": round(M * K * 3 / t_q / 1e3, 1)}
            del x, ws, qs, wq, sc, o8
        out["act_quant_four_passes_us"] = round(quant_total, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
