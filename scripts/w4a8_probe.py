#!/usr/bin/env python3
"""What the MXFP4 x FP8 prefill GEMMs (W4A8, `prefill_w4a8`) buy at the Mistral-7B dims, one process on one box:

    python scripts/w4a8_probe.py [--layers 32] [--reps 5]

Times (HIP events on the launch stream; warm-up first, same discipline as bench.py and scripts/w8a8_probe.py):
  (a) a prefill of 4096 and of 2048 tokens on four routes - the bf16 model, the MXFP4 model on the weight-only route (one
      dequantisation pass per linear group in front of the bf16 GEMM), the same MXFP4 model with `prefill_w4a8`, and the FP8 model
      with `prefill_fp8` - each measured twice, interleaved (bf16, w4, w4a8, w8a8, bf16, ...), so that a drifting clock or power
      state shows as a spread;
  (b) per linear group of a layer (q|k|v, wo, w1|w3, w2) at 4096 rows and for every route: the leaf's time, and the GEMM alone - for
      the two FP8-activation routes the leaf minus the quantiser pass timed on its own, for the weight-only MXFP4 route the leaf as
      it is (dequantisation pass + bf16 GEMM), for bf16 gemm256 - in microseconds and TF/s, and the W4A8 GEMM's rate against the
      W8A8 GEMM's: the mixed e2m1 x e4m3 instruction's apparent rate against e4m3 x e4m3 in the same kernel structure.
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
from mistral_inference.args import TransformerArgs  # noqa: E402
from mistral_inference.quant import Mxfp4Linear, quantize_blocks, quantize_rows  # noqa: E402
from mistral_inference.transformer import Transformer  # noqa: E402
from w8a8_probe import leaf_us, prefill_runner  # noqa: E402


def build_mxfp4(layers: int):
    """fp8_probe.build for an MXFP4 model: N(0, 1 / in) weights quantised on the device, one linear at a time."""
    a = TransformerArgs.from_dict(dict(DIMS, n_layers=layers, quantization=dict(qformat_weight="mxfp4")))
    a.max_batch_size = 3
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, Mxfp4Linear):
                w = torch.empty((mod.out_features, mod.in_features), device=DEV, dtype=torch.bfloat16)
                mod.load_quantized(*quantize_blocks(w.normal_(0.0, mod.in_features ** -0.5, generator=g)))
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            elif t.dtype == torch.bfloat16:
                t.normal_(0.0, t.shape[-1] ** -0.5, generator=g)
    m._weights_changed()
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    o = ap.parse_args()
    out = {"layers": o.layers, "reps": o.reps}
    D, F = DIMS["dim"], DIMS["hidden_dim"]
    nq, nkv = DIMS["n_heads"] * DIMS["head_dim"], DIMS["n_kv_heads"] * DIMS["head_dim"]
    with torch.inference_mode():
        plain, w4, fp8 = build(o.layers, False), build_mxfp4(o.layers), build(o.layers, True)
        fp8.prefill_fp8 = True
        for T in (4096, 2048):
            runs = {"bf16": (plain, None), "w4": (w4, False), "w4a8": (w4, True), "w8a8": (fp8, None)}
            ms = {k: [] for k in runs}
            for _ in range(2):
                for name, (model, flag) in runs.items():
                    if flag is not None:
                        model.prefill_w4a8 = flag
                    run = prefill_runner(model, T)
                    run()
                    torch.cuda.synchronize()
                    ms[name].append(event_ms(run, o.reps))
            for name, v in ms.items():
                out[f"{name}_prefill{T}_ms"] = [round(x, 2) for x in v]
                out[f"{name}_prefill{T}_tok_s"] = round(T / min(v) * 1e3)
        del plain, w4, fp8
        torch.cuda.empty_cache()

        # ---- the leaves at 4096 rows: (name, K, segment rows, epilogue, fused norm)
        M = 4096
        g = torch.Generator(device=DEV).manual_seed(2)
        groups = [("qkv", D, (nq, nkv, nkv), _hip.EPI_STORE, True), ("wo", nq, (D,), _hip.EPI_RESIDUAL, False),
                  ("w13", D, (F, F), _hip.EPI_SWIGLU, True), ("w2", F, (D,), _hip.EPI_RESIDUAL, False)]
        for name, K, segs, epi, norm in groups:
            x = torch.empty((M, K), device=DEV, dtype=torch.bfloat16).normal_(0.0, 1.0, generator=g)
            ws = [torch.empty((n, K), device=DEV, dtype=torch.bfloat16).normal_(0.0, K ** -0.5, generator=g) for n in segs]
            q8 = [quantize_rows(w) for w in ws]
            w8, s8 = [q.view(torch.uint8) for q, _ in q8], [s for _, s in q8]
            q4 = [quantize_blocks(w) for w in ws]
            c4, s4 = [c for c, _ in q4], [s for _, s in q4]
            nw = torch.ones(K, device=DEV, dtype=torch.bfloat16) if norm else None
            N = segs[0] if epi == _hip.EPI_SWIGLU else sum(segs)
            res = torch.zeros((M, N), device=DEV, dtype=torch.bfloat16) if epi == _hip.EPI_RESIDUAL else None
            ob = torch.empty((M, N), device=DEV, dtype=torch.bfloat16)
            flops = 2.0 * M * K * sum(segs)
            t = {
                "w4a8_leaf": leaf_us(lambda: _hip.linear_w4a8(x, c4, s4, epi, residual=res, norm_w=nw, eps=1e-5, out=ob), o.reps),
                "w8a8_leaf": leaf_us(lambda: _hip.linear_w8a8(x, w8, s8, epi, residual=res, norm_w=nw, eps=1e-5, out=ob), o.reps),
                "act_quant": leaf_us(lambda: _hip.act_quant_e4m3(x, norm_w=nw, eps=1e-5), o.reps),
                "w4_dequant_gemm": leaf_us(lambda: _hip.linear_w4(x, c4, s4, epi, residual=res, out=ob), o.reps),
                "bf16_gemm256": leaf_us(lambda: _hip.linear(x, ws, epi, residual=res, out=ob), o.reps),  # (the norm is a launch of its own, not timed)
            }
            t["w4a8_gemm"], t["w8a8_gemm"] = t["w4a8_leaf"] - t["act_quant"], t["w8a8_leaf"] - t["act_quant"]
            r = {k + "_us": round(v, 1) for k, v in t.items()}
            for k in ("w4a8_gemm", "w8a8_gemm", "w4_dequant_gemm", "bf16_gemm256"):
                r[k + "_tfs"] = round(flops / t[k] / 1e6, 1)
            r["w4a8_over_w8a8_rate"] = round(t["w8a8_gemm"] / t["w4a8_gemm"], 3)
            out[name] = r
            del x, ws, q8, w8, s8, q4, c4, s4, ob
    print(json.dumps(out))


if __name__ == "__main__":
    main()
