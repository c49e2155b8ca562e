#!/usr/bin/env python3
"""What weight-only MXFP4 buys at the Mistral-7B dims (32 layers) beside FP8 and bf16, one process on one box:

    python scripts/mxfp4_probe.py [--layers 32] [--steps 64] [--only-step]

Times (HIP events on the launch stream around queued steps; warm-up first: the first steps size the workspace and capture the
decode graph - same discipline as bench.py and scripts/fp8_probe.py), each of the three models built, timed and freed in turn:
  (a) the decode step at batch 1 and 3, always on the launch path (the engine is switched off for bf16; it declines the others);
  (b) a 4096-token prefill (FP8 / MXFP4: one dequantisation pass per linear group in front of every GEMM);
  (c) the bytes a batch-1 step must read (weights + scales + LM head + the K/V rings at the probe's context) and the fraction of
      8 TB/s each timing stands for.
The comparison is between the three numbers of ONE run; boxes differ by a few percent.  Weights are random (timing only).
`--only-step` runs nothing but the MXFP4 model's batch-1 decode steps: the form to put under
`rocprofv3 --kernel-trace --stats -- python scripts/mxfp4_probe.py --only-step` for the per-kernel table (counters, if wanted, in a
run of their own), and under MI_GEMV_W4_RP=1 / 2 for the A/B of the rows per unit (csrc/gemv_w4.hip).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mistral_inference import _hip  # noqa: E402
from mistral_inference.args import TransformerArgs  # noqa: E402
from mistral_inference.quant import Fp8Linear, Mxfp4Linear, quantize_blocks, quantize_rows  # noqa: E402
from mistral_inference.transformer import Transformer  # noqa: E402

from fp8_probe import DEV, DIMS, HBM_BYTES_PER_S, PROMPT, decode_step_us, prefill_ms  # noqa: E402


def build(layers: int, qformat):
    p = dict(DIMS, n_layers=layers)
    if qformat:
        p["quantization"] = dict(qformat_weight=qformat)
    a = TransformerArgs.from_dict(p)
    a.max_batch_size = 3
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (Fp8Linear, Mxfp4Linear)):  # quantised on the device, one linear at a time
                w = torch.empty((mod.out_features, mod.in_features), device=DEV, dtype=torch.bfloat16)
                w.normal_(0.0, mod.in_features ** -0.5, generator=g)
                mod.load_quantized(*(quantize_blocks(w) if isinstance(mod, Mxfp4Linear) else quantize_rows(w)))
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            elif t.dtype == torch.bfloat16:
                t.normal_(0.0, t.shape[-1] ** -0.5, generator=g)
    m._weights_changed()
    return m.eval()


def step_bytes(layers: int, qformat, kv_len: int) -> int:
    """Bytes one batch-1 decode step must read: the seven linears of every layer (+ their scales), the LM head, the K/V rings."""
    D, F, V = DIMS["dim"], DIMS["hidden_dim"], DIMS["vocab_size"]
    nq, nkv = DIMS["n_heads"] * DIMS["head_dim"], DIMS["n_kv_heads"] * DIMS["head_dim"]
    elems = (nq + 2 * nkv) * D + D * nq + 3 * F * D
    rows = (nq + 2 * nkv) + D + 2 * F + D
    per_layer = {None: 2 * elems, "fp8_e4m3": elems + 4 * rows, "mxfp4": elems // 2 + elems // 32}[qformat]
    return layers * (per_layer + 2 * kv_len * nkv * 2) + 2 * V * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--only-step", action="store_true")
    o = ap.parse_args()
    kv_len = PROMPT + 8 + 2 * o.steps   # the middle of the timed steps, near enough
    out = {"layers": o.layers, "steps": o.steps, "gemv_w4_rp": os.environ.get("MI_GEMV_W4_RP", "rule")}
    prev = _hip.set_decode_engine(False)   # every step below is the launch path
    with torch.inference_mode():
        for name, qformat in (("mxfp4", "mxfp4"), ("fp8", "fp8_e4m3"), ("bf16", None)):
            model = build(o.layers, qformat)
            nbytes = step_bytes(o.layers, qformat, kv_len)
            out[f"{name}_step_bytes_gb"] = round(nbytes / 1e9, 2)
            out[f"{name}_step_us_b1"] = round(decode_step_us(model, 1, o.steps), 1)
            out[f"{name}_frac_of_8TBs_b1"] = round(nbytes / (out[f"{name}_step_us_b1"] * 1e-6) / HBM_BYTES_PER_S, 3)
            if o.only_step:
                break
            out[f"{name}_step_us_b3"] = round(decode_step_us(model, 3, o.steps), 1)
            out[f"{name}_prefill4096_ms"] = round(prefill_ms(model), 2)
            out[f"{name}_prefill4096_tok_s"] = round(4096 / out[f"{name}_prefill4096_ms"] * 1e3)
            out[f"{name}_engine_launches"] = _hip.decode_engine_status(model._backend._workspace)["engine_launches"]
            del model
            torch.cuda.empty_cache()
    _hip.set_decode_engine(prev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
