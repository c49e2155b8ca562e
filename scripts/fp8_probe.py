#!/usr/bin/env python3
"""What weight-only FP8 (e4m3) buys at the Mistral-7B dims (32 layers), one process on one box:

    python scripts/fp8_probe.py [--layers 32] [--steps 64] [--only-fp8-step]

Times (HIP events on the launch stream around queued steps; warm-up first: the first steps size the workspace, capture the
decode graph and, for the engine, run its residency census - same discipline as bench.py and scripts/lora_probe.py):
  (a) the bf16 decode step on the launch path (engine off), batch 1 and 3;   (b) the bf16 step on the persistent engine, batch 1;
  (c) the FP8 decode step, batch 1 and 3 (always the launch path: the engine declines e4m3 weights);
  (d) a 4096-token prefill, bf16 and FP8 (FP8: one dequantisation pass per linear group in front of every GEMM);
  (e) the bytes a batch-1 step must read (weights + row scales + LM head + the K/V rings at the probe's context) and the
      fraction of 8 TB/s each timing stands for.
Weights are random (timing only).  `--only-fp8-step` runs nothing but the FP8 model's batch-1 decode steps: the form to put
under `rocprofv3 --kernel-trace --stats -- python scripts/fp8_probe.py --only-fp8-step` for the per-kernel table, and under
MI_GEMV_W8_RP=1 / 2 for the A/B of two- against four-row units (csrc/gemv_w8.hip).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))

import torch  # noqa: E402

from mistral_inference import _hip  # noqa: E402
from mistral_inference.args import TransformerArgs  # noqa: E402
from mistral_inference.cache import BufferCache  # noqa: E402
from mistral_inference.quant import Fp8Linear, quantize_rows  # noqa: E402
from mistral_inference.transformer import Transformer  # noqa: E402

DEV = "cuda:0"
PROMPT = 32
HBM_BYTES_PER_S = 8e12
DIMS = dict(dim=4096, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=32768)


def build(layers: int, fp8: bool):
    p = dict(DIMS, n_layers=layers)
    if fp8:
        p["quantization"] = dict(qformat_weight="fp8_e4m3")
    a = TransformerArgs.from_dict(p)
    a.max_batch_size = 3
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, Fp8Linear):  # quantised on the device, one linear at a time
                w = torch.empty((mod.out_features, mod.in_features), device=DEV, dtype=torch.bfloat16)
                mod.load_quantized(*quantize_rows(w.normal_(0.0, mod.in_features ** -0.5, generator=g)))
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            elif t.dtype == torch.bfloat16:
                t.normal_(0.0, t.shape[-1] ** -0.5, generator=g)
    m._weights_changed()
    return m.eval()


def step_bytes(layers: int, fp8: bool, kv_len: int) -> int:
    """Bytes one batch-1 decode step must read: the seven linears of every layer (+ fp32 row scales), the LM head, the K/V rings."""
    D, F, V = DIMS["dim"], DIMS["hidden_dim"], DIMS["vocab_size"]
    nq, nkv = DIMS["n_heads"] * DIMS["head_dim"], DIMS["n_kv_heads"] * DIMS["head_dim"]
    elems = (nq + 2 * nkv) * D + D * nq + 3 * F * D
    rows = (nq + 2 * nkv) + D + 2 * F + D
    per_layer = elems + 4 * rows if fp8 else 2 * elems
    return layers * (per_layer + 2 * kv_len * nkv * 2) + 2 * V * D


def event_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def decode_step_us(model, B: int, steps: int) -> float:
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, 4096, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    cache.reset()
    ids = torch.randint(0, a.vocab_size, (PROMPT * B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    logits = model.forward(ids, [PROMPT] * B, cache)
    first = logits[torch.arange(B, device=DEV) * PROMPT + PROMPT - 1].argmax(-1)
    sess = model.greedy_session(cache, first)
    sess.run(8)          # warm-up: eager step, graph capture, replays
    sess.collect()
    ms = event_ms(lambda: sess.run(steps))
    sess.collect()
    return ms * 1000.0 / steps


def prefill_ms(model, T: int = 4096) -> float:
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, T, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    ids = torch.randint(0, a.vocab_size, (T,), generator=torch.Generator().manual_seed(0)).to(DEV)

    def run():
        cache.reset()
        model.forward_partial(ids, [T], cache)
    run()
    torch.cuda.synchronize()
    return event_ms(run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--only-fp8-step", action="store_true")
    o = ap.parse_args()
    kv_len = PROMPT + 8 + 2 * o.steps   # the middle of the timed steps, near enough
    out = {"layers": o.layers, "steps": o.steps, "gemv_w8_rp": os.environ.get("MI_GEMV_W8_RP", "rule")}

    def frac(us, nbytes):
        return round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)

    with torch.inference_mode():
        fp8 = build(o.layers, True)
        b8 = step_bytes(o.layers, True, kv_len)
        out["fp8_step_bytes_gb"] = round(b8 / 1e9, 2)
        out["fp8_step_us_b1"] = round(decode_step_us(fp8, 1, o.steps), 1)
        out["fp8_frac_of_8TBs_b1"] = frac(out["fp8_step_us_b1"], b8)
        if o.only_fp8_step:
            print(json.dumps(out))
            return
        out["fp8_step_us_b3"] = round(decode_step_us(fp8, 3, o.steps), 1)
        out["fp8_prefill4096_ms"] = round(prefill_ms(fp8), 2)
        out["fp8_prefill4096_tok_s"] = round(4096 / out["fp8_prefill4096_ms"] * 1e3)
        out["fp8_engine_launches"] = _hip.decode_engine_status(fp8._backend._workspace)["engine_launches"]
        del fp8
        torch.cuda.empty_cache()
        plain = build(o.layers, False)
        b16 = step_bytes(o.layers, False, kv_len)
        out["bf16_step_bytes_gb"] = round(b16 / 1e9, 2)
        prev = _hip.set_decode_engine(False)
        out["bf16_launch_step_us_b1"] = round(decode_step_us(plain, 1, o.steps), 1)
        out["bf16_launch_frac_of_8TBs_b1"] = frac(out["bf16_launch_step_us_b1"], b16)
        out["bf16_launch_step_us_b3"] = round(decode_step_us(plain, 3, o.steps), 1)
        _hip.set_decode_engine(True)
        out["bf16_engine_step_us_b1"] = round(decode_step_us(plain, 1, o.steps), 1)
        out["bf16_engine_frac_of_8TBs_b1"] = frac(out["bf16_engine_step_us_b1"], b16)
        out["bf16_engine_launches"] = _hip.decode_engine_status(plain._backend._workspace)["engine_launches"]
        _hip.set_decode_engine(prev)
        out["bf16_prefill4096_ms"] = round(prefill_ms(plain), 2)
        out["bf16_prefill4096_tok_s"] = round(4096 / out["bf16_prefill4096_ms"] * 1e3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
