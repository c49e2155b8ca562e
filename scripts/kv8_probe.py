#!/usr/bin/env python3
"""What K/V rings of e4m3 bytes (BufferCache(dtype=torch.float8_e4m3fn)) cost and buy at the Mistral-7B dims, one process on one box:

    python scripts/kv8_probe.py [--layers 32] [--steps 64] [--weights bf16,fp8,mxfp4] [--only-kernels]

Every ring is FULL: a 4096-slot window, 4096 tokens of context before the first timed step.  Times are HIP events on the launch
stream around queued work, after a warm-up (same discipline as bench.py and scripts/mxfp4_probe.py); the bf16-cache and the
FP8-cache figure of a pair are taken one after the other on the same model in the same process:
  (a) per layer, the decode attention (split kernel + combine) and the ring write of one step at batch 1 and 3, on bf16 rings and
      on e4m3 rings: a captured graph of one call per layer over `--layers` different ring pairs (more bytes than the caches
      hold), replayed;
  (b) the decode step on the launch path (the engine is switched off: it declines e4m3 rings) at batch 1 and 3 with a bf16 and
      with an FP8 cache, for bf16, FP8 and MXFP4 weights;
  (c) a 4096-token prefill in chunks of 1024 at batch 1 (FP8 cache: one dequantisation of the layer's rings per layer and chunk).
Weights are random (timing only).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mistral_inference import _hip  # noqa: E402
from mistral_inference.cache import KV_FP8, BufferCache  # noqa: E402

from fp8_probe import DEV, DIMS, event_ms  # noqa: E402
from mxfp4_probe import build  # noqa: E402

W, CONTEXT, CHUNK = 4096, 4096, 1024
KV = (("bf16", torch.bfloat16), ("fp8", KV_FP8))
H, HKV, DH = DIMS["n_heads"], DIMS["n_kv_heads"], DIMS["head_dim"]


def ring_bytes(layers: int, B: int, dtype) -> int:
    """Bytes of K and V that one decode step of B sequences reads from full rings."""
    return layers * 2 * B * W * HKV * DH * (1 if dtype == KV_FP8 else 2)


def graph_us(fn, reps: int = 5) -> float:
    fn()                                    # warm-up: code objects, scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return event_ms(g.replay, reps) * 1000.0


def kernel_times(layers: int) -> dict:
    """(a): microseconds per layer of attn_decode (+ combine) and of kv_write, per ring dtype and batch."""
    out = {}
    for B in (1, 3):
        q = torch.randn((B, H * DH), device=DEV).to(torch.bfloat16)
        rows = torch.randn((B, 2 * HKV * DH), device=DEV).to(torch.bfloat16)
        pos = torch.full((B,), CONTEXT + 7, dtype=torch.int32, device=DEV)
        seq = torch.arange(B, dtype=torch.int32, device=DEV)
        q_start = torch.arange(B + 1, dtype=torch.int32, device=DEV)
        for name, dtype in KV:
            c = BufferCache(layers, B, W, HKV, DH, None, device=DEV, dtype=dtype)
            for l in range(layers):     # finite values in every slot
                for t in (c.cache_k[l], c.cache_v[l]):
                    t.view(torch.uint8 if dtype == KV_FP8 else torch.int16).random_(0, 0x78 if dtype == KV_FP8 else 0x4000)

            def attn():
                for l in range(layers):
                    _hip.attn_decode(q, c.cache_k[l], c.cache_v[l], H, pos)

            def write():
                for l in range(layers):
                    _hip.kv_write(c.cache_k[l], c.cache_v[l], rows[:, :HKV * DH], rows[:, HKV * DH:], seq, pos, q_start)
            out[f"attn_decode_us_per_layer_{name}_b{B}"] = round(graph_us(attn) / layers, 2)
            out[f"kv_write_us_per_layer_{name}_b{B}"] = round(graph_us(write) / layers, 2)
            out[f"ring_gb_{name}_b{B}"] = round(ring_bytes(layers, B, dtype) / 1e9, 3)
            del c
            torch.cuda.empty_cache()
    return out


def filled_cache(model, B: int, dtype):
    """A cache whose rings are full: CONTEXT tokens per sequence in chunks of CHUNK; returns (cache, next token, ms of chunks 2..)."""
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, 2 * W, a.n_kv_heads, a.head_dim, W, device=DEV, dtype=dtype)
    cache.reset()
    ids = torch.randint(0, a.vocab_size, (CONTEXT // CHUNK, CHUNK * B), generator=torch.Generator().manual_seed(0)).to(DEV)
    model.forward_partial(ids[0], [CHUNK] * B, cache)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(1, CONTEXT // CHUNK - 1):
        model.forward_partial(ids[i], [CHUNK] * B, cache)
    e1.record()
    logits = model.forward(ids[-1], [CHUNK] * B, cache)
    torch.cuda.synchronize()
    first = logits[torch.arange(B, device=DEV) * CHUNK + CHUNK - 1].argmax(-1)
    return cache, first, e0.elapsed_time(e1) / (CONTEXT // CHUNK - 2)


def step_us(model, B: int, dtype, steps: int):
    cache, first, chunk_ms = filled_cache(model, B, dtype)
    sess = model.greedy_session(cache, first)
    sess.run(8)          # warm-up: eager step, graph capture, replays
    sess.collect()
    ms = event_ms(lambda: sess.run(steps))
    sess.collect()
    return ms * 1000.0 / steps, chunk_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--weights", default="bf16,fp8,mxfp4")
    ap.add_argument("--only-kernels", action="store_true")
    o = ap.parse_args()
    qformats = {"bf16": None, "fp8": "fp8_e4m3", "mxfp4": "mxfp4"}
    out = {"layers": o.layers, "steps": o.steps, "window": W, "context": CONTEXT}
    prev = _hip.set_decode_engine(False)   # every step below is the launch path
    with torch.inference_mode():
        out.update(kernel_times(o.layers))
        for wname in ([] if o.only_kernels else o.weights.split(",")):
            model = build(o.layers, qformats[wname])
            for B in (1, 3):
                for _ in range(2):         # the pair twice, alternating: the spread between the two rounds is in the output
                    for kname, dtype in KV:
                        us, chunk_ms = step_us(model, B, dtype, o.steps)
                        out.setdefault(f"{wname}_step_us_b{B}_{kname}_cache", []).append(round(us, 1))
                        if B == 1:
                            out.setdefault(f"{wname}_prefill_chunk1024_ms_{kname}_cache", []).append(round(chunk_ms, 2))
            out[f"{wname}_engine_launches"] = _hip.decode_engine_status(model._backend._workspace)["engine_launches"]
            del model
            torch.cuda.empty_cache()
    _hip.set_decode_engine(prev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
