#!/usr/bin/env python3
"""Attention of one Pixtral vision-tower layer (16 heads x 64, bf16, all patches attend to each other) at T = 1024, 4096, 16384
patches (and 512, where the launcher picks its smallest block): the 64-wide kernel (csrc/attn_prefill64.hip) against the route it replaced - zero-pad every head to 128 with torch, the
128-wide prefill kernel, slice the 64 real columns back out, the torch ops INSIDE the bracket since a layer paid for them - and
against the 128-wide kernel alone on input padded beforehand.  The native kernel is also timed with each block shape pinned
(MI_ATTN64_QUERIES), which is what the launcher's choice rests on.

All routes run in one process, interleaved, every route twice (two passes); each bracket is a 50 ms idle period, 3 warm-up
launches, then `n` launches between two HIP events.  One JSON line per (T, route): both passes in microseconds per call, and
TFLOP/s of the useful work 4 T^2 H 64 at the better pass; one line per T with max |native - padded route| on the same input.
    python scripts/vision_attn_probe.py > profiles/vision_attn_probe.json.log"""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
import torch  # noqa: E402
from mistral_inference import _hip  # noqa: E402

H, DH = 16, 64
dev = torch.device("cuda:0")


def native(qkv, T, queries=None):
    def f():
        if queries:
            os.environ["MI_ATTN64_QUERIES"] = queries
        else:
            os.environ.pop("MI_ATTN64_QUERIES", None)
        return _hip.attn_prefill(qkv, H, H, DH, None, None, T, None, None, 1, T, causal=False, softmax_scale=DH ** -0.5)
    return f


def padded_route(qkv, T):
    def f():
        pad = torch.zeros((T, 3 * H, 128), dtype=qkv.dtype, device=dev)
        pad[:, :, :DH] = qkv.view(T, 3 * H, DH)
        att = _hip.attn_prefill(pad.view(T, 3 * H * 128), H, H, 128, None, None, T, None, None, 1, T, causal=False, softmax_scale=DH ** -0.5)
        return att.view(T, H, 128)[:, :, :DH].reshape(T, H * DH).contiguous()
    return f


def bracket(f, n):
    time.sleep(0.05)
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


torch.manual_seed(11)
for T in (512, 1024, 4096, 16384):
    qkv = torch.randn(T, 3 * H * DH, device=dev).to(torch.bfloat16)
    pre = torch.zeros((T, 3 * H, 128), dtype=qkv.dtype, device=dev)
    pre[:, :, :DH] = qkv.view(T, 3 * H, DH)
    pre = pre.view(T, 3 * H * 128)
    routes = {"native64": native(qkv, T), "pad_128_slice": padded_route(qkv, T),
              "kernel128_prepadded": lambda: _hip.attn_prefill(pre, H, H, 128, None, None, T, None, None, 1, T, causal=False, softmax_scale=DH ** -0.5),
              "native64_q64": native(qkv, T, "64"), "native64_q128": native(qkv, T, "128"), "native64_q256": native(qkv, T, "256")}
    diff = float((routes["native64"]().float() - routes["pad_128_slice"]().float()).abs().max())
    n = 40 if T <= 4096 else 10
    us = {name: [] for name in routes}
    for _ in range(2):
        for name, f in routes.items():
            us[name].append(round(bracket(f, n), 1))
    os.environ.pop("MI_ATTN64_QUERIES", None)
    for name, t in us.items():
        print(json.dumps({"T": T, "H": H, "head_dim": DH, "route": name, "us_per_call": t, "launches_per_bracket": n,
                          "useful_tflops": round(4.0 * T * T * H * DH / min(t) / 1e6, 1)}), flush=True)
    print(json.dumps({"T": T, "max_abs_native_minus_padded_route": diff, "device": torch.cuda.get_device_name(0)}), flush=True)
