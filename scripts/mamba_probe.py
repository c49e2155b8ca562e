#!/usr/bin/env python3
"""Mamba2 at Codestral-Mamba dims (dim 4096, 64 layers, 8 groups, vocabulary 32768) with random weights on one MI355X: prefill
tokens/s at 2048 and 4096 tokens, decode ms/step at batch 1 and 3, and the per-kernel split of one layer (device events around
each leaf).  Prints one JSON line.  Nothing here is a pass condition."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
from mistral_inference import _hip  # noqa: E402
from mistral_inference.args import MambaArgs  # noqa: E402
from mistral_inference.mamba import Mamba, MambaCache, MambaDims  # noqa: E402

DEV = "cuda:0"


def timed(fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main(n_layers=64):
    args = MambaArgs(dim=4096, n_layers=n_layers, vocab_size=32768, n_groups=8, rms_norm=True, residual_in_fp32=True, fused_add_norm=True,
                     pad_vocab_size_multiple=8, tie_embeddings=False)
    d = MambaDims(args)
    rnd = lambda *s, scale=1.0, dt=torch.bfloat16: (torch.randn(*s, device=DEV, dtype=torch.float32) * scale).to(dt)
    layer = lambda: {"norm": rnd(d.D) * 0.1 + 1, "in_proj": rnd(d.in_proj_rows, d.D, scale=d.D ** -0.5), "conv_w": rnd(d.conv_dim, 1, 4, scale=0.4),
                     "conv_b": rnd(d.conv_dim, scale=0.1), "dt_bias": rnd(d.H, dt=torch.float32) - 3, "A_log": torch.rand(d.H, device=DEV).log(),
                     "D": torch.ones(d.H, device=DEV), "gated_norm": rnd(d.I) * 0.1 + 1, "out_proj": rnd(d.D, d.I, scale=d.I ** -0.5)}
    w = {"embedding": rnd(d.V, d.D), "norm_f": rnd(d.D) * 0.1 + 1, "lm_head": rnd(d.V, d.D, scale=d.D ** -0.5), "layers": [layer() for _ in range(n_layers)]}
    model = Mamba(args, w, device=DEV)
    out = {"config": f"dim 4096, {n_layers} layers, 8 groups, vocabulary 32768, random bf16 weights", "prefill": {}, "decode": {}, "layer_split_us": {}}
    for L in (2048, 4096):
        ids = torch.randint(0, d.V, (1, L), device=DEV)
        ms = timed(lambda: model.forward(ids, cache=MambaCache(model, 1), last_only=True), warmup=2, iters=4)
        out["prefill"][str(L)] = {"ms": round(ms, 2), "tokens_per_s": round(L / ms * 1e3)}
    for B in (1, 3):
        cache = MambaCache(model, B)
        tok = torch.randint(0, d.V, (B, 1), device=DEV)
        ms = timed(lambda: model.forward(tok, cache=cache, last_only=True), warmup=5, iters=30)
        state = B * d.H * 64 * 128 * 4 * 2                                    # the step kernel reads and writes the state once
        weights = (d.in_proj_rows + d.I) * d.D * 2
        out["decode"][f"batch{B}"] = {"ms_per_step": round(ms, 3), "bytes_per_layer": {"state_rw": state, "weights": weights},
                                      "ms_at_8TBps": round(n_layers * (state + weights) / 8e12 * 1e3 + d.V * d.D * 2 / 8e12 * 1e3, 3)}
    ly = w["layers"][0]
    for name, B, L in (("prefill_4096", 1, 4096), ("decode_b1", 1, 1)):
        T = B * L
        res, h = torch.zeros(T, d.D, device=DEV), rnd(T, d.D)
        u = _hip.mamba_add_norm(res, h, ly["norm"], 1e-5)
        ld = (d.in_proj_rows + 7) // 8 * 8
        zx = torch.empty(T, ld, dtype=torch.bfloat16, device=DEV)
        conv, ssm = torch.zeros(B, 3, d.conv_dim, dtype=torch.bfloat16, device=DEV), torch.zeros(B, d.H, 64, 128, device=DEV)
        in_proj = lambda: _hip.linear(u, [ly["in_proj"]], out=zx[:, :d.in_proj_rows])
        in_proj()
        scan = lambda: _hip.mamba_scan(zx.view(B, L, ld), ly["conv_w"], ly["conv_b"], ly["dt_bias"], ly["A_log"], ly["D"], conv, ssm, d.G)
        y = scan().view(T, d.I)
        o = _hip.mamba_gated_norm(y, zx, ly["gated_norm"], d.G, 1e-5)
        out["layer_split_us"][name] = {k: round(timed(f) * 1e3, 1) for k, f in (
            ("add_norm", lambda: _hip.mamba_add_norm(res, h, ly["norm"], 1e-5)), ("in_proj", in_proj), ("scan_and_conv_state", scan),
            ("gated_norm", lambda: _hip.mamba_gated_norm(y, zx, ly["gated_norm"], d.G, 1e-5)), ("out_proj", lambda: _hip.linear(o, [ly["out_proj"]])))}
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
