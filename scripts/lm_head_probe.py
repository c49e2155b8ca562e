#!/usr/bin/env python3
"""What a quantised LM head (quantize_lm_head) buys, one process on one box:

    python scripts/lm_head_probe.py [--dims 7b,nemo] [--layers N] [--steps 64] [--reps 200]

At the Mistral-7B dims (vocab 32768, dim 4096, 32 layers) and the Mistral-Nemo dims (vocab 131072, dim 5120, 40 layers), for
FP8 (e4m3) and MXFP4, each pair interleaved and measured twice (bf16, quantised, bf16, quantised):
  (a) the head launch alone at T = 1, 4, 8 with the final RMSNorm fused: mi_linear(MI_EPI_LOGITS) on the bf16 head against
      mi_lm_head_q on the quantised one - HIP events around `--reps` queued launches after a warm-up, and the bytes each must read;
  (b) the launch-path decode step at batch 1 of a model whose layers are quantised, with the bf16 head and with the quantised head
      (the same layers: the head module is exchanged) - events around `--steps` queued steps of a greedy session after its warm-up
      (workspace, graph capture), as scripts/fp8_probe.py times its steps.
Weights are random (timing only).  Nothing is compared against a threshold: the expectation is the ratio of the bytes, printed
beside every pair.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from mistral_inference import _hip  # noqa: E402
from mistral_inference.args import TransformerArgs  # noqa: E402
from mistral_inference.cache import BufferCache  # noqa: E402
from mistral_inference.quant import QUANT_LINEARS, QuantLinear  # noqa: E402
from mistral_inference.transformer import Transformer  # noqa: E402

DEV = "cuda:0"
PROMPT = 32
DIMS = {"7b": dict(dim=4096, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=32768, n_layers=32),
        "nemo": dict(dim=5120, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=131072, n_layers=40)}
FORMATS = ("fp8_e4m3", "mxfp4")


def head_bytes(qformat, V, D):
    """Bytes a launch over the head must read: weights and their scales."""
    return {None: 2 * V * D, "fp8_e4m3": V * D + 4 * V, "mxfp4": V * D // 2 + V * D // 32}[qformat]


def quantised(cls, out_features, in_features, g):
    """A random linear of the format, quantised on the device."""
    mod = cls(in_features, out_features)
    w = torch.empty((out_features, in_features), device=DEV, dtype=torch.bfloat16).normal_(0.0, in_features ** -0.5, generator=g)
    mod.load_quantized(*cls.quantize(w))
    return mod


def event_us(fn, n):
    """Median of three timings of n queued calls, per call."""
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / n)
    return sorted(ts)[1]


def head_alone(p, reps):
    """(a): per format and T, [bf16, quantised, bf16, quantised] us per launch."""
    V, D = p["vocab_size"], p["dim"]
    g = torch.Generator(device=DEV).manual_seed(2)
    w = torch.empty((V, D), device=DEV, dtype=torch.bfloat16).normal_(0.0, D ** -0.5, generator=g)
    nw = torch.ones(D, device=DEV, dtype=torch.bfloat16)
    out = {}
    for qformat in FORMATS:
        q = quantised(QUANT_LINEARS[qformat], V, D, g)
        for T in (1, 4, 8):
            x = torch.randn((T, D), device=DEV, generator=g).to(torch.bfloat16)
            logits = torch.empty((T, V), device=DEV, dtype=torch.float32)
            plain = lambda: _hip.linear(x, (w,), _hip.EPI_LOGITS, norm_w=nw, eps=1e-5, out=logits)  # noqa: E731
            quant = lambda: _hip.lm_head_q(q.hip, x, q.weight, q.qscale_weight, norm_w=nw, eps=1e-5, out=logits)  # noqa: E731
            for fn in (plain, quant):  # warm-up: code objects, the LDS opt-in of each instantiation
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            us = [round(event_us(fn, reps), 1) for fn in (plain, quant, plain, quant)]
            b16, bq = head_bytes(None, V, D), head_bytes(qformat, V, D)
            out[f"{qformat}_T{T}"] = {"bf16_us": us[0::2], "quant_us": us[1::2], "bytes_ratio": round(bq / b16, 3),
                                      "time_ratio": round(min(us[1::2]) / min(us[0::2]), 3),
                                      "bf16_TBs": round(b16 / min(us[0::2]) / 1e6, 2), "quant_TBs": round(bq / min(us[1::2]) / 1e6, 2)}
        del q
    return out


def build(p, qformat, layers):
    a = TransformerArgs.from_dict(dict(p, n_layers=layers, quantization=dict(qformat_weight=qformat)))
    a.max_batch_size = 1
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, QuantLinear):  # quantised on the device, one linear at a time
                w = torch.empty((mod.out_features, mod.in_features), device=DEV, dtype=torch.bfloat16)
                mod.load_quantized(*type(mod).quantize(w.normal_(0.0, mod.in_features ** -0.5, generator=g)))
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            elif t.dtype == torch.bfloat16:
                t.normal_(0.0, t.shape[-1] ** -0.5, generator=g)
    m._weights_changed()
    return m.eval(), g


def decode_step_us(model, steps):
    a = model.args
    cache = BufferCache(model.n_local_layers, 1, 4096, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    cache.reset()
    ids = torch.randint(0, a.vocab_size, (PROMPT,), generator=torch.Generator().manual_seed(0)).to(DEV)
    first = model.forward(ids, [PROMPT], cache)[-1:].argmax(-1)
    sess = model.greedy_session(cache, first)
    sess.run(8)          # warm-up: eager step, graph capture, replays
    sess.collect()
    us = event_us(lambda: sess.run(steps), 1) / steps
    sess.collect()
    return us


def step_bytes(p, layers, qformat, head_format, kv_len):
    """Bytes a batch-1 decode step must read: the seven linears of every layer with their scales, the head, the K/V rings."""
    D, F, V = p["dim"], p["hidden_dim"], p["vocab_size"]
    nq, nkv = p["n_heads"] * p["head_dim"], p["n_kv_heads"] * p["head_dim"]
    elems = (nq + 2 * nkv) * D + D * nq + 3 * F * D
    rows = (nq + 2 * nkv) + D + 2 * F + D
    per_layer = elems + 4 * rows if qformat == "fp8_e4m3" else elems // 2 + elems // 32
    return layers * (per_layer + 2 * kv_len * nkv * 2) + head_bytes(head_format, V, D)


def decode_steps(p, layers, steps):
    """(b): per format, [bf16 head, quantised head, bf16 head, quantised head] us per step on the same layers."""
    out = {}
    for qformat in FORMATS:
        model, g = build(p, qformat, layers)
        heads = {"bf16": model.output, "quant": quantised(QUANT_LINEARS[qformat], p["vocab_size"], p["dim"], g)}
        assert isinstance(heads["bf16"], nn.Linear)
        us = []
        for which in ("bf16", "quant", "bf16", "quant"):
            model.output = heads[which]
            model._weights_changed()
            us.append(round(decode_step_us(model, steps), 1))
            assert _hip.decode_engine_status(model._backend._workspace)["engine_launches"] == 0
        kv_len = PROMPT + 8 + 2 * steps
        b16, bq = step_bytes(p, layers, qformat, None, kv_len), step_bytes(p, layers, qformat, qformat, kv_len)
        out[qformat] = {"bf16_head_step_us": us[0::2], "quant_head_step_us": us[1::2], "step_bytes_gb": [round(b16 / 1e9, 2), round(bq / 1e9, 2)],
                        "bytes_ratio": round(bq / b16, 3), "time_ratio": round(min(us[1::2]) / min(us[0::2]), 3)}
        del model, heads
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="7b,nemo")
    ap.add_argument("--layers", type=int, default=0, help="layers of the decode-step models (0: the model's own 32 / 40)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    o = ap.parse_args()
    out = {"steps": o.steps, "reps": o.reps}
    with torch.inference_mode():
        for name in o.dims.split(","):
            p = DIMS[name]
            layers = o.layers or p["n_layers"]
            out[name] = {"layers": layers, "head_alone": head_alone(p, o.reps), "decode_step": decode_steps(p, layers, o.steps)}
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
