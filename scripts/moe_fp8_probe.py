#!/usr/bin/env python3
"""What FP8 (e4m3) experts buy at the Mixtral-8x7B dims, both models resident in one process on one box:

    python scripts/moe_fp8_probe.py [--layers 4] [--steps 64] [--rounds 3] [--only-fp8-step | --prefill-routes]

The bf16 MoE model and the FP8 one (attention linears and experts e4m3, `quantization.experts`) are built with the same
number of layers (4 by default: 11.8 GB + 6.0 GB; 32 layers of bf16 experts alone are 90 GB) and timed ALTERNATELY - bf16, FP8,
bf16, FP8 ... for `--rounds` rounds, the median of each arm reported beside every round - so that clock and neighbour drift of
a shared box falls on both arms alike.  HIP events on the launch stream around queued steps, warm-up first (workspace sizing and
graph capture), as scripts/fp8_probe.py.  Both arms on the launch path (engine off): the engine declines e4m3 weights.
  (a) the decode step at batch 1 and 3;   (b) a 2048-token prefill (FP8: one dequantisation launch per projection family of all
  experts in front of each token-grouped GEMM);   (c) the bytes a batch-1 step must read - the top_k chosen experts, the attention
  linears, the router, the LM head, the K/V rings - and the fraction of 8 TB/s each step time stands for.
Weights are random (timing only; no claim about model quality).  `--only-fp8-step`: nothing but the FP8 model's batch-1 decode
steps, the form to put under `rocprofv3 --kernel-trace --stats -- python scripts/moe_fp8_probe.py --only-fp8-step`.
`--prefill-routes`: nothing but prefills of 256, 2048 and 4096 tokens on three arms timed alternately in one process - the bf16
model, the FP8 model on the dequantisation route, and the same FP8 model with `prefill_fp8_experts` on (attention linears on
gemm256_w8a8, experts on the token-grouped gemm256_moe_w8a8) - and the workspace bytes of the two FP8 routes at each length.  At 256
tokens with k = 2, E = 8 an expert has 64 rows on average: mostly-empty 256-row tiles.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
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
DIMS = dict(dim=4096, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=32000,
            moe=dict(num_experts=8, num_experts_per_tok=2))


def build(layers: int, fp8: bool):
    p = dict(DIMS, n_layers=layers)
    if fp8:
        p["quantization"] = dict(qformat_weight="fp8_e4m3", experts=True)
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
    """Bytes one batch-1 decode step must read."""
    D, F, V, E, k = DIMS["dim"], DIMS["hidden_dim"], DIMS["vocab_size"], 8, 2
    nq, nkv = DIMS["n_heads"] * DIMS["head_dim"], DIMS["n_kv_heads"] * DIMS["head_dim"]
    elems = (nq + 2 * nkv) * D + D * nq + k * 3 * F * D
    rows = (nq + 2 * nkv) + D + k * (2 * F + D)
    per_layer = (elems + 4 * rows if fp8 else 2 * elems) + 2 * E * D
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


def decode_session(model, B: int):
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, 4096, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    cache.reset()
    ids = torch.randint(0, a.vocab_size, (PROMPT * B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    logits = model.forward(ids, [PROMPT] * B, cache)
    sess = model.greedy_session(cache, logits[torch.arange(B, device=DEV) * PROMPT + PROMPT - 1].argmax(-1))
    sess.run(8)          # warm-up: eager step, graph capture, replays
    sess.collect()
    return sess


def step_us(sess, steps: int) -> float:
    ms = event_ms(lambda: sess.run(steps), reps=1)
    sess.collect()
    return ms * 1000.0 / steps


def prefill_ms(model, T: int) -> float:
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, T, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    ids = torch.randint(0, a.vocab_size, (T,), generator=torch.Generator().manual_seed(0)).to(DEV)

    def run():
        cache.reset()
        model.forward_partial(ids, [T], cache)
    run()
    torch.cuda.synchronize()
    return event_ms(run, reps=1)


def prefill_routes(out, arms, n_rounds: int):
    """bf16 | FP8 dequantisation route | FP8 token-grouped W8A8 route, alternately; medians, ratios and workspace bytes.  The third
    arm is the whole switch - its attention linears run on gemm256_w8a8 too, which the second arm cannot take (refused) - so its
    ratio to the second is not the expert kernel's gain alone."""
    fp8 = arms["fp8"]
    routes = {"bf16": (arms["bf16"], False), "fp8_deq": (fp8, False), "fp8_w8a8": (fp8, True)}
    for T in (256, 2048, 4096):
        rounds = {n: [] for n in routes}
        for _ in range(n_rounds):
            for n, (m, on) in routes.items():
                if m is fp8:
                    m.prefill_fp8_experts = on
                rounds[n].append(round(prefill_ms(m, T), 2))
        for n in routes:
            out[f"{n}_prefill{T}_ms_rounds"] = rounds[n]
            out[f"{n}_prefill{T}_ms"] = statistics.median(rounds[n])
        for n in ("fp8_deq", "fp8_w8a8"):
            out[f"{n}_over_bf16_prefill{T}"] = round(out[f"{n}_prefill{T}_ms"] / out[f"bf16_prefill{T}_ms"], 3)
        out[f"fp8_w8a8_over_deq_prefill{T}"] = round(out[f"fp8_w8a8_prefill{T}_ms"] / out[f"fp8_deq_prefill{T}_ms"], 3)
        be = fp8._backend
        m, L = be.plan(fp8), _hip.lib()
        for n, q in (("fp8_deq", L.mi_workspace_bytes_moe_w8), ("fp8_w8a8", L.mi_workspace_bytes_moe_w8a8)):
            out[f"{n}_workspace_mb_T{T}"] = round(q(C.byref(m), C.byref(be._quant[0]), be._moe_q, None, T, 1, T, 0) / 1e6, 1)
    fp8.prefill_fp8_experts = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only-fp8-step", action="store_true")
    ap.add_argument("--prefill-routes", action="store_true")
    o = ap.parse_args()
    kv_len = PROMPT + 8 + o.steps * o.rounds // 2
    out = {"layers": o.layers, "steps": o.steps, "rounds": o.rounds}
    prev = _hip.set_decode_engine(False)
    with torch.inference_mode():
        arms = {"fp8": build(o.layers, True)}
        if o.only_fp8_step:
            sess = decode_session(arms["fp8"], 1)
            out["fp8_step_us_b1"] = round(step_us(sess, o.steps), 1)
            print(json.dumps(out))
            return
        arms = {"bf16": build(o.layers, False), **arms}
        if o.prefill_routes:
            prefill_routes(out, arms, o.rounds)
            print(json.dumps(out))
            return
        for B in (1, 3):
            sess = {n: decode_session(m, B) for n, m in arms.items()}
            rounds = {n: [] for n in arms}
            for _ in range(o.rounds):          # bf16, FP8, bf16, FP8, ...
                for n in arms:
                    rounds[n].append(round(step_us(sess[n], o.steps), 1))
            for n in arms:
                out[f"{n}_step_us_b{B}_rounds"] = rounds[n]
                out[f"{n}_step_us_b{B}"] = statistics.median(rounds[n])
            out[f"fp8_over_bf16_b{B}"] = round(out[f"fp8_step_us_b{B}"] / out[f"bf16_step_us_b{B}"], 3)
            del sess
        for n in arms:
            nbytes = step_bytes(o.layers, n == "fp8", kv_len)
            out[f"{n}_step_bytes_gb"] = round(nbytes / 1e9, 3)
            out[f"{n}_frac_of_8TBs_b1"] = round(nbytes / (out[f"{n}_step_us_b1"] * 1e-6) / HBM_BYTES_PER_S, 3)
        rounds = {n: [] for n in arms}
        for _ in range(o.rounds):
            for n, m in arms.items():
                rounds[n].append(round(prefill_ms(m, 2048), 2))
        for n in arms:
            out[f"{n}_prefill2048_ms_rounds"] = rounds[n]
            out[f"{n}_prefill2048_ms"] = statistics.median(rounds[n])
        out["fp8_over_bf16_prefill2048"] = round(out["fp8_prefill2048_ms"] / out["bf16_prefill2048_ms"], 3)
    _hip.set_decode_engine(prev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
