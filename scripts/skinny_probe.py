#!/usr/bin/env python3
"""Same-process, same-box A/B of the weight-streaming GEMM of 9 .. 64 rows (csrc/gemm_skinny.hip, mi_debug_set_gemm_skinny): switch
off = the tile kernels, i.e. the routes of before, interleaved with switch on.

    python scripts/skinny_probe.py [reps] [--no-steps] > profiles/skinny_probe.json.log

Part 1, per kernel: the four linears and the LM head of Mistral-7B at M = 9, 16, 32, 48, 64 and - the route's bound lifted for the
probe only - 96 and 128 rows.  Every launch of a timed window reads another copy of the weights (copies of more than 512 MB in all per
linear: nothing is served from a cache), the window is one captured graph of launches timed with events, and the figure is
microseconds per launch (median, min, max over `reps` interleaved passes) and TB/s of weight bytes.
Part 2, per step: launch-path decode steps (Transformer.forward, plain launches, events around 8 steps) of the 32-layer model at
batch 16, 32 and 64 on both routes."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))
sys.path.insert(0, ROOT)

D, HID, HEADS, KV, DH, VOCAB = 4096, 14336, 32, 8, 128, 32768
MS = [9, 16, 32, 48, 64, 96, 128]


def stats(v):
    v = sorted(v)
    return {"us": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def kernels(torch, _hip, reps):
    dev = torch.device("cuda:0")

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev, dtype=torch.float32) * scale).to(torch.bfloat16)

    # name -> (K, row counts, epilogue)
    linears = {"qkv": (D, (HEADS * DH, KV * DH, KV * DH), _hip.EPI_STORE), "wo": (D, (D,), _hip.EPI_RESIDUAL),
               "w1w3": (D, (HID, HID), _hip.EPI_SWIGLU), "w2": (HID, (D,), _hip.EPI_RESIDUAL), "head": (D, (VOCAB,), _hip.EPI_LOGITS)}
    out = {}
    for name, (K, rows, epi) in linears.items():
        nbytes = sum(rows) * K * 2
        copies = (512 << 20) // nbytes + 2
        ws = [tuple(rnd(n, K, scale=K ** -0.5) for n in rows) for _ in range(copies)]
        N = rows[0] if epi == _hip.EPI_SWIGLU else sum(rows)
        for M in MS:
            x = rnd(M, K)
            res = rnd(M, N) if epi == _hip.EPI_RESIDUAL else None
            y = torch.empty(M, N, device=dev, dtype=torch.float32 if epi == _hip.EPI_LOGITS else torch.bfloat16)
            graphs = {}
            for mode in (0, 128):
                _hip.debug_set_gemm_skinny(mode)
                for w in ws[:2]:
                    _hip.linear(x, w, epi, residual=res, out=y)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for w in ws:
                        _hip.linear(x, w, epi, residual=res, out=y)
                graphs[mode] = g
            times = {0: [], 128: []}
            for _ in range(reps):
                for mode, g in graphs.items():
                    g.replay()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[mode].append(e0.elapsed_time(e1) * 1e3 / (2 * copies))
            r = {"off": stats(times[0]), "on": stats(times[128]), "weight_bytes": nbytes, "copies": copies}
            for k in ("off", "on"):
                r[k]["TBs"] = round(nbytes / r[k]["us"] / 1e6, 3)
                r[k]["share_of_8TBs"] = round(r[k]["TBs"] / 8.0, 3)
            out[f"{name}.m{M}"] = r
            print(f"{name:5s} M={M:3d}  off {r['off']['us']:8.2f} us [{r['off']['min']:.2f} .. {r['off']['max']:.2f}] {r['off']['TBs']:.2f} TB/s   "
                  f"on {r['on']['us']:8.2f} us [{r['on']['min']:.2f} .. {r['on']['max']:.2f}] {r['on']['TBs']:.2f} TB/s", flush=True)
        del ws
        torch.cuda.empty_cache()
    _hip.debug_set_gemm_skinny(1)
    return out


def steps(torch, _hip, reps):
    import bench
    from mistral_inference.args import TransformerArgs
    from mistral_inference.cache import BufferCache
    from mistral_inference.transformer import Transformer
    dev = "cuda:0"
    args = TransformerArgs.from_dict(bench.MISTRAL_7B)
    args.max_batch_size = 64
    with torch.device("meta"):
        model = Transformer(args)
    model = model.to(torch.bfloat16).to_empty(device=dev)
    bench.init_weights_(model, seed=42)
    model._backend.invalidate()
    model.eval()
    out = {}
    with torch.inference_mode():
        for B in (16, 32, 64):
            caches = {}
            for mode in (0, 1):
                _hip.debug_set_gemm_skinny(mode)
                c = BufferCache(model.n_local_layers, B, 256, args.n_kv_heads, args.head_dim, args.sliding_window, device=dev, dtype=torch.bfloat16)
                c.reset()
                prompt = torch.randint(0, args.vocab_size, (B * 32,), generator=torch.Generator().manual_seed(B)).to(dev)
                model.forward(prompt, [32] * B, c)
                caches[mode] = c
            nxt = torch.arange(B, device=dev)
            times = {0: [], 1: []}
            for rep in range(reps + 1):
                for mode in (0, 1):
                    _hip.debug_set_gemm_skinny(mode)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(8):
                        model.forward(nxt, [1] * B, caches[mode])
                    e1.record()
                    torch.cuda.synchronize()
                    if rep:         # (the first pass warms up)
                        times[mode].append(e0.elapsed_time(e1) * 1e3 / 8)
            out[f"step.b{B}"] = {"off": stats(times[0]), "on": stats(times[1])}
            print(f"step  B={B:3d}  off {out[f'step.b{B}']['off']}  on {out[f'step.b{B}']['on']}", flush=True)
    _hip.debug_set_gemm_skinny(1)
    return out


# ---- the quantised arm (--quant): csrc/gemm_skinny_q.hip.  Switch off = dequantise + GEMM, switch on = the weight bytes streamed,
# and the bf16 linear of the same shape (switch on), all three in one process, interleaved.
QMS = [16, 32, 64]


def _quant_weights(torch, fmt, n, K, dev):
    """Random weight bytes and harmless scales of one linear: e4m3 codes below the NaN code with scale 2^-8, or any e2m1 byte with
    block scale 2^-7.  Times do not depend on the values."""
    if fmt == "w8":
        return torch.randint(0, 0x78, (n, K), device=dev, dtype=torch.uint8), torch.full((n,), 2.0 ** -8, device=dev)
    return torch.randint(0, 256, (n, K // 2), device=dev, dtype=torch.uint8), torch.full((n, K // 32), 120, device=dev, dtype=torch.uint8)


def quant_kernels(torch, _hip, reps):
    dev = torch.device("cuda:0")
    linears = {"qkv": (D, (HEADS * DH, KV * DH, KV * DH), _hip.EPI_STORE), "wo": (D, (D,), _hip.EPI_RESIDUAL),
               "w1w3": (D, (HID, HID), _hip.EPI_SWIGLU), "w2": (HID, (D,), _hip.EPI_RESIDUAL)}
    out = {}
    for name, (K, rows, epi) in linears.items():
        N = rows[0] if epi == _hip.EPI_SWIGLU else sum(rows)
        for fmt, per_weight in (("w8", 1.0), ("w4", 0.53125), ("bf16", 2.0)):
            nbytes = int(sum(rows) * K * per_weight)
            copies = (512 << 20) // nbytes + 2
            if fmt == "bf16":
                ws = [tuple((torch.randn(n, K, device=dev) * K ** -0.5).to(torch.bfloat16) for n in rows) for _ in range(copies)]
                call = lambda x, w, res, y: _hip.linear(x, w, epi, residual=res, out=y)  # noqa: E731
            else:
                ws = [tuple(zip(*[_quant_weights(torch, fmt, n, K, dev) for n in rows])) for _ in range(copies)]
                fn = _hip.linear_w8 if fmt == "w8" else _hip.linear_w4
                call = lambda x, w, res, y: fn(x, list(w[0]), list(w[1]), epi, residual=res, out=y)  # noqa: E731
            for M in QMS:
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)
                res = torch.randn(M, N, device=dev).to(torch.bfloat16) if epi == _hip.EPI_RESIDUAL else None
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                graphs = {}
                for mode in ((64,) if fmt == "bf16" else (0, 64)):
                    _hip.debug_set_gemm_skinny(mode)
                    for w in ws[:2]:
                        call(x, w, res, y)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for w in ws:
                            call(x, w, res, y)
                    graphs[mode] = g
                times = {m: [] for m in graphs}
                for _ in range(reps):
                    for mode, g in graphs.items():
                        g.replay()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        g.replay()
                        g.replay()
                        e1.record()
                        torch.cuda.synchronize()
                        times[mode].append(e0.elapsed_time(e1) * 1e3 / (2 * copies))
                r = {("off" if m == 0 else "on"): stats(t) for m, t in times.items()}
                r["weight_bytes"] = nbytes
                r["on"]["TBs"] = round(nbytes / r["on"]["us"] / 1e6, 3)
                out[f"{name}.{fmt}.m{M}"] = r
                print(f"{name:5s} {fmt:4s} M={M:3d}  " + "  ".join(f"{k} {v['us']:8.2f} us [{v['min']:.2f} .. {v['max']:.2f}]"
                                                                 for k, v in r.items() if isinstance(v, dict)) + f"  on {r['on']['TBs']:.2f} TB/s", flush=True)
            del ws
            torch.cuda.empty_cache()
    _hip.debug_set_gemm_skinny(1)
    return out


def quant_steps(torch, _hip, reps):
    """Launch-path decode steps of the 32-layer model at batch 16, 32, 64: FP8 and MXFP4 weights, switch off and on, and the bf16
    model (switch on), interleaved."""
    import bench
    from mistral_inference.args import QuantizationArgs, TransformerArgs
    from mistral_inference.cache import BufferCache
    from mistral_inference.transformer import Transformer
    dev = "cuda:0"
    models = {}
    for fmt, qformat in (("w8", "fp8_e4m3"), ("w4", "mxfp4"), ("bf16", None)):
        args = TransformerArgs.from_dict(bench.MISTRAL_7B)
        args.max_batch_size = 64
        if qformat:
            args.quantization = QuantizationArgs(qformat)
        with torch.device("meta"):
            model = Transformer(args)
        model = model.to(torch.bfloat16).to_empty(device=dev)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.dtype == torch.uint8:   # weight bytes / e8m0 block scales
                    p.copy_(torch.full_like(p, 120) if name.endswith("qscale_weight") else torch.randint(0, 0x78 if fmt == "w8" else 256, p.shape, device=dev, dtype=torch.uint8))
                elif p.dtype == torch.float32:
                    p.fill_(2.0 ** -8)
                elif name.endswith("norm.weight"):
                    p.fill_(1.0)
                else:
                    p.copy_(torch.randn(p.shape, device=dev) * 0.02)
        model._backend.invalidate()
        models[fmt] = model.eval()
    arms = [("w8", 0), ("w8", 1), ("w4", 0), ("w4", 1), ("bf16", 1)]
    out = {}
    with torch.inference_mode():
        for B in QMS:
            caches = {}
            for fmt, mode in arms:
                _hip.debug_set_gemm_skinny(mode)
                c = BufferCache(models[fmt].n_local_layers, B, 256, args.n_kv_heads, args.head_dim, args.sliding_window, device=dev, dtype=torch.bfloat16)
                c.reset()
                prompt = torch.randint(0, VOCAB, (B * 32,), generator=torch.Generator().manual_seed(B)).to(dev)
                models[fmt].forward(prompt, [32] * B, c)
                caches[(fmt, mode)] = c
            nxt = torch.arange(B, device=dev)
            times = {a: [] for a in arms}
            for rep in range(reps + 1):
                for fmt, mode in arms:
                    _hip.debug_set_gemm_skinny(mode)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(8):
                        models[fmt].forward(nxt, [1] * B, caches[(fmt, mode)])
                    e1.record()
                    torch.cuda.synchronize()
                    if rep:         # (the first pass warms up)
                        times[(fmt, mode)].append(e0.elapsed_time(e1) * 1e3 / 8)
            out[f"step.b{B}"] = {f"{fmt}.{'on' if mode else 'off'}": stats(t) for (fmt, mode), t in times.items()}
            print(f"step  B={B:3d}  " + "  ".join(f"{k} {v['us']:.1f}" for k, v in out[f"step.b{B}"].items()), flush=True)
    _hip.debug_set_gemm_skinny(1)
    return out


def main():
    import torch
    from mistral_inference import _hip
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(argv[0]) if argv else 5
    torch.manual_seed(1234)
    if "--quant" in sys.argv:
        res = {"device": torch.cuda.get_device_name(0), "kernels": quant_kernels(torch, _hip, reps)}
        if "--no-steps" not in sys.argv:
            res["steps"] = quant_steps(torch, _hip, reps)
        print("RESULT " + json.dumps(res))
        return
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels(torch, _hip, reps)}
    if "--no-steps" not in sys.argv:
        res["steps"] = steps(torch, _hip, reps)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
