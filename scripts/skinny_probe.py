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


def main():
    import torch
    from mistral_inference import _hip
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(argv[0]) if argv else 5
    torch.manual_seed(1234)
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels(torch, _hip, reps)}
    if "--no-steps" not in sys.argv:
        res["steps"] = steps(torch, _hip, reps)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
