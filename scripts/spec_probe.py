#!/usr/bin/env python3
"""What a verify step of speculative greedy decoding costs at the Mistral-7B dims (32 layers), every ring full at 4096 slots,
one process on one box:

    python scripts/spec_probe.py [--layers 32] [--steps 64] [--only-rows M] [--sampled]

Times (HIP events on the launch stream around queued steps, median of three windows, warm-up first - the discipline of
bench.py and scripts/fp8_probe.py):
  (a) the verify step at m = 1, 2, 3, 4, 6, 8 rows of one sequence (launch by launch, nothing read back between steps);
  (b) the plain decode step on the persistent engine, batch 1;
  (c) the plain decode step on the launch path (engine off), batch 1 and batch m for the same m;
  (d) the attention of ONE layer for each: mi_attn_verify at m rows, mi_attn_decode at batch 1 and batch m (split + combine
      launches together).  The engine has no attention launch of its own to time.
Derived: break_even[m] = verify_ms(m) / engine_ms, the tokens a step must emit on average to match the engine; tokens/s under
an oracle drafter whose every draft is right with probability r = 0.3, 0.6, 0.9 independently (k = m - 1 drafts: a step emits
(1 - r^m) / (1 - r) tokens on average) - arithmetic on the measured step times, NOT a measured acceptance: the weights are
random and say nothing about how often a real model confirms a prompt-lookup draft.  Prints one JSON line.
The per-layer attention figures of (d) come from Python calls of the leaves and are bound below by the host's ~19 us per call;
`--only-rows M` runs nothing but the verify step at M rows and the launch-path decode step at batch M: the form to put under
`rocprofv3 --kernel-trace --stats -- python scripts/spec_probe.py --only-rows 8 --steps 16` for the per-kernel table.
`--sampled` runs nothing but (e): the verify step at m = 1, 4, 8 rows with the greedy tail (argmax + acceptance) and with the
sampled one (temperature 0.7, top-p 0.8: accept / residual draw per row + scan), alternating greedy, sampled, greedy, sampled on
the same full wrapped rings, and their difference.  The ids are random and the weights too (a nucleus of thousands of tokens),
so nearly every drafted row rejects and draws: the sampled tail at its dearest."""
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
from mistral_inference.transformer import Transformer  # noqa: E402

DEV = "cuda:0"
W = 4096
SEEN = 2 * W + 100           # every ring full and wrapped
ROWS = [1, 2, 3, 4, 6, 8]
RATES = [0.3, 0.6, 0.9]
SAMPLED_ROWS = [1, 4, 8]
DIMS = dict(dim=4096, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=32768, sliding_window=W)


def build(layers: int):
    a = TransformerArgs.from_dict(dict(DIMS, n_layers=layers))
    a.max_batch_size = max(ROWS)
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            else:
                t.normal_(0.0, t.shape[-1] ** -0.5, generator=g)
    m._weights_changed()
    return m.eval()


def full_cache(model, B: int) -> BufferCache:
    """B sequences with SEEN positions behind them: rings of random K/V (timing only), every slot in use."""
    a = model.args
    cache = BufferCache(model.n_local_layers, B, SEEN + 4096, a.n_kv_heads, a.head_dim, W, device=DEV, dtype=torch.bfloat16)
    assert set(cache.cache_sizes) == {W}
    g = torch.Generator(device=DEV).manual_seed(2)
    for i in range(cache.n_layers):
        cache.cache_k[i].normal_(generator=g)
        cache.cache_v[i].normal_(generator=g)
    cache.init_kvseqlens(B)
    cache.kv_seqlens.fill_(SEEN)
    cache._seen = [SEEN] * B
    return cache


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


def verify_step_ms(model, m: int, steps: int, temperature: float = 0.0) -> float:
    cache = full_cache(model, 1)
    ids = torch.randint(0, model.args.vocab_size, (m,), generator=torch.Generator().manual_seed(m)).to(DEV)
    kw = dict(temperature=temperature, top_p=0.8, seed=1) if temperature > 0 else {}

    def run():
        for i in range(steps):
            model._verify_launch(ids, [m], cache, offset=i, **kw)   # (the host mirror stays: every step sits at the same positions)
    for _ in range(4):
        model._verify_launch(ids, [m], cache, **kw)
    torch.cuda.synchronize()
    return event_ms(run) / steps


def decode_step_ms(model, B: int, steps: int) -> float:
    cache = full_cache(model, B)
    first = torch.randint(0, model.args.vocab_size, (B,), generator=torch.Generator().manual_seed(B)).to(DEV)
    sess = model.greedy_session(cache, first)
    sess.run(8)          # warm-up: eager step, graph capture, replays
    sess.collect()
    ms = event_ms(lambda: sess.run(steps))
    sess.collect()
    return ms / steps


def attention_us(model, m: int, reps: int = 200):
    """One layer's attention launches: verify at m rows, decode at batch m."""
    a = model.args
    H, Hkv, Dh = a.n_heads, a.n_kv_heads, a.head_dim
    g = torch.Generator(device=DEV).manual_seed(3)
    ring = lambda B: torch.empty((B, Hkv, W, Dh), device=DEV, dtype=torch.bfloat16).normal_(generator=g).permute(0, 2, 1, 3)  # noqa: E731
    qkv = torch.empty((m, (H + 2 * Hkv) * Dh), device=DEV, dtype=torch.bfloat16).normal_(generator=g)
    k1, v1, km, vm = ring(1), ring(1), ring(m), ring(m)
    q_start = torch.tensor([0, m], dtype=torch.int32, device=DEV)
    kv_before = torch.tensor([SEEN], dtype=torch.int32, device=DEV)
    pos = torch.full((m,), SEEN, dtype=torch.int32, device=DEV)
    verify = lambda: [_hip.attn_verify(qkv, H, k1, v1, q_start, kv_before, 1) for _ in range(reps)]  # noqa: E731
    decode = lambda: [_hip.attn_decode(qkv, km, vm, H, pos) for _ in range(reps)]  # noqa: E731
    verify(), decode()
    torch.cuda.synchronize()
    return event_ms(verify) * 1e3 / reps, event_ms(decode) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--only-rows", type=int, default=0)
    ap.add_argument("--sampled", action="store_true")
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_probe: no HIP device (timings come from the GPU only)")
    out = {"layers": o.layers, "steps": o.steps, "ring_slots": W, "seen": SEEN}
    r3 = lambda x: round(x, 4)  # noqa: E731
    with torch.inference_mode():
        model = build(o.layers)
        if o.sampled:
            _hip.set_decode_engine(False)
            res = {"rows": SAMPLED_ROWS, "temperature": 0.7, "top_p": 0.8}
            for rnd in ("", "_again"):
                for name, t in (("greedy", 0.0), ("sampled", 0.7)):
                    res[name + "_verify_ms" + rnd] = {str(m): r3(verify_step_ms(model, m, o.steps, t)) for m in SAMPLED_ROWS}
            res["sampled_minus_greedy_ms"] = {str(m): r3(res["sampled_verify_ms"][str(m)] - res["greedy_verify_ms"][str(m)]) for m in SAMPLED_ROWS}
            res["sampled_minus_greedy_ms_again"] = {
                str(m): r3(res["sampled_verify_ms_again"][str(m)] - res["greedy_verify_ms_again"][str(m)]) for m in SAMPLED_ROWS}
            print(json.dumps(dict(out, **res)))
            return
        if o.only_rows:
            _hip.set_decode_engine(False)
            m = o.only_rows
            print(json.dumps({"rows": m, "verify_ms": r3(verify_step_ms(model, m, o.steps)), "launch_ms": r3(decode_step_ms(model, m, o.steps))}))
            return
        prev = _hip.set_decode_engine(True)
        out["engine_ms_b1"] = r3(decode_step_ms(model, 1, o.steps))
        out["engine_launches"] = _hip.decode_engine_status(model._backend._workspace)["engine_launches"]
        _hip.set_decode_engine(False)
        out["launch_ms"] = {str(m): r3(decode_step_ms(model, m, o.steps)) for m in ROWS}
        out["verify_ms"] = {str(m): r3(verify_step_ms(model, m, o.steps)) for m in ROWS}
        out["launch_ms_again"] = {str(m): r3(decode_step_ms(model, m, o.steps)) for m in (1, 8)}     # the spread of a repeat
        out["verify_ms_again"] = {str(m): r3(verify_step_ms(model, m, o.steps)) for m in (1, 8)}
        _hip.set_decode_engine(prev)
        att = {m: attention_us(model, m) for m in ROWS}
        out["attn_verify_us_per_layer"] = {str(m): round(att[m][0], 2) for m in ROWS}
        out["attn_decode_us_per_layer"] = {str(m): round(att[m][1], 2) for m in ROWS}
    eng = out["engine_ms_b1"]
    out["engine_tok_s"] = round(1e3 / eng, 1)
    out["break_even_tokens_per_step"] = {str(m): round(out["verify_ms"][str(m)] / eng, 3) for m in ROWS}
    out["verify_over_launch_batch_m"] = {str(m): round(out["verify_ms"][str(m)] / out["launch_ms"][str(m)], 3) for m in ROWS}
    out["oracle_drafter_tok_s"] = {
        str(r): {str(m): round((m if r == 1 else (1 - r ** m) / (1 - r)) / out["verify_ms"][str(m)] * 1e3, 1) for m in ROWS} for r in RATES}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
