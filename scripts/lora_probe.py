#!/usr/bin/env python3
"""What un-merged LoRA costs at the Mistral-7B dims (32 layers, rank 64), one process on one box:

    python scripts/lora_probe.py [--layers 32] [--rank 64] [--steps 64] [--only-lora-step] [--slots 3 --mix "none;0,0,0;0,1,2"]

Times (HIP events on the launch stream; warm-up first: the first steps size the workspace, capture the decode graph and, for the
engine, run its residency census - same discipline as bench.py):
  * the decode step of the LoRA model, batch 1 and batch 3 (launch path: the engine declines adapters);
  * the same dims without adapters ("merged": a merged adapter is a plain weight) on the launch path (engine off) and, batch 1,
    on the persistent engine;
  * a 4096-token prefill, LoRA and merged.
Weights are random (timing only).  `--only-lora-step` runs nothing but the LoRA model's decode steps: the form to put under
`rocprofv3 --kernel-trace --stats -- python scripts/lora_probe.py --only-lora-step` for the per-kernel table.
`--slots S --mix ...` runs nothing but the LoRA model's decode steps with a bank of S adapter sets, once per mix (";"-separated;
a mix is one adapter slot per sequence, -1 = no adapter, or "none" = `adapters=None`: slot 0 in the kernels' single-adapter mode) -
what one adapter per sequence costs over one adapter per batch: `lora_step_us[<mix>]`.
Prints one JSON line."""
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


def build(layers: int, rank: int):
    p = dict(dim=4096, n_layers=layers, head_dim=128, hidden_dim=14336, n_heads=32, n_kv_heads=8, norm_eps=1e-5, vocab_size=32768)
    if rank:
        p["lora"] = dict(rank=rank, scaling=2.0)
    a = TransformerArgs.from_dict(p)
    a.max_batch_size = 3
    with torch.device("meta"):
        m = Transformer(a)
    m = m.to(torch.bfloat16).to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for name, t in m.named_parameters():
            if name.endswith("norm.weight"):
                t.fill_(1.0)
            else:
                t.normal_(0.0, 0.25 * t.shape[-1] ** -0.5 if "lora_B" in name else t.shape[-1] ** -0.5, generator=g)
    return m.eval()


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


def decode_step_us(model, B: int, steps: int, **fwd) -> float:
    """fwd: `adapters=...` of the prefill; the session's steps run with the same choice."""
    a = model.args
    cache = BufferCache(model.n_local_layers, 3, 4096, a.n_kv_heads, a.head_dim, None, device=DEV, dtype=torch.bfloat16)
    cache.reset()
    ids = torch.randint(0, a.vocab_size, (32 * B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    logits = model.forward(ids, [32] * B, cache, **fwd)
    first = logits[torch.arange(B, device=DEV) * 32 + 31].argmax(-1)
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
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--only-lora-step", action="store_true")
    ap.add_argument("--slots", type=int, default=1, help="adapter sets per LoRA linear (Transformer.set_lora_slots)")
    ap.add_argument("--mix", default="", help='";"-separated mixes, each "none" or one slot per sequence: "none;0,0,0;0,1,2"')
    o = ap.parse_args()
    out = {"layers": o.layers, "rank": o.rank, "steps": o.steps}
    lora = build(o.layers, o.rank)
    if o.mix:
        out["slots"] = o.slots
        if o.slots > 1:
            lora.set_lora_slots(o.slots)
            g = torch.Generator(device=DEV).manual_seed(2)
            with torch.no_grad():
                for mod in lora.modules():   # (timing only: every slot gets adapters of the usual scale)
                    if getattr(mod, "bank_A", None) is not None:
                        mod.bank_A[1:].normal_(0.0, mod.in_features ** -0.5, generator=g)
                        mod.bank_B[1:].normal_(0.0, 0.25 * mod.rank ** -0.5, generator=g)
        for mix in o.mix.split(";"):
            adapters = None if mix == "none" else [int(x) for x in mix.split(",")]
            out[f"lora_step_us[{mix}]"] = round(decode_step_us(lora, 3 if adapters is None else len(adapters), o.steps, adapters=adapters), 1)
        print(json.dumps(out))
        return
    out["lora_step_us_b1"] = round(decode_step_us(lora, 1, o.steps), 1)
    if not o.only_lora_step:
        out["lora_step_us_b3"] = round(decode_step_us(lora, 3, o.steps), 1)
        out["lora_prefill4096_ms"] = round(prefill_ms(lora), 2)
        st = _hip.decode_engine_status(lora._backend._workspace)
        out["lora_engine_launches"] = st["engine_launches"]
        del lora
        torch.cuda.empty_cache()
        plain = build(o.layers, 0)
        prev = _hip.set_decode_engine(False)
        out["merged_launch_step_us_b1"] = round(decode_step_us(plain, 1, o.steps), 1)
        out["merged_launch_step_us_b3"] = round(decode_step_us(plain, 3, o.steps), 1)
        _hip.set_decode_engine(True)
        out["merged_engine_step_us_b1"] = round(decode_step_us(plain, 1, o.steps), 1)
        out["merged_engine_launches"] = _hip.decode_engine_status(plain._backend._workspace)["engine_launches"]
        _hip.set_decode_engine(prev)
        out["merged_prefill4096_ms"] = round(prefill_ms(plain), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
