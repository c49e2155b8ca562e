#!/usr/bin/env python3
"""Generate tests/golden/lora_*.safetensors by running the UNMODIFIED reference with un-merged LoRA layers on CPU.

Run in the build container only (needs the reference source):

    python tests/make_golden_lora.py

Same discipline as oracle/make_golden.py, whose TINY dims and synthetic base weights (`synth_weights(seed=42)`) it uses: the
reference package is imported as-is through oracle/shim and every stored logit / token / log-probability is an OUTPUT of the
reference's `generate()` on a model built with `args.lora` (14 `LoRALinear` modules), the base checkpoint loaded in the plain
`<name>.weight` key form (lora.py:76-89) and the adapters assigned by `_load_lora_state_dict` (lora.py:140-155).  The adapters
come from `lora_util.make_adapters` (seeded CPU generator) and are stored beside the outputs, one file per layer, with a float64
checksum in tests/golden/lora_index.json.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("MISTRAL_REFERENCE_SRC", "/root/reference/src")
sys.path[:0] = [os.path.join(ROOT, "oracle", "shim"), REF, os.path.join(ROOT, "oracle"), HERE]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

import lora_util  # noqa: E402
import mistral_oracle as mo  # noqa: E402
from mistral_inference.args import TransformerArgs  # noqa: E402  (the reference)
from mistral_inference.cache import BufferCache  # noqa: E402
from mistral_inference.generate import generate  # noqa: E402
from mistral_inference.lora import LoRALinear  # noqa: E402
from mistral_inference.transformer import Transformer  # noqa: E402

assert os.path.realpath(sys.modules["mistral_inference"].__file__).startswith(os.path.realpath(REF)), \
    "golden vectors must come from the reference package"

OUT = os.path.join(HERE, "golden")
TINY = dict(dim=256, n_layers=2, head_dim=128, hidden_dim=512, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512)  # oracle/make_golden.py
SEED, ADAPTER_SEED, SCALING = 42, 1234, 2.0
SWA_PROMPTS = [[(3 * i + 1) % 512 for i in range(13)], [(7 * i + 2) % 512 for i in range(14)]]  # those of swa_chunk_bf16

CASES = {
    # name: (args overrides, rank, prompts, max_tokens, chunk_size)
    "lora_dense_bf16": (dict(), 16, [[1, 5, 9, 200, 17, 3, 44], [7, 300, 2], [11, 12, 13, 14, 15]], 6, None),
    "lora_swa_chunk_bf16": (dict(sliding_window=8), 8, SWA_PROMPTS, 5, 4),
    "lora_r64_bf16": (dict(), 64, [[4, 3, 2, 1, 0, 9, 8, 7, 6, 5, 4, 3]], 4, None),
}


def build(over, rank, adapters):
    """The reference model of a case; adapters None: the same model with the zero adapters of a base checkpoint."""
    p = dict(TINY)
    p.update(over)
    oargs = mo.OracleArgs.from_params(p)
    w = mo.synth_weights(oargs, seed=SEED, dtype=torch.bfloat16)
    p["lora"] = dict(rank=rank, scaling=SCALING)
    rargs = TransformerArgs.from_dict(p)
    rargs.max_batch_size = 4
    model = Transformer(rargs)
    assert sum(isinstance(m, LoRALinear) for m in model.modules()) == 7 * p["n_layers"]
    model.load_state_dict({k: v.clone() for k, v in w.items()}, assign=True, strict=True)
    model = model.to("cpu", dtype=torch.bfloat16).eval()
    if adapters is not None:
        model._load_lora_state_dict({k: v.clone() for k, v in adapters.items()})
    return p, w, model


def replay(model, prompts, tokens, chunk, max_tokens):
    """Teacher-forced logits of every forward of a case's schedule (prefill chunks, then one decode step per token)."""
    a = model.args
    lens = [len(x) for x in prompts]
    cache = BufferCache(model.n_local_layers, a.max_batch_size, max(lens) + max_tokens, a.n_kv_heads, a.head_dim, a.sliding_window)
    cache.to(device=model.device, dtype=model.dtype)
    cache.reset()
    chunk = chunk or max(lens)
    outs = []
    with torch.inference_mode():
        for s in range(0, max(lens), chunk):
            parts = [x[s:s + chunk] for x in prompts]
            outs.append(model.forward(torch.tensor(sum(parts, []), dtype=torch.long), seqlens=[len(x) for x in parts], cache=cache).float())
        for step in range(len(tokens[0])):
            outs.append(model.forward(torch.tensor([t[step] for t in tokens], dtype=torch.long), seqlens=[1] * len(tokens), cache=cache).float())
    return outs


def main(out_dir: str = OUT, only=None) -> None:
    os.makedirs(out_dir, exist_ok=True)
    index = {}
    for name, (over, rank, prompts, max_tokens, chunk) in CASES.items():
        if only is not None and name not in only:
            continue
        p0 = dict(TINY)
        p0.update(over)
        adapters = lora_util.make_adapters(p0, rank, ADAPTER_SEED)
        params, w, model = build(over, rank, adapters)
        fwd_out = []
        ref_forward = model.forward

        def observed_forward(*a, **k):
            o = ref_forward(*a, **k)
            fwd_out.append(o.detach().clone())
            return o

        model.forward = observed_forward
        with torch.inference_mode():
            toks, lps = generate(prompts, model, max_tokens=max_tokens, temperature=0.0, chunk_size=chunk)
        del model.forward
        n_chunks = 1 if chunk is None else -(-max(len(x) for x in prompts) // chunk)
        tensors = {}
        for c in range(n_chunks):
            tensors[f"prefill_logits.{c}"] = fwd_out[c].float().contiguous()
        for s in range(n_chunks, len(fwd_out)):
            tensors[f"decode_logits.{s - n_chunks}"] = fwd_out[s].float().contiguous()
        tensors["tokens"] = torch.tensor(toks, dtype=torch.int64)
        width = max(len(x) for x in lps)
        lp = torch.full((len(lps), width), float("nan"), dtype=torch.float64)
        for b, x in enumerate(lps):
            lp[b, : len(x)] = torch.tensor(x, dtype=torch.float64)
        tensors["logprobs"] = lp
        save_file(tensors, os.path.join(out_dir, f"{name}.safetensors"))
        for layer in range(params["n_layers"]):
            save_file({k: v.contiguous() for k, v in adapters.items() if k.startswith(f"layers.{layer}.")},
                      os.path.join(out_dir, f"{name}.adapters.{layer}.safetensors"))
        index[name] = {"params": params, "dtype": "bfloat16", "prompts": prompts, "max_tokens": max_tokens, "chunk_size": chunk,
                       "seed": SEED, "adapter_seed": ADAPTER_SEED, "max_batch_size": 4,
                       "weights_checksum": lora_util.checksum(w), "adapters_checksum": lora_util.checksum(adapters)}
        print(f"{name}: {len(tensors)} tensors, tokens={toks}")
    with open(os.path.join(out_dir, "lora_index.json"), "w") as f:
        json.dump(index, f, indent=1)


if __name__ == "__main__":
    main()
