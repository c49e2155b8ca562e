"""Shared by the un-merged LoRA tests and their golden recipe (tests/make_golden_lora.py): the numerics contract of a LoRA linear
restated in torch, the seeded adapter generator, and the loader of tests/golden/lora_*.safetensors."""
import json
import os

import torch
import torch.nn.functional as F

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LORA_INDEX = os.path.join(GOLDEN, "lora_index.json")
LINEARS = ("attention.wq", "attention.wk", "attention.wv", "attention.wo", "feed_forward.w1", "feed_forward.w2", "feed_forward.w3")


def _mm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x @ w^T on bf16 tensors with fp32 accumulation, NOT rounded."""
    return F.linear(x.float(), w.float())


def lora_linear_ref(x, w, a, b, s, t_fp32: bool = False, parts: bool = False):
    """Reference lora.py:71-74 on bf16 tensors, every rounding point written out:
        t = bf16(A x);  d = bf16(bf16(B t) * s);  y = bf16(bf16(W x) + d).
    t_fp32 (a mutant for the tests): t is kept in fp32.  parts: returns (y, bf16(W x), d) instead of y."""
    t = _mm(x, a)
    t = t if t_fp32 else t.to(BF).float()
    bt = F.linear(t, b.float()).to(BF)
    d = (bt.float() * float(s)).to(BF)
    base = _mm(x, w).to(BF)
    y = (base.float() + d.float()).to(BF)
    return (y, base, d) if parts else y


def linear_dims(p: dict) -> dict:
    """(in, out) of the seven linears of a layer from params.json fields."""
    nq, nkv, D, Fh = p["n_heads"] * p["head_dim"], p["n_kv_heads"] * p["head_dim"], p["dim"], p["hidden_dim"]
    return {"attention.wq": (D, nq), "attention.wk": (D, nkv), "attention.wv": (D, nkv), "attention.wo": (nq, D),
            "feed_forward.w1": (D, Fh), "feed_forward.w2": (Fh, D), "feed_forward.w3": (D, Fh)}


def make_adapters(p: dict, rank: int, seed: int, b_factor: float = 0.25) -> dict:
    """Adapters of every linear of every layer from one seeded CPU generator, in a fixed order:
    A [rank, in] ~ N(0, 1 / in), B [out, rank] ~ b_factor * N(0, 1 / rank) (rank is B's `in`), both bf16."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for layer in range(p["n_layers"]):
        for name in LINEARS:
            fin, fout = linear_dims(p)[name]
            out[f"layers.{layer}.{name}.lora_A.weight"] = (torch.randn(rank, fin, generator=g) / fin ** 0.5).to(BF)
            out[f"layers.{layer}.{name}.lora_B.weight"] = (b_factor * torch.randn(fout, rank, generator=g) / rank ** 0.5).to(BF)
    return out


def checksum(tensors: dict) -> float:
    return float(sum(v.double().abs().sum().item() for v in tensors.values()))


def lora_index() -> dict:
    with open(LORA_INDEX) as f:
        return json.load(f)


class LoraCase:
    """One case of tests/golden/lora_index.json: reference outputs in lora_<name>.safetensors, the adapters of layer l in
    lora_<name>.adapters.<l>.safetensors."""

    def __init__(self, name: str):
        from safetensors.torch import load_file
        import mistral_oracle as mo
        self.name = name
        self.meta = lora_index()[name]
        self.params = self.meta["params"]
        self.t = load_file(os.path.join(GOLDEN, f"{name}.safetensors"))
        self.adapters = {}
        for layer in range(self.params["n_layers"]):
            self.adapters.update(load_file(os.path.join(GOLDEN, f"{name}.adapters.{layer}.safetensors")))
        assert checksum(self.adapters) == self.meta["adapters_checksum"], "adapter fixtures do not match their checksum"
        self.prompts, self.max_tokens, self.chunk_size = self.meta["prompts"], self.meta["max_tokens"], self.meta["chunk_size"]
        self.max_batch_size = self.meta["max_batch_size"]
        base = {k: v for k, v in self.params.items() if k != "lora"}
        self.args = mo.OracleArgs.from_params(base)  # (the oracle knows no adapters: dims and the base weights only)

    def weights(self):
        import mistral_oracle as mo
        w = mo.synth_weights(self.args, seed=self.meta["seed"], dtype=BF)
        assert checksum(w) == self.meta["weights_checksum"], "synthetic weights no longer regenerate bit-identically"
        return w

    def tokens(self):
        return self.t["tokens"].tolist()

    def logprobs(self):
        return [[x for x in row.tolist() if x == x] for row in self.t["logprobs"]]

    def schedule(self):
        """Sequence lengths of every forward of the case: the prefill chunks, then the decode steps."""
        lens = [len(p) for p in self.prompts]
        chunk = self.chunk_size or max(lens)
        pre = [[len(p[s:s + chunk]) for p in self.prompts] for s in range(0, max(lens), chunk)]
        return pre, len(self.tokens()[0])


def write_lora_checkpoint(folder, case_params: dict, weights: dict) -> str:
    """params.json (with its `lora` block) + a base checkpoint in the plain `<name>.weight` key form."""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "params.json"), "w") as f:
        json.dump(case_params, f)
    save_file({k: v.contiguous() for k, v in weights.items()}, os.path.join(folder, "consolidated.safetensors"))
    return str(folder)
