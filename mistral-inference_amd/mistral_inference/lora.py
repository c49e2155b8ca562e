"""Un-merged LoRA layers (reference lora.py:12-89) over the HIP operators.

`LoRALinear` keeps the adapter beside the frozen weight - parameters `linear.weight`, `lora_A.weight`, `lora_B.weight`, the
reference's names - and its `forward` is one `mi_lora_linear` call (csrc/lora.hip) with the reference's rounding points:

    t = bf16(A x);  d = bf16(bf16(B t) * scaling);  y = bf16(bf16(W x) + d)

A model built with `params.json` `lora` runs these through `mi_forward`; `Transformer.load_lora` then copies adapters into
the existing tensors, so one set of base weights serves any number of fine-tunes.  bf16 dense models only.

Adapter banks (`Transformer.set_lora_slots`): a layer then owns `n` adapter sets in two contiguous tensors [n, rank, in] /
[n, out, rank]; `lora_A.weight` / `lora_B.weight` are views of slot 0, and `forward(..., adapters=[...])` picks a slot per
sequence inside one batch (csrc/lora.hip, the bank mode of its kernels)."""
from typing import Optional

import torch
from torch import nn

from . import _hip
from .args import LoraArgs  # noqa: F401  (re-exported: the reference defines it here, lora.py:12-19)

MAX_RANK = 64  # csrc/lora.hip: ranks that are multiples of 8 up to 64 (mistral-finetune's default is 64)


def check_rank(rank: int) -> None:
    if rank % 8 != 0 or not 8 <= rank <= MAX_RANK:
        raise NotImplementedError(f"un-merged LoRA rank {rank}: the HIP kernels take multiples of 8 up to {MAX_RANK} "
                                  "(merge the adapter with Transformer.load_lora on a model without `lora` instead)")


class LoRALinear(nn.Module):
    """Reference lora.py:22-89.  Freezing is the caller's business, as in the reference."""

    def __init__(self, in_features: int, out_features: int, rank: int, scaling: float, bias: bool = False):
        super().__init__()
        assert not bias
        check_rank(rank)
        self.in_features, self.out_features = in_features, out_features
        self.bias = bias
        self.rank, self.scaling = rank, scaling
        self.lora_A = nn.Linear(in_features, rank, bias=False)
        self.lora_B = nn.Linear(rank, out_features, bias=False)
        self.linear = nn.Linear(in_features, out_features, bias=False)

        self.register_load_state_dict_post_hook(_forgive_absent_adapters)
        # adapter bank (set_slots): [n, rank, in] / [n, out, rank]; None: one slot, the two parameters above own their storage
        self.bank_A: Optional[torch.Tensor] = None
        self.bank_B: Optional[torch.Tensor] = None

    @property
    def slots(self) -> int:
        return 1 if self.bank_A is None else int(self.bank_A.shape[0])

    @torch.no_grad()
    def set_slots(self, n: int) -> None:
        """A bank of `n` adapter sets: slot 0 carries the current adapters, the others are zero (the base model).  `lora_A.weight`
        / `lora_B.weight` stay parameters of the same names and shapes - views of slot 0 - so state_dict(), load_state_dict(),
        copies into them and `forward` (slot 0) behave as without a bank.  The frozen weight is not touched.  Called again
        (to grow or shrink the bank), the slots that both banks have keep their adapters; the tensors are new ones."""
        if n < 1:
            raise ValueError(f"set_slots({n}): a bank has at least one slot")
        a, b = self.lora_A.weight, self.lora_B.weight
        bank_a = torch.zeros((n, *a.shape), dtype=a.dtype, device=a.device)
        bank_b = torch.zeros((n, *b.shape), dtype=b.dtype, device=b.device)
        if self.bank_A is not None and self.bank_B is not None and self.bank_is_bound():
            keep = min(n, self.slots)
            bank_a[:keep].copy_(self.bank_A[:keep])
            bank_b[:keep].copy_(self.bank_B[:keep])
        bank_a[0].copy_(a)   # (slot 0 is whatever the two parameters hold now, bound to the old bank or not)
        bank_b[0].copy_(b)
        self.bank_A, self.bank_B = bank_a, bank_b
        self._bind_slot0()

    def _bind_slot0(self) -> None:
        assert self.bank_A is not None and self.bank_B is not None
        for lin, bank in ((self.lora_A, self.bank_A), (self.lora_B, self.bank_B)):
            lin.weight = nn.Parameter(bank[0], requires_grad=lin.weight.requires_grad and bank.is_floating_point())

    def bank_is_bound(self) -> bool:
        """False after something REBOUND lora_A.weight / lora_B.weight (load_state_dict(assign=True)): slot 0 of the bank is then
        stale and set_slots has to be called again."""
        return self.bank_A is None or (self.lora_A.weight.data_ptr() == self.bank_A.data_ptr()
                                       and self.lora_B.weight.data_ptr() == self.bank_B.data_ptr())

    def _apply(self, fn, *a, **k):  # .to() / dtype casts: the bank moves as one tensor and the two parameters are re-viewed
        out = super()._apply(fn, *a, **k)
        if self.bank_A is not None:
            self.bank_A, self.bank_B = fn(self.bank_A), fn(self.bank_B)
            self._bind_slot0()
        return out

    @property
    def weight(self) -> torch.Tensor:
        """The frozen weight (what callers of a plain nn.Linear read)."""
        return self.linear.weight

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, x.shape[-1])
        out = _hip.lora_linear(x2, (self.linear.weight,), (self.lora_A.weight,), (self.lora_B.weight,), self.scaling)
        return out.view(*x.shape[:-1], self.out_features)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Base checkpoints name the frozen matrix `<prefix>weight`.  This module owns no such parameter, so torch would neither
        load nor report it: take it here as `linear.weight` and start both adapters at zero (the layer then computes the base
        model).  The un-merged key form (`<prefix>linear.weight`, `<prefix>lora_A.weight`, ...) needs nothing from this method -
        torch loads it child by child."""
        self._load_prefix, self._took_plain_key = prefix, False   # read by the post-hook of the same load
        plain = state_dict.get(prefix + "weight")
        if plain is None:
            return
        if tuple(plain.shape) != tuple(self.linear.weight.shape):
            error_msgs.append(f"size mismatch for {prefix}weight: checkpoint {tuple(plain.shape)}, model {tuple(self.linear.weight.shape)}")
            return
        rebind = bool(local_metadata.get("assign_to_params_buffers", False))
        with torch.no_grad():
            for child, value in ((self.linear, plain), (self.lora_A, None), (self.lora_B, None)):
                if rebind or child.weight.is_meta:
                    new = value if value is not None else torch.zeros(child.weight.shape, dtype=plain.dtype, device=plain.device)
                    child.weight = nn.Parameter(new, requires_grad=child.weight.requires_grad and new.is_floating_point())
                elif value is not None:
                    child.weight.copy_(value)
                else:
                    child.weight.zero_()
        self._took_plain_key = True


def _forgive_absent_adapters(module: "LoRALinear", incompatible_keys) -> None:
    """load_state_dict post-hook of a LoRALinear: a checkpoint without this layer's adapters is a base checkpoint, not a broken
    one, and after a plain `<prefix>weight` key was taken all three parameters are set.  Only THIS module's keys are forgiven:
    what another module misses is still reported."""
    prefix = module.__dict__.pop("_load_prefix", "")
    names = ["lora_A.weight", "lora_B.weight"] + (["linear.weight"] if module.__dict__.pop("_took_plain_key", False) else [])
    forgiven = {prefix + n for n in names}
    incompatible_keys.missing_keys[:] = [k for k in incompatible_keys.missing_keys if k not in forgiven]


def maybe_lora(lora: "LoraArgs | None"):
    """nn.Linear, or LoRALinear bound to the adapter's rank and scaling (reference transformer_layers.py:22-27)."""
    if lora is None:
        return nn.Linear
    from functools import partial
    return partial(LoRALinear, rank=lora.rank, scaling=lora.scaling)
