"""Mamba2 models (Codestral-Mamba) on the HIP path: reference mamba.py:23-83, which hands the whole model to the external
`mamba_ssm` package.  Here the layer stack is `mi_forward_mamba` of libmistral_hip (csrc/mamba.hip, include/mistral_hip.h
"Mamba2" states the rule); this module owns the weights, the per-layer states and the workspace.

The checkpoint key names and the fixed dimensions are mamba_ssm 2.x's as far as they are known here: compatibility with a real
Codestral-Mamba folder has not been checked.  KEYS below is the one table a correction would touch.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Dict, List, Optional, Union

import safetensors
import safetensors.torch
import torch

from . import _hip
from .args import MambaArgs

D_STATE, D_CONV, EXPAND, HEADDIM, EPS = 128, 4, 2, 64, 1e-5

# checkpoint key -> (field, dtype on the device).  `{i}`: the layer index.  dt_bias, A_log and D become fp32 once, at load.
KEYS = {
    "model.backbone.embedding.weight": ("embedding", torch.bfloat16),
    "model.backbone.layers.{i}.norm.weight": ("norm", torch.bfloat16),
    "model.backbone.layers.{i}.mixer.in_proj.weight": ("in_proj", torch.bfloat16),
    "model.backbone.layers.{i}.mixer.conv1d.weight": ("conv_w", torch.bfloat16),
    "model.backbone.layers.{i}.mixer.conv1d.bias": ("conv_b", torch.bfloat16),
    "model.backbone.layers.{i}.mixer.dt_bias": ("dt_bias", torch.float32),
    "model.backbone.layers.{i}.mixer.A_log": ("A_log", torch.float32),
    "model.backbone.layers.{i}.mixer.D": ("D", torch.float32),
    "model.backbone.layers.{i}.mixer.norm.weight": ("gated_norm", torch.bfloat16),
    "model.backbone.layers.{i}.mixer.out_proj.weight": ("out_proj", torch.bfloat16),
    "model.backbone.norm_f.weight": ("norm_f", torch.bfloat16),
    "model.lm_head.weight": ("lm_head", torch.bfloat16),
}


class MambaDims:
    """Everything that follows from MambaArgs and the fixed Mamba2 defaults."""

    def __init__(self, args: MambaArgs):
        self.D = args.dim
        self.I = EXPAND * args.dim
        self.H = self.I // HEADDIM
        self.G = args.n_groups
        self.conv_dim = self.I + 2 * self.G * D_STATE
        self.in_proj_rows = 2 * self.I + 2 * self.G * D_STATE + self.H
        m = max(1, args.pad_vocab_size_multiple)
        self.V = (args.vocab_size + m - 1) // m * m

    def shapes(self) -> Dict[str, tuple]:
        return {"embedding": (self.V, self.D), "norm": (self.D,), "in_proj": (self.in_proj_rows, self.D),
                "conv_w": (self.conv_dim, 1, D_CONV), "conv_b": (self.conv_dim,), "dt_bias": (self.H,), "A_log": (self.H,),
                "D": (self.H,), "gated_norm": (self.I,), "out_proj": (self.D, self.I), "norm_f": (self.D,), "lm_head": (self.V, self.D)}


def check_args(args: MambaArgs, dtype: Optional[torch.dtype] = torch.bfloat16, num_pipeline_ranks: int = 1) -> None:
    """The forms the kernels do not take, refused by name before anything is loaded."""
    if not args.rms_norm:
        raise NotImplementedError("Mamba with rms_norm=False (LayerNorm) is not implemented (MI_ERR_UNSUPPORTED)")
    if not args.residual_in_fp32:
        raise NotImplementedError("Mamba with residual_in_fp32=False is not implemented: the residual stream is fp32 (MI_ERR_UNSUPPORTED)")
    if args.tie_embeddings:
        raise NotImplementedError("Mamba with tie_embeddings=True is not implemented (MI_ERR_UNSUPPORTED)")
    if args.dim % 64 != 0:
        raise NotImplementedError(f"Mamba dim {args.dim} is not a multiple of 64 (MI_ERR_SHAPE)")
    H = EXPAND * args.dim // HEADDIM
    if args.n_groups <= 0 or H % args.n_groups != 0:
        raise NotImplementedError(f"Mamba n_heads {H} % n_groups {args.n_groups} != 0 (MI_ERR_SHAPE)")
    if dtype not in (None, torch.bfloat16):
        raise NotImplementedError(f"Mamba with {dtype} storage is not implemented: the kernels are bf16 (MI_ERR_UNSUPPORTED)")
    if num_pipeline_ranks != 1:
        raise NotImplementedError(f"Mamba across pipeline ranks (num_pipeline_ranks = {num_pipeline_ranks}) is not implemented (MI_ERR_UNSUPPORTED)")


def map_state_dict(loaded: Dict[str, torch.Tensor], args: MambaArgs) -> Dict[str, object]:
    """Strict: every key of KEYS for every layer must be there with its shape, and nothing else.  Returns
    {"embedding", "norm_f", "lm_head": tensor, "layers": [{field: tensor}]} in the dtypes of KEYS."""
    dims, shapes = MambaDims(args), MambaDims(args).shapes()
    out: Dict[str, object] = {"layers": [dict() for _ in range(args.n_layers)]}
    expected = {}
    for pat, (field, dt) in KEYS.items():
        for i in (range(args.n_layers) if "{i}" in pat else [None]):
            expected[pat.format(i=i)] = (field, dt, i)
    missing = sorted(set(expected) - set(loaded))
    unexpected = sorted(set(loaded) - set(expected))
    if missing or unexpected:
        raise RuntimeError(f"Mamba checkpoint: missing key(s) {missing}; unexpected key(s) {unexpected}")
    for key, (field, dt, i) in expected.items():
        t = loaded[key]
        if tuple(t.shape) != shapes[field]:
            raise RuntimeError(f"Mamba checkpoint: {key} has shape {tuple(t.shape)}, expected {shapes[field]} "
                               f"(dim {dims.D}, n_groups {dims.G}, padded vocabulary {dims.V})")
        t = t.to(dt).contiguous()
        if i is None:
            out[field] = t
        else:
            out["layers"][i][field] = t
    return out


class MambaCache:
    """The per-layer states of `batch` sequences: the conv state (the last 3 raw xBC rows, bf16 [batch, 3, conv_dim], oldest first)
    and the SSM state (fp32 [batch, H, 64, 128]).  Zeros = a fresh sequence."""

    def __init__(self, model: "Mamba", batch: int):
        d = model.dims
        self.batch = batch
        self.conv = [torch.zeros((batch, D_CONV - 1, d.conv_dim), dtype=torch.bfloat16, device=model.device) for _ in range(model.args.n_layers)]
        self.ssm = [torch.zeros((batch, d.H, HEADDIM, D_STATE), dtype=torch.float32, device=model.device) for _ in range(model.args.n_layers)]
        self.seqlen = 0

    def reset(self) -> None:
        for t in self.conv + self.ssm:
            t.zero_()
        self.seqlen = 0


class Mamba:
    def __init__(self, args: MambaArgs, weights: Dict[str, object], device: Union[torch.device, str] = "cuda"):
        check_args(args)
        self.args = args
        self.dims = MambaDims(args)
        self._device = torch.device(device)
        self._w = {k: (v.to(self._device) if k != "layers" else [{f: t.to(self._device) for f, t in ly.items()} for ly in v])
                   for k, v in weights.items()}
        self._layers = (_hip.MiMambaLayer * args.n_layers)()
        for i, ly in enumerate(self._w["layers"]):
            for f, t in ly.items():
                setattr(self._layers[i], f, _hip.dev_ptr(t, t.dtype))
        self._model = _hip.MiMambaModel(dim=args.dim, n_layers=args.n_layers, vocab_size=self.dims.V, n_groups=args.n_groups, eps=EPS,
                                        embedding=_hip.dev_ptr(self._w["embedding"]), norm_f=_hip.dev_ptr(self._w["norm_f"]),
                                        lm_head=_hip.dev_ptr(self._w["lm_head"]),
                                        layers=C.cast(self._layers, C.POINTER(_hip.MiMambaLayer)))
        self._workspace: Optional[torch.Tensor] = None

    @property
    def dtype(self) -> torch.dtype:
        return torch.bfloat16

    @property
    def device(self) -> torch.device:
        return self._w["embedding"].device

    def _workspace_for(self, B: int, L: int) -> torch.Tensor:
        need = _hip.lib().mi_workspace_bytes_mamba(C.byref(self._model), B, L)
        if need == 0:
            raise RuntimeError(f"mi_workspace_bytes_mamba: {_hip.lib().mi_last_error_detail().decode()}")
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    @torch.inference_mode()
    def forward(self, input_ids: torch.Tensor, seqlens: Optional[List[int]] = None, cache: Optional[MambaCache] = None,
                last_only: bool = False) -> torch.Tensor:
        """input_ids [B, L] -> fp32 logits [B, L, V] over the padded vocabulary ([B, V] with last_only).  With a cache the call
        continues from its states and updates them; without one it starts from zeros, as the reference does (`seqlens` is
        accepted and ignored, as there: every sequence has L tokens)."""
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
        B, L = input_ids.shape
        _hip.check_ids_on_host(input_ids, self.dims.V)
        ids = input_ids.to(device=self.device, dtype=torch.long).contiguous()
        if cache is None:
            cache = MambaCache(self, B)
        if cache.batch != B:
            raise ValueError(f"MambaCache of {cache.batch} sequences used with a batch of {B}")
        ws = self._workspace_for(B, L)
        logits = torch.empty((B, self.dims.V) if last_only else (B, L, self.dims.V), dtype=torch.float32, device=self.device)
        n = self.args.n_layers
        conv = (C.c_void_p * n)(*[_hip.dev_ptr(t) for t in cache.conv])
        ssm = (C.c_void_p * n)(*[_hip.dev_ptr(t, torch.float32) for t in cache.ssm])
        bt = _hip.MiMambaBatch(ids=_hip.dev_ptr(ids, torch.long), B=B, L=L, conv_state=C.cast(conv, C.POINTER(C.c_void_p)),
                               ssm_state=C.cast(ssm, C.POINTER(C.c_void_p)), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                               logits=_hip.dev_ptr(logits, torch.float32), last_only=int(last_only))
        _hip.check(_hip.lib().mi_forward_mamba(C.byref(self._model), C.byref(bt), _hip.stream_ptr(self.device)), "mi_forward_mamba")
        cache.seqlen += L
        return logits

    __call__ = forward

    @staticmethod
    def from_folder(folder: Union[Path, str], max_batch_size: int = 1, num_pipeline_ranks: int = 1,
                    device: Union[torch.device, str] = "cuda", dtype: Optional[torch.dtype] = None) -> "Mamba":
        with open(Path(folder) / "params.json", "r") as f:
            args = MambaArgs.from_dict(json.load(f))
        check_args(args, dtype, num_pipeline_ranks)
        model_file = Path(folder) / "consolidated.safetensors"
        assert model_file.exists(), f"Make sure {model_file} exists."
        return Mamba(args, map_state_dict(safetensors.torch.load_file(str(model_file)), args), device=device)
