"""Weight-only FP8 (OCP e4m3) linears over the HIP operators, and the quantiser that writes such checkpoints.

A quantised linear stores `weight` as e4m3fn bytes [out, in] and `qscale_weight` as fp32 [out]; the real-valued weight is
`qscale_weight[r] * e4m3(weight[r, k])`.  The reference has no quantised layer: `Fp8Linear` (a `QuantLinear`, which carries what every weight format
shares) stands where its `nn.Linear` stands (reference transformer_layers.py:51-54,101-103) and its `forward` is one
`mi_linear_w8` call (csrc/gemv_w8.hip):

    T <= 8:  acc = sum_k e4m3(W[r, k]) x[k] in fp32;  y = bf16(acc * qscale_weight[r])
    T  > 8:  W' = bf16(qscale_weight[r] * e4m3(W[r, k])) into a scratch, then the bf16 MFMA GEMM on W'

`quantize_rows` produces power-of-two row scales only; W' is then exact in bf16 and both forms compute the bf16 model on the
dequantised weights, up to fp32 summation order.  Other positive finite scales (checkpoints made elsewhere) are accepted; the
two forms then differ by one bf16 rounding of each weight.  Embeddings, norms, the LM head, the MoE gate, the vision tower and
the K/V rings stay bf16.  Dense bf16 models without un-merged LoRA only.

Checkpoint layout: `<linear>.weight` with dtype F8_E4M3, `<linear>.qscale_weight` fp32 [out] (a scalar or [1] is broadcast at
load), `params.json` with `"quantization": {"qformat_weight": "fp8_e4m3"}`.  Compatibility is claimed only with checkpoints
that `quantize_checkpoint` wrote.

MXFP4 (`qformat_weight` "mxfp4", OCP microscaling): e2m1 codes in blocks of 32 along `in`, one e8m0 scale byte per block, 4.25 bits
per weight.  `<linear>.weight` is U8 [out, in / 2], two codes per byte with the LOW nibble at the even k; `<linear>.qscale_weight`
is U8 [out, in / 32], byte b meaning 2^(b - 127) (255, the e8m0 NaN, is refused).  The real-valued weight is
`2^(b - 127) * e2m1(code)`, exact in bf16, so `Mxfp4Linear` (one `mi_linear_w4` call, csrc/gemv_w4.hip) computes the bf16 model on
the dequantised weights up to fp32 summation order, at any number of rows.  `in` must be a multiple of 32.

FP8 prefill GEMMs (`prefill_fp8=True`, FP8 e4m3 weights only, opt-in): a linear of T >= 256 rows, `in` % 128 == 0 and `in` <= 16384 quantises its
input rows too, per row (per token), by the rule of `quantize_rows` (`quantize_activations` names it):

    s_x[t] = 2^ceil(log2(amax_k |x[t, k]| / 448))  (an all-zero row: 1),   x_q[t, k] = e4m3_rne(clamp(x[t, k] / s_x[t], +-448))
    y[t, r] = bf16((sum_k e4m3(x_q[t, k]) e4m3(W[r, k])) * (s_x[t] * qscale_weight[r]))        (csrc/gemm256_w8a8.hip)

with the sum in fp32 on the FP8 MFMA and no dequantisation pass.  In front of q|k|v and w1|w3 the row quantised is the bf16 output
of the RMSNorm.  Activations keep three mantissa bits: on inputs that e4m3 holds exactly the route is lossless, on real activations
it is a different (coarser) model than the weight-only one, and nobody claims model quality for it - it ships with its measured
speed (README) and is off unless asked for.  Every other shape - decode steps, verify steps, short chunks - takes the weight-only
routes above, bit for bit.

MXFP4 x FP8 prefill GEMMs (`prefill_w4a8=True`, MXFP4 weights only, opt-in): the same on an MXFP4 model.  A linear of the same
shapes quantises its input rows by the same rule (s_x, x_q as above) and contracts them with the e2m1 codes on the mixed form of
the block-scaled MFMA, which takes the checkpoint's e8m0 bytes as its block scales:

    y[t, r] = bf16((sum_k e4m3(x_q[t, k]) * e2m1(c[r, k]) * 2^(qscale_weight[r, k / 32] - 127)) * s_x[t])   (csrc/gemm256_w4a8.hip)

with the sum in fp32 and no dequantisation pass.  On activations that e4m3 holds exactly under the row scale this is the
weight-only route up to fp32 summation order (lossless); on real activations it is a coarser model, nobody claims model quality for
it, and it is off unless asked for.  For scale bytes below 3 the weight-only route's bf16 image holds subnormals, which it may
flush and this route does not.  Every other shape takes the weight-only MXFP4 routes, bit for bit.

A quantised LM head (`quantization.lm_head`, opt-in: `quantize_checkpoint(..., lm_head=True)`, `from_folder(...,
quantize_lm_head=True)`): `output.weight` / `output.qscale_weight` in the layers' format, `model.output` the format's QuantLinear.
On quantised layers the bf16 head is the largest tensor a decode step reads (1.34 GB at vocab 131072 x dim 5120).  At T <= 8 the
head is the format's GEMV with the bf16 head's epilogue - logit = float(bf16(acc * qscale_weight[r])), MXFP4 float(bf16(acc)); above,
its bf16 image is made in slices of 8192 vocabulary rows in front of the bf16 GEMM (csrc/api.hip head_gemm_sliced), bit-equal to
the GEMM on the whole image.  The embedding table stays bf16.  Nobody claims model quality."""
import json
import re
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import _hip
from .args import QFORMAT_FP8_E4M3, QFORMAT_MXFP4, QFORMATS, QuantizationArgs  # noqa: F401

QSCALE_KEY = "qscale_weight"   # `<linear>.qscale_weight`: the one place that names the checkpoint key of a row scale
QSCALE_ACT_KEY = "qscale_act"  # per-tensor activation scales of FP8-activation checkpoints: not implemented, a foreign key here
E4M3_MAX = 448.0
# the linears that are quantised: the seven of every dense layer, nothing else
_QUANT_KEY = re.compile(r"^layers\.\d+\.(attention\.w[qkvo]|feed_forward\.w[123])\.weight$")

# What a quantised model cannot be combined with: one text per kind, the format's name filled in (refusal()).
_REFUSALS = {
    "lora": ("un-merged LoRA on an {name}-quantised base is not implemented; merge the adapter into the bf16 weights "
             "(Transformer.load_lora on a bf16 model) and quantise the result"),
    "moe": "{name} weight-only quantisation of a MoE model is not implemented (the expert kernels read bf16 weights)",
    "merge": ("load_lora: merging an adapter into {name}-quantised weights is not implemented (the merge needs the bf16 "
              "weights); merge into the bf16 checkpoint and quantise the result"),
    "storage": ("{name} weight-only quantisation with fp16 / fp32 storage ({dtype}) is not implemented: the "
                "activations, norms and the LM head of a quantised model are bfloat16"),
    "shape": ("{name} weight-only quantisation on a model shape outside the tuned bf16 kernels (head_dim "
              "128, dim / hidden_dim multiples of {k_multiple}) is not implemented"),
    "pth": "{name} weight-only models load from consolidated.safetensors (a .pth checkpoint is not implemented)",
    "prefill_fp8": ("prefill_fp8=True on {what} is not implemented: the FP8 prefill GEMMs read FP8 (e4m3) weights beside bfloat16 "
                    "activations (quantize=\"fp8_e4m3\", or a folder that quantize_checkpoint wrote, with bfloat16 storage)"),
    "prefill_w4a8": ("prefill_w4a8=True on {what} is not implemented: the MXFP4 x FP8 prefill GEMMs read MXFP4 weights beside bfloat16 "
                     "activations (quantize=\"mxfp4\", or a folder that quantize_checkpoint wrote, with bfloat16 storage)"),
}
MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitude of code & 7; code & 8 is the sign


def refusal(kind: str, quantization: QuantizationArgs, **kw) -> str:
    cls = quantized_linear_cls(quantization)
    return _REFUSALS[kind].format(name=cls.name, k_multiple=cls.k_multiple, **kw)


def check_quantize_arg(quantize: Optional[str]) -> None:
    if quantize is not None and quantize not in QFORMATS:
        raise NotImplementedError(f"quantize={quantize!r} is not implemented "
                                  f"(the weight formats are {', '.join(repr(q) for q in QFORMATS)})")


def refuse_quant_combinations(args, dtype: Optional[torch.dtype]) -> None:
    """What a quantised model cannot be combined with, by name, before anything is read from disk."""
    if args.quantization is None:
        return
    if args.lora is not None:
        raise NotImplementedError(refusal("lora", args.quantization))
    if args.moe is not None:
        raise NotImplementedError(refusal("moe", args.quantization))
    if dtype is not None and dtype != torch.bfloat16:
        raise NotImplementedError(refusal("storage", args.quantization, dtype=dtype))


def refuse_prefill_fp8(args, dtype: Optional[torch.dtype]) -> None:
    """`prefill_fp8=True` on a model whose weights are not FP8 e4m3 (bf16, MXFP4) or whose storage is not bfloat16, by name."""
    qz = args.quantization
    if qz is None:
        what = "a model without FP8 weights" if dtype in (None, torch.bfloat16) else f"a model with {dtype} storage"
    elif qz.qformat_weight != QFORMAT_FP8_E4M3:
        what = f"{quantized_linear_cls(qz).name} weights"
    elif dtype not in (None, torch.bfloat16):
        what = f"{dtype} storage"
    else:
        return
    raise NotImplementedError(_REFUSALS["prefill_fp8"].format(what=what))


def refuse_prefill_w4a8(args, dtype: Optional[torch.dtype]) -> None:
    """`prefill_w4a8=True` on a model whose weights are not MXFP4 (bf16, FP8) or whose storage is not bfloat16, by name."""
    qz = args.quantization
    if qz is None:
        what = "a model without MXFP4 weights" if dtype in (None, torch.bfloat16) else f"a model with {dtype} storage"
    elif qz.qformat_weight != QFORMAT_MXFP4:
        what = f"{quantized_linear_cls(qz).name} weights"
    elif dtype not in (None, torch.bfloat16):
        what = f"{dtype} storage"
    else:
        return
    raise NotImplementedError(_REFUSALS["prefill_w4a8"].format(what=what))


def is_quantized_linear_key(key: str) -> bool:
    return _QUANT_KEY.match(key) is not None


def quantize_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[out, in] (bf16 / fp32) -> (q float8_e4m3fn [out, in], scale fp32 [out]) with the power-of-two row scale
    2^ceil(log2(amax / 448)): for a nonzero row amax / scale lies in (224, 448].  An all-zero row gets scale 1.  The cast
    saturates (at +-448, and below the largest bf16 after scaling) and never produces the NaN codes 0x7F / 0xFF.  Integer
    exponent arithmetic (frexp / ldexp), so the CPU and the device give the same bytes."""
    assert w.dim() == 2 and w.is_floating_point()
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_rows: the weight holds inf or NaN")
    mant, ex = torch.frexp(amax)                     # amax = mant * 2^ex, mant in [0.5, 1)
    # amax / 448 = (2 mant / 1.75) * 2^(ex - 9): the ceil of its log2 is ex - 9, one more when 2 mant > 1.75
    e = ex - 9 + (mant > 0.875).to(ex.dtype)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    scale = torch.ldexp(torch.ones_like(amax), e)
    q = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    # a row whose amax sits in bf16's top binade can round UP past the largest bf16 (255 -> 256 at scale 2^120): such a code
    # steps down to the next smaller magnitude, so that the dequantised weight saturates instead of becoming inf
    over = (q.float().abs() * scale[:, None]) > torch.finfo(torch.bfloat16).max
    if bool(over.any()):
        codes = q.view(torch.uint8)
        q = torch.where(over, codes - 1, codes).view(torch.float8_e4m3fn)
    return q, scale


def quantize_activations(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[T, in] bf16 activation rows -> (x_q float8_e4m3fn [T, in], s_x fp32 [T]): `quantize_rows`, one power-of-two scale per row
    (per token).  The host-side statement of what `_hip.act_quant_e4m3` computes, byte for byte."""
    return quantize_rows(x)


def dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bf16(scale[r] * e4m3(q[r, k])); exact for power-of-two scales.  q: float8_e4m3fn or its bytes as uint8."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    return (q.float() * scale.float().reshape(-1, 1)).to(torch.bfloat16)


def expand_scale(scale: torch.Tensor, out_features: int) -> torch.Tensor:
    """A checkpoint's row scale as fp32 [out]: a scalar or [1] is broadcast."""
    s = scale.float().reshape(-1)
    if s.numel() == 1:
        s = s.expand(out_features)
    if s.numel() != out_features:
        raise ValueError(f"{QSCALE_KEY} has {s.numel()} entries for {out_features} output rows")
    return s.contiguous()


class QuantLinear(nn.Module):
    """`nn.Linear(bias=False)` on quantised weight bytes and their scales: what every weight-only format shares.  Both are
    parameters whose dtype no cast touches (uint8 bytes; uint8 or fp32 scales): `model.to(dtype=...)` would otherwise convert a
    float8 parameter silently, and without its scale.  A format supplies the class attributes below, `empty`, `load_quantized`,
    `from_checkpoint`, `check_bound` and `dequantized`."""
    name: str                 # in messages: "FP8"
    qformat: str              # params.json `quantization.qformat_weight`
    k_multiple: int           # what in_features (and the model's dim / hidden_dim) must be a multiple of
    hip: _hip.QuantFormat     # the format's entry points of the library
    prefill_fp8 = False       # FP8 linears: Transformer.prefill_fp8 sets it on every linear of the model (mi_linear_w8a8)
    prefill_w4a8 = False      # MXFP4 linears: Transformer.prefill_w4a8 likewise (mi_linear_w4a8)
    quantize = None           # staticmethod: bf16 [out, in] -> (weight, scale) as a checkpoint stores them

    def __init__(self, in_features: int, out_features: int, bias: bool = False):
        super().__init__()
        assert not bias
        self.in_features, self.out_features = in_features, out_features
        self._bind(*self.empty(in_features, out_features))

    def _bind(self, weight: torch.Tensor, scale: torch.Tensor) -> None:
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.qscale_weight = nn.Parameter(scale, requires_grad=False)

    def _apply(self, fn, recurse: bool = True):
        def keep_dtype(t: torch.Tensor) -> torch.Tensor:  # device moves pass; a dtype cast touches neither bytes nor scales
            out = fn(t)
            return out if out.dtype == t.dtype else t.to(device=out.device)
        return nn.Module._apply(self, keep_dtype, recurse)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape
        out = linear_quant(x.reshape(-1, shape[-1]), (self,), _hip.EPI_STORE)
        return out.view(*shape[:-1], self.out_features)


def linear_quant(x: torch.Tensor, mods: Sequence[QuantLinear], epilogue: int = _hip.EPI_STORE, residual: Optional[torch.Tensor] = None,
                 norm_w: Optional[torch.Tensor] = None, eps: float = 0.0) -> torch.Tensor:
    """`_hip.linear` over up to three quantised linears of one format that share an input (q|k|v; SWIGLU: w1, w3)."""
    return _hip.linear_quant(mods[0].hip, x, [m.weight for m in mods], [m.qscale_weight for m in mods], epilogue, residual, norm_w, eps,
                             a8=bool(mods[0].prefill_w4a8 if mods[0].hip.suffix == "w4" else mods[0].prefill_fp8))


class Fp8Linear(QuantLinear):
    """e4m3 weight bytes [out, in] (a uint8 parameter) and fp32 row scales [out]."""
    name, qformat, k_multiple, hip = "FP8", QFORMAT_FP8_E4M3, 16, _hip.W8
    quantize = staticmethod(quantize_rows)

    @staticmethod
    def empty(in_features: int, out_features: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return torch.zeros((out_features, in_features), dtype=torch.uint8), torch.ones(out_features, dtype=torch.float32)

    @torch.no_grad()
    def load_quantized(self, q: torch.Tensor, scale: torch.Tensor) -> None:
        """Bind e4m3 weights (float8_e4m3fn or uint8 bytes) and their row scales (fp32 [out], scalar or [1])."""
        assert tuple(q.shape) == (self.out_features, self.in_features), (tuple(q.shape), self.out_features, self.in_features)
        self._bind(weight_bytes(q), expand_scale(scale, self.out_features).to(q.device))

    def from_checkpoint(self, name: str, w: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """A checkpoint's tensors as the parameters hold them: bytes as uint8, fp32 [out] row scales (a scalar or [1] is broadcast)."""
        if not scale.is_floating_point() or tuple(w.shape) != (self.out_features, self.in_features):
            raise ValueError(f"{name}: not an FP8 linear (weight {tuple(w.shape)} {w.dtype}, scale {scale.dtype})")
        return weight_bytes(w), expand_scale(scale, self.out_features)

    def check_bound(self, name: str) -> None:
        assert tuple(self.qscale_weight.shape) == (self.out_features,)

    def dequantized(self) -> torch.Tensor:
        return dequantize(self.weight, self.qscale_weight)


def weight_bytes(q: torch.Tensor) -> torch.Tensor:
    if q.dtype == torch.float8_e4m3fn:
        return q.contiguous().view(torch.uint8)
    if q.dtype != torch.uint8:
        raise ValueError(f"a quantised weight is F8_E4M3 (torch.float8_e4m3fn), got {q.dtype}")
    return q.contiguous()


def quantize_blocks(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[out, in] (bf16 / fp32), in % 32 == 0 -> (packed uint8 [out, in / 2], scale uint8 [out, in / 32]): OCP MXFP4.  Per block
    of 32 the scale is 2^e with e = ceil(log2(amax / 6)), so amax / scale lies in (3, 6]; an all-zero block gets e = 0 (byte
    127); e is clamped to [-127, 127].  Codes are round-to-nearest, ties to the even code, onto +-{0, .5, 1, 1.5, 2, 3, 4, 6},
    saturating at +-6; a code whose dequantised value would pass the largest bf16 (a block holding bf16 max) steps down.  Two
    codes per byte, the low nibble at the even k.  Integer exponent arithmetic and comparisons only, so the CPU and the device
    give the same bytes."""
    assert w.dim() == 2 and w.is_floating_point()
    out, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quantize_blocks: in = {K} must be a multiple of {MXFP4_BLOCK} (one e8m0 scale per block of 32)")
    wf = w.float().reshape(out, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=2)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_blocks: the weight holds inf or NaN")
    mant, ex = torch.frexp(amax)                     # amax = mant * 2^ex, mant in [0.5, 1)
    # amax / 6 = (mant / 0.75) * 2^(ex - 3): the ceil of its log2 is ex - 3, one more when mant > 0.75
    e = ex - 3 + (mant > 0.75).to(ex.dtype)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp_(-127, 127)
    scale = torch.ldexp(torch.ones_like(amax), e)
    v = wf / scale[:, :, None]                       # exact: a power of two
    a = v.abs()
    idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
           + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    tab = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=w.device)
    over = tab[idx.long()] * scale[:, :, None] > torch.finfo(torch.bfloat16).max
    idx = torch.where(over, idx - 1, idx)
    codes = torch.where((v < 0) & (idx > 0), idx | 8, idx).reshape(out, K)
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return packed.contiguous(), (e + 127).to(torch.uint8).contiguous()


def check_mxfp4_tensors(packed: torch.Tensor, scale: torch.Tensor, out_features: int, in_features: int, what: str = "MXFP4") -> None:
    """What the tensors of an MXFP4 linear must be (ValueError otherwise); nothing here reads the device unless they live there."""
    if in_features % MXFP4_BLOCK:
        raise ValueError(f"{what}: in = {in_features} must be a multiple of {MXFP4_BLOCK} (one e8m0 scale per block of 32)")
    if packed.dtype != torch.uint8 or scale.dtype != torch.uint8:
        raise ValueError(f"{what}: an MXFP4 linear is U8 codes and U8 e8m0 scales, got {packed.dtype} and {scale.dtype}")
    if tuple(packed.shape) != (out_features, in_features // 2) or tuple(scale.shape) != (out_features, in_features // MXFP4_BLOCK):
        raise ValueError(f"{what}: MXFP4 codes {tuple(packed.shape)} / scales {tuple(scale.shape)} do not fit a linear "
                         f"[{out_features}, {in_features}] (codes [out, in / 2], scales [out, in / 32])")
    if not scale.is_meta and bool((scale == 255).any()):
        raise ValueError(f"{what}: scale byte 255 (the e8m0 NaN)")


def dequantize_mxfp4(packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bf16 [out, in] of 2^(scale - 127) * e2m1(code): exact."""
    out, half = packed.shape
    tab = torch.tensor(E2M1_VALUES + tuple(-x for x in E2M1_VALUES), dtype=torch.float32, device=packed.device)
    vals = torch.stack((tab[(packed & 15).long()], tab[(packed >> 4).long()]), dim=2).reshape(out, half * 2 // MXFP4_BLOCK, MXFP4_BLOCK)
    sc = torch.ldexp(torch.ones(scale.shape, dtype=torch.float32, device=scale.device), scale.to(torch.int32) - 127)
    return (vals * sc[:, :, None]).reshape(out, half * 2).to(torch.bfloat16)


class Mxfp4Linear(QuantLinear):
    """MXFP4 weights: e2m1 codes [out, in / 2] and e8m0 block scales [out, in / 32], both uint8 parameters."""
    name, qformat, k_multiple, hip = "MXFP4", QFORMAT_MXFP4, MXFP4_BLOCK, _hip.W4
    quantize = staticmethod(quantize_blocks)

    @staticmethod
    def empty(in_features: int, out_features: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if in_features % MXFP4_BLOCK:
            raise ValueError(f"Mxfp4Linear: in = {in_features} must be a multiple of {MXFP4_BLOCK} (one e8m0 scale per block of 32)")
        return (torch.zeros((out_features, in_features // 2), dtype=torch.uint8),
                torch.full((out_features, in_features // MXFP4_BLOCK), 127, dtype=torch.uint8))

    @torch.no_grad()
    def load_quantized(self, packed: torch.Tensor, scale: torch.Tensor) -> None:
        check_mxfp4_tensors(packed, scale, self.out_features, self.in_features, "Mxfp4Linear.load_quantized")
        self._bind(packed.contiguous(), scale.contiguous().to(packed.device))

    def from_checkpoint(self, name: str, w: torch.Tensor, scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        check_mxfp4_tensors(w, scale, self.out_features, self.in_features, name)
        return w, scale

    def check_bound(self, name: str) -> None:
        check_mxfp4_tensors(self.weight, self.qscale_weight, self.out_features, self.in_features, name)

    def dequantized(self) -> torch.Tensor:
        return dequantize_mxfp4(self.weight, self.qscale_weight)


QUANT_LINEARS = {cls.qformat: cls for cls in (Fp8Linear, Mxfp4Linear)}


def quantized_linear_cls(quantization: QuantizationArgs):
    return QUANT_LINEARS[quantization.qformat_weight]


LM_HEAD_KEY = "output.weight"                                  # the LM head: quantised only on request (`lm_head`)
LM_HEAD_SCALE_KEY = "output." + QSCALE_KEY


def refuse_lm_head_arg(quantize_lm_head: bool, quantization: Optional[QuantizationArgs]) -> None:
    """`quantize_lm_head=True` on a model without a weight format, by name, before anything is read from disk."""
    if quantize_lm_head and quantization is None:
        raise NotImplementedError("quantize_lm_head=True without a weight format is not implemented: the LM head is quantised in the "
                                  "format of the model's layers (quantize=\"fp8_e4m3\" / \"mxfp4\", or a folder that quantize_checkpoint wrote)")


def check_lm_head_tensors(folder, quantization: QuantizationArgs, keys) -> None:
    """A quantised folder's `lm_head` flag and its tensors must agree (ValueError otherwise): the flag promises
    `output.qscale_weight` beside the head's bytes, its absence a bf16 `output.weight` alone."""
    has_scale = LM_HEAD_SCALE_KEY in keys
    if quantization.lm_head and not has_scale:
        raise ValueError(f"{folder}: params.json says quantization.lm_head but the checkpoint has no {LM_HEAD_SCALE_KEY} "
                         "(the flag and the tensors disagree)")
    if has_scale and not quantization.lm_head:
        raise ValueError(f"{folder}: the checkpoint has {LM_HEAD_SCALE_KEY} but params.json does not say quantization.lm_head "
                         "(the flag and the tensors disagree)")


def quantize_state_tensor(key: str, t: torch.Tensor, qformat: str = QFORMAT_FP8_E4M3, lm_head: bool = False) -> Dict[str, torch.Tensor]:
    """One checkpoint tensor -> the tensors that replace it: a quantised linear becomes its bytes and its row (MXFP4: block)
    scales, anything else stays as it is.  lm_head: `output.weight` is such a linear too."""
    check_quantize_arg(qformat)
    if not (is_quantized_linear_key(key) or (lm_head and key == LM_HEAD_KEY)):
        return {key: t}
    cls = QUANT_LINEARS[qformat]
    if t.dtype != torch.bfloat16:
        raise NotImplementedError(f"{key}: {cls.name} quantisation starts from a bfloat16 checkpoint, got {t.dtype}")
    q, scale = cls.quantize(t)
    return {key: q, key[:-len("weight")] + QSCALE_KEY: scale}


def quantize_checkpoint(src_folder: Union[Path, str], dst_folder: Union[Path, str], qformat: str = QFORMAT_FP8_E4M3,
                        lm_head: bool = False) -> Path:
    """bf16 folder (params.json + consolidated.safetensors) -> weight-only quantised folder, tensor by tensor on the CPU: the
    seven linears of every layer become `<linear>.weight` (F8_E4M3) + `<linear>.qscale_weight` (fp32 [out]), or with
    qformat="mxfp4" U8 [out, in / 2] + U8 [out, in / 32]; everything else is copied.  lm_head=True (opt-in): `output.weight`
    and `output.qscale_weight` likewise, and `"lm_head": true` in the `quantization` block; without it the block has no such key
    and the head stays bf16.  Other files of the folder (tokenizer) are the caller's to copy."""
    import safetensors
    from safetensors.torch import save_file
    from .args import TransformerArgs

    check_quantize_arg(qformat)
    src, dst = Path(src_folder), Path(dst_folder)
    with open(src / "params.json", "r") as f:
        params = json.load(f)
    args = TransformerArgs.from_dict(params)
    if args.quantization is not None:
        raise ValueError(f"{src} is already quantised ({args.quantization.qformat_weight})")
    args.quantization = QuantizationArgs(qformat)
    refuse_quant_combinations(args, None)
    st_file = src / "consolidated.safetensors"
    assert st_file.exists(), f"{st_file} does not exist (quantize_checkpoint reads safetensors)"
    out: Dict[str, torch.Tensor] = {}
    with safetensors.safe_open(str(st_file), framework="pt", device="cpu") as f:
        for k in f.keys():
            out.update(quantize_state_tensor(k, f.get_tensor(k), qformat, lm_head))
    if lm_head and LM_HEAD_SCALE_KEY not in out:
        raise ValueError(f"{src}: lm_head=True but the checkpoint has no {LM_HEAD_KEY}")
    dst.mkdir(parents=True, exist_ok=True)
    save_file(out, str(dst / "consolidated.safetensors"))
    params["quantization"] = {"qformat_weight": qformat, **({"lm_head": True} if lm_head else {})}
    with open(dst / "params.json", "w") as f:
        json.dump(params, f)
    return dst
