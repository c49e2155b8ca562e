"""The Mamba2 rule of include/mistral_hip.h as a plain token-serial recurrence in torch (no chunking, nothing kernel-shaped), plus
the random weights and the checkpoint folder the Mamba tests share.  `dtype` is the arithmetic's; `round_bf16` applies the rule's
bf16 rounding points (off: the same arithmetic with no rounding at all)."""
import json
import math
import os

import torch

N, P, K, EPS = 128, 64, 4, 1e-5


def _r(x, on):
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def scan(zx, conv_w, conv_b, dt_bias, A_log, D, conv_state, ssm_state, G, dtype=torch.float64, round_bf16=True):
    """Steps 3 and 4 for zx [B, L, >= width].  Returns y [B, L, I] BEFORE its rounding, the sum of the absolute contributions to each
    y, the new conv state (raw rows), the new SSM state and the sum of the absolute contributions to each of its elements."""
    B, L, _ = zx.shape
    H = dt_bias.numel()
    I, Cc = H * P, H * P + 2 * G * N
    raw = torch.cat([conv_state.to(dtype), zx[:, :, I:I + Cc].to(dtype)], 1)          # [B, 3 + L, Cc]
    w = conv_w.reshape(Cc, K).to(dtype)
    a = conv_b.to(dtype) + sum(w[:, j] * raw[:, j:j + L] for j in range(K))
    xbc = _r(a * torch.sigmoid(a), round_bf16)
    x = xbc[..., :I].reshape(B, L, H, P)
    Bm = xbc[..., I:I + G * N].reshape(B, L, G, N).repeat_interleave(H // G, 2)
    Cm = xbc[..., I + G * N:].reshape(B, L, G, N).repeat_interleave(H // G, 2)
    dtr = zx[:, :, I + Cc:I + Cc + H].to(dtype) + dt_bias.to(dtype)
    dt = torch.where(dtr > 20, dtr, torch.log1p(torch.exp(dtr)))
    decay = torch.exp(dt * -torch.exp(A_log.to(dtype)))
    S = ssm_state.to(dtype).clone()
    Sabs = S.abs()
    ys, terms = [], []
    for t in range(L):
        upd = dt[:, t, :, None, None] * x[:, t, :, :, None] * Bm[:, t, :, None, :]
        S = decay[:, t, :, None, None] * S + upd
        Sabs = decay[:, t, :, None, None] * Sabs + upd.abs()
        skip = D.to(dtype)[None, :, None] * x[:, t]
        ys.append((S * Cm[:, t, :, None, :]).sum(-1) + skip)
        terms.append((Sabs * Cm[:, t, :, None, :].abs()).sum(-1) + skip.abs())
    return torch.stack(ys, 1).reshape(B, L, I), torch.stack(terms, 1).reshape(B, L, I), raw[:, L:], S, Sabs


def add_norm(res, h, w, dtype, round_bf16=True):
    res = res.to(dtype) + (0 if h is None else h.to(dtype))
    return _r(res * torch.rsqrt((res * res).mean(-1, keepdim=True) + EPS) * w.to(dtype), round_bf16), res


def gated_norm(y, z, w, G, dtype, round_bf16=True):
    v = y.to(dtype) * z.to(dtype) * torch.sigmoid(z.to(dtype))
    vg = v.reshape(*v.shape[:-1], G, -1)
    return _r((vg * torch.rsqrt((vg * vg).mean(-1, keepdim=True) + EPS)).reshape(v.shape) * w.to(dtype), round_bf16)


def forward(w, ids, G, dtype=torch.float64, round_bf16=False):
    """Logits [B, L, V] of the whole rule from zero states."""
    h = w["embedding"][ids].to(dtype)
    B, L, D = h.shape
    I, H = 2 * D, 2 * D // P
    res = torch.zeros_like(h)
    for ly in w["layers"]:
        u, res = add_norm(res, h, ly["norm"], dtype, round_bf16)
        zx = _r(u @ ly["in_proj"].to(dtype).T, round_bf16)
        y = scan(zx, ly["conv_w"], ly["conv_b"], ly["dt_bias"], ly["A_log"], ly["D"], torch.zeros(B, K - 1, I + 2 * G * N),
                 torch.zeros(B, H, P, N), G, dtype, round_bf16)[0]
        o = gated_norm(_r(y, round_bf16), zx[..., :I], ly["gated_norm"], G, dtype, round_bf16)
        h = _r(o @ ly["out_proj"].to(dtype).T, round_bf16)
    u, _ = add_norm(res, h, w["norm_f"], dtype, round_bf16)
    return _r(u @ w["lm_head"].to(dtype).T, round_bf16)


def synth_layer(D, G, gen, a_lo=0.05, a_hi=1.0):
    """Random weights of one layer in their checkpoint dtypes (bf16; the three per-head vectors fp32)."""
    I, H = 2 * D, 2 * D // P
    Cc = I + 2 * G * N
    rnd = lambda *s: torch.randn(*s, generator=gen)
    dt = torch.exp(torch.rand(H, generator=gen) * (math.log(0.3) - math.log(0.01)) + math.log(0.01))
    return {"norm": (1 + 0.1 * rnd(D)).bfloat16(), "in_proj": (rnd(2 * I + 2 * G * N + H, D) / math.sqrt(D)).bfloat16(),
            "conv_w": (rnd(Cc, 1, K) * 0.4).bfloat16(), "conv_b": (rnd(Cc) * 0.1).bfloat16(),
            "dt_bias": dt + torch.log(-torch.expm1(-dt)), "A_log": torch.log(a_lo + (a_hi - a_lo) * torch.rand(H, generator=gen)),
            "D": 1 + 0.1 * rnd(H), "gated_norm": (1 + 0.1 * rnd(I)).bfloat16(), "out_proj": (rnd(D, I) / math.sqrt(I)).bfloat16()}


def synth_weights(D, n_layers, V, G, seed):
    gen = torch.Generator().manual_seed(seed)
    return {"embedding": torch.randn(V, D, generator=gen).bfloat16(), "layers": [synth_layer(D, G, gen) for _ in range(n_layers)],
            "norm_f": (1 + 0.1 * torch.randn(D, generator=gen)).bfloat16(), "lm_head": (torch.randn(V, D, generator=gen) / math.sqrt(D)).bfloat16()}


def params(D, n_layers, V, G, **over):
    return dict({"dim": D, "n_layers": n_layers, "vocab_size": V, "n_groups": G, "rms_norm": True, "residual_in_fp32": True,
                 "fused_add_norm": True, "pad_vocab_size_multiple": 8, "tie_embeddings": False, "model_type": "mamba"}, **over)


def state_dict(w):
    """The weights under their checkpoint keys (mistral_inference.mamba.KEYS)."""
    from mistral_inference.mamba import KEYS
    out = {}
    for pat, (field, _) in KEYS.items():
        for i in (range(len(w["layers"])) if "{i}" in pat else [None]):
            out[pat.format(i=i)] = (w[field] if i is None else w["layers"][i][field]).contiguous()
    return out


def write_folder(folder, D, n_layers, V, G, w):
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "params.json"), "w") as f:
        json.dump(params(D, n_layers, V, G), f)
    save_file(state_dict(w), os.path.join(folder, "consolidated.safetensors"))
    return str(folder)
