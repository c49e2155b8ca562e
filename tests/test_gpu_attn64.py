"""csrc/attn_prefill64.hip - non-causal, cache-less attention on 64-wide heads - through _hip.attn_prefill(head_dim=64) against an
fp64 softmax of the same bf16 inputs.  T sits at one row and just below, at and just past the 64-key half, the 128-key tile and
the 64 / 128 / 256-query blocks; H = 3 makes the row pitch no power of two; `qb` pins each of the three block shapes
(MI_ATTN64_QUERIES), since inputs this small would only ever choose the 64-query one."""
import pytest
import torch

import vision_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DH = 64
SHAPES = pytest.mark.parametrize("T, H", [(T, H) for T in (1, 63, 64, 65, 129, 257, 300) for H in (1, 3)])
BLOCKS = pytest.mark.parametrize("qb", ["auto", "128", "256"])


def _run64(q, k, v, qb, monkeypatch):
    """q, k, v: [T, H, 64] bf16 on the host -> out [T, H, 64] fp64 of the native route."""
    from mistral_inference import _hip as h
    if qb != "auto":
        monkeypatch.setenv("MI_ATTN64_QUERIES", qb)
    T, H, _ = q.shape
    qkv = torch.cat([q, k, v], dim=1).reshape(T, 3 * H * DH).cuda()
    return h.attn_prefill(qkv, H, H, DH, None, None, T, None, None, 1, T, causal=False).cpu().view(T, H, DH).double()


def _weights(q, k):
    """fp64 softmax weights [H, T, T] at the default scale 1/8."""
    return torch.softmax(q.double().transpose(0, 1) @ k.double().permute(1, 2, 0) / 8.0, dim=-1)


@BLOCKS
@SHAPES
def test_one_key_per_query_address_coded_v(T, H, qb, monkeypatch):
    """Query i sees key pi(i) = (37 i + 11) mod T alone (Q[i] = 8 K[pi(i)], K rows of +-1); V[j, h, d] is an integer code of
    (j, h, d) whose first three columns fix j by the Chinese remainder theorem (moduli 61, 63, 65).  A misplaced key, tile, head or
    d column moves some output by at least 1; the bound is one bf16 spacing (P is rounded to bf16, the row sum is not)."""
    g = torch.Generator().manual_seed(1000 * T + H)
    k = (torch.randint(0, 2, (T, H, DH), generator=g) * 2 - 1).to(BF)
    pi = (37 * torch.arange(T) + 11) % T
    assert sorted(pi.tolist()) == list(range(T))
    q = (8 * k[pi].float()).to(BF)
    j, hh, d = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(DH), indexing="ij")
    v = (((j + 1) * (d + 1) + 17 * hh) % (61 + 2 * (d % 3)) - 32).to(BF)
    assert float(v.float().abs().max()) <= 63 and len(torch.unique(v[:, 0, :3].float(), dim=0)) == T
    w = _weights(q, k)
    assert float(w[:, torch.arange(T), pi].min()) >= 1 - 2.0 ** -20      # the construction's condition, on the reference
    want = v[pi].double()
    got = _run64(q, k, v, qb, monkeypatch)
    assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs().clamp(min=1)).all()), float((got - want).abs().max())


@BLOCKS
@pytest.mark.parametrize("order", ["flat", "rising"])
@SHAPES
def test_every_key_counts(T, H, order, qb, monkeypatch):
    """randn q, k, v with near-uniform weights ("flat"), and with scores that rise by 8 nats = 11.5 in the exponent's base-2 domain
    per 64 keys ("rising": past the deferred-rescale threshold of 8, so every half tile rescales): a missing tail mask, a lost
    rescale or a wrong row sum moves the result by far more than the bound 4 * 2^-9 * max|v| - half a bf16 ulp each for P's
    rounding against the unrounded row sum, for the mismatch of the two, for the output's rounding, and one of headroom for exp2
    and the fp32 summation order.  The padded 128-wide route is held to the same bound on the same inputs."""
    from mistral_inference import _hip as h
    g = torch.Generator().manual_seed(7 * T + H)
    q, k, v = (torch.randn(T, H, DH, generator=g) for _ in range(3))
    if order == "flat":
        q = q / 4
    else:  # q . k / 8 ~ j / 8 + noise: along u = (1/8, ..., 1/8), |u| = 1
        q = 0.25 * q + 1.0
        k = 0.25 * k + torch.arange(T).view(T, 1, 1) / 64.0
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    ref = (_weights(q, k) @ v.double().transpose(0, 1)).transpose(0, 1)
    bound = 4 * 2.0 ** -9 * float(v.float().abs().max())
    pad = torch.zeros(T, 3 * H, 128, dtype=BF)
    pad[:, :, :DH] = torch.cat([q, k, v], dim=1)
    old = h.attn_prefill(pad.view(T, -1).cuda(), H, H, 128, None, None, T, None, None, 1, T, causal=False, softmax_scale=0.125)
    e_old = float((old.cpu().view(T, H, 128)[:, :, :DH].double() - ref).abs().max())
    e_new = float((_run64(q, k, v, qb, monkeypatch) - ref).abs().max())
    print(f"\nattn64 T={T} H={H} {order} qb={qb}: max|native - fp64| {e_new:.3e}, padded 128 route {e_old:.3e}, bound {bound:.3e}")
    assert e_new <= bound and e_old <= bound, (e_new, e_old, bound)


def test_tower_runs_the_native_route(monkeypatch):
    """A bf16 tower with 64-wide heads (hidden 128, 2 heads, 2 layers, two images of different grids) against the CPU oracle, at
    the vision tests' bound; the attention operator is handed the fused q|k|v rows as they are (3 * H * 64 columns, head_dim 64)."""
    from mistral_inference import _hip
    from mistral_inference.args import VisionEncoderArgs
    from mistral_inference.vision_encoder import VisionTransformer
    va = vo.VisionArgs(hidden_size=128, num_channels=3, image_size=32, patch_size=4, intermediate_size=256, num_hidden_layers=2,
                       num_attention_heads=2)
    w = vo.synth_vision_weights(va, 128, seed=5)
    tower = VisionTransformer(VisionEncoderArgs(**{f: getattr(va, f) for f in VisionEncoderArgs.__dataclass_fields__}))
    tower.load_state_dict({n[len("vision_encoder."):]: t for n, t in w.items() if n.startswith("vision_encoder.")})
    tower = tower.to("cuda", dtype=BF)
    g = torch.Generator().manual_seed(6)
    images = [torch.randn(3, 32, 20, generator=g).to(BF), torch.randn(3, 12, 28, generator=g).to(BF)]   # 8x5 and 3x7 patches
    seen, inner = [], _hip.attn_prefill
    monkeypatch.setattr(_hip, "attn_prefill", lambda qkv, H, Hkv, dh, *a, **kw: (seen.append((qkv.shape[1], dh)), inner(qkv, H, Hkv, dh, *a, **kw))[1])
    got = tower([im.cuda() for im in images]).float().cpu()
    ref = vo.vision_encoder(images, w, va).float()
    assert seen == [(3 * 2 * 64, 64)] * 2
    assert float((got - ref).abs().max()) <= 4e-2 * max(1.0, float(ref.abs().max()))
