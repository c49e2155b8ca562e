"""Mamba2 on the GPU through the C ABI (csrc/mamba.hip) against the token-serial fp64 recurrence of tests/mamba_ref.py.

Bound of the scan tests, per element: beside the rule's own roundings (which the reference shares) every term passes through at
most two more bf16-rounded operands of relative error 2^-9 each (bf16((C B^T) o M); or the scaled B rows and bf16(S_prev)), the sums
are fp32 and y is rounded once, so |y - y_ref| <= 2^-7 * (sum of the absolute contributions), about twice the first-order bound."""
import pytest
import torch

import mamba_ref as mr
from mistral_inference import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, H, B = 64, 4, 2
I = H * mr.P


def _scan_case(G, L, start, seed=0, impulse=None):
    """bf16 inputs of one scan call.  impulse = s: x' is non-zero at token s only (the x channels' convolution is the identity tap,
    no bias) and dt_raw = -3.5 with dt_bias 0 keeps the decay over 131 tokens above 2^-6 (dt = 0.0298, A <= 1)."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * L + G)
    Cc = I + 2 * G * mr.N
    ld = (I + Cc + H + 7) // 8 * 8
    w = mr.synth_layer(I // 2, G, gen, a_lo=0.2 if impulse is not None else 0.05)
    zx = torch.randn(B, L, ld, generator=gen).bfloat16()
    if impulse is not None:
        zx[:, :, I:2 * I] = 0
        zx[:, impulse, I:2 * I] = torch.randn(B, I, generator=gen).bfloat16()
        zx[:, :, I + Cc:] = -3.5
        w["dt_bias"] = torch.zeros(H)
        w["conv_w"][:I] = torch.tensor([0, 0, 0, 1.0]).bfloat16()
        w["conv_b"][:I] = 0
    conv = torch.zeros(B, 3, Cc).bfloat16()
    ssm = torch.zeros(B, H, mr.P, mr.N)
    if start == "random":
        conv = torch.randn(B, 3, Cc, generator=gen).bfloat16()
        ssm = torch.randn(B, H, mr.P, mr.N, generator=gen)
        if impulse is not None:
            conv[:, :, :I] = 0
    return w, zx, conv, ssm


def _run(w, zx, conv, ssm, G):
    """mi_mamba_scan on copies of the states: (y, conv state, SSM state) back on the CPU."""
    d = lambda t: t.to(DEV).contiguous()
    conv_d, ssm_d = d(conv), d(ssm)
    y = _hip.mamba_scan(d(zx), d(w["conv_w"]), d(w["conv_b"]), d(w["dt_bias"]), d(w["A_log"]), d(w["D"]), conv_d, ssm_d, G)
    return y.cpu(), conv_d.cpu(), ssm_d.cpu()


def _check(w, zx, conv, ssm, G, got, factor=1.0):
    y_ref, terms, conv_ref, S_ref, S_terms = mr.scan(zx, w["conv_w"], w["conv_b"], w["dt_bias"], w["A_log"], w["D"], conv, ssm, G)
    y, conv_new, S = got
    ey = ((y.double() - y_ref).abs() / (terms + 1e-30)).max().item()
    eS = ((S.double() - S_ref).abs() / (S_terms + 1e-30)).max().item()
    print(f"worst |y - ref| / sum|terms| = {ey:.3e}, state {eS:.3e} (bound {factor * 2 ** -7:.3e})")
    assert torch.equal(conv_new.view(torch.int16), conv_ref.bfloat16().view(torch.int16))
    assert ((y.double() - y_ref).abs() <= factor * 2.0 ** -7 * terms).all(), ey
    assert ((S.double() - S_ref).abs() <= factor * 2.0 ** -7 * S_terms).all(), eS


@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("L", [1, 2, Q - 1, Q, Q + 1, 2 * Q + 3])
@pytest.mark.parametrize("G", [1, 2])
def test_scan_matches_the_fp64_recurrence(G, L, start):
    w, zx, conv, ssm = _scan_case(G, L, start)
    _check(w, zx, conv, ssm, G, _run(w, zx, conv, ssm, G))


@pytest.mark.parametrize("s", [0, Q - 1, Q, 2 * Q + 2])
@pytest.mark.parametrize("G", [1, 2])
def test_scan_impulse_at_one_token(G, s):
    w, zx, conv, ssm = _scan_case(G, 2 * Q + 3, "zero", seed=1, impulse=s)
    _check(w, zx, conv, ssm, G, _run(w, zx, conv, ssm, G))


@pytest.mark.parametrize("G", [1, 2])
def test_scan_continues_through_its_states(G):
    w, zx, conv, ssm = _scan_case(G, 2 * Q + 3, "random", seed=2)
    whole = _run(w, zx, conv, ssm, G)
    ys, t0 = [], 0
    for n in (Q + 1, 1, Q + 1):
        y, conv, ssm = _run(w, zx[:, t0:t0 + n].contiguous(), conv, ssm, G)
        ys.append(y)
        t0 += n
    w0, zx0, conv0, ssm0 = _scan_case(G, 2 * Q + 3, "random", seed=2)
    _check(w0, zx0, conv0, ssm0, G, (torch.cat(ys, 1), conv, ssm), factor=1.0)  # the pieces meet the bound themselves ...
    terms = mr.scan(zx0, w["conv_w"], w["conv_b"], w["dt_bias"], w["A_log"], w["D"], conv0, ssm0, G)[1]
    assert ((torch.cat(ys, 1).double() - whole[0].double()).abs() <= 2 * 2.0 ** -7 * terms).all()  # ... and the one call within twice it
    assert torch.equal(conv.view(torch.int16), whole[1].view(torch.int16))


def _within_one_bf16_ulp(got, ref):
    ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 8)
    return ((got.double() - ref).abs() <= ulp).all()


@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("D", [64, 4096])
def test_add_norm_row_kernel(D, with_h):
    gen = torch.Generator().manual_seed(D)
    res, h = torch.randn(5, D, generator=gen), torch.randn(5, D, generator=gen).bfloat16()
    w = (1 + 0.1 * torch.randn(D, generator=gen)).bfloat16()
    res_d = res.to(DEV)
    out = _hip.mamba_add_norm(res_d, h.to(DEV) if with_h else None, w.to(DEV), mr.EPS)
    ref, res_ref = mr.add_norm(res, h if with_h else None, w, torch.float64, round_bf16=False)
    torch.testing.assert_close(res_d.cpu().double(), res_ref, rtol=2.0 ** -22, atol=0)
    assert _within_one_bf16_ulp(out.cpu(), ref)


@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("D", [64, 4096])
def test_gated_norm_row_kernel(D, G):
    gen = torch.Generator().manual_seed(D + G)
    n = 2 * D
    y, zx = torch.randn(5, n, generator=gen).bfloat16(), torch.randn(5, n + 24, generator=gen).bfloat16()
    w = (1 + 0.1 * torch.randn(n, generator=gen)).bfloat16()
    out = _hip.mamba_gated_norm(y.to(DEV), zx.to(DEV), w.to(DEV), G, mr.EPS)
    assert _within_one_bf16_ulp(out.cpu(), mr.gated_norm(y, zx[:, :n], w, G, torch.float64, round_bf16=False))


@pytest.fixture(scope="module")
def tiny_model(tmp_path_factory):
    from mistral_inference.mamba import Mamba
    w = mr.synth_weights(128, 2, 512, 1, seed=5)
    return Mamba.from_folder(mr.write_folder(tmp_path_factory.mktemp("mamba"), 128, 2, 512, 1, w), device=DEV, dtype=torch.bfloat16), w


def test_model_logits_against_the_fp64_restatement(tiny_model):
    """2 layers, dim 128, vocabulary 512, one group, 2 sequences of Q + 5 tokens.  Measured on an MI355X:
    max|hip - ref64| = 2.78e-02, max|ref_bf16 - ref64| = 3.33e-02 (logits up to 4.4 in magnitude)."""
    model, w = tiny_model
    ids = torch.randint(0, 512, (2, Q + 5), generator=torch.Generator().manual_seed(3))
    got = model.forward(ids).cpu().double()
    ref64 = mr.forward(w, ids, 1, torch.float64, round_bf16=False)
    ref_bf16 = mr.forward(w, ids, 1, torch.float32, round_bf16=True).double()
    e_hip, e_ref = (got - ref64).abs().max().item(), (ref_bf16 - ref64).abs().max().item()
    print(f"max|hip - ref64| = {e_hip:.3e}, max|ref_bf16 - ref64| = {e_ref:.3e}, max|logit| = {ref64.abs().max().item():.2f}")
    assert e_hip <= 3 * e_ref


@pytest.mark.parametrize("chunk_size", [None, 3])
def test_generate_mamba_greedy_equals_repeated_full_forwards(tiny_model, chunk_size):
    from mistral_inference.generate import generate_mamba
    model, _ = tiny_model
    prompts = [[1, 5, 9, 200, 17, 3, 44], [7, 300, 2, 11, 12, 13, 14]]
    toks, scores = generate_mamba(prompts, model, max_tokens=8, temperature=0.0, chunk_size=chunk_size)
    assert [len(x) for x in scores] == [8, 8]
    seqs = [list(p) for p in prompts]
    for i in range(8):
        logits = model.forward(torch.tensor(seqs))[:, -1]
        nxt = logits.argmax(-1).tolist()
        assert [t[i] for t in toks] == nxt, (i, toks, nxt)
        for b in range(2):
            seqs[b].append(nxt[b])
