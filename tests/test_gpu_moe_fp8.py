"""FP8 (e4m3) MoE experts on the device: the expert leaves behind `_hip.moe_experts(..., scale_tab=...)` - GEMV_MOE_W13 on e4m3 rows
and moe_w2_w8_kernel at T <= 8, the per-family dequantisation launch + the token-grouped GEMMs above - and a whole MoE model loaded
with quantize_experts=True.

The exact family of moe_cases.py (W in {-1, 0, 1, 16}) is stored as e4m3 codes W / s_r with the power-of-two row scale
s_r = 2^((r + e) % 3 - 1), different from row to row and from expert to expert: codes +-0.5, +-1, +-2, 8, 16, 32.  The model on the
dequantised weights is then the bf16 model, so moe_cases.reference(case) is the expected output bit for bit; a dropped, shifted or
neighbouring-expert scale changes a result by a factor of 2 or more."""
import pytest
import torch

import moe_cases as mc
import mistral_oracle as mo
from hip_util import write_checkpoint

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

DECODE = [mc.Case(f"fp8-decode-k{k}t{T}f{F}", 8, k, T, D=272, F=F, order="mixed") for k in (1, 2, 4) for T in (1, 3, 8) for F in (272, 528, 1552)]
LDS_EDGE = [mc.Case("fp8-decode-lds-k4f8192", 4, 4, 8, F=8192, order="mixed", w2_density=1 / 256, mutants=False)]  # top_k F 2 == 65536
PREFILL = [mc.Case("fp8-e8k2t300-edges", 8, 2, 300, (0, 1, 127, 128, 129, 215, 0, 0), D=272, F=528),
           mc.Case("fp8-e3k2t768-ragged255", 3, 2, 768, (768, 767, 1))]


def _hip():
    from mistral_inference import _hip
    return _hip


def _quantise(w, e):
    """(e4m3 bytes on the device, fp32 row scales on the device) of an exact-family matrix of expert e; the codes are exact."""
    s = torch.ldexp(torch.ones(w.shape[0]), (torch.arange(w.shape[0]) + e) % 3 - 1)
    q = (w.float() / s[:, None]).to(torch.float8_e4m3fn)
    assert torch.equal(q.float() * s[:, None], w.float())
    return q.view(torch.uint8).cuda(), s.cuda()


def _run(case):
    mc.conditions(case)
    inp = mc.inputs(case)
    dev = [[_quantise(w, e) for w in ex] for e, ex in enumerate(inp.experts)]
    tab = torch.tensor([[q.data_ptr() for q, _ in ex] for ex in dev], dtype=torch.int64, device="cuda")
    stab = torch.tensor([[s.data_ptr() for _, s in ex] for ex in dev], dtype=torch.int64, device="cuda")
    got = _hip().moe_experts(inp.x.cuda(), tab, case.E, case.F, inp.sel_idx.cuda(), inp.sel_w.cuda(), residual=inp.h.cuda(), scale_tab=stab).cpu()
    ref = mc.reference(case)[0]
    bad = torch.nonzero((got != ref).any(dim=1))[:, 0].tolist()
    assert not bad, (case, len(bad), "rows differ", mc.describe_rows(case, bad), "got", got[bad[0]].float()[:8].tolist(),
                     "ref", ref[bad[0]].float()[:8].tolist())


@pytest.mark.parametrize("case", DECODE + LDS_EDGE, ids=repr)
def test_fp8_experts_decode_leaf(case):
    assert case.path == "decode" and case.D % 16 == 0 and case.F % 16 == 0
    _run(case)


@pytest.mark.parametrize("case", PREFILL, ids=repr)
def test_fp8_experts_grouped_leaf(case):
    assert [c.path for c in PREFILL] == ["g128", "g256"]
    _run(case)


def test_fp8_experts_model_equals_the_bf16_model_on_the_dequantised_weights(tmp_path):
    """2 layers, E = 4, k = 2, dim 512.  Every row of every quantised linear holds ONE nonzero, +-2^j with j varying by row: each
    dot product is one exact product, so the e4m3 GEMVs and the bf16 GEMVs give the same bits in any summation order, the row
    scales are powers of two that differ from row to row, and everything that is not quantised (embedding, norms, attention, router,
    LM head) is the same kernel on the same bits.  Logits of a 16-token prefill and of one decode step, and the greedy tokens."""
    from mistral_inference.cache import BufferCache
    from mistral_inference.quant import QuantLinear
    from mistral_inference.transformer import Transformer
    args = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                         num_experts=4, num_experts_per_tok=2)
    w = mo.synth_weights(args, seed=11)
    g = torch.Generator().manual_seed(12)
    for key, t in w.items():
        if ".attention.w" in key or ".experts." in key:
            rows, cols = t.shape
            one = torch.zeros(rows, cols)
            val = torch.ldexp(torch.ones(rows), torch.randint(-2, 2, (rows,), generator=g)) * (torch.randint(0, 2, (rows,), generator=g) * 2 - 1)
            one[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = val
            w[key] = one.to(BF)
    folder = write_checkpoint(tmp_path / "moe", args, w)
    plain = Transformer.from_folder(folder, max_batch_size=1, device="cuda", dtype=BF)
    quant = Transformer.from_folder(folder, max_batch_size=1, device="cuda", dtype=BF, quantize="fp8_e4m3", quantize_experts=True)
    mods = {n: m for n, m in quant.named_modules() if isinstance(m, QuantLinear)}
    assert len(mods) == 2 * (4 + 4 * 3) and not isinstance(quant.layers["0"].feed_forward.gate, QuantLinear)
    for n, m in mods.items():
        assert torch.equal(m.dequantized().cpu(), w[n + ".weight"]), n
    assert len({float(s) for s in quant.layers["1"].feed_forward.experts[3].w2.qscale_weight.cpu()}) > 1
    ids = torch.randint(0, 512, (16,), generator=g).cuda()
    out = []
    for model in (plain, quant):
        cache = BufferCache(2, 1, 64, 2, 128, None, device="cuda", dtype=BF)
        pre = model.forward(ids, [16], cache)
        tok = pre[-1:].argmax(dim=-1)
        out.append((pre.cpu(), tok.cpu(), model.forward(tok, [1], cache).cpu()))
    (pre0, tok0, dec0), (pre1, tok1, dec1) = out
    assert torch.equal(pre0, pre1), float((pre0 - pre1).abs().max())
    assert torch.equal(tok0, tok1)
    assert torch.equal(dec0, dec1) and torch.equal(dec0.argmax(dim=-1), dec1.argmax(dim=-1)), float((dec0 - dec1).abs().max())
