"""Token-grouped W8A8 prefill GEMMs on FP8 experts (csrc/gemm256_moe_w8a8.hip): the leaf mi_moe_grouped_gemm_w8a8 against an fp64
statement of its rule (include/mistral_hip.h) on chosen routing, its fallback outside the predicate, and a model with the switch.
Exact family: moe_cases' (x integers in [-2, 2], x[:, 0] = 8; W in {-1, 0, 1}, W1[:, 0] = 16) with token t scaled by 2^(t % 3) and
the weights stored as e4m3 codes W / s, s = 2^((row + expert) % 3 - 1), as in test_gpu_moe_fp8.  Every code and every fp32 sum is
exact and a >= 24, so that bf16(silu(a)) == a for the fast SwiGLU too: the bf16 grouped SwiGLU test's envelope on such inputs is bit
equality, and so it is here.  Check A: the kernel's hid, read back from the leaf's scratch, equals the fp64 chain.  Check B: from
the kernel's own hid, y and the combined output equal it bit for bit.
Gaussian case: the emulation is fp32 where the kernel is (moe_cases._mm sums, the scale products, the SiLU).  Its sums alone give NO
spread against the fp64 rule (products of two e4m3 codes carry 8 significant bits); what moves bits is swiglu_bf_fast's documented
relative error of ~1e-6 (common.cuh): with it on every SiLU the emulation reaches 0.3151 (+) / 0.2191 (-) of 2^-7 S
(moe_cases.gauss_ratio), so GAUSS_HONEST = 0.32, re-measured by the test; the device may reach three times that, as
moe_cases.GAUSS_C allows.  Measured on the MI355X: 0.447."""
import ctypes as C

import pytest
import torch

import moe_cases as mc
import mistral_oracle as mo
from hip_util import write_checkpoint
from mistral_inference import _hip, quant
from test_moe_fp8_host import ARGS  # dim 512, 2 layers, hidden 1024, 4 experts, top-2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
E, K_TOP, T = 4, 2, 300
GAUSS_HONEST, SILU_FAST_ERR = 0.32, 1e-6


def _case(D, F, counts, gauss=False):
    """(inputs, x, per expert the e4m3 codes (w1q, w2q, w3q), per expert the fp32 row scales)."""
    inp = mc.inputs(mc.Case(f"w8a8-d{D}f{F}-{counts[0]}{'-g' if gauss else ''}", E, K_TOP, T, counts, D=D, F=F, gauss=gauss))
    if gauss:
        qs = [[quant.quantize_rows(w) for w in ex] for ex in inp.experts]
        return inp, inp.x, [[q for q, _ in ex] for ex in qs], [[s for _, s in ex] for ex in qs]
    x = (inp.x.float() * torch.ldexp(torch.ones(T), torch.arange(T) % 3)[:, None]).to(BF)
    scales = [[torch.ldexp(torch.ones(w.shape[0]), (torch.arange(w.shape[0]) + e) % 3 - 1) for w in ex] for e, ex in enumerate(inp.experts)]
    codes = [[(w.float() / s[:, None]).to(torch.float8_e4m3fn) for w, s in zip(ex, ss)] for ex, ss in zip(inp.experts, scales)]
    return inp, x, codes, scales


def _rule(x, hid_in, codes, scales, inp, lists, mm, silu_err=0.0):
    """The rule in compact rows, in the dtype that the matmul mm(a, w) -> a @ w^T returns (fp64, or the emulation's fp32).  hid_in:
    the hid quantised for the W2 stage (None: this chain's own); silu_err: relative error on every SiLU.  -> hid, y, out, S."""
    erow, tok_of, row_of = lists
    hid, y = torch.zeros(T * K_TOP, codes[0][0].shape[0], dtype=BF), torch.zeros(T * K_TOP, x.shape[1], dtype=BF)
    Sy = torch.zeros(y.shape, dtype=torch.float64)
    groups = [(e, rows) for e in range(E) for rows in [torch.where(erow == e)[0]] if rows.numel()]

    def gemm(a, s_a, w, s_w):  # (a w^T) * (s_a s_w): the product of the two scales is formed first
        acc = mm(a.double(), w.double())
        return acc * (s_a.to(acc.dtype)[:, None] * s_w.to(acc.dtype)[None, :])
    xq, sx = quant.quantize_rows(x)
    for e, rows in groups:
        a, b = (gemm(xq[tok_of[rows]], sx[tok_of[rows]], codes[e][i], scales[e][i]) for i in (0, 2))
        a, b = a.to(BF).to(a.dtype), b.to(BF).to(a.dtype)
        hid[rows] = ((a / (1.0 + torch.exp(-a)) * (1.0 + silu_err)).to(BF).to(a.dtype) * b).to(BF)
    hq, sh = quant.quantize_rows(hid if hid_in is None else hid_in)
    for e, rows in groups:
        y[rows] = gemm(hq[rows], sh[rows], codes[e][1], scales[e][1]).to(BF)
        Sy[rows] = (hq[rows].double().abs() * sh[rows].double()[:, None]) @ (codes[e][1].double().abs() * scales[e][1].double()[:, None]).T
    out = mc._combine(y.float(), inp.h, inp.sel_idx, inp.sel_w, row_of)
    return hid, y, out, inp.h.double().abs() + (inp.sel_w.double()[:, :, None] * Sy[row_of]).sum(dim=1)


def _device(x, codes, scales, inp, w8=False):
    """The leaf with its scratch views and the kernel's own lists as (expert of row, tok_of, row_of); w8: mi_moe_grouped_gemm_w8's output."""
    keep = [[(q.view(torch.uint8).cuda(), s.cuda()) for q, s in zip(cq, cs)] for cq, cs in zip(codes, scales)]
    tab, stab = (torch.tensor([[t[i].data_ptr() for t in ex] for ex in keep], dtype=torch.int64, device="cuda") for i in (0, 1))
    args = (E, codes[0][0].shape[0], inp.sel_idx.cuda(), inp.sel_w.cuda())
    if w8:
        return _hip.moe_experts(x.cuda(), tab, *args, residual=inp.h.cuda(), scale_tab=stab).cpu()
    out, v = _hip.moe_grouped_w8a8(x.cuda(), tab, stab, *args, residual=inp.h.cuda(), debug=True)
    v = {k: t.cpu() for k, t in v.items()}
    tok_of, row_of = v["tok_of"].long(), v["row_of"].long()
    erow = torch.empty(row_of.numel(), dtype=torch.long)
    erow[row_of.reshape(-1)] = inp.sel_idx.reshape(-1).long()
    return out.cpu(), v, (erow, tok_of, row_of)


@pytest.mark.parametrize("counts", [(0, 256, 257, 87), (300, 0, 0, 300)], ids=["edges", "short-table"])
@pytest.mark.parametrize("D,F", [(384, 640), (128, 128), (256, 1152)])
def test_leaf_is_the_fp64_rule_bit_for_bit_on_exact_inputs(D, F, counts):
    inp, x, codes, scales = _case(D, F, counts)
    out, v, lists = _device(x, codes, scales, inp)
    hid = _rule(x, None, codes, scales, inp, lists, lambda a, w: a @ w.T)[0]
    _, y, want, _ = _rule(x, v["hid"], codes, scales, inp, lists, lambda a, w: a @ w.T)
    for name, got, ref in (("hid (check A)", v["hid"], hid), ("y (check B)", v["y"], y), ("out (check B)", out, want)):
        bad = torch.nonzero((got != ref).any(dim=1))[:, 0].tolist()
        assert not bad, (name, len(bad), "rows differ; first (row, expert, token):", [(r, int(lists[0][r]), int(lists[1][r])) for r in bad[:6]])


def test_gaussian_leaf_inside_three_times_the_emulations_spread():
    inp, x, codes, scales = _case(384, 640, (0, 256, 257, 87), gauss=True)
    out, _, lists = _device(x, codes, scales, inp)
    _, _, ref, S = _rule(x, None, codes, scales, inp, lists, lambda a, w: a @ w.T)
    emu = [mc.gauss_ratio(_rule(x, None, codes, scales, inp, lists, mc._mm, silu_err=e)[2], ref, S) for e in (0.0, SILU_FAST_ERR, -SILU_FAST_ERR)]
    got = mc.gauss_ratio(out, ref, S)
    print("fp32 emulation to fp64 rule (sums alone, + and - the fast SiLU's error), then the device, of 2^-7 S:", emu, got)
    assert max(emu) <= GAUSS_HONEST and got <= 3 * GAUSS_HONEST, (emu, got)


@pytest.mark.parametrize("Tn,D", [(255, 384), (300, 272)], ids=["T255", "D272"])
def test_outside_the_predicate_the_leaf_is_the_dequantisation_route(Tn, D):
    """The bytes of mi_moe_grouped_gemm_w8 (D = 264 is refused by both leaves alike, test_moe_w8a8_host: D = 272 stands for it)."""
    inp, x, codes, scales = _case(D, 640, (0, 256, 257, 87))
    inp = mc.Inputs(x[:Tn], inp.h[:Tn], inp.experts, inp.sel_idx[:Tn], inp.sel_w[:Tn])
    assert torch.equal(_device(inp.x, codes, scales, inp)[0], _device(inp.x, codes, scales, inp, w8=True))


def test_model_with_the_switch(tmp_path):
    """300 rows: the envelope of test_gpu_w8a8's long-prompt test against the weight-only model (finite, the route really taken, the
    figure printed).  12 rows and decode steps: the switch changes no bit.  A workspace one byte short: MI_ERR_WORKSPACE."""
    from mistral_inference.cache import BufferCache
    from mistral_inference.transformer import Transformer
    src = write_checkpoint(tmp_path / "bf16", ARGS, mo.synth_weights(ARGS, seed=5))
    folder = str(quant.quantize_checkpoint(src, tmp_path / "fp8", experts=True))
    model = Transformer.from_folder(folder, max_batch_size=1, device="cuda", dtype=BF, prefill_fp8_experts=True)
    ids = torch.randint(0, 512, (T,), generator=torch.Generator().manual_seed(300)).cuda()
    prompt = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8], device="cuda")
    runs = []
    with torch.inference_mode():
        for on in (False, True):
            model.prefill_fp8_experts = on
            cache = BufferCache(2, 1, 512, 2, 128, None, device="cuda", dtype=BF)
            steps = [model.forward(prompt, [12], cache)]
            for _ in range(4):
                steps.append(model.forward(steps[-1][-1:].argmax(-1), [1], cache))
            runs.append((model.forward(ids, [T], None), steps))
    (off, steps_off), (on, steps_on) = runs
    print(f"logits on to off: max |d| = {float((on - off).abs().max()):.4e}")
    assert bool(torch.isfinite(on).all()) and not torch.equal(on, off)
    assert all(torch.equal(a, b) for a, b in zip(steps_on, steps_off))
    be, L = model._backend, _hip.lib()
    m, qm = be.plan(model), be._quant[0]
    need = L.mi_workspace_bytes_moe_w8a8(C.byref(m), C.byref(qm), be._moe_q, None, T, 1, 1, 0)
    assert 0 < need <= be._workspace.numel() and need < L.mi_workspace_bytes_moe_w8(C.byref(m), C.byref(qm), be._moe_q, None, T, 1, 1, 0)
    i32, hbuf = torch.zeros(T + 2, dtype=torch.int32, device="cuda"), torch.zeros(T, 512, dtype=BF, device="cuda")
    bt = _hip.MiBatch()
    bt.T, bt.B, bt.branch, bt.max_q_len, bt.input_ids = T, 1, _hip.BRANCH_NOCACHE, T, ids.data_ptr()
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = i32.data_ptr()
    bt.h, bt.workspace, bt.workspace_bytes = hbuf.data_ptr(), be._workspace.data_ptr(), need - 1
    assert L.mi_forward_moe_w8a8(C.byref(m), C.byref(qm), be._moe_q, None, C.byref(bt), None) == -3 and "workspace" in L.mi_last_error_detail().decode()
