"""A quantised LM head on the host: the conditions of lm_head_cases' inputs, its emulation against the reference, the single
faults a test on those inputs can see, and the host logic of the feature - the params.json flag, the refusals, the checkpoint
writer, the new C symbols and their argument checks.  Nothing here needs a device."""
import ctypes as C
import json

import pytest
import safetensors
import torch
from safetensors.torch import save_file

import lm_head_cases as lc
import mistral_oracle as mo
from hip_util import write_checkpoint
from mistral_inference import _hip
from mistral_inference.args import QuantizationArgs, TransformerArgs
from mistral_inference.quant import QSCALE_KEY, QUANT_LINEARS, QuantLinear, quantize_checkpoint
from mistral_inference.transformer import Transformer

ARGS = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                     sliding_window=16)
K, M = 288, 5
SHAPES = [(kind, n) for kind in lc.KINDS for n in (520, 521)]
FORMATS = [("fp8_e4m3", torch.float8_e4m3fn, torch.float32), ("mxfp4", torch.uint8, torch.uint8)]


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("kind,N", SHAPES)
def test_conditions_round_trip_and_emulation(kind, N):
    """The quantiser reproduces every weight, every sum is an exact integer sum below 2^24, at least a quarter of the sums are
    not bf16 values (the issue's two families: 256 < |y| < 1024 and at least 5 % exact ties, the shares of linear_cases'
    rounding family), and the emulation of the kernel's arithmetic is the fp64 reference bit for bit."""
    hd, x = lc.head(kind, N, K), lc.x_rows(kind, M, K)
    fig = lc.conditions(hd, x)
    print(f"{kind} N={N}: scales {fig['scales']}, {fig['miny']:.0f} <= |y| <= {fig['maxy']:.0f}, sum|w x| <= {fig['bound']:.0f}, "
          f"not bf16 values {100 * fig['inexact']:.1f} %, ties {100 * fig['ties']:.1f} %, zeros {100 * fig['zeros']:.1f} %")
    if kind == lc.FP8:
        assert fig["scales"] == [0.125, 0.25]
    if kind == lc.MXFP4:
        assert fig["scales"] == [125, 127]
    if kind == lc.FP8_HAND:
        assert fig["scales"] == [0.75, 1.5, 3.0]
        lin = QUANT_LINEARS["fp8_e4m3"](K, N)
        lin.load_quantized(hd.weight, hd.scale)                      # hand-made scales are bound as they are
        assert torch.equal(lin.qscale_weight, hd.scale) and torch.equal(lin.weight, hd.weight)
    assert torch.equal(lc.emulate(hd, x), lc.reference(hd, x))


def test_a_weight_off_the_e4m3_grid_does_not_survive():
    """c = 68 (not a multiple of 8 in [56, 104]) under the row scale 0.25 is 272: e4m3 holds 256 and 288 there."""
    from mistral_inference.quant import dequantize, quantize_rows
    w = torch.ones(2, 16)
    w[0, 0], w[1, 0] = 68.0, 72.0
    q, s = quantize_rows(w.to(lc.BF))
    back = dequantize(q, s).float()
    assert not torch.equal(back[0], w[0]) and torch.equal(back[1], w[1])


@pytest.mark.parametrize("fault", lc.FAULTS)
def test_every_single_fault_changes_some_case(fault):
    seen, lines = 0, []
    for kind, N in SHAPES:
        hd, x = lc.head(kind, N, K), lc.x_rows(kind, M, K)
        got = lc.emulate(hd, x, fault)
        if got is None:
            continue
        n = int((got != lc.reference(hd, x)).sum())
        lines.append(f"{kind}/{N}: {n}")
        seen += n > 0
    print(f"{fault}: differing logits per case (of {M} x N) - " + ", ".join(lines))
    assert lines and seen > 0, fault
    if fault in ("piece_dropped", "not_rounded", "odd_row_aliased"):   # ... and these on every case they apply to
        assert seen == len(lines), (fault, lines)
    if fault == "scale_next_row":                                      # invisible only where all rows share their scales: plain mxfp4
        assert seen == len(lines) - 2, (fault, lines)


# ------------------------------------------------------------------------------------------------ params.json, writer, loader
def test_params_flag_round_trip_and_default():
    base = mo.params_json(ARGS)
    a = TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "mxfp4", "lm_head": True}})
    assert a.quantization == QuantizationArgs("mxfp4", lm_head=True) and a.quantization.lm_head is True
    assert TransformerArgs.from_dict(a.to_dict()).quantization == a.quantization
    b = TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "mxfp4"}})   # a folder without the key: as before
    assert b.quantization == QuantizationArgs("mxfp4") and b.quantization.lm_head is False


@pytest.fixture(scope="module")
def bf16_folder(tmp_path_factory):
    w = mo.synth_weights(ARGS, seed=21)
    return write_checkpoint(tmp_path_factory.mktemp("lm_head") / "bf16", ARGS, w), w


def _tensors(folder):
    with safetensors.safe_open(str(folder / "consolidated.safetensors"), framework="pt", device="cpu") as f:
        return {k: f.get_tensor(k) for k in f.keys()}


@pytest.mark.parametrize("qformat,wdt,sdt", FORMATS)
def test_checkpoint_writer_with_and_without_the_head(bf16_folder, tmp_path, qformat, wdt, sdt):
    src, w = bf16_folder
    cls = QUANT_LINEARS[qformat]
    plain = quantize_checkpoint(src, tmp_path / "plain", qformat=qformat)
    assert json.load(open(plain / "params.json"))["quantization"] == {"qformat_weight": qformat}      # no key: exactly as before
    sd = _tensors(plain)
    assert sd["output.weight"].dtype == torch.bfloat16 and torch.equal(sd["output.weight"], w["output.weight"])
    assert "output." + QSCALE_KEY not in sd
    full = quantize_checkpoint(src, tmp_path / "full", qformat=qformat, lm_head=True)
    assert json.load(open(full / "params.json"))["quantization"] == {"qformat_weight": qformat, "lm_head": True}
    sdh = _tensors(full)
    qw, qs = cls.quantize(w["output.weight"])
    assert sdh["output.weight"].dtype == wdt and sdh["output." + QSCALE_KEY].dtype == sdt
    assert torch.equal(sdh["output.weight"].view(torch.uint8), qw.view(torch.uint8)) and torch.equal(sdh["output." + QSCALE_KEY], qs)
    assert sdh["tok_embeddings.weight"].dtype == torch.bfloat16                                        # the embedding table stays
    assert set(sdh) == set(sd) | {"output." + QSCALE_KEY}
    for k in sd:
        if k != "output.weight":
            assert torch.equal(sdh[k].view(torch.uint8) if sdh[k].dtype == wdt else sdh[k], sd[k].view(torch.uint8) if sd[k].dtype == wdt else sd[k]), k

    # the loader: the folder's flag builds the format's QuantLinear as the head; without it the head is nn.Linear as ever
    m = Transformer.from_folder(full, device="cpu")
    assert isinstance(m.output, cls) and m.args.quantization.lm_head and m.dtype == torch.bfloat16
    assert torch.equal(m.output.weight, qw.view(torch.uint8)) and torch.equal(m.output.qscale_weight, qs)
    assert isinstance(m.tok_embeddings, torch.nn.Embedding) and m.tok_embeddings.weight.dtype == torch.bfloat16
    p = Transformer.from_folder(plain, device="cpu")
    assert type(p.output) is torch.nn.Linear and p.output.weight.dtype == torch.bfloat16 and not p.args.quantization.lm_head
    # quantise while loading: from the bf16 folder, and the head alone on top of a folder whose layers are quantised
    for folder, kw in ((src, dict(quantize=qformat, quantize_lm_head=True)), (plain, dict(quantize_lm_head=True))):
        o = Transformer.from_folder(folder, device="cpu", **kw)
        assert isinstance(o.output, cls) and o.args.quantization.lm_head
        pm, po = dict(m.named_parameters()), dict(o.named_parameters())
        assert set(pm) == set(po) and all(pm[k].dtype == po[k].dtype and torch.equal(pm[k], po[k]) for k in pm)

    # a folder whose flag and tensors disagree is refused by name, either way round
    bad = tmp_path / "flag_without_tensors"
    bad.mkdir()
    json.dump(json.load(open(full / "params.json")), open(bad / "params.json", "w"))
    save_file(sd, str(bad / "consolidated.safetensors"))
    with pytest.raises(ValueError, match="lm_head.*disagree"):
        Transformer.from_folder(bad, device="cpu")
    bad2 = tmp_path / "tensors_without_flag"
    bad2.mkdir()
    json.dump(json.load(open(plain / "params.json")), open(bad2 / "params.json", "w"))
    save_file(sdh, str(bad2 / "consolidated.safetensors"))
    with pytest.raises(ValueError, match="lm_head.*disagree"):
        Transformer.from_folder(bad2, device="cpu")


def test_quantize_lm_head_without_a_weight_format_is_refused_by_name(bf16_folder):
    with pytest.raises(NotImplementedError, match="quantize_lm_head=True without a weight format"):
        Transformer.from_folder(bf16_folder[0], device="cpu", quantize_lm_head=True)


def test_only_the_last_pipeline_rank_holds_a_quantised_head():
    a = TransformerArgs.from_dict({**mo.params_json(ARGS), "quantization": {"qformat_weight": "fp8_e4m3", "lm_head": True}})
    with torch.device("meta"):
        first, last = (Transformer(a, pipeline_rank=r, num_pipeline_ranks=2).to(torch.bfloat16) for r in (0, 1))
    assert first.output is None and not any(k.startswith("output") for k in first.state_dict())
    assert isinstance(last.output, QuantLinear) and last.output.weight.dtype == torch.uint8 and last.dtype == torch.bfloat16
    assert (last.output.out_features, last.output.in_features) == (ARGS.vocab_size, ARGS.dim)


def test_the_tools_take_the_flag():
    import inspect
    from mistral_inference import main
    for fn in (main.interactive, main.demo):
        assert inspect.signature(fn).parameters["quantize_lm_head"].default is False


# ------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("mi_lm_head_q_scratch_bytes", "mi_lm_head_q", "mi_lm_head_logprobs_q_scratch_bytes", "mi_lm_head_logprobs_q",
               "mi_workspace_bytes_q", "mi_forward_q")
FAKE = 0x10000  # never dereferenced: every call below is refused before any launch


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _hip.lib()
    assert L.mi_abi_version() == 9 == _hip.MI_ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert C.sizeof(_hip.MiLmHeadQuant) == 16 and _hip.MI_LM_HEAD_SLICE_ROWS == 8192


def _model(**kw):
    layers = (_hip.MiLayer * 2)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 2
    m.norm_eps = 1e-5
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    for k, v in kw.items():
        setattr(m, k, v)
    return m, layers


def _quant_structs():
    s8, s4 = (_hip.MiW8Layer * 2)(), (_hip.MiW4Layer * 2)()
    w8, w4 = _hip.MiW8Model(), _hip.MiW4Model()
    w8.format, w8.layers = _hip.MI_W8_FP8_E4M3, C.cast(s8, C.POINTER(_hip.MiW8Layer))
    w4.format, w4.layers = _hip.MI_W4_MXFP4, C.cast(s4, C.POINTER(_hip.MiW4Layer))
    return w8, w4, (s8, s4)


def _head(fmt, scale=FAKE):
    hq = _hip.MiLmHeadQuant()
    hq.format, hq.scale = fmt, scale
    return hq


def _detail():
    return _hip.lib().mi_last_error_detail().decode()


def test_the_entry_with_a_null_head_answers_as_the_old_entries():
    """Argument errors of mi_forward, _w8, _w4, _w8a8, _w4a8 and _verify, and the same call through mi_forward_q(head = NULL): the
    same code and the same detail (the old entry's name included)."""
    L = _hip.lib()
    w8, w4, _keep = _quant_structs()
    bt, vo = _hip.MiBatch(), _hip.MiVerifyOut()
    dense, _k0 = _model()
    moe, _k1 = _model(num_experts=8, top_k=2)
    lora, _k2 = _model(lora_rank=8, lora_scaling=2.0)
    odd, _k3 = _model(hidden_dim=1032)
    bad8 = _hip.MiW8Model()
    bad8.format, bad8.layers = 2, w8.layers
    R8, R4, RB = C.byref(w8), C.byref(w4), C.byref(bt)
    pairs = []
    for m in (dense, moe, lora, odd):
        Rm = C.byref(m)
        pairs += [(lambda Rm=Rm: L.mi_forward(Rm, RB, None), lambda Rm=Rm: L.mi_forward_q(Rm, None, None, None, RB, None, 0, None)),
                  (lambda Rm=Rm: L.mi_forward_w8(Rm, R8, RB, None), lambda Rm=Rm: L.mi_forward_q(Rm, R8, None, None, RB, None, 0, None)),
                  (lambda Rm=Rm: L.mi_forward_w4(Rm, R4, RB, None), lambda Rm=Rm: L.mi_forward_q(Rm, None, R4, None, RB, None, 0, None)),
                  (lambda Rm=Rm: L.mi_forward_w8a8(Rm, R8, RB, None), lambda Rm=Rm: L.mi_forward_q(Rm, R8, None, None, RB, None, 1, None)),
                  (lambda Rm=Rm: L.mi_forward_w4a8(Rm, R4, RB, None), lambda Rm=Rm: L.mi_forward_q(Rm, None, R4, None, RB, None, 1, None)),
                  (lambda Rm=Rm: L.mi_forward_verify(Rm, R8, None, RB, C.byref(vo), None),
                   lambda Rm=Rm: L.mi_forward_q(Rm, R8, None, None, RB, C.byref(vo), 0, None)),
                  (lambda Rm=Rm: L.mi_forward_verify(Rm, R8, R4, RB, C.byref(vo), None),
                   lambda Rm=Rm: L.mi_forward_q(Rm, R8, R4, None, RB, C.byref(vo), 0, None))]
    Rd = C.byref(dense)
    pairs.append((lambda: L.mi_forward_w8(Rd, C.byref(bad8), RB, None), lambda: L.mi_forward_q(Rd, C.byref(bad8), None, None, RB, None, 0, None)))
    codes = set()
    for old, new in pairs:
        rc_old, d_old = old(), _detail()
        rc_new, d_new = new(), _detail()
        assert rc_old != 0 and (rc_new, d_new) == (rc_old, d_old), (rc_old, d_old, rc_new, d_new)
        codes.add(rc_old)
    assert {-1, -4, _hip.MI_ERR_SHAPE} <= codes, codes
    assert L.mi_forward_q(Rd, None, None, None, RB, None, 1, None) == -1 and "a8 without w8 or w4" in _detail()

    # ... and sizes a workspace as the old queries do
    for T, B, W in ((1, 1, 16), (3, 3, 4096), (12, 1, 16), (300, 2, 64)):
        for kvl in (0, 1):
            assert L.mi_workspace_bytes_q(Rd, None, None, None, T, B, W, kvl, 0, 0) == L.mi_workspace_bytes_kv(Rd, 0, T, B, W, kvl)
            assert L.mi_workspace_bytes_q(Rd, R8, None, None, T, B, W, kvl, 0, 0) == L.mi_workspace_bytes_kv(Rd, 1, T, B, W, kvl)
            assert L.mi_workspace_bytes_q(Rd, None, R4, None, T, B, W, kvl, 0, 0) == L.mi_workspace_bytes_kv(Rd, 1, T, B, W, kvl)
            assert L.mi_workspace_bytes_q(Rd, R8, None, None, T, B, W, kvl, 1, 0) == L.mi_workspace_bytes_w8a8(Rd, R8, T, B, W, kvl)
            assert L.mi_workspace_bytes_q(Rd, None, R4, None, T, B, W, kvl, 1, 0) == L.mi_workspace_bytes_w4a8(Rd, R4, T, B, W, kvl)
            assert L.mi_workspace_bytes_q(Rd, R8, None, None, T, B, W, kvl, 0, 1) == L.mi_workspace_bytes_verify(Rd, 1, T, W, kvl)
            # a head: exactly the slice behind everything else, for more than 8 rows only (vocab 512 < 8192: the whole head)
            extra = L.mi_workspace_bytes_q(Rd, R8, None, C.byref(_head(1)), T, B, W, kvl, 0, 0) - L.mi_workspace_bytes_kv(Rd, 1, T, B, W, kvl)
            assert extra == (512 * 512 * 2 if T > 8 else 0), (T, extra)
    big, _k4 = _model(vocab_size=131072)
    Rb = C.byref(big)
    extra = L.mi_workspace_bytes_q(Rb, None, R4, C.byref(_head(2)), 300, 1, 64, 0, 0, 0) - L.mi_workspace_bytes_kv(Rb, 1, 300, 1, 64, 0)
    assert extra == 8192 * 512 * 2                                    # does not grow with the vocabulary
    assert L.mi_workspace_bytes_q(Rd, None, None, C.byref(_head(1)), 12, 1, 16, 0, 0, 0) == 0   # a head without quantised layers


def test_the_new_refusals_name_themselves():
    L = _hip.lib()
    w8, w4, _keep = _quant_structs()
    bt = _hip.MiBatch()
    dense, _k0 = _model()
    Rd, RB = C.byref(dense), C.byref(bt)
    assert L.mi_forward_q(Rd, C.byref(w8), None, C.byref(_head(_hip.MI_W4_MXFP4)), RB, None, 0, None) == -4
    assert "mi_forward_q" in _detail() and "LM head format 2" in _detail() and "MI_W8_FP8_E4M3" in _detail()
    assert L.mi_forward_q(Rd, None, C.byref(w4), C.byref(_head(_hip.MI_W8_FP8_E4M3)), RB, None, 0, None) == -4
    assert "LM head format 1" in _detail() and "MI_W4_MXFP4" in _detail()
    assert L.mi_forward_q(Rd, None, None, C.byref(_head(1)), RB, None, 0, None) == -4
    assert "a quantised LM head on a model without quantised layers" in _detail()
    assert L.mi_forward_q(Rd, C.byref(w8), None, C.byref(_head(1, None)), RB, None, 0, None) == -1 and "without row scales" in _detail()
    for fmt, q, dim in ((1, dict(w8=C.byref(w8), w4=None), 520), (2, dict(w8=None, w4=C.byref(w4)), 528)):   # 520 % 16, 528 % 32 != 0
        m, _k = _model(dim=dim)
        assert L.mi_forward_q(C.byref(m), q["w8"], q["w4"], C.byref(_head(fmt)), RB, None, 0, None) == _hip.MI_ERR_SHAPE
        assert "mi_forward_q" in _detail() and "dim" in _detail() and str(16 * fmt) in _detail()
    moe, _k1 = _model(num_experts=8, top_k=2)                         # whatever the old entries refuse, under the new name
    assert L.mi_forward_q(C.byref(moe), C.byref(w8), None, C.byref(_head(1)), RB, None, 0, None) == -4 and "MoE" in _detail()


def test_the_leaves_check_their_arguments():
    L = _hip.lib()

    def logits(K=32, M=2, fmt=1, scale=FAKE, w=FAKE, scratch=None, nbytes=0, norm=None, head=True):
        return L.mi_lm_head_q(FAKE, 64, FAKE, K, M, K, w, 64, C.byref(_head(fmt, scale)) if head else None, norm, 0.0, scratch, nbytes, None)

    assert logits(w=None) == -1 and logits(head=False) == -1 and logits(scale=None) == -1
    assert logits(fmt=3) == -4 and "LM head format 3" in _detail()
    assert logits(K=24) == _hip.MI_ERR_SHAPE and "mi_lm_head_q" in _detail() and "16" in _detail()
    assert logits(K=48, fmt=2) == _hip.MI_ERR_SHAPE and "32" in _detail()
    assert logits(M=9) == -3 and "scratch" in _detail()                # more than 8 rows: needs the slice
    assert logits(M=9, scratch=FAKE, nbytes=1 << 20, norm=FAKE) == -4 and "fused RMSNorm" in _detail()
    assert L.mi_lm_head_q_scratch_bytes(8, 512, 131072) == 0
    assert L.mi_lm_head_q_scratch_bytes(9, 512, 131072) == 8192 * 512 * 2 == L.mi_lm_head_q_scratch_bytes(4096, 512, 8192)
    assert L.mi_lm_head_q_scratch_bytes(9, 512, 521) == (521 * 512 * 2 + 255) // 256 * 256
    # the old leaves keep refusing the head by name (test_fp8_host / test_mxfp4_host pin it; restated where the new leaf is)
    base = L.mi_lm_head_logprobs_scratch_bytes(300, 8492)
    assert L.mi_lm_head_logprobs_q_scratch_bytes(300, 512, 8492) == (base + 255) // 256 * 256 + 8192 * 512 * 2
    assert L.mi_lm_head_logprobs_q_scratch_bytes(4, 512, 8492) == (L.mi_lm_head_logprobs_scratch_bytes(4, 8492) + 255) // 256 * 256
    lp = lambda K=32, fmt=1, nbytes=1 << 30: L.mi_lm_head_logprobs_q(FAKE, FAKE, K, 2, K, FAKE, 64, C.byref(_head(fmt)), FAKE, FAKE, nbytes, None)  # noqa: E731
    assert lp(K=24) == _hip.MI_ERR_SHAPE and lp(fmt=0) == -4 and lp(nbytes=8) == -3 and "mi_lm_head_logprobs_q" in _detail()
