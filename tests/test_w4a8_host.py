"""MXFP4 x FP8 prefill GEMMs (W4A8), host side: the structured cases of tests/w4a8_cases.py are what they claim (activations lossless
under quantize_rows, exact sums, the SwiGLU and rounding-point conditions, the fp64-chain reference reproduced by the CPU emulation
of the route and missed by every single-fault mutant), the refusal texts of `prefill_w4a8`, the CLI flag, the ABI entries."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

import linear_cases as lc
import mistral_oracle as mo
import w4a8_cases as wc
from mistral_inference import _hip, main, quant
from mistral_inference.transformer import Transformer

CASES = wc.all_cases()
ARGS = mo.OracleArgs(dim=512, n_layers=2, head_dim=128, hidden_dim=1024, n_heads=4, n_kv_heads=2, norm_eps=1e-5, vocab_size=512,
                     sliding_window=16)
GROUPS = [lc.STORE, lc.RESIDUAL, lc.SWIGLU, lc.QKV]


def test_the_case_list_reaches_every_edge():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.M for c in CASES} == {256, 257, 300, 512, 513} and {c.K for c in CASES} == {128, 256, 384, 1152}
    for epi in (lc.STORE, lc.RESIDUAL):
        assert {c.segs for c in CASES if c.epi == epi} == set(wc.SEGS)
    assert {c.N for c in CASES if c.epi == lc.SWIGLU} == {64, 128, 136}
    assert {c.qkv[:2] for c in CASES if c.epi == lc.QKV} == {(1, 1), (2, 1)}
    assert all(c.M >= wc.MIN_M and c.K % wc.K_MOD == 0 for c in CASES)                  # every case takes the new route
    for epi in (lc.RESIDUAL, lc.SWIGLU, lc.QKV):
        assert {c.fam for c in CASES if c.epi == epi} == {"plain", "round"}


@pytest.mark.parametrize("group", GROUPS)
def test_activations_round_trip_sums_are_exact_and_the_conditions_hold(group):
    """x of every case is dequantize(quantize_rows(x)) bit for bit; per output sum |w x| stays below 2^24 units of its smallest
    product; the SwiGLU and rounding-point conditions hold; neighbouring blocks, rows, K tiles and segments carry different scales,
    and neighbouring activation rows too."""
    seen_sx = False
    for case in (c for c in CASES if c.epi == group):
        assert wc.round_trips(case), case
        fig = wc.conditions(case)
        assert fig["bound"] < 2 ** 24
        inp = wc.inputs(case)
        sx = quant.quantize_rows(inp.x)[1]
        seen_sx = seen_sx or bool((sx[0::2][:case.M // 2] != sx[1::2][:case.M // 2]).any())
        for s in inp.scales:
            assert bool((s[:, :-1] != s[:, 1:]).any()) or s.shape[1] == 1            # blocks
            assert s.shape[0] == 1 or bool((s[:-1] != s[1:]).any(dim=1).all())        # every row against the row beside
            if case.K >= 256:
                assert bool((s[:, :-4] != s[:, 4:]).any())                             # the same block one K tile on
        if len(inp.scales) > 1:
            n = min(inp.scales[0].shape[0], inp.scales[1].shape[0])
            assert bool((inp.scales[0][:n] != inp.scales[1][:n]).any())               # segments
        print(f"{case.name:36s} " + " ".join(f"{k} {v:.3f}" for k, v in fig.items() if not isinstance(v, tuple)))
    assert seen_sx


@pytest.mark.parametrize("group", GROUPS)
def test_the_emulated_route_is_the_reference_and_every_mutant_is_seen(group):
    """emulate(case) - quantise, contract block by block under the block's scale, s_x in fp32, epilogue - is bit-equal to the
    fp64-chain reference inside its guard buffer on every case, and each single-fault mutant changes at least one case it applies
    to - in every group, i.e. in every instantiation of the kernel's epilogue."""
    seen = {m: [0, 0] for m in wc.MUTANTS}
    for case in (c for c in CASES if c.epi == group):
        want = wc.expected(case)
        assert torch.equal(wc.emulate(case), want), (case, lc.describe(case, wc.emulate(case), want))
        for m in wc.MUTANTS:
            if wc.applies(case, m) and seen[m][0] < 3:      # (three sightings are proof enough: the rest of the cases are not run)
                seen[m][1] += 1
                seen[m][0] += int(not torch.equal(wc.emulate(case, m), want))
    for m, (hit, n) in seen.items():
        print(f"{group:9s} {m:28s} seen in {hit}/{n} cases")
    absent = {"scale_wrong_segment"} if group == lc.SWIGLU else {"w1_w3_exchanged"}  # (W1 | W3 is not a segmented group, and the reverse)
    must = [m for m in wc.MUTANTS if m not in absent]
    assert all(seen[m][1] >= 1 and seen[m][0] >= 1 for m in must), seen


def test_the_documents_state_the_contract():
    assert "prefill_w4a8" in quant.__doc__ and "gemm256_w4a8.hip" in quant.__doc__ and "below 3" in quant.__doc__


def test_prefill_w4a8_is_refused_by_name_where_the_weights_are_not_mxfp4(tmp_path):
    base = mo.params_json(ARGS)

    def folder(name, extra):
        d = tmp_path / name
        d.mkdir()
        json.dump({**base, **extra}, open(d / "params.json", "w"))
        return d
    text = quant._REFUSALS["prefill_w4a8"]
    assert text.count("{what}") == 1 and text.startswith("prefill_w4a8=True on ")
    pat = re.escape(text.split("{what}")[1][:60])
    with pytest.raises(NotImplementedError, match="without MXFP4 weights.*" + pat):
        Transformer.from_folder(folder("bf16", {}), device="cpu", prefill_w4a8=True)
    with pytest.raises(NotImplementedError, match="FP8 weights.*" + pat):
        Transformer.from_folder(folder("w8", {"quantization": {"qformat_weight": "fp8_e4m3"}}), device="cpu", prefill_w4a8=True)
    with pytest.raises(NotImplementedError, match="FP8 weights.*" + pat):
        Transformer.from_folder(folder("w8b", {}), device="cpu", quantize="fp8_e4m3", prefill_w4a8=True)
    with pytest.raises(NotImplementedError, match="float16 storage.*" + pat):
        Transformer.from_folder(folder("f16", {}), device="cpu", dtype=torch.float16, prefill_w4a8=True)
    with pytest.raises(NotImplementedError, match="float32 storage.*" + pat):
        Transformer.from_folder(folder("f32", {"quantization": {"qformat_weight": "mxfp4"}}), device="cpu", dtype=torch.float32,
                                prefill_w4a8=True)
    with pytest.raises(NotImplementedError, match="float16 storage.*" + pat):
        Transformer.from_folder(folder("f16q", {}), device="cpu", dtype=torch.float16, quantize="mxfp4", prefill_w4a8=True)
    # prefill_fp8 on MXFP4 weights stays refused, with its own text
    with pytest.raises(NotImplementedError, match="prefill_fp8=True on MXFP4 weights"):
        Transformer.from_folder(folder("w4", {"quantization": {"qformat_weight": "mxfp4"}}), device="cpu", prefill_fp8=True)
    # the settable attribute refuses the same way, and leaves the flag off
    from mistral_inference.args import TransformerArgs
    with torch.device("meta"):
        plain = Transformer(TransformerArgs.from_dict(base))
        fp8 = Transformer(TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "fp8_e4m3"}}))
        w4 = Transformer(TransformerArgs.from_dict({**base, "quantization": {"qformat_weight": "mxfp4"}}))
    with pytest.raises(NotImplementedError, match="without MXFP4 weights"):
        plain.prefill_w4a8 = True
    with pytest.raises(NotImplementedError, match="FP8 weights"):
        fp8.prefill_w4a8 = True
    assert plain.prefill_w4a8 is False and fp8.prefill_w4a8 is False
    assert not any(m.prefill_w4a8 for m in fp8.modules() if isinstance(m, quant.QuantLinear))
    w4.prefill_w4a8 = True
    assert w4.prefill_w4a8 is True and all(m.prefill_w4a8 for m in w4.modules() if isinstance(m, quant.Mxfp4Linear))
    assert any(isinstance(m, quant.Mxfp4Linear) for m in w4.modules()) and w4.prefill_fp8 is False
    w4.prefill_w4a8 = False
    assert not any(m.prefill_w4a8 for m in w4.modules() if isinstance(m, quant.Mxfp4Linear))


class _Stop(Exception):
    pass


def test_cli_flag_reaches_from_folder(monkeypatch):
    """`mistral-chat` / `mistral-demo` are Fire(interactive) / Fire(demo): a bool keyword is the `--prefill_w4a8` flag.  Called with
    the loader stubbed, the keyword must arrive at from_folder - True when given, False by default."""
    seen = []

    class FakeModel:
        @staticmethod
        def from_folder(folder, **kw):
            seen.append(kw)
            raise _Stop

    class FakeTok:
        class instruct_tokenizer:
            tokenizer = None
    monkeypatch.setattr(main, "get_model_cls", lambda path: FakeModel)
    monkeypatch.setattr(main, "load_tokenizer", lambda path: FakeTok)
    monkeypatch.setattr(main, "init_pipeline", lambda: 1)
    monkeypatch.setattr(main, "is_torchrun", lambda: False)
    for fn in (main.interactive, main.demo):
        assert inspect.signature(fn).parameters["prefill_w4a8"].default is False
        for kw, want in (({}, False), ({"prefill_w4a8": True}, True), ({"prefill_w4a8": 1, "quantize": "mxfp4"}, True)):
            with pytest.raises(_Stop):
                fn("/nonexistent/model", **kw)
            assert seen[-1]["prefill_w4a8"] is want and seen[-1]["prefill_fp8"] is False and seen[-1]["quantize"] == kw.get("quantize"), \
                (fn.__name__, kw, seen[-1])
    assert len(seen) == 6
    assert inspect.signature(Transformer.from_folder).parameters["prefill_w4a8"].default is False


NEW = ["mi_linear_w4a8_scratch_bytes", "mi_linear_w4a8", "mi_qkv_rope_w4a8", "mi_workspace_bytes_w4a8", "mi_forward_w4a8"]


def test_header_and_exported_symbols_agree_on_the_new_entries():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mistral_hip.h")).read()
    L = _hip.lib()
    for n in NEW:
        assert n in _hip.EXPORTED_SYMBOLS and re.search(r"\b" + n + r"\(", header) and hasattr(L, n), n
    assert callable(_hip.linear_w4a8) and callable(_hip.qkv_rope_w4a8)


_vp = C.c_void_p
FAKE = 0x10000  # never dereferenced: every call below is refused before any launch


def test_argument_checks_scratch_sizes_and_workspace_sizes():
    L = _hip.lib()
    nr = (C.c_int * 3)(64, 32, 0)
    # outside the route's shape - few rows, K % 128 != 0, K above the quantiser's 16384 - the leaf is mi_linear_w4: its scratch
    for M, K in ((8, 256), (9, 256), (255, 256), (256, 64), (300, 192), (512, 1056), (300, 16512), (4096, 28672)):
        assert L.mi_linear_w4a8_scratch_bytes(M, K, nr, _hip.EPI_STORE) == L.mi_linear_w4_scratch_bytes(M, K, nr, _hip.EPI_STORE)
    # inside it: the larger of x_q | s_x and mi_linear_w4's image (misaligned operands still take that route)
    assert L.mi_linear_w4a8_scratch_bytes(256, 128, nr, _hip.EPI_STORE) == max(256 * 128 + 256 * 4, 96 * 128 * 2)
    assert L.mi_linear_w4a8_scratch_bytes(300, 384, nr, _hip.EPI_SWIGLU) == max(300 * 384 + (300 * 4 + 255) // 256 * 256, 128 * 384 * 2)
    big = (C.c_int * 3)(4096, 0, 0)
    assert L.mi_linear_w4a8_scratch_bytes(256, 128, big, _hip.EPI_STORE) == 4096 * 128 * 2 == L.mi_linear_w4_scratch_bytes(256, 128, big, _hip.EPI_STORE)
    wp, sp = (_vp * 3)(FAKE, None, None), (_vp * 3)(FAKE, None, None)
    n1 = (C.c_int * 3)(64, 0, 0)
    call = lambda M, K, epi, scratch=None, nbytes=0: L.mi_linear_w4a8(FAKE, 64, FAKE, K, M, K, wp, n1, epi, None, None, 0.0, sp, scratch, nbytes, None)  # noqa: E731
    assert call(300, 128, _hip.EPI_LOGITS) == -4
    assert call(300, 128, _hip.EPI_STORE) == -3 and "mi_linear_w4a8" in L.mi_last_error_detail().decode()
    assert call(300, 128, _hip.EPI_STORE, FAKE, 300 * 128) == -3                  # one byte class short: x_q without s_x
    assert call(16, 128, _hip.EPI_STORE) == -3
    # K = 16512 (a multiple of 128 above the quantiser's limit) is no new error: what mi_linear_w4 answers, its scratch size named
    w4call = lambda M, K: L.mi_linear_w4(FAKE, 64, FAKE, K, M, K, wp, n1, _hip.EPI_STORE, None, None, 0.0, sp, None, 0, None)  # noqa: E731
    assert call(300, 16512, _hip.EPI_STORE) == w4call(300, 16512) == -3
    assert str(64 * 16512 * 2) in L.mi_last_error_detail().decode()
    assert call(300, 16512, _hip.EPI_STORE, FAKE, 64 * 16512 * 2 - 1) == -3
    assert call(300, 24, _hip.EPI_STORE) == w4call(300, 24) and call(300, 24, _hip.EPI_STORE) < 0   # K % 32 != 0: mi_linear_w4's answer
    qkv = lambda D, wq=FAKE, sq=FAKE, nbytes=1 << 30: L.mi_qkv_rope_w4a8(FAKE, 512, FAKE, D, 300, D, wq, FAKE, FAKE, sq, FAKE, FAKE, 2, 1, 128,  # noqa: E731
                                                                         None, 0.0, FAKE, 16, FAKE, FAKE, nbytes, None)
    assert qkv(16512) == -4 and "mi_qkv_rope_w4a8" in L.mi_last_error_detail().decode()
    assert "mi_qkv_rope_kvwrite_w4" in L.mi_last_error_detail().decode()
    assert qkv(128, wq=FAKE + 8) == -4                 # a code matrix that is not 16-byte aligned
    assert qkv(128, sq=FAKE + 2) == -4                 # a scale matrix the 4-byte DMA of the scale strip cannot read
    assert qkv(128, nbytes=300 * 128) == -3            # scratch: x_q without s_x
    assert L.mi_qkv_rope_w4a8(FAKE, 512, FAKE, 128, 300, 128, FAKE, FAKE, None, FAKE, FAKE, FAKE, 2, 1, 128, None, 0.0, FAKE, 16, FAKE, FAKE,
                              1 << 30, None) == -1
    # workspace: x_q | s_x behind everything else, only with the flag
    layers = (_hip.MiLayer * 2)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 512, 4, 2, 128, 1024, 512, 2
    m.norm_eps = 1e-5
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    scales = (_hip.MiW4Layer * 2)()
    w4 = _hip.MiW4Model()
    w4.format, w4.layers = _hip.MI_W4_MXFP4, C.cast(scales, C.POINTER(_hip.MiW4Layer))
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for T, B, W, lay in ((1, 1, 16, 0), (12, 1, 16, 0), (300, 1, 64, 0), (4096, 1, 4096, 1), (300, 2, 64, _hip.KV_E4M3)):
        base = L.mi_workspace_bytes_kv(C.byref(m), 1, T, B, W, lay)
        assert L.mi_workspace_bytes_w4a8(C.byref(m), C.byref(w4), T, B, W, lay) == base + up(T * 1024) + up(T * 4)
    assert L.mi_workspace_bytes_w4a8(C.byref(m), None, 300, 1, 64, 0) == 0
    bt = _hip.MiBatch()
    assert L.mi_forward_w4a8(C.byref(m), None, C.byref(bt), None) == -1
    assert "mi_forward_w4a8" in L.mi_last_error_detail().decode()
    moe = _hip.MiModel()
    C.memmove(C.byref(moe), C.byref(m), C.sizeof(m))
    moe.num_experts, moe.top_k = 8, 2
    assert L.mi_forward_w4a8(C.byref(moe), C.byref(w4), C.byref(bt), None) == -4
    assert "MoE" in L.mi_last_error_detail().decode() and "mi_forward_w4a8" in L.mi_last_error_detail().decode()
    lora = _hip.MiModel()
    C.memmove(C.byref(lora), C.byref(m), C.sizeof(m))
    lora.lora_rank, lora.lora_scaling = 8, 2.0
    assert L.mi_forward_w4a8(C.byref(lora), C.byref(w4), C.byref(bt), None) == -4
    assert "LoRA" in L.mi_last_error_detail().decode() and "mi_forward_w4a8" in L.mi_last_error_detail().decode()
    fp8 = _hip.MiW4Model()
    fp8.format, fp8.layers = _hip.MI_W8_FP8_E4M3, C.cast(scales, C.POINTER(_hip.MiW4Layer))
    assert L.mi_forward_w4a8(C.byref(m), C.byref(fp8), C.byref(bt), None) == -4   # the struct names another format
