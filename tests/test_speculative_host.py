"""Speculative greedy decoding, host side (no GPU): the prompt-lookup drafter on hand-written histories, every refusal by name,
what mi_forward_verify decides before any launch (never-dereferenced pointers, as test_fp8_host.py), and the workspace query."""
import ctypes as C
import types

import pytest
import torch

from mistral_inference import _hip
from mistral_inference.generate import SpeculativeArgs, generate, ngram_draft, refuse_speculative
from mistral_inference.transformer import Transformer
from test_abi import _tiny_model, _valid_decode_batch


# ------------------------------------------------------------------------------------------------ the drafter
def test_longest_match_wins():
    #         0  1  2  3  4  5  6  7  8  9 10 11
    h = [1, 2, 3, 7, 7, 9, 2, 3, 8, 1, 2, 3]
    # suffix (1, 2, 3) occurs at 0 -> 7, 7, 9; the shorter suffix (2, 3) also occurs at 6 -> 8, which is more recent but shorter
    assert ngram_draft(h, 3, ngram_max=3, ngram_min=1) == [7, 7, 9]
    assert ngram_draft(h, 3, ngram_max=2, ngram_min=1) == [8, 1, 2]


def test_most_recent_occurrence():
    h = [5, 6, 1, 5, 6, 2, 5, 6]
    assert ngram_draft(h, 2, ngram_max=2) == [2, 5]           # (5, 6) at 3, not at 0
    assert ngram_draft([4, 4, 4, 4], 3, ngram_max=2) == [4]   # overlapping: the occurrence one step back, one token follows it


def test_no_match_gives_nothing():
    assert ngram_draft([1, 2, 3, 4], 3) == []
    assert ngram_draft([], 3) == [] and ngram_draft([7], 3) == []
    assert ngram_draft([1, 2, 1, 3], 3, ngram_max=3, ngram_min=2) == []   # only a 1-gram matches, below ngram_min


def test_never_more_than_k_drafts():
    h = [1, 2, 3, 4, 5, 6, 7, 8, 1]
    assert ngram_draft(h, 3) == [2, 3, 4] and ngram_draft(h, 7) == [2, 3, 4, 5, 6, 7, 8] and ngram_draft(h, 1) == [2]
    a = SpeculativeArgs(k=2, drafter=lambda hist: [9, 9, 9, 9, 9])
    assert a.draft(h) == [9, 9]
    assert SpeculativeArgs(k=3).draft(h) == [2, 3, 4]
    assert SpeculativeArgs(k=3, ngram_max=1).draft([1, 2, 3]) == []


def test_speculative_args_are_checked():
    for k in (0, 8, -1):
        with pytest.raises(ValueError, match="1 .. 7 drafts"):
            SpeculativeArgs(k=k)
    with pytest.raises(ValueError, match="ngram_min"):
        SpeculativeArgs(ngram_min=0)
    with pytest.raises(ValueError, match="ngram_min"):
        SpeculativeArgs(ngram_min=4, ngram_max=3)
    a = SpeculativeArgs()
    assert (a.k, a.ngram_max, a.ngram_min, a.drafter) == (3, 3, 1, None)


# ------------------------------------------------------------------------------------------------ refusals, by name
def _stub(**kw):
    base = dict(num_pipeline_ranks=1, dtype=torch.bfloat16, _backend=types.SimpleNamespace(generic=False),
                args=types.SimpleNamespace(lora=None))
    base.update(kw)
    m = types.SimpleNamespace(**base)
    m.refuse_verify = lambda cache, model_only=False: Transformer.refuse_verify(m, cache, model_only)
    m.verify_step = None
    return m


def test_generate_refusals():
    ok = _stub()
    refuse_speculative(ok, 1, 0.0, None)
    refuse_speculative(ok, 1, 0.0, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="temperature 0.7 > 0"):
        refuse_speculative(ok, 1, 0.7, None)
    with pytest.raises(NotImplementedError, match="2 prompts"):
        refuse_speculative(ok, 2, 0.0, None)
    with pytest.raises(NotImplementedError, match="FP8 K/V cache"):
        refuse_speculative(ok, 1, 0.0, torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="un-merged LoRA"):
        refuse_speculative(_stub(args=types.SimpleNamespace(lora=object())), 1, 0.0, None)
    with pytest.raises(NotImplementedError, match="pipeline ranks"):
        refuse_speculative(_stub(num_pipeline_ranks=2), 1, 0.0, None)
    for dt in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="fp16 / fp32 storage"):
            refuse_speculative(_stub(dtype=dt), 1, 0.0, None)
    with pytest.raises(NotImplementedError, match="no verify_step"):
        refuse_speculative(types.SimpleNamespace(), 1, 0.0, None)


def test_generate_refuses_before_anything_runs():
    """The refusal comes first: the model below has nothing generate() could run."""
    with pytest.raises(NotImplementedError, match="temperature"):
        generate([[1, 2]], _stub(), max_tokens=4, temperature=0.5, speculative=SpeculativeArgs())
    with pytest.raises(NotImplementedError, match="one prompt per call"):
        generate([[1, 2], [3]], _stub(), max_tokens=4, temperature=0.0, speculative=SpeculativeArgs())


def test_verify_step_refuses_a_missing_or_e4m3_cache():
    m = _stub()
    with pytest.raises(ValueError, match="needs a cache"):
        Transformer.refuse_verify(m, None)
    from mistral_inference.cache import BufferCache
    c8 = BufferCache(1, 1, 16, 2, 128, dtype=torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="FP8 K/V cache"):
        Transformer.refuse_verify(m, c8)
    Transformer.refuse_verify(m, BufferCache(1, 1, 16, 2, 128, dtype=torch.bfloat16))


def test_cache_verify_metadata_is_the_prefill_shape_at_any_row_count():
    from mistral_inference.cache import BufferCache
    c = BufferCache(1, 2, 64, 2, 128, sliding_window=16, dtype=torch.bfloat16)
    c.init_kvseqlens(2)
    c._seen = [20, 3]
    for lens in ([1, 1], [3, 5]):
        md = c.verify_metadata(lens)
        assert md.branch == _hip.BRANCH_PREFILL and md.max_q_len == max(lens)
        assert md.q_start.tolist() == [0, lens[0], sum(lens)] and md.kv_before.tolist() == [20, 3]
        assert md.tok_seq.tolist() == [0] * lens[0] + [1] * lens[1]
        assert md.tok_pos.tolist() == [20 + i for i in range(lens[0])] + [3 + i for i in range(lens[1])]
    assert c.batch_metadata([1, 1]).branch == _hip.BRANCH_DECODE      # the plain route is unchanged
    assert c._seen == [20, 3]


# ------------------------------------------------------------------------------------------------ the library, before any launch
def _verify_batch(T=3, B=1, max_q_len=None, **kw):
    bt = _valid_decode_batch(B=B)
    bt.T, bt.branch, bt.max_q_len = T, _hip.BRANCH_PREFILL, (T - B + 1 if max_q_len is None else max_q_len)
    bt.input_ids = 1
    for k, v in kw.items():
        setattr(bt, k, v)
    return bt


def _out(tokens=1, logprobs=1, n_accept=1):
    vo = _hip.MiVerifyOut()
    vo.tokens, vo.logprobs, vo.n_accept = tokens, logprobs, n_accept
    return vo


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _hip.lib()
    assert L.mi_abi_version() == 9
    for name in ("mi_attn_verify", "mi_attn_verify_scratch_bytes", "mi_forward_verify", "mi_workspace_bytes_verify"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(L, name)


def test_mi_forward_verify_argument_checks():
    L = _hip.lib()
    m = _tiny_model()
    m.tok_embeddings = 1

    def call(bt, vo=None, model=m, w8=None, w4=None):
        vo = _out() if vo is None else vo
        return L.mi_forward_verify(C.byref(model), w8, w4, C.byref(bt), C.byref(vo), None), L.mi_last_error_detail().decode()

    assert L.mi_forward_verify(C.byref(m), None, None, C.byref(_verify_batch()), None, None) == -1
    rc, why = call(_verify_batch(), _out(n_accept=None))
    assert rc == -1 and "mi_forward_verify: outputs" in why
    lora = _tiny_model()
    lora.tok_embeddings, lora.lora_rank, lora.lora_scaling = 1, 8, 2.0
    rc, why = call(_verify_batch(), model=lora)
    assert rc == -4 and "un-merged LoRA" in why and "mi_forward_verify" in why
    rc, why = call(_verify_batch(kv_layout=0x11))
    assert rc == -4 and "MI_KV_E4M3" in why
    rc, why = call(_verify_batch(T=9))
    assert rc == -4 and "T = 9" in why and "at most 8" in why
    rc, why = call(_verify_batch(T=2, B=3))
    assert rc == -1 and "m_b >= 1" in why
    rc, why = call(_verify_batch(T=4, B=2, max_q_len=4))            # 4 rows of one sequence leave none for the other
    assert rc == -1 and "m_b >= 1" in why
    rc, why = call(_verify_batch(T=4, B=2, max_q_len=0))
    assert rc == -1 and "m_b >= 1" in why
    rc, why = call(_verify_batch(branch=_hip.BRANCH_NOCACHE))
    assert rc == -1 and "needs a cache" in why
    rc, why = call(_verify_batch(branch=_hip.BRANCH_DECODE, T=1))
    assert rc == -1 and "needs a cache" in why
    rc, why = call(_verify_batch(kv_seqlens=None))
    assert rc == -1 and "needs a cache" in why
    rc, why = call(_verify_batch(logits=None))
    assert rc == -1 and "logits" in why
    rc, why = call(_verify_batch(input_ids=None))
    assert rc == -1 and "input_ids" in why
    big = _verify_batch()
    big._keep[2][0] = 4097
    rc, why = call(big)
    assert rc == -4 and "4097 slots" in why
    rc, why = call(_verify_batch(workspace_bytes=64))
    assert rc == -3 and "workspace 64 < required" in why
    need = L.mi_workspace_bytes_verify(C.byref(m), 0, 3, 16, 0)
    assert f"required {need}" in why
    # at most one weight format; a quantised MoE model is refused as mi_forward_w8 refuses it
    w8, w4 = _hip.MiW8Model(), _hip.MiW4Model()
    rc, why = call(_verify_batch(), w8=C.byref(w8), w4=C.byref(w4))
    assert rc == -1 and "both w8 and w4" in why
    w8.format = _hip.MI_W8_FP8_E4M3
    moe = _tiny_model(E=8, k=2)
    moe.tok_embeddings = 1
    scales = (_hip.MiW8Layer * 1)()
    w8.layers = C.cast(scales, C.POINTER(_hip.MiW8Layer))
    rc, why = call(_verify_batch(), model=moe, w8=C.byref(w8))
    assert rc == -4 and "MoE" in why and "mi_forward_verify" in why
    odd = _tiny_model()
    odd.head_dim = 64
    rc, why = call(_verify_batch(), model=odd)
    assert rc == _hip.MI_ERR_SHAPE                                  # a shape the tuned kernels decline


@pytest.mark.parametrize("model_kw", [dict(dim=512, hidden_dim=1024, vocab=512), dict(dim=512, hidden_dim=1024, vocab=512, E=4, k=2)])
def test_workspace_query_is_the_kv_query_plus_exactly_the_stash(model_kw):
    L = _hip.lib()
    m = _tiny_model(**model_kw)
    for n_layers in (1, 2, 32):
        m.n_layers = n_layers
        for T in range(1, 9):
            for W in (1, 16, 300, 4096):
                stash = n_layers * T * 2 * m.n_kv_heads * m.head_dim * 2
                for qz in (0, 1):
                    for lay in (0, 1):
                        # (the attention's split partials are per row: T stands where the kv query takes the batch size)
                        want = L.mi_workspace_bytes_kv(C.byref(m), qz, T, T, W, lay) + stash
                        assert L.mi_workspace_bytes_verify(C.byref(m), qz, T, W, lay) == want, (n_layers, T, W, qz, lay)
    m.n_layers = 1
    assert L.mi_workspace_bytes_verify(C.byref(m), 0, 9, 16, 0) == 0 and L.mi_workspace_bytes_verify(C.byref(m), 0, 0, 16, 0) == 0
    assert L.mi_workspace_bytes_verify(C.byref(m), 0, 4, 16, 0x10) == 0 and L.mi_workspace_bytes_verify(None, 0, 4, 16, 0) == 0
    assert L.mi_workspace_bytes_verify(C.byref(m), 0, 4, 16, 2) == 0


def test_cli_flag_is_plumbed_like_kv_dtype():
    import inspect
    from mistral_inference import main
    assert main.speculative_arg(None) is None and main.speculative_arg(0) is None
    assert main.speculative_arg(3).k == 3 and main.speculative_arg("5").k == 5
    with pytest.raises(ValueError, match="1 .. 7 drafts"):
        main.speculative_arg(9)
    for fn in (main.interactive, main.demo):
        assert inspect.signature(fn).parameters["speculative"].default is None
