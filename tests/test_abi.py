"""The C-ABI library builds, loads without a GPU and exports every symbol include/*.h declares (mistral_hip.h: the product
boundary; mistral_hip_debug.h: engine diagnostics)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header=None):
    names = set()
    for h in ([header] if header else sorted(os.listdir(os.path.join(ROOT, "include")))):
        if not h.endswith(".h"):
            continue
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_debug_entry_points_live_in_their_own_header():
    """Diagnostics (trace, knobs, sabotage) are not part of the boundary a maintainer binds."""
    assert not [n for n in _declared("mistral_hip.h") if n.startswith("mi_debug_")]
    assert all(n.startswith("mi_debug_") for n in _declared("mistral_hip_debug.h"))


def test_header_symbols_exported():
    from mistral_inference import _hip
    handle = ctypes.CDLL(_hip.LIB_PATH)
    names = _declared()
    assert len(names) >= 14
    for n in names:
        assert hasattr(handle, n), f"{n} declared in mistral_hip.h but not exported"
    assert set(names) == set(_hip.EXPORTED_SYMBOLS), set(names) ^ set(_hip.EXPORTED_SYMBOLS)


def test_abi_version_and_error_strings():
    from mistral_inference import _hip
    L = _hip.lib()
    assert L.mi_abi_version() == _hip.MI_ABI_VERSION
    assert L.mi_error_string(0) == b"ok"
    assert b"shape" in L.mi_error_string(-2)
    # argument checks run before any device work, so they are testable on a box without a GPU
    assert L.mi_rmsnorm(None, None, None, 1, 8, 1e-5, None) == -1
    assert b"mi_rmsnorm" in L.mi_last_error_detail()
    assert L.mi_workspace_bytes(None, 1, 1, 1) == 0


def test_no_oracle_import_in_product():
    """The shipped package must never reach into oracle/ (it has no CPU path to fall back to)."""
    pkg = os.path.join(ROOT, "mistral-inference_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cuh")):
                text = open(os.path.join(dirpath, f)).read()
                assert "mistral_oracle" not in text and "import oracle" not in text, os.path.join(dirpath, f)


def test_unsupported_shapes_fail_loudly_before_any_device_work():
    """mi_forward validates the model description first: wrong head_dim / head counts / MoE width come back as MI_ERR_SHAPE
    with a message, never as a silent wrong answer (checked without a GPU: validation precedes every launch)."""
    import ctypes as C
    from mistral_inference import _hip
    L = _hip.lib()
    layers = (_hip.MiLayer * 1)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = 256, 4, 2, 64, 512, 100, 1
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    bt = _hip.MiBatch()
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -2 and b"head_dim" in L.mi_last_error_detail()
    m.head_dim, m.n_heads, m.n_kv_heads = 128, 7, 2   # 7 query heads over 2 kv heads: not a GQA layout
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -2 and b"n_heads" in L.mi_last_error_detail()
    m.n_heads = 6                                     # ratio 3 is fine (query heads are grouped 3 x 1)
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1
    m.n_heads, m.num_experts, m.top_k = 4, 32, 2
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -2 and b"MoE" in L.mi_last_error_detail()
    m.num_experts = m.top_k = 0
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1     # valid model, empty batch -> MI_ERR_ARG
    assert L.mi_attn_decode(1, 1, 128, 1, 1, 16, 1, 4, 2, 64, 1, 1, 0, None) == -2   # head_dim 64
    assert L.mi_attn_decode(1, 1, 128, 1, 1, 16, 1, 4, 2, 128, 1, 1, 2, None) == -1  # ABI v7: an unknown K/V ring layout code
    bt.kv_layout = 7
    assert L.mi_forward(C.byref(m), C.byref(bt), None) == -1
    bt.kv_layout = 0


def test_generic_entry_takes_what_mi_forward_declines():
    """mi_forward_generic (ABI v6): the shapes above that are MI_ERR_SHAPE for the tuned kernels pass ITS validation (and
    stop at the empty batch, MI_ERR_ARG); an unknown dtype code, an odd head_dim and top_k > num_experts are refused before any
    device work.  The host-side predicate that routes a model (`tuned_kernels_take`) agrees with the library on every case."""
    import ctypes as C
    from mistral_inference import _hip
    from mistral_inference.args import MoeArgs, TransformerArgs
    from mistral_inference.transformer import tuned_kernels_take
    L = _hip.lib()
    layers = (_hip.MiLayer * 1)()
    bt = _hip.MiBatch()

    def both(dim=256, n_heads=4, n_kv_heads=2, head_dim=128, hidden_dim=512, E=0, k=0):
        m = _hip.MiModel()
        m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = dim, n_heads, n_kv_heads, head_dim, hidden_dim, 100, 1
        m.num_experts, m.top_k = E, k
        m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
        a = TransformerArgs(dim=dim, n_layers=1, head_dim=head_dim, hidden_dim=hidden_dim, n_heads=n_heads, n_kv_heads=n_kv_heads,
                            norm_eps=1e-5, vocab_size=100, moe=MoeArgs(num_experts=E, num_experts_per_tok=k) if E else None)
        tuned = L.mi_forward(C.byref(m), C.byref(bt), None)
        assert (tuned != _hip.MI_ERR_SHAPE) == tuned_kernels_take(a), (dim, n_heads, n_kv_heads, head_dim, hidden_dim, E, k)
        return tuned, [L.mi_forward_generic(C.byref(m), C.byref(bt), d, None) for d in (0, 1, 2)], m

    assert both()[:2] == (-1, [-1, -1, -1])
    assert both(head_dim=64)[:2] == (-2, [-1, -1, -1])
    assert both(head_dim=256, n_heads=2, n_kv_heads=1)[:2] == (-2, [-1, -1, -1])
    assert both(E=32, k=2)[:2] == (-2, [-1, -1, -1])
    assert both(E=8, k=3)[:2] == (-2, [-1, -1, -1])
    assert both(E=8, k=2)[:2] == (-1, [-1, -1, -1])
    assert both(head_dim=100)[:2] == (-2, [-2, -2, -2])            # not a multiple of 8
    assert both(E=2, k=3)[1] == [-2, -2, -2] and b"top_k" in L.mi_last_error_detail()
    m = both()[2]
    assert L.mi_forward_generic(C.byref(m), C.byref(bt), 7, None) == -1 and b"dtype" in L.mi_last_error_detail()
    assert L.mi_workspace_bytes_generic(C.byref(m), 16, 2) > L.mi_workspace_bytes_generic(C.byref(m), 16, 0) > 4096
    assert L.mi_workspace_bytes_generic(None, 16, 0) == 0


def test_header_is_c99_and_a_c_program_can_drive_the_library(tmp_path):
    """include/mistral_hip.h must be consumable from plain C (the boundary a cgo / JNI / ctypes shim binds): compile it
    with gcc -std=c99 -pedantic, then build examples/abi_probe.c and run it against the in-tree library (argument
    validation only - no device work)."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hdr.c"
    src.write_text('#include "mistral_hip.h"\nint main(void) { return MI_ABI_VERSION == 0; }\n')
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), "-c",
                    str(src), "-o", str(tmp_path / "hdr.o")], check=True)
    exe = tmp_path / "abi_probe"
    subprocess.run([gcc, "-std=c99", "-Wall", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "abi_probe.c"), "-ldl", "-o", str(exe)], check=True)
    from mistral_inference import _hip
    r = subprocess.run([str(exe), _hip.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "head_dim 96" in r.stdout and "workspace" in r.stdout


def _tiny_model(E=0, k=0, lm_head=True, n_kv_heads=2, dim=256, hidden_dim=512, vocab=100):
    """A model description whose pointers are never dereferenced (validation precedes every launch)."""
    import ctypes as C
    from mistral_inference import _hip
    layers = (_hip.MiLayer * 1)()
    m = _hip.MiModel()
    m.dim, m.n_heads, m.n_kv_heads, m.head_dim, m.hidden_dim, m.vocab_size, m.n_layers = dim, 2 * n_kv_heads, n_kv_heads, 128, hidden_dim, vocab, 1
    m.num_experts, m.top_k = E, k
    m.layers = C.cast(layers, C.POINTER(_hip.MiLayer))
    if lm_head:
        m.final_norm = m.output = 1
    m._keep = layers
    return m


def _valid_decode_batch(B=1, workspace_bytes=1 << 30):
    import ctypes as C
    from mistral_inference import _hip
    bt = _hip.MiBatch()
    bt.T = bt.B = B
    bt.branch, bt.max_q_len = 2, 1
    bt.q_start = bt.kv_before = bt.tok_seq = bt.tok_pos = bt.kv_seqlens = bt.h = bt.workspace = bt.logits = 1
    bt._keep = ((_hip._vp * 1)(), (_hip._vp * 1)(), (C.c_int32 * 1)(16))
    bt.cache_k, bt.cache_v = bt._keep[0], bt._keep[1]
    bt.cache_sizes = bt._keep[2]
    bt.workspace_bytes = workspace_bytes
    return bt


# (what to break in a valid one-sequence decode batch, return code, substring of mi_last_error_detail) - one row per check of
# the validation the two forward entry points share, in the order the checks fire.  {e}: the entry's name.  Recorded from
# the library as it was before the two copies of the validation were merged; "tuned": mi_forward only.
_BATCH_ERRORS = [
    ("null batch", "both", -1, "{e}: batch"),
    ("T = 0", "both", -1, "{e}: batch"),
    ("no workspace pointer", "both", -1, "{e}: batch"),
    ("missing metadata", "both", -1, "{e}: metadata"),
    ("cache pointers missing", "both", -1, "{e}: cache"),
    ("bad kv_layout", "both", -1, "{e}: kv_layout"),
    ("decode with T != B", "both", -1, "{e}: decode needs T == B"),
    ("decode without kv_seqlens", "both", -1, "{e}: decode needs T == B"),
    ("B * n_kv_heads > 1024", "tuned", -2, "B * n_kv_heads > 1024"),
    ("logits without LM head", "both", -1, "{e}: logits on a rank without LM head"),
    ("workspace too small", "both", -3, "workspace 64 < required "),
    ("greedy_token on PREFILL", "both", -1, "{e}: greedy_token needs the DECODE branch, logits and greedy_logprob"),
    ("greedy_token without greedy_logprob", "both", -1, "{e}: greedy_token needs the DECODE branch, logits and greedy_logprob"),
    ("hist_len without buffers", "both", -1, "{e}: hist_len > 0 without history buffers"),
    ("negative temperature", "both", -1, "{e}: sample_temperature"),
    ("top_p = 1.5", "both", -1, "{e}: sample_temperature"),
    ("top_p = -0.5", "both", -1, "{e}: sample_temperature"),
]


def _break(case, m_kw, bt):
    """Applies `case` to a valid batch; returns (model kwargs, batch or None)."""
    if case == "null batch":
        return m_kw, None
    if case == "T = 0":
        bt.T = 0
    elif case == "no workspace pointer":
        bt.workspace = None
    elif case == "missing metadata":
        bt.tok_seq = None
    elif case == "cache pointers missing":
        bt.cache_sizes = None
    elif case == "bad kv_layout":
        bt.kv_layout = 2
    elif case == "decode with T != B":
        bt.T = 2
    elif case == "decode without kv_seqlens":
        bt.kv_seqlens = None
    elif case == "B * n_kv_heads > 1024":
        bt.T = bt.B = 513
    elif case == "logits without LM head":
        m_kw = dict(m_kw, lm_head=False)
    elif case == "workspace too small":
        bt.workspace_bytes = 64
    elif case == "greedy_token on PREFILL":
        bt.branch, bt.greedy_token, bt.greedy_logprob = 1, 1, 1
    elif case == "greedy_token without greedy_logprob":
        bt.greedy_token = 1
    elif case == "hist_len without buffers":
        bt.greedy_token = bt.greedy_logprob = 1
        bt.hist_len = 4
    elif case == "negative temperature":
        bt.sample_temperature = -0.5
    elif case in ("top_p = 1.5", "top_p = -0.5"):
        bt.greedy_token = bt.greedy_logprob = 1
        bt.sample_temperature, bt.sample_top_p = 0.7, float(case.split("= ")[1])
    else:
        raise KeyError(case)
    return m_kw, bt


def _batch_error(entry, case, moe=False):
    import ctypes as C
    from mistral_inference import _hip
    L = _hip.lib()
    m_kw, bt = _break(case, dict(E=8, k=2) if moe else {}, _valid_decode_batch())
    m = _tiny_model(**m_kw)
    btp = C.byref(bt) if bt is not None else None
    rc = L.mi_forward(C.byref(m), btp, None) if entry == "mi_forward" else L.mi_forward_generic(C.byref(m), btp, 1, None)
    return rc, L.mi_last_error_detail().decode()


@pytest.mark.parametrize("entry", ["mi_forward", "mi_forward_generic"])
def test_forward_entries_refuse_bad_batches_with_the_recorded_codes_and_messages(entry):
    """Every check of the batch validation, on both entry points, for a dense and a MoE model: return code and message (with the
    entry's own name in it) as recorded in _BATCH_ERRORS.  No GPU: validation precedes every launch."""
    for case, which, code, text in _BATCH_ERRORS:
        if which == "tuned" and entry != "mi_forward":
            continue
        for moe in (False, True):
            rc, detail = _batch_error(entry, case, moe)
            assert rc == code and text.format(e=entry) in detail, (entry, case, moe, rc, detail)
    # the checks fire in the table's order: a batch broken in two ways reports the earlier one
    import ctypes as C
    from mistral_inference import _hip
    L = _hip.lib()
    bt = _valid_decode_batch()
    bt.kv_layout, bt.workspace_bytes, bt.sample_temperature = 2, 64, -1.0
    m = _tiny_model()
    call = (lambda: L.mi_forward(C.byref(m), C.byref(bt), None)) if entry == "mi_forward" else \
        (lambda: L.mi_forward_generic(C.byref(m), C.byref(bt), 1, None))
    assert call() == -1 and b"kv_layout" in L.mi_last_error_detail()
    bt.kv_layout = 1
    assert call() == -3 and b"workspace 64" in L.mi_last_error_detail()
    bt.workspace_bytes = 1 << 30
    assert call() == -1 and b"sample_temperature" in L.mi_last_error_detail()


# Sizes the library reports, recorded before the launch sequences that use them were shared between entry points.
# model key -> kwargs of _tiny_model; mi_workspace_bytes rows are (T, B, max_cache_size), generic rows (T, dtype code).
_SIZE_MODELS = {"dense": dict(dim=512, hidden_dim=1024, vocab=512), "moe": dict(dim=512, hidden_dim=1024, vocab=512, E=8, k=2)}
_WORKSPACE_BYTES = {
    ('dense', 1, 1, 64): 198400,
    ('dense', 8, 2, 1): 243456,
    ('dense', 8, 8, 64): 255744,
    ('dense', 9, 9, 4096): 844288,
    ('dense', 300, 3, 4096): 2236928,
    ('moe', 1, 1, 64): 202496,
    ('moe', 8, 2, 1): 276224,
    ('moe', 8, 8, 64): 288512,
    ('moe', 9, 9, 4096): 881152,
    ('moe', 300, 3, 4096): 3470848,
}
_WORKSPACE_BYTES_GENERIC = {
    ('dense', 1, 0): 45568,
    ('dense', 1, 1): 45568,
    ('dense', 1, 2): 53760,
    ('dense', 8, 0): 335872,
    ('dense', 8, 1): 335872,
    ('dense', 8, 2): 401408,
    ('dense', 9, 0): 377344,
    ('dense', 9, 1): 377344,
    ('dense', 9, 2): 451072,
    ('dense', 300, 0): 2461696,
    ('dense', 300, 1): 2461696,
    ('dense', 300, 2): 4919296,
    ('moe', 1, 0): 48896,
    ('moe', 1, 1): 48896,
    ('moe', 1, 2): 59136,
    ('moe', 8, 0): 353536,
    ('moe', 8, 1): 353536,
    ('moe', 8, 2): 435456,
    ('moe', 9, 0): 397056,
    ('moe', 9, 1): 397056,
    ('moe', 9, 2): 489472,
    ('moe', 300, 0): 3088640,
    ('moe', 300, 1): 3088640,
    ('moe', 300, 2): 6165504,
}
_MOE_SCRATCH_BYTES = {   # (T, D, F, E, top_k)
    (1, 256, 512, 4, 1): 2560,
    (1, 512, 1024, 8, 2): 7168,
    (1, 4096, 14336, 8, 2): 74752,
    (8, 256, 512, 4, 1): 13312,
    (8, 512, 1024, 8, 2): 50176,
    (8, 4096, 14336, 8, 2): 590848,
    (9, 256, 512, 4, 1): 14848,
    (9, 512, 1024, 8, 2): 56320,
    (9, 4096, 14336, 8, 2): 664576,
    (300, 256, 512, 4, 1): 463872,
    (300, 512, 1024, 8, 2): 1848832,
    (300, 4096, 14336, 8, 2): 22124032,
}
_LOGPROB_SCRATCH_BYTES = {  # (M, vocab)
    (1, 512): 2048,
    (1, 1000): 4000,
    (1, 32768): 131072,
    (8, 512): 16384,
    (8, 1000): 32000,
    (8, 32768): 1048576,
    (9, 512): 18432,
    (9, 1000): 36000,
    (9, 32768): 1179648,
    (300, 512): 262144,
    (300, 1000): 512000,
    (300, 32768): 16777216,
}
_ATTN_DECODE_SCRATCH_BYTES = {  # (B, n_heads, n_kv_heads, head_dim, W)
    (1, 4, 2, 128, 64): 6400,
    (1, 32, 8, 128, 64): 20736,
    (1, 48, 8, 128, 64): 29184,
    (8, 4, 2, 128, 4096): 536576,
    (8, 32, 8, 128, 4096): 4263936,
    (8, 48, 8, 128, 4096): 6393856,
    (9, 4, 2, 128, 4096): 603136,
    (9, 32, 8, 128, 4096): 4796416,
    (9, 48, 8, 128, 4096): 7192576,
    (300, 4, 2, 128, 32768): 19972096,
    (300, 32, 8, 128, 32768): 159748096,
    (300, 48, 8, 128, 32768): 239620096,
}


def _size_cases():
    ws = [(name, T, B, W) for name in _SIZE_MODELS for (T, B, W) in ((1, 1, 64), (8, 8, 64), (9, 9, 4096), (300, 3, 4096), (8, 2, 1))]
    gen = [(name, T, dt) for name in _SIZE_MODELS for T in (1, 8, 9, 300) for dt in (0, 1, 2)]
    moe = [(T, D, F, E, k) for (D, F, E, k) in ((512, 1024, 8, 2), (4096, 14336, 8, 2), (256, 512, 4, 1)) for T in (1, 8, 9, 300)]
    lp = [(M, V) for V in (512, 32768, 1000) for M in (1, 8, 9, 300)]
    attn = [(B, H, Hkv, 128, W) for (H, Hkv) in ((4, 2), (32, 8), (48, 8)) for (B, W) in ((1, 64), (8, 4096), (9, 4096), (300, 32768))]
    return ws, gen, moe, lp, attn


def _sizes_now():
    import ctypes as C
    from mistral_inference import _hip
    L = _hip.lib()
    ws, gen, moe, lp, attn = _size_cases()
    models = {k: _tiny_model(**kw) for k, kw in _SIZE_MODELS.items()}
    return ({c: L.mi_workspace_bytes(C.byref(models[c[0]]), *c[1:]) for c in ws},
            {c: L.mi_workspace_bytes_generic(C.byref(models[c[0]]), *c[1:]) for c in gen},
            {c: L.mi_moe_grouped_gemm_scratch_bytes(*c) for c in moe},
            {c: L.mi_lm_head_logprobs_scratch_bytes(*c) for c in lp},
            {c: L.mi_attn_decode_scratch_bytes(*c) for c in attn})


def test_workspace_and_scratch_sizes_are_the_recorded_ones():
    """mi_workspace_bytes, mi_workspace_bytes_generic and the three scratch-size queries over dense and MoE models, T in
    {1, 8, 9, 300} (both sides of the GEMV / GEMM threshold) and every dtype code: the layouts a caller allocated for stay valid."""
    got = _sizes_now()
    want = (_WORKSPACE_BYTES, _WORKSPACE_BYTES_GENERIC, _MOE_SCRATCH_BYTES, _LOGPROB_SCRATCH_BYTES, _ATTN_DECODE_SCRATCH_BYTES)
    for g, w in zip(got, want):
        assert len(w) == len(g) >= 10
        assert g == w, {c: (g[c], w.get(c)) for c in g if g[c] != w.get(c)}
