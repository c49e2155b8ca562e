"""FP8 (e4m3) K/V rings on the device (include/mistral_hip.h MI_KV_E4M3; the rule: mistral_inference.cache.kv_quantize /
kv_dequantize).  Dequantisation is exact, so every attention result on an e4m3 ring must equal, bit for bit, the bf16 kernel's
result on a bf16 ring holding the dequantised values: the kernel-level and the prefill-level tests rest on that.  The decode steps
of a whole model are held to the oracle restated on an e4m3 ring (kv8_util.attention_block_kv8)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

import mistral_oracle as mo
import quant_util as qu
from attn_cases import PREFILL_CASES
from hip_util import write_checkpoint
from kv8_util import BF, F8, all_finite_bf16, attention_block_kv8, e4m3_ring, host_values
from test_gpu_engine import SHAPES, _model
from test_gpu_kv_layout import dev_ring, rnd

pytestmark = pytest.mark.gpu


def _hip():
    from mistral_inference import _hip
    return _hip


def _rule():
    from mistral_inference import cache
    return cache


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _bytes_ring(B, W, Hkv, Dh, hm, fill=0x55):
    """Device ring of e4m3 bytes, every byte `fill` (0x55 = 0.3125: neither zero nor a NaN code)."""
    return dev_ring(torch.full((B, W, Hkv, Dh), fill, dtype=torch.uint8), hm).view(F8)


def _host_bytes(ring8):
    return ring8.view(torch.uint8).cpu().contiguous()


# ------------------------------------------------------------------------------------------------ 1. ring write
@pytest.mark.parametrize("hm", [False, True])
def test_ring_write_over_every_finite_bf16_pattern(hm):
    h, c = _hip(), _rule()
    Hkv, Dh, T, W = 2, 128, 255, 256
    pat = all_finite_bf16()
    k, v = pat.reshape(T, Hkv * Dh), pat.flip(0).reshape(T, Hkv * Dh)
    rk, rv = _bytes_ring(1, W, Hkv, Dh, hm), _bytes_ring(1, W, Hkv, Dh, hm)
    assert h._kv_layout2(rk, rv) == (int(hm) | h.KV_E4M3)
    h.kv_write(rk, rv, k.cuda(), v.cuda(), _i32([0] * T), _i32(list(range(T))), _i32([0, T]))
    gk, gv = _host_bytes(rk), _host_bytes(rv)
    for got, src in ((gk, k), (gv, v)):
        want = c.kv_quantize(src).view(torch.uint8).reshape(T, Hkv, Dh)
        bad = (got[0, :T] != want).nonzero()
        assert bad.numel() == 0, [(src.reshape(T, Hkv, Dh)[tuple(i)].view(torch.int16).item() & 0xFFFF, int(got[0, :T][tuple(i)]),
                                   int(want[tuple(i)])) for i in bad[:8]]
        assert bool((got[0, T:] == 0x55).all())                      # the slot no token went to
    # +-inf saturate to +-448 (0x7E / 0xFE), a NaN stays a NaN code
    row = torch.full((1, Hkv * Dh), float("inf"), dtype=BF)
    nan = torch.full((1, Hkv * Dh), float("nan"), dtype=BF)
    h.kv_write(rk, rv, torch.cat([row, nan]).cuda(), torch.cat([-row, nan]).cuda(), _i32([0, 0]), _i32([256, 257]), _i32([0, 2]))
    gk, gv = _host_bytes(rk), _host_bytes(rv)
    assert bool((gk[0, 0] == 0x7E).all()) and bool((gv[0, 0] == 0xFE).all())
    assert bool(((gk[0, 1] & 0x7F) == 0x7F).all()) and bool(((gv[0, 1] & 0x7F) == 0x7F).all())
    assert torch.equal(gk[0, 2:T], c.kv_quantize(k).view(torch.uint8).reshape(T, Hkv, Dh)[2:])   # and nothing else moved


@pytest.mark.parametrize("hm", [False, True])
def test_ring_write_window_drop(hm):
    """cache.py:83-92: of a chunk longer than the window only the last W tokens are stored, at pos % W; a second, short sequence
    leaves the slots it does not reach alone."""
    h, c = _hip(), _rule()
    Hkv, Dh, W, new, first = 2, 128, 16, [40, 3], [5, 9]
    T = sum(new)
    k, v = rnd(T, Hkv * Dh, seed=31, scale=3.0), rnd(T, Hkv * Dh, seed=32, scale=3.0)
    rk, rv = _bytes_ring(2, W, Hkv, Dh, hm), _bytes_ring(2, W, Hkv, Dh, hm)
    pos = [first[0] + i for i in range(new[0])] + [first[1] + i for i in range(new[1])]
    h.kv_write(rk, rv, k.cuda(), v.cuda(), _i32([0] * new[0] + [1] * new[1]), _i32(pos), _i32([0, new[0], T]))
    for got, src in ((_host_bytes(rk), k), (_host_bytes(rv), v)):
        q = c.kv_quantize(src).view(torch.uint8).reshape(T, Hkv, Dh)
        want = torch.full((2, W, Hkv, Dh), 0x55, dtype=torch.uint8)
        for t in range(new[0] - W, new[0]):
            want[0, pos[t] % W] = q[t]
        for t in range(new[0], T):
            want[1, pos[t] % W] = q[t]
        assert torch.equal(got, want)
        assert int((got[1] == 0x55).all(-1).all(-1).sum()) == W - new[1]


@pytest.mark.parametrize("weights", ["bf16", "fp8", "mxfp4"])
def test_qkv_leaf_writes_e4m3_rings(weights):
    """mi_qkv_rope_kvwrite / _w8 / _w4 on e4m3 rings: the GEMV without its fused write, then the e4m3 ring write - the ring holds
    the rule applied to the k | v columns of the returned rows, and those rows are the ones a bf16 ring gets."""
    from mistral_inference import quant
    h, c = _hip(), _rule()
    B, W, Hkv, Dh, H, D, Td = 3, 8, 2, 128, 4, 512, 3
    x = rnd(Td, D, seed=9, scale=2.0).cuda()
    ws = [rnd(n, D, seed=10 + i, scale=D ** -0.5) for i, n in enumerate((H * Dh, Hkv * Dh, Hkv * Dh))]
    cs = mo.rope_angles(Dh, 100, 1e6).cuda()
    pos, seq = _i32([3, 50, 9]), _i32([2, 0, 1])
    outs = []
    for hm in (False, True):
        rk, rv = _bytes_ring(B, W, Hkv, Dh, hm), _bytes_ring(B, W, Hkv, Dh, hm)
        bk, bv = dev_ring(torch.zeros(B, W, Hkv, Dh, dtype=BF), hm), dev_ring(torch.zeros(B, W, Hkv, Dh, dtype=BF), hm)
        if weights == "bf16":
            w = [t.cuda() for t in ws]
            call = lambda ck, cv: h.qkv_rope_kvwrite(x, *w, Dh, cs, pos, cache_k=ck, cache_v=cv, tok_seq=seq)  # noqa: E731
        else:
            fmt, quantise = (h.W8, quant.quantize_rows) if weights == "fp8" else (h.W4, quant.quantize_blocks)
            qs = [quantise(t) for t in ws]
            w, sc = [q.cuda() for q, _ in qs], [s.cuda() for _, s in qs]
            call = lambda ck, cv: h.qkv_rope_kvwrite_quant(fmt, x, *w, *sc, Dh, cs, pos, cache_k=ck, cache_v=cv, tok_seq=seq)  # noqa: E731
        out8, out16 = call(rk, rv).cpu(), call(bk, bv).cpu()
        assert torch.equal(out8, out16)
        gk, gv = _host_bytes(rk), _host_bytes(rv)
        want_k = torch.full((B, W, Hkv, Dh), 0x55, dtype=torch.uint8)
        want_v = want_k.clone()
        for t, (p, b) in enumerate(zip([3, 50, 9], [2, 0, 1])):
            want_k[b, p % W] = c.kv_quantize(out8[t, H * Dh:(H + Hkv) * Dh]).view(torch.uint8).reshape(Hkv, Dh)
            want_v[b, p % W] = c.kv_quantize(out8[t, (H + Hkv) * Dh:]).view(torch.uint8).reshape(Hkv, Dh)
        assert torch.equal(gk, want_k) and torch.equal(gv, want_v)
        outs.append(out8)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 2. decode attention
DECODE_HEADS = [(8, 2), (32, 8), (4, 4), (12, 2), (8, 1), (4, 2)]   # query heads per block R = 4, 4, 1, 6, 8, 2
DECODE_RINGS = [(16, [5, 16, 40]), (300, [1, 299, 300]), (4096, [4096, 17, 5000]), (5000, [5000, 4999, 1])]


@functools.lru_cache(maxsize=None)
def _decode_base(W):
    """One random ring pair per ring length, shared by every head layout (sliced) - host bf16 [3, W, 8, 128]."""
    return rnd(3, W, 8, 128, seed=100 + W), rnd(3, W, 8, 128, seed=200 + W)


def _decode_case(H, Hkv, W, lens, hm, B):
    h = _hip()
    bk, bv = _decode_base(W)
    bk, bv = bk[:B, :, :Hkv].contiguous(), bv[:B, :, :Hkv].contiguous()
    q = rnd(B, H * 128, seed=3 + H).cuda()
    pos = _i32([n - 1 for n in lens[:B]])
    k8, v8 = e4m3_ring(bk, hm), e4m3_ring(bv, hm)
    k16, v16 = dev_ring(host_values(k8), hm), dev_ring(host_values(v8), hm)
    assert k8.dtype == F8 and k16.dtype == BF and h.kv_layout_of(k8) == h.kv_layout_of(k16) == (int(hm) if Hkv > 1 else 0)
    got, ref = h.attn_decode(q, k8, v8, H, pos).cpu(), h.attn_decode(q, k16, v16, H, pos).cpu()
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    assert torch.equal(got, ref), (int((got != ref).sum()), float((got.float() - ref.float()).abs().max()))


@pytest.mark.parametrize("B", [3, 1], ids=["batch3", "batch1"])
@pytest.mark.parametrize("hm", [False, True], ids=["slot_major", "head_major"])
@pytest.mark.parametrize("W,lens", DECODE_RINGS, ids=[f"W{w}" for w, _ in DECODE_RINGS])
@pytest.mark.parametrize("H,Hkv", DECODE_HEADS)
def test_decode_attention_bit_equal(H, Hkv, W, lens, hm, B):
    """Query-head groups of 1, 4, 6 and 8 per block; batches of three (the all-in form where R is 4 and a split has at most 128
    slots, else the stepping forms) and the first sequence alone (the non-SMALL stepping form); rings of one split, of three, of
    exactly 32 and of 32 widened ones (W = 5000)."""
    _decode_case(H, Hkv, W, lens, hm, B)


def test_decode_attention_bit_equal_without_the_allin_form():
    """MI_ATTN_ALLIN=0 is read once per process: the batch-3 cases again in a fresh child, where they take the SMALL stepping form."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MI_ATTN_ALLIN="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_kv8.py"), "-q", "-x", "-k",
                        "test_decode_attention_bit_equal and batch3"], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(here), timeout=600)
    n = len(DECODE_HEADS) * len(DECODE_RINGS) * 2
    assert r.returncode == 0 and f"{n} passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 3. prefill over an e4m3 ring
@pytest.mark.parametrize("hm", [False, True], ids=["slot_major", "head_major"])
@pytest.mark.parametrize("W,seen,new", PREFILL_CASES, ids=[f"W{w}_{sum(n)}" for w, _, n in PREFILL_CASES])
def test_prefill_attention_and_dequant_bit_equal(W, seen, new, hm):
    h = _hip()
    H, Hkv, Dh, B, T = 8, 2, 128, len(new), sum(new)
    bk, bv = rnd(B, W, Hkv, Dh, seed=4), rnd(B, W, Hkv, Dh, seed=5)
    qkv = rnd(T, (H + 2 * Hkv) * Dh, seed=6).cuda()
    q_start = _i32([0] + list(torch.tensor(new).cumsum(0)))
    kv_before = _i32(seen)
    k8, v8 = e4m3_ring(bk, hm), e4m3_ring(bv, hm)
    # mi_kv_dequant alone: the read rule, in the ring's own layout
    dk, dv = h.kv_dequant(k8, v8)
    assert dk.dtype == BF and h.kv_layout_of(dk) == int(hm) and dk.shape == k8.shape
    assert torch.equal(dk.cpu(), host_values(k8)) and torch.equal(dv.cpu(), host_values(v8))
    got = h.attn_prefill(qkv, H, Hkv, Dh, k8, v8, W, q_start, kv_before, B, max(new)).cpu()
    ref = h.attn_prefill(qkv, H, Hkv, Dh, dev_ring(host_values(k8), hm), dev_ring(host_values(v8), hm), W, q_start, kv_before, B,
                         max(new)).cpu()
    assert torch.equal(got, ref)
    # the entry point itself reads no e4m3 ring
    out = torch.empty((T, H * Dh), dtype=BF, device="cuda")
    rc = h.lib().mi_attn_prefill(out.data_ptr(), qkv.data_ptr(), qkv.stride(0), k8.data_ptr(), v8.data_ptr(), W, B, max(new), H, Hkv, Dh,
                                 q_start.data_ptr(), kv_before.data_ptr(), 1, 0.0, h.kv_layout_code(k8), h.stream_ptr(qkv.device))
    assert rc == -4 and b"mi_kv_dequant" in h.lib().mi_last_error_detail()


# ------------------------------------------------------------------------------------------------ 4. / 5. the stack
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("kv8")
    w = mo.synth_weights(qu.MODEL, seed=21)
    return write_checkpoint(d / "bf16", qu.MODEL, w), w


def _kv_cache(B, dtype):
    from mistral_inference.cache import BufferCache
    return BufferCache(qu.MODEL.n_layers, B, 64, qu.MODEL.n_kv_heads, qu.MODEL.head_dim, qu.MODEL.sliding_window, device="cuda", dtype=dtype)


def _round_rings(cache):
    """Every ring of a bf16 cache through the rule (on the host; allocator garbage in slots never written turns into other
    garbage that nobody reads)."""
    c = _rule()
    for d in (cache.cache_k, cache.cache_v):
        for t in d.values():
            t.copy_(c.kv_dequantize(c.kv_quantize(t.cpu()), BF))


@pytest.mark.parametrize("quantize", [None, "mxfp4"])
def test_stack_prefill_chunks_bit_equal(folder, quantize):
    """12 tokens in chunks of 5, 5, 2 - every forward takes the prefill branch: keys older than the forward come from the ring
    (dequantised into the scratch), the chunk's own rows from the activations, unrounded.  A bf16 cache whose rings the test rounds
    by the rule after each forward holds the same values: the logits are the same bits."""
    model = qu._load(folder[0], B=1, **({"quantize": quantize} if quantize else {}))
    runs = {}
    for name, dtype in (("bf16", BF), ("fp8", F8)):
        cache, out = _kv_cache(1, dtype), []
        with torch.inference_mode():
            for ids, lens in qu._schedule(1, 5):
                out.append(model.forward(torch.tensor(ids, device="cuda"), lens, cache).cpu())
                if dtype == BF:
                    _round_rings(cache)
        runs[name] = (out, cache)
    assert len(runs["bf16"][0]) == 3
    for a, b in zip(runs["bf16"][0], runs["fp8"][0]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), float((a - b).abs().max())
    for l in range(qu.MODEL.n_layers):   # and the rings hold the same values (12 of 16 slots written)
        assert torch.equal(host_values(runs["fp8"][1].cache_k[l])[:, :12], runs["bf16"][1].cache_k[l][:, :12].cpu())
        assert torch.equal(host_values(runs["fp8"][1].cache_v[l])[:, :12], runs["bf16"][1].cache_v[l][:, :12].cpu())


def _oracle_runs(weights, cache_dtype, fed_from=None):
    """quant_util.make_oracle_runs with a cache of `cache_dtype`; fed_from: runs whose greedy tokens are fed (teacher forcing)."""
    om = mo.OracleModel(qu.MODEL, weights)
    runs = {}
    for B, chunk in ((1, None), (1, 5), (3, None)):
        oc = mo.OracleCache(qu.MODEL.n_layers, B, 64, qu.MODEL.n_kv_heads, qu.MODEL.head_dim, qu.MODEL.sliding_window, dtype=cache_dtype)
        logits, fed = [], []
        for ids, lens in qu._schedule(B, chunk):
            logits.append(om.forward(torch.tensor(ids), lens, oc))
        ends = torch.tensor(qu._schedule(B, chunk)[-1][1]).cumsum(0) - 1
        tok = logits[-1][ends].argmax(-1)
        for i in range(qu.N_DECODE if chunk is None else 3):
            tok = tok if fed_from is None else fed_from[(B, chunk)][1][i]
            fed.append(tok)
            logits.append(om.forward(tok, [1] * B, oc))
            tok = logits[-1].argmax(-1)
        runs[(B, chunk)] = (logits, fed)
    return runs


def _replay(model, B, chunk, fed, dtype):
    cache, out = _kv_cache(B, dtype), []
    with torch.inference_mode():
        for ids, lens in qu._schedule(B, chunk):
            out.append(model.forward(torch.tensor(ids, device="cuda"), lens, cache).cpu())
        for tok in fed:
            out.append(model.forward(tok.cuda(), [1] * B, cache).cpu())
    return out


def test_stack_against_the_oracle_on_an_e4m3_ring(folder, monkeypatch):
    """Prompt forwards and 24 teacher-forced decode steps across the wrap of the 16-slot ring (B = 1, B = 1 in chunks of 5, B = 3):
    HIP on an FP8 cache against the oracle restated on an e4m3 ring, within the project's bf16 tolerance on logits at these dims.
    Printed beside it: HIP on a bf16 cache against the bf16 oracle on the same tokens, and the distance between the two oracles
    - how much of the budget the cache itself uses."""
    model = qu._load(folder[0], B=3)
    with monkeypatch.context() as mp:
        mp.setattr(mo, "attention_block", attention_block_kv8)
        ref8 = _oracle_runs(folder[1], F8)
    ref16 = _oracle_runs(folder[1], BF, fed_from=ref8)
    worst = {"fp8": 0.0, "bf16": 0.0, "oracles": 0.0}
    for (B, chunk), (logits8, fed) in ref8.items():
        got8, got16 = _replay(model, B, chunk, fed, F8), _replay(model, B, chunk, fed, BF)
        logits16 = ref16[(B, chunk)][0]
        assert len(got8) == len(logits8) == len(logits16)
        d8 = max(float((g - r).abs().max()) for g, r in zip(got8, logits8))
        d16 = max(float((g - r).abs().max()) for g, r in zip(got16, logits16))
        do = max(float((a - b).abs().max()) for a, b in zip(logits8, logits16))
        print(f"B={B} chunk={chunk}: HIP(fp8 cache) to e4m3 oracle {d8:.4e}; HIP(bf16 cache) to bf16 oracle {d16:.4e}; "
              f"e4m3 oracle to bf16 oracle {do:.4e}; over {len(logits8)} forwards")
        worst = {"fp8": max(worst["fp8"], d8), "bf16": max(worst["bf16"], d16), "oracles": max(worst["oracles"], do)}
    print(f"max |dlogit|: HIP(fp8 cache) to e4m3 oracle {worst['fp8']:.4e}; HIP(bf16 cache) to bf16 oracle {worst['bf16']:.4e}; "
          f"between the oracles {worst['oracles']:.4e}; bound {qu.LOGIT_ATOL}")
    assert worst["oracles"] > 0                       # the restated oracle does round
    assert worst["fp8"] <= qu.LOGIT_ATOL, worst
    st = _hip().decode_engine_status(model._backend._workspace)
    assert st["status"] == 0 and st["bad_id"] == 0, st


# ------------------------------------------------------------------------------------------------ 6. generate
def test_generate_with_an_fp8_cache(folder):
    from mistral_inference.generate import generate
    h = _hip()
    model = qu._load(folder[0], B=1)
    prompt = qu.PROMPTS[1][0]
    toks, lps = generate([prompt], model, max_tokens=qu.N_DECODE, temperature=0.0, kv_dtype=F8)
    st = h.decode_engine_status(model._backend._workspace)
    assert st["engine_launches"] == 0 and st["steps"] >= qu.N_DECODE - 1 and st["status"] == 0, st
    assert len(toks[0]) == qu.N_DECODE and len(lps[0]) == len(prompt) - 1 + qu.N_DECODE
    with torch.inference_mode():
        cache = _kv_cache(1, F8)
        # the prompt as generate() runs it: its log-probabilities and the last token's logits by prompt_logprobs (whose one-row LM
        # head sums in another order than the 12-row forward's, as tests/test_gpu_fp8.py notes), every decode step by forward
        ids = torch.tensor(prompt, device="cuda")
        tgt = torch.tensor(prompt[1:] + [-1], dtype=torch.int32, device="cuda")
        lp_rows, last = model.prompt_logprobs(ids, [len(prompt)], cache, tgt)
        full = torch.log_softmax(model.forward(ids, [len(prompt)], _kv_cache(1, F8)), dim=-1)
        want = full[torch.arange(len(prompt) - 1), torch.tensor(prompt[1:])]
        assert float((lp_rows[:-1] - want).abs().max()) <= 1e-3
        assert lps[0][:len(prompt) - 1] == lp_rows[:-1].tolist()
        tok = last.argmax(-1)
        lp = torch.log_softmax(last, dim=-1).gather(1, tok[:, None])[:, 0]   # the first sample is drawn by torch in generate()
        ref_t, ref_lp = [int(tok)], [float(lp)]
        for _ in range(qu.N_DECODE - 1):
            tok, lp = h.greedy_sample(model.forward(tok, [1], cache))
            ref_t.append(int(tok))
            ref_lp.append(float(lp))
    assert toks[0] == ref_t
    assert lps[0][len(prompt) - 1:] == ref_lp
    # the default is the model's dtype, and that generation differs somewhere (the cache does round)
    toks16, lps16 = generate([prompt], model, max_tokens=qu.N_DECODE, temperature=0.0)
    assert lps16 != lps


# ------------------------------------------------------------------------------------------------ 7. engine
def test_engine_declines_an_fp8_cache():
    """Dims at which a dense batch-1 step runs on the persistent engine: with an FP8 cache every step takes the launch path."""
    from mistral_inference.cache import BufferCache
    h = _hip()
    m, _ = _model(mo.OracleArgs(**SHAPES["gqa4_window_wraps"]), seed=23)
    a = m.args
    ids = torch.randint(0, a.vocab_size, (40,), generator=torch.Generator().manual_seed(3)).cuda()
    prev = h.set_decode_engine(True)
    try:
        for dtype in (F8, BF):     # (one workspace: the launch counter is read after each run)
            c = BufferCache(m.n_local_layers, 1, 64, a.n_kv_heads, a.head_dim, a.sliding_window, device="cuda", dtype=dtype)
            c.reset()
            with torch.inference_mode():
                outs = [m.forward(ids[:30], [30], c)]
                for i in range(30, 40):
                    outs.append(m.forward(ids[i:i + 1], [1], c).clone())
            torch.cuda.synchronize()
            st = h.decode_engine_status(m._backend._workspace)
            assert st["status"] == 0 and all(bool(torch.isfinite(o).all()) for o in outs), st
            if dtype == F8:
                assert st["engine_launches"] == 0, st
            else:
                assert st["engine_launches"] > 0, st
    finally:
        h.set_decode_engine(prev)


# ------------------------------------------------------------------------------------------------ 8. refusals on the device
def test_fp16_model_refuses_an_fp8_cache():
    from mistral_inference.args import TransformerArgs
    from mistral_inference.cache import BufferCache
    from mistral_inference.transformer import Transformer
    args = qu.MODEL
    targs = TransformerArgs.from_dict(mo.params_json(args))
    targs.max_batch_size = 1
    with torch.device("meta"):
        m = Transformer(targs)
    m = m.to(torch.float16).to_empty(device="cuda")
    m.load_state_dict({k: v.to(torch.float16).cuda() for k, v in mo.synth_weights(args, seed=21).items()}, assign=True)
    m.eval()
    ids = torch.tensor([3, 1, 4], device="cuda")
    c8 = BufferCache(args.n_layers, 1, 64, args.n_kv_heads, args.head_dim, args.sliding_window, device="cuda", dtype=F8)
    with pytest.raises(NotImplementedError, match=r"FP8 K/V cache.*float16"):
        m.forward(ids, [3], c8)
    cb = BufferCache(args.n_layers, 1, 64, args.n_kv_heads, args.head_dim, args.sliding_window, device="cuda", dtype=BF)
    with pytest.raises(RuntimeError, match="cache dtype torch.bfloat16 != model dtype torch.float16"):   # every other mismatch, as ever
        m.forward(ids, [3], cb)
    cf = BufferCache(args.n_layers, 1, 64, args.n_kv_heads, args.head_dim, args.sliding_window, device="cuda", dtype=torch.float16)
    assert bool(torch.isfinite(m.forward(ids, [3], cf)).all())
    # the library's own refusal, whatever Python checks
    L = _hip().lib()
    from test_abi import _tiny_model, _valid_decode_batch
    bt = _valid_decode_batch()
    bt.kv_layout = 0x11
    assert L.mi_forward_generic(C.byref(_tiny_model()), C.byref(bt), 1, None) == -4 and b"MI_KV_E4M3" in L.mi_last_error_detail()
