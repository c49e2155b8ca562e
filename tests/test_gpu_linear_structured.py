"""The dense linears behind `_hip.linear` and `_hip.qkv_rope_kvwrite` - gemv_kernel / gemv_kernel_nw at M <= 8, the 128 x 128 and
256 x 256 MFMA kernels with the tail split above, generic.hip and the fp16 compile of gemm256.hip for fp16 storage - on inputs
whose every contraction is an exact integer sum (linear_cases.py), compared with torch.equal to one fp64 reference that rounds
where the model rounds.  Every case first asserts the route its shape takes at this device's CU count (the mirror of the
launchers in linear_cases.route), writes into a view of a sentinel-filled buffer (two rows above and below, ldo = N + 8; the
residual has the same stride; the rings are full of the sentinel) that is compared WHOLE, and runs twice with bit-equal results.
That the emulated kernels equal the reference and that every single fault - one weight piece, one row at a segment boundary, one
K slice of one tile, one rounding point - changes the cases it applies to is proved on the CPU in test_linear_cases_host.py.

The fused RMSNorm forms are not here: rsqrt(ms + eps) is not exact, they stay under the envelopes of test_gpu_ops.py and
test_gpu_fp8.py."""
import ctypes as C

import pytest
import torch

import linear_cases as lc

pytestmark = pytest.mark.gpu

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
CASES = lc.all_cases(CUS)


def _hip():
    from mistral_inference import _hip
    return _hip


def _group(g, tail=False):
    return [c for c in CASES if c.group == g and ("-tail" in c.name) == tail]


def _guarded(M, N, dtype, fill=None):
    buf = torch.full((M + 4, N + 8), lc.SENT, dtype=dtype, device="cuda")
    view = buf[2:2 + M, :N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _linear_once(case, x, w, inp):
    h = _hip()
    buf, out = _guarded(case.M, case.N, case.odt)
    res = _guarded(case.M, case.N, case.R, inp.res)[1] if case.epi == lc.RESIDUAL else None
    assert out.stride(0) == case.N + 8 and (res is None or res.stride(0) == out.stride(0))
    got = h.linear(x, w, lc.EPI_CODE[case.epi], residual=res, out=out)
    assert got.data_ptr() == out.data_ptr()
    return [buf.cpu()]


def _qkv_once(case, x, w, inp, dev):
    h = _hip()
    H, Hkv, layout, seq = case.qkv
    N = (H + 2 * Hkv) * lc.HEAD
    buf, out = _guarded(case.M, N, lc.BF)
    ck = cv = None
    code = h.KV_SLOT_MAJOR
    if layout is not None:
        ck, cv = lc.new_ring(case).cuda(), lc.new_ring(case).cuda()
        code = h._kv_layout2(ck, cv)
        assert code == (h.KV_HEAD_MAJOR if layout == "head" else h.KV_SLOT_MAJOR) and ck.shape[1] == lc.RING_W
    h.check(h.lib().mi_qkv_rope_kvwrite(h.dev_ptr(out), out.stride(0), h.dev_ptr(x), x.stride(0), case.M, case.K, h.dev_ptr(w[0]), h.dev_ptr(w[1]),
                                        h.dev_ptr(w[2]), H, Hkv, lc.HEAD, None, C.c_float(0.0), h.dev_ptr(dev["cs"], torch.float32), lc.ROPE_LEN,
                                        h.dev_ptr(dev["pos"], torch.int32), h.dev_ptr(dev["seq"], torch.int32), h.ring_ptr(ck), h.ring_ptr(cv),
                                        lc.RING_W if ck is not None else 0, code, h.stream_ptr(x.device)), "mi_qkv_rope_kvwrite")
    return [buf.cpu()] + ([ck.cpu(), cv.cpu()] if ck is not None else [])


def _check(case):
    assert lc.route(case.M, case.K, case.N, case.epi, CUS, case.dtype, case.tail) == case.path, (case, CUS)
    assert case.blocks is None or lc.block_plan(case.M, case.K, case.N, case.epi, CUS) == case.blocks, (case, CUS)
    inp = lc.inputs(case)
    x, w = inp.x.cuda(), [wi.cuda() for wi in inp.w]
    if case.epi == lc.QKV:
        dev = dict(cs=inp.rope_cs.cuda(), pos=inp.tok_pos.cuda(), seq=inp.tok_seq.cuda() if inp.tok_seq is not None else None)
        run = lambda: _qkv_once(case, x, w, inp, dev)          # noqa: E731
    else:
        run = lambda: _linear_once(case, x, w, inp)            # noqa: E731
    got, again = run(), run()
    assert lc.differing(got, again) == 0, (case, "the second run differs", lc.describe(case, again, got))
    want = lc.expected(case)
    assert all(g.shape == e.shape and g.dtype == e.dtype for g, e in zip(got, want)) and len(got) == len(want)
    bad = lc.describe(case, got, want)
    assert not bad, (case, case.path, "(tensor, differing elements, first (row, col, ..) of the view - outside it: a guard element -, got, expected)", bad)
    assert all(torch.equal(g, e) for g, e in zip(got, want))


@pytest.mark.parametrize("case", _group("gemv"), ids=repr)
def test_gemv_leaf(case):
    _check(case)


@pytest.mark.parametrize("case", _group("qkv"), ids=repr)
def test_qkv_rope_kvwrite_leaf(case):
    _check(case)


@pytest.mark.parametrize("case", _group("g128"), ids=repr)
def test_gemm_128_tiles(case):
    _check(case)


@pytest.mark.parametrize("case", _group("g256"), ids=repr)
def test_gemm_256_tiles(case):
    _check(case)


@pytest.mark.parametrize("case", _group("g256", tail=True) or [None], ids=repr)
def test_gemm_tail_split(case):
    """launch_gemm's column split at gemm_tail = 2 (half-height tiles), 1 (the 128 kernel) and 0 (none), on tile counts built from
    this device's CU count."""
    if case is None:
        pytest.skip(f"no tile counts at {CUS} CUs for which launch_gemm splits the columns and the tail takes half-height tiles")
    h = _hip()
    try:
        h.debug_set_prefill_kernels(gemm_tail=case.tail)
        _check(case)
    finally:
        h.debug_set_prefill_kernels(gemm_tail=2)


@pytest.mark.parametrize("case", _group("f16"), ids=repr)
def test_fp16_linear(case):
    _check(case)


def test_qkv_w8_second_pass_without_tok_seq_keeps_its_ring_rows():
    """The pass loop is shared with the e4m3 leaf: two passes (D = 10240, 6 + 2 rows), a bf16 ring and no tok_seq - tokens 6, 7 are
    sequences 6, 7 in the second pass too.  Plain family: W in {-1, +1} is exact in e4m3, the row scales are 1, so the leaf must
    give the reference of the bf16 case bit for bit, rings included."""
    h = _hip()
    case = lc.Case("qkv-w8-h4kv2d10240t8-slot-noseq-plain", 8, 10240, (4 * lc.HEAD, 2 * lc.HEAD, 2 * lc.HEAD), lc.QKV, "gemv/TT=6/dma/2-pass",
                   qkv=(4, 2, "slot", False))
    assert lc.route(case.M, case.K, case.N, case.epi, CUS) == case.path and lc.passes(case.M, case.K) == [(0, 6), (6, 2)]
    lc.conditions(case)
    inp = lc.inputs(case)
    w8 = [wi.to(torch.float8_e4m3fn) for wi in inp.w]
    assert all(torch.equal(q.to(lc.BF), wi) for q, wi in zip(w8, inp.w))
    w8 = [q.cuda() for q in w8]
    sc = [torch.ones(q.shape[0], dtype=torch.float32, device="cuda") for q in w8]
    x, cs, pos = inp.x.cuda(), inp.rope_cs.cuda(), inp.tok_pos.cuda()
    want = lc.reference(case)
    for _ in range(2):
        ck, cv = lc.new_ring(case).cuda(), lc.new_ring(case).cuda()
        out = h.qkv_rope_kvwrite_w8(x, w8[0], w8[1], w8[2], sc[0], sc[1], sc[2], lc.HEAD, cs, pos, cache_k=ck, cache_v=cv, tok_seq=None)
        got = [out.cpu(), ck.cpu(), cv.cpu()]
        assert all(torch.equal(g, e) for g, e in zip(got, want)), lc.describe(case, [torch.nn.functional.pad(got[0], (0, 8, 2, 2))] + got[1:],
                                                                              [torch.nn.functional.pad(want[0], (0, 8, 2, 2))] + list(want[1:]))
