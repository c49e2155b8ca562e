"""The generic-storage linears (csrc/generic.hip: g_gemv_kernel, g_gemm_mfma_kernel, g_gemm_kernel) in fp32, fp16 and bf16 on
inputs whose every contraction is an exact integer sum (generic_linear_cases.py), compared bit for bit, sentinels included, with
one fp64 reference that rounds where the kernels round.  Every case first asserts the route its call takes (the mirror of
linear_t / launch_g_linear in generic_linear_cases.route) and prints the label; x has ldx > K, the output is a view of a
sentinel-filled buffer (ldo = N + 8) that is compared WHOLE, the residual has a row stride of its own where the entry takes one,
and the call runs twice with bit-equal results.  Plain calls go through mi_linear_generic with the case's dtype code - bf16
included, so that the sbf16 compile of the three kernels runs, not the tuned bf16 path -, the fused forms (three matrices in one
launch, the RMSNorm prologue, SwiGLU, `active`, ldr != ldo) through mi_debug_linear_generic_fused.  Nothing here sets
MI_GENERIC_MFMA or MI_GENERIC_G256: the cases take the default routes.

That the emulated kernels equal the reference and that every single fault - a piece, a chunk tail, a surplus row, a column past
N, a segment boundary, a K slab, a rounding point, a stride - changes the cases it applies to is proved on the CPU in
test_generic_linear_cases_host.py."""
import ctypes as C

import pytest
import torch

import generic_linear_cases as glc
import linear_cases as lc

pytestmark = pytest.mark.gpu

CASES = glc.all_cases()


def _once(h, case, inp, x, w, norm_w, active):
    out_buf = torch.full((case.M + 4, case.N + 8), lc.SENT, dtype=case.odt, device="cuda")
    out = out_buf[2:2 + case.M, :case.N]
    res = glc.res_view(inp.resbuf.cuda(), case) if case.epi == lc.RESIDUAL else None
    assert out.stride(0) == case.N + 8 and (res is None or (res.stride(0) == case.ldr and (res.stride(0) != out.stride(0)) == case.own_ldr))
    epi = lc.EPI_CODE[case.epi]
    if case.leaf:
        h.debug_linear_generic_fused(x, w, epi, out, residual=res, norm_w=norm_w, eps=0.0, active=active)
    else:
        wp = (C.c_void_p * 3)(h.dev_ptr(w[0], case.R), None, None)
        nr = (C.c_int * 3)(case.N, 0, 0)
        h.check(h.lib().mi_linear_generic(h.dev_ptr(out, case.odt), out.stride(0), h.dev_ptr(x, case.R), x.stride(0), case.M, case.K, wp, nr, epi,
                                          h.dev_ptr(res, case.R), glc.DT_CODE[case.dtype], h.stream_ptr(x.device)), "mi_linear_generic")
    return out_buf.cpu()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_generic_linear(case):
    from mistral_inference import _hip as h
    assert glc.case_route(case) == case.path, (case, glc.case_route(case))
    print(f"{case}: {case.path}" + (" (debug leaf)" if case.leaf else ""))
    inp = glc.inputs(case)
    x = glc.x_view(inp.xbuf.cuda(), case)
    assert x.stride(0) == case.ldx > case.K and (x.data_ptr() % 16 == 8) == case.misalign
    w = [wi.cuda() for wi in inp.w]
    norm_w = inp.norm_w.cuda() if case.norm else None
    active = case.active_rows().cuda() if case.active is not None else None
    got, again = _once(h, case, inp, x, w, norm_w, active), _once(h, case, inp, x, w, norm_w, active)
    assert glc.mismatch(case, again, got) is None, ("the second run differs", glc.mismatch(case, again, got))
    want = glc.expected(case)
    assert got.dtype == want.dtype
    bad = glc.mismatch(case, got, want)
    assert bad is None, bad


def test_fused_forms_without_a_kernel_are_refused():
    """More than 8 rows: no kernel takes three matrices, a norm prologue or SwiGLU (fp16 from 256 rows aside) - the leaf says so
    before any launch, as g_linear_fused_ok does for mi_forward_generic."""
    from mistral_inference import _hip as h
    assert glc.route(9, 64, 16, 64, True, "bf16", "fused") == "unsupported"
    x = torch.zeros(9, 64, dtype=torch.bfloat16, device="cuda")
    w = [torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    out = torch.full((9, 16), lc.SENT, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="no kernel takes this fused form"):
        h.debug_linear_generic_fused(x, w, lc.EPI_CODE[lc.STORE], out)
    assert bool((out == lc.SENT).all())
