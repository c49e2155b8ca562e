"""The switch of the weight-streaming GEMM of 9 .. 64 rows (csrc/gemm_skinny.hip) is host state: testable without a GPU."""


def test_debug_set_gemm_skinny_returns_the_previous_mode():
    from mistral_inference import _hip
    first = _hip.debug_set_gemm_skinny(-1)          # negative: keep
    assert first in (0, 1) and _hip.debug_set_gemm_skinny(-1) == first
    try:
        assert _hip.debug_set_gemm_skinny(0) == first
        assert _hip.debug_set_gemm_skinny(1) == 0
        assert _hip.debug_set_gemm_skinny(-1) == 1
    finally:
        _hip.debug_set_gemm_skinny(first)
