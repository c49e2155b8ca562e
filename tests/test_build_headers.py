"""Every header under csrc/ is a dependency of the build (build_native.HEADERS): objects are rebuilt only when a listed file is
newer, so a header that is not listed silently ships stale objects after an edit.  CPU only; reads the project's sources."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))


def test_every_csrc_header_is_a_build_dependency():
    import build_native as b
    headers = sorted(f for f in os.listdir(b.CSRC) if f.endswith((".cuh", ".h")))
    listed = {os.path.realpath(h) for h in b.HEADERS}
    assert len(headers) >= 5 and "gemm256_core.cuh" in headers  # the directory was read
    assert [h for h in headers if os.path.realpath(os.path.join(b.CSRC, h)) not in listed] == []
