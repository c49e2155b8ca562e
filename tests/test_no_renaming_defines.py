"""No source under csrc/ #defines a name that a shared header declares as a function, a type or a namespace: such a #define
renames the header's helper for one translation unit (or for the part of it behind the #define), and `bf_round` then rounds to
whatever the including file chose.  The per-element code goes through the structs ElemBf16 / ElemF16 of common.cuh instead.
CPU only; reads the project's sources."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))

SHARED_HEADERS = ["common.cuh", "kernels.h", "gemv_core.cuh", "attn_decode_core.cuh", "gemm256_core.cuh"]
# what may stand in front of `name(` without making it a declaration
_NOT_A_TYPE = {"return", "else", "case", "do", "new", "delete", "throw", "sizeof", "typename", "goto", "co_return"}


def _code(text):
    """The text without comments and string literals."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)


def _defined(text):
    return set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)", _code(text), flags=re.M))


def _declared(text):
    """Names a header declares as a namespace, a type (struct / class / enum / typedef / using) or a function."""
    code = re.sub(r"^[ \t]*#[^\n]*(?:\\\n[^\n]*)*", " ", _code(text), flags=re.M)  # preprocessor lines are not declarations
    names = set(re.findall(r"\bnamespace\s+([A-Za-z_]\w*)", code))
    names |= set(re.findall(r"\b(?:struct|class|enum(?:\s+class)?)\s+([A-Za-z_]\w*)", code))
    names |= set(re.findall(r"\busing\s+([A-Za-z_]\w*)\s*=", code))
    names |= set(re.findall(r"\btypedef\b[^;{}]*?\b([A-Za-z_]\w*)\s*(?:__attribute__\s*\(\([^;]*\)\))?\s*;", code))
    # a function: `name(` with a type in front of it (an identifier, `*`, `&` or `>`), not an operator, a comma or a keyword
    for m in re.finditer(r"(?:\b([A-Za-z_]\w*)\s+|[*&>]\s*)\b([A-Za-z_]\w*)\s*\(", code):
        if m.group(1) not in _NOT_A_TYPE:
            names.add(m.group(2))
    return names


def _hits(sources, declared):
    """(file, name) of every #define in `sources` ({file: text}) whose name is in `declared`."""
    return sorted((f, n) for f, text in sources.items() for n in _defined(text) & declared)


def _csrc():
    import build_native as b
    return {f: open(os.path.join(b.CSRC, f)).read() for f in sorted(os.listdir(b.CSRC)) if f.endswith((".hip", ".cuh", ".h"))}


def test_no_source_defines_a_name_that_a_shared_header_declares():
    src = _csrc()
    declared = set().union(*(_declared(src[h]) for h in SHARED_HEADERS))
    # the parse sees all three kinds in all five headers
    assert {"bf_round", "pack_bf2", "dot2_bf16", "swiglu_bf", "cvt_pk_bf16", "bf16x8", "ElemBf16", "ElemF16", "launch_gemv", "launch_gemm256",
            "gemm256_applicable", "attn_prefill_set_mode", "seg_row", "GemvArgs", "gemv_core", "gemv_body", "W16", "attn_core", "gemm256_core", "k_loop", "epilogue16", "ScaleRowCol", "i32x8"} <= declared
    assert len(src) >= 18 and sum(len(_defined(t)) for t in src.values()) > 50  # every file read, their #defines found
    assert not _hits(src, declared)


def test_the_check_sees_a_define_that_renames_a_helper():
    src = _csrc()
    declared = set().union(*(_declared(src[h]) for h in SHARED_HEADERS))
    assert _hits({"x.hip": "#if G256_F16\n#define bf_round g256_h_round\n#endif\n"}, declared) == [("x.hip", "bf_round")]
    assert _hits({"x.hip": "  #  define gemv_core gemv_core_f16\n#define bf16x8 g256_f16x8\n"}, declared) == [("x.hip", "bf16x8"), ("x.hip", "gemv_core")]
    assert _hits({"x.hip": "// #define bf_round g256_h_round\n#define G256_MFMA bf_round\n"}, declared) == []
