"""What the engine objects export (csrc/kernels.h: EngineBuild).  csrc/decode_engine.hip holds the kernels and is compiled once per
build; each of those objects defines ONE external name, the accessor to its descriptor - everything else about the engine is
csrc/decode_engine_host.hip, compiled once, which alone defines the residency census kernel.  CPU only: the objects are those
of build_native.build(), the symbol tables are read with nm.  Names only; no instruction is looked at."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))

ACCESSORS = {"decode_engine.o": "decode_engine_build()", "decode_engine_next.o": "decode_engine_build_next()",
             "decode_engine_nemo.o": "decode_engine_build_nemo()", "decode_engine_wide.o": "decode_engine_build_wide()",
             "decode_engine_moe.o": "decode_engine_build_moe()"}


def _externals(obj):
    """Demangled names of the external symbols an object defines, without the compiler's own (`__hip_cuid_...`, `DW.ref...`)."""
    import build_native as b
    b.build(verbose=False)
    llvm = os.path.join(os.path.dirname(os.path.realpath(b._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    nm = llvm if os.path.exists(llvm) else (shutil.which("llvm-nm") or shutil.which("nm"))
    assert nm, "neither llvm-nm nor nm found"
    r = subprocess.run([nm, "--defined-only", "--extern-only", "--demangle", os.path.join(b.OBJ, obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = [line.split(None, 2)[2] for line in r.stdout.splitlines() if len(line.split(None, 2)) == 3]
    return [n for n in names if not n.startswith(("__", "DW.ref."))]


def test_every_build_is_listed():
    import build_native as b
    objs = ["decode_engine.o"] + [o for o, (src, _) in b.VARIANT_OBJECTS.items() if src == "decode_engine.hip"]
    assert sorted(objs) == sorted(ACCESSORS)
    assert "decode_engine_host.hip" in b.SOURCES and "decode_engine_host.hip" not in b.PER_FILE_FLAGS


@pytest.mark.parametrize("obj", sorted(ACCESSORS))
def test_engine_object_exports_its_accessor_and_nothing_else(obj):
    assert _externals(obj) == [ACCESSORS[obj]]


def test_host_object_defines_the_census_kernel_once():
    names = _externals("decode_engine_host.o")
    assert sum(n.startswith("engine_census_kernel(") for n in names) == 1, names
    for obj in ACCESSORS:
        assert not any("engine_census_kernel" in n for n in _externals(obj)), obj
