"""Every -D<NAME> that a build recipe passes names a macro that the source it is compiled with reads: an entry whose switch has
left the source would build the stock kernel and report "no difference" for an experiment that never ran.  And the decode engine
refuses the switch values whose code was removed.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))


def _macros(flags):
    return [m.group(1) for f in flags for m in [re.match(r"-D([A-Za-z_][A-Za-z0-9_]*)(=|$)", f)] if m]


def _recipes():
    """(where, source file, flags) of every compile that build_native.py and scripts/build_variants.py describe."""
    import build_native as b
    import build_variants as v
    out = [(f"build_native.VARIANT_OBJECTS[{o}]", src, flags) for o, (src, flags) in b.VARIANT_OBJECTS.items()]
    out += [(f"build_native.{n}", "decode_engine.hip", getattr(b, n)) for n in dir(b) if re.fullmatch(r"ENGINE_[A-Z0-9_]*FLAGS", n)]
    out += [(f"build_variants.VARIANTS[{n}]", "decode_engine.hip", flags) for n, flags in v.VARIANTS.items()]  # whole-build flags
    out += [(f"build_variants.FILE_VARIANTS[{n}]", src, flags) for n, (src, flags) in v.FILE_VARIANTS.items()]
    out += [(f"build_variants.ENGINE_SLOTS[{n}]", "decode_engine.hip", flags) for n, flags in v.ENGINE_SLOTS.items()]
    return out


def test_every_macro_a_recipe_passes_is_read_by_its_source():
    import build_native as b
    recipes = _recipes()
    seen = {m for _, _, f in recipes for m in _macros(f)}
    assert {"ENG_SADDR", "ENG_HOLD_GATE", "ENG_STALL_TRACE", "ENG_HOLDERS", "G256_PRIO", "ATT_PRIO", "GEMV_F16"} <= seen  # all five tables parsed
    text = {}
    missing = []
    for where, src, flags in recipes:
        if src not in text:
            text[src] = open(os.path.join(b.CSRC, src)).read()
        missing += [(where, m) for m in _macros(flags) if not re.search(rf"\b{m}\b", text[src])]
    assert not missing, missing


def test_the_check_sees_a_macro_that_no_source_reads():
    assert _macros(["-DENG_NO_SUCH_SWITCH=1", "-O2", "-mllvm", "-DX"]) == ["ENG_NO_SUCH_SWITCH", "X"]
    import build_native as b
    assert not re.search(r"\bENG_NO_SUCH_SWITCH\b", open(os.path.join(b.CSRC, "decode_engine.hip")).read())


def _preprocess_engine(flags):
    import build_native as b
    return subprocess.run([b._hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-E", "-P", "-std=c++17", *flags,
                           os.path.join(b.CSRC, "decode_engine.hip"), "-o", os.devnull], capture_output=True, text=True)


@pytest.mark.parametrize("flag", ["-DENG_SADDR=1", "-DENG_QKV_HOLD=1", "-DENG_HOLD_STAGE=0"])
def test_engine_refuses_a_switch_value_that_is_not_built(flag):
    r = _preprocess_engine([flag])
    assert r.returncode != 0 and "error:" in r.stderr, r.stderr[-2000:]
    assert flag[2:].split("=")[0] in r.stderr


def test_engine_accepts_the_values_that_are_built():
    assert _preprocess_engine(["-DENG_SADDR=2", "-DENG_QKV_HOLD=2", "-DENG_HOLD_STAGE=1"]).returncode == 0
