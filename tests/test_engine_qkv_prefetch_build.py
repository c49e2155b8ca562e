"""Static checks of the round-10 code of the headline engine build (ENG_QKV_HOLD=3, the source's default for a dense build that
passes ENG_HOLD_GATE=1, i.e. for build_native.ENGINE_NEXT_FLAGS): only decode_engine_next.o compiles it, the preprocessed
device source of every other engine object names nothing of round 10 (csrc/decode_engine.hip header: the kernel's speed moves with any change of its code), and the two measured alternatives
(scripts/build_variants.py: six held units, a fetch that ignores the hid sweep) still compile without a spill and without a
compiler-inserted wait in the loader's loops.  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))

ROUND10 = ("run_holder_both", "hold_may_fetch_qkv", "C_LEND", "C_HIDSWEEP", "QKV_WAVES")


def test_only_the_next_build_is_gated_and_so_gets_the_second_duty():
    import build_native as b
    assert "-DENG_HOLD_GATE=1" in b.ENGINE_NEXT_FLAGS and not any(f.startswith("-DENG_QKV_HOLD") for f in b.ENGINE_NEXT_FLAGS)
    for obj, (_, flags) in b.VARIANT_OBJECTS.items():
        if obj != "decode_engine_next.o":
            assert "-DENG_QKV_HOLD=3" not in flags and not any(f.startswith("-DENG_HOLD_GATE") for f in flags), obj
            assert not any(f.startswith(("-DENG_QKV_WAVES", "-DENG_QKV_SWEEP")) for f in flags), obj


def test_defaults_of_a_gated_build_are_the_measured_winner_and_zero_restores_round7():
    """The shipped flags, the same with ENG_QKV_HOLD=3 ENG_QKV_WAVES=2 spelt out (slot `r10_qh4`): one device source.  With
    ENG_QKV_HOLD=0 (slot `r7_gate_only`) nothing of round 10 is left."""
    import build_native as b
    import build_variants as bv
    base = ["-DENG_SUFFIX=_chk", "-DENG_HEADLINE_ONLY=1"]
    shipped = _device_tokens(base + list(bv.ENGINE_SLOTS["shipped"]))
    assert shipped == _device_tokens(base + list(bv.ENGINE_SLOTS["r10_qh4"]))
    only = _device_tokens(base + list(bv.ENGINE_SLOTS["r7_gate_only"]))
    assert not any(name in only for name in ROUND10) and "run_holder_x" in only


def _device_tokens(flags):
    import build_native as b
    clang = os.path.join(os.path.dirname(os.path.realpath(b._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    r = subprocess.run([clang, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-E", "-P", "-std=c++17", *flags,
                        os.path.join(b.CSRC, "decode_engine.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_round10_code_is_compiled_out_of_the_other_engine_objects():
    import build_native as b
    sets = [[]] + [flags for obj, (src, flags) in b.VARIANT_OBJECTS.items() if src == "decode_engine.hip" and obj != "decode_engine_next.o"]
    assert len(sets) >= 4
    for flags in sets:
        text = _device_tokens(flags)
        for name in ROUND10:
            assert name not in text, (flags, name)
    nxt = _device_tokens(list(b.ENGINE_NEXT_FLAGS))
    assert all(name in nxt for name in ROUND10)


def test_second_duty_needs_the_gate():
    """ENG_QKV_HOLD=3 without ENG_HOLD_GATE is refused at compile time: the fetch rule reads the loader's ring-full word."""
    import build_native as b
    flags = [f for f in b.ENGINE_NEXT_FLAGS if not f.startswith("-DENG_HOLD_GATE")] + ["-DENG_QKV_HOLD=3"]
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    r = subprocess.run([clang, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-E", "-P", "-std=c++17", *flags,
                        os.path.join(b.CSRC, "decode_engine.hip")], capture_output=True, text=True)
    assert r.returncode != 0 and "ENG_QKV_HOLD = 3" in r.stderr


@pytest.mark.parametrize("slot", ["r10_qh", "r10_qh4_sweep"])
def test_measured_alternatives_stay_clean(slot):
    import build_native as b
    import build_variants as bv
    import engine_loader_waits as w
    flags = ["-DENG_SUFFIX=_chk", "-DENG_HEADLINE_ONLY=1", *bv.ENGINE_SLOTS[slot]]
    with tempfile.TemporaryDirectory() as d:
        path = w.compile_to_asm(flags, d)
        reps, _ = w.analyse(path)
        asm = open(path).read()
    assert len(reps) == 1 and reps[0]["dma"] >= 60
    assert not [x for x in reps[0]["suspicious"] if x[3] > 0]
    assert max(int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", asm)) <= 256
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm))
    assert all(int(x) == 0 for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm))
    assert not [l for l in asm.splitlines() if re.match(r"\s*scratch_\w+", l)]
