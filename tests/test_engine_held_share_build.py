"""Static checks of the round-7 headline engine build (build_native.ENGINE_NEXT_FLAGS: ENG_HOLD_GATE): no spill, no scratch
instruction, at most 256 VGPRs, and the round-7 switches stay out of every other engine object, whose source tokens must not change (csrc/decode_engine.hip header: the
kernel's speed moves with any change of its code).  CPU only: hipcc cross-compiles."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "mistral-inference_amd"))


def test_next_build_takes_the_round7_switches_and_no_other_object_does():
    import build_native as b
    assert "-DENG_HOLD_GATE=1" in b.ENGINE_NEXT_FLAGS
    for obj, (_, flags) in b.VARIANT_OBJECTS.items():
        if obj != "decode_engine_next.o":
            assert not any(f.startswith(("-DENG_HOLD_GATE", "-DENG_STALL_TRACE")) for f in flags), obj
    for flags in b.PER_FILE_FLAGS.values():
        assert not any("ENG_HOLD_GATE" in f for f in flags)


def test_next_build_has_no_spill_and_no_scratch():
    import build_native as b
    import engine_loader_waits as w
    flags = [f for f in b.ENGINE_NEXT_FLAGS if not f.startswith("-DENG_SUFFIX")] + ["-DENG_SUFFIX=_chk"]
    with tempfile.TemporaryDirectory() as d:
        asm = open(w.compile_to_asm(flags, d)).read()
    kernels = [m for m in re.finditer(r"\.vgpr_count:\s+(\d+)", asm)]
    assert kernels
    assert max(int(m.group(1)) for m in kernels) <= 256
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm))
    assert all(int(x) == 0 for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm))
    scratch = [l for l in asm.splitlines() if re.match(r"\s*scratch_\w+", l)]
    assert not scratch, scratch[:4]


def _device_tokens(flags):
    import build_native as b
    clang = os.path.join(os.path.dirname(os.path.realpath(b._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    r = subprocess.run([clang, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-E", "-P", "-std=c++17", *flags,
                        os.path.join(b.CSRC, "decode_engine.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_round7_code_is_compiled_out_of_the_other_engine_objects():
    """The preprocessed device source of the default, wide, MoE and Nemo objects does not name anything of round 7."""
    import build_native as b
    sets = [[]] + [flags for obj, (src, flags) in b.VARIANT_OBJECTS.items() if src == "decode_engine.hip" and obj != "decode_engine_next.o"]
    assert len(sets) >= 4
    for flags in sets:
        text = _device_tokens(flags)
        for name in ("run_holder_x", "hold_may_fetch", "st_attn", "C_LFULL"):
            assert name not in text, (flags, name)
    nxt = _device_tokens(list(b.ENGINE_NEXT_FLAGS))
    assert "run_holder_x" in nxt and "C_LFULL" in nxt and "hold_may_fetch" in nxt

