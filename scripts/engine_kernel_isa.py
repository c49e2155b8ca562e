#!/usr/bin/env python3
"""Hash of the gfx950 ISA of every decode_engine_kernel<...> instantiation of an engine object, one kernel at a time.

    python scripts/engine_kernel_isa.py mistral-inference_amd/build/decode_engine_next.o [more objects]
    python scripts/engine_kernel_isa.py --symbol gemm256_w8a8_kernel mistral-inference_amd/build/gemm256_w8a8.o

--symbol NAME hashes the instantiations of another kernel template (default: decode_engine_kernel).

scripts/engine_isa_hash.sh hashes the whole disassembly of an object, which also moves when a kernel is added to or taken out
of the object.  This one cuts `llvm-objdump -d` at the kernels' symbols and drops the address column, so a kernel keeps its hash
wherever it sits in the object: what an edit that must leave the kernels alone is held to (profiles/engine_host_split_isa.txt).
Prints `object  instantiation  lines  md5`, the instantiations sorted by name.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj, symbol="decode_engine_kernel"):
    with tempfile.TemporaryDirectory() as d:
        x = os.path.join(d, "x.o")
        with open(obj, "rb") as f, open(x, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "x.o"], cwd=d, check=True, capture_output=True)
        dev = [f for f in os.listdir(d) if "gfx950" in f]
        if not dev:
            return {}
        r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", os.path.join(d, dev[0])], check=True, capture_output=True, text=True)
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip():
            out[name].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())  # the address column goes, the encoding stays
    return {k: v for k, v in out.items() if symbol in k}


if __name__ == "__main__":
    args, symbol = sys.argv[1:], "decode_engine_kernel"
    if args[:1] == ["--symbol"]:
        symbol, args = args[1], args[2:]
    for obj in args:
        for name, lines in sorted(kernels(obj, symbol).items()):
            short = re.search(re.escape(symbol) + r"<[^>]*>", name).group(0).replace(" ", "")
            print(os.path.basename(obj), short, len(lines), hashlib.md5("\n".join(lines).encode()).hexdigest())
