#!/usr/bin/env python3
"""tools/code_object_ab.py — is a kernel of one built object the same instructions as a kernel of another?  Works on what the Makefile
built, not on a second compile: takes the gfx950 code object out of each host object's .hip_fatbin (objcopy, clang-offload-bundler),
disassembles it (llvm-objdump -d, no addresses, no encodings) and compares the two kernels' text line by line from the entry to
s_endpgm (behind it lies the padding to the next kernel, which depends on what follows).  No GPU needed.

    tools/build_ab.sh                      # the parent commit's objects -> meters.lv2_amd/lib_ab/obj
    python3 tools/code_object_ab.py meters.lv2_amd/lib_ab/obj/mtr_bank.o _Z6k_bank13mtr_bank_args \\
                                    meters.lv2_amd/lib/obj/mtr_bank.o _Z6k_bankI13mtr_bank_argsEvT_
Exit status 0: identical.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def kernel(obj, sym, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    targets = subprocess.check_output([LLVM + "/clang-offload-bundler", "--list", "--type=o", "--input=" + fat], text=True).split()
    target = [t for t in targets if "gfx950" in t][0]
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + target, "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, on = [], False
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.*)>:", line)
        if m:
            on = m.group(1) == sym
            continue
        if on and line.strip():
            out.append(re.sub(r"\s+", " ", re.sub(r"\s*//.*$", "", line.strip())))
            if out[-1].startswith("s_endpgm"):
                break
    if not out:
        sys.exit(f"{obj}: no kernel {sym}")
    return out


if __name__ == "__main__":
    if len(sys.argv) != 5:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernel(sys.argv[1], sys.argv[2], tmp, "a"), kernel(sys.argv[3], sys.argv[4], tmp, "b")
    same = a == b
    print(f"{sys.argv[2]}: {len(a)} instructions; {sys.argv[4]}: {len(b)} instructions; {'identical' if same else 'DIFFERENT'}")
    if not same:
        for i, line in enumerate(difflib.unified_diff(a, b, lineterm="", n=1)):
            if i < 60:
                print(line)
    sys.exit(0 if same else 1)
