#!/usr/bin/env python3
"""tools/isa_ab.py — do two builds' kernels compile to the same code?  Per kernel of two hipcc -save-temps device assemblies
(OLD NEW: *-hip-amdgcn-amd-amdhsa-gfx950.s of the same TU): the instruction census by class (tools/isa_blocks.py's classes) and
the VGPR / SGPR / scratch of the kernel metadata.  A kernel that gained a trailing `bool LEN` template parameter (or whose
argument type became std::conditional<false, ...>) is matched with its dense instantiation.

    hipcc --offload-arch=gfx950 -O3 -std=c++20 -Iinclude -Imeters.lv2_amd/csrc <the TU's flags from csrc/Makefile> -save-temps -c TU.hip
    python3 tools/isa_ab.py old/mtr_seg-hip-amdgcn-amd-amdhsa-gfx950.s new/mtr_seg-hip-amdgcn-amd-amdhsa-gfx950.s [--hunks]

--hunks: for every kernel that differs, also where: the two instruction streams with register numbers and label names taken out,
aligned, and each stretch that was inserted, deleted or replaced with its position, its length and its opcodes by count — a change
confined to a cold branch shows as a few long insertions, one per copy of the branch, and nothing else.
"""
import collections
import difflib
import re
import subprocess
import sys


def classify(op, line):
    if op.startswith("v_mfma") or op.startswith("v_smfma"): return "mfma"
    if op.startswith("v_"):
        if "dpp" in line or "row_shr" in line or "row_bcast" in line or "wave_shr" in line or "quad_perm" in line: return "vdpp"
        if op.startswith("v_pk_"): return "vpk"
        if op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane"): return "vlane"
        return "valu"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"): return "wait"
    if op.startswith("s_cbranch") or op.startswith("s_branch") or op.startswith("s_endpgm") or op.startswith("s_setpc"): return "br"
    if op.startswith("s_load") or op.startswith("s_buffer_load") or op.startswith("s_memtime"): return "smem"
    if op.startswith("s_"): return "salu"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"): return "vmem"
    if op.startswith("ds_"): return "lds"
    return "other"


def census(path):
    out, cur = {}, None
    for l in open(path):
        if re.match(r"^_Z\S+:", l):
            cur = l.split(":")[0]; out[cur] = collections.Counter(); continue
        s = l.strip()
        if cur and s.startswith(".Lfunc_end"): cur = None; continue
        if cur and s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
            out[cur][classify(s.split()[0], s)] += 1
    return out


def resources(path):
    res = {}
    for blk in re.split(r"\n  - \.", open(path).read()):
        n = re.search(r"\.name:\s+(_Z\S+)", blk)
        if n:
            g = lambda k: (re.search(k + r":\s+(\d+)", blk) or [None, "?"])[1]
            res[n.group(1)] = dict(vgpr=g(r"\.vgpr_count"), sgpr=g(r"\.sgpr_count"), scratch=g(r"\.private_segment_fixed_size"))
    return res


def stream(path):
    """{kernel: [instruction lines, registers and labels anonymous]}"""
    out, cur = {}, None
    for l in open(path):
        if re.match(r"^_Z\S+:", l):
            cur = l.split(":")[0]; out[cur] = []; continue
        s = l.strip()
        if cur and s.startswith(".Lfunc_end"): cur = None; continue
        if cur and s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
            s = re.sub(r"\s*;.*$", "", s)
            s = re.sub(r"\.LBB\d+_\d+", "LBB", s)
            s = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", s)
            out[cur].append(re.sub(r"\b([vsa])\d+\b", r"\1", s))
    return out


def hunks(a, b):
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    for tag, i1, i2, j1, j2 in sm.get_opcodes():
        if tag == "equal": continue
        ops = collections.Counter(["- " + x.split()[0] for x in a[i1:i2]] + ["+ " + x.split()[0] for x in b[j1:j2]])
        print("     %-7s old[%d:%d] (%d)  new[%d:%d] (%d)  %s" % (tag, i1, i2, i2 - i1, j1, j2, j2 - j1, dict(ops)))


def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()


def dense_name(n):
    d = re.sub(r"^void ", "", demangle(n))
    d = re.sub(r"std::conditional<false, (\w+), (\w+)>::type", r"\2", d)
    return re.sub(r"(, false>|<false>)\(", lambda m: ">(" if m.group(1) == ", false>" else "(", d)


def main(old, new, with_hunks=False):
    co, cn, ro, rn = census(old), census(new), resources(old), resources(new)
    so, sn = (stream(old), stream(new)) if with_hunks else ({}, {})
    by_dense = {dense_name(k): k for k in cn}
    same_all = True
    for k in co:
        kn = by_dense.get(re.sub(r"^void ", "", demangle(k)), k)
        same = co[k] == cn.get(kn) and ro.get(k) == rn.get(kn)
        same_all &= same
        print("%-4s %-60s %s" % ("SAME" if same else "DIFF", re.sub(r"\(anonymous namespace\)::", "", demangle(k))[:60], ro.get(k)))
        if not same:
            print("     old", dict(co[k]), "\n     new", dict(cn.get(kn, {})), rn.get(kn))
            if with_hunks and kn in sn: hunks(so[k], sn[kn])
    print("every kernel of the old build compiles to the same code" if same_all else "DIFFERENCES")
    return 0 if same_all else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], "--hunks" in sys.argv[3:]))
