#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libaeonflux_gpu.so, symbol by symbol (no GPU needed).

    python tools/kernel_diff.py variants/parent/aeonflux_amd/lib/libaeonflux_gpu.so aeonflux_amd/lib/libaeonflux_gpu.so

The code object is taken out of each library the way tests/test_kernel_isa.py does (llvm-objdump --offloading on a copy,
llvm-readelf --notes, llvm-objdump -d).  One row per kernel: VGPRs, SGPRs, scratch bytes, LDS bytes, instruction count of A -> B,
the waves per SIMD the registers allow (floor(512 / VGPRs rounded up to 8), at most 8; the launch bounds are the source's and are
the same on both sides when the source keeps them, so the uncapped figure compares at least as strictly), and whether the two
instruction streams are the same.  Instructions are compared as text without addresses; a PC-relative literal (the s_add_u32 /
s_addc_u32 after s_getpc_b64) is replaced by the symbol it reaches, so that a kernel does not count as changed because ANOTHER
kernel's size moved it or the constant it reads.  It compares two builds and nothing else.
Exit status 1 when the symbol sets differ or a kernel's scratch, LDS or waves per SIMD differ."""
import bisect
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def load(lib, d):
    os.makedirs(d)
    copy = shutil.copy(lib, os.path.join(d, "lib.so"))
    run(LLVM + "/llvm-objdump", "--offloading", copy, cwd=d)
    cos = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(cos) == 1, os.listdir(d)
    co = os.path.join(d, cos[0])
    notes = run(LLVM + "/llvm-readelf", "--notes", co)
    meta = {}
    for blk in notes.split(".args:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in FIELDS}
    # symbol table: address -> name, to name what a PC-relative literal reaches
    syms = sorted({(int(m.group(1), 16), m.group(2)) for m in re.finditer(r"^([0-9a-f]{16}) .{7} \S+\s+[0-9a-f]+ (?:\.\w+ )?(\S+)$", run(LLVM + "/llvm-objdump", "-t", co), re.M)})
    addrs = [a for a, _ in syms]

    def reaches(target):
        i = bisect.bisect_right(addrs, target) - 1
        return "<%s+%d>" % (syms[i][1], target - addrs[i]) if i >= 0 else "<pcrel>"

    bodies = {}
    dis = run(LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co)
    for f in re.split(r"\n(?=[0-9a-f]{16} <)", dis):
        m = re.match(r"[0-9a-f]{16} <(\S+)>:", f)
        if not m or m.group(1) not in meta:
            continue
        ins, pc, pcreg = [], None, None
        for ln in f.split("\n")[1:]:
            a = re.search(r"//\s*([0-9A-Fa-f]+):", ln)
            text = re.sub(r"\s*//.*", "", ln).strip()
            if not text or text.startswith(("s_nop", "s_code_end")):
                continue
            g = re.match(r"s_getpc_b64 s\[(\d+):\d+\]", text)
            if g and a:
                pcreg, pc = int(g.group(1)), int(a.group(1), 16) + 4   # the address of the next instruction
            elif pcreg is not None:
                lo = re.match(r"(s_add_u32 s%d, s%d, )(0x[0-9a-f]+|-?\d+)$" % (pcreg, pcreg), text)
                hi = re.match(r"(s_addc_u32 s%d, s%d, )(0x[0-9a-f]+|-?\d+)$" % (pcreg + 1, pcreg + 1), text)
                if lo:
                    v = int(lo.group(2), 0) & 0xffffffff
                    text = lo.group(1) + reaches(pc + (v - (1 << 32) if v >> 31 else v))
                elif hi:
                    text, pcreg = hi.group(1) + "<hi>", None
            ins.append(text)
        bodies[m.group(1)] = ins
    return meta, bodies


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    a_lib, b_lib = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        ma, ba = load(a_lib, os.path.join(d, "a"))
        mb, bb = load(b_lib, os.path.join(d, "b"))
    bad = 0
    only_a, only_b = sorted(set(ma) - set(mb)), sorted(set(mb) - set(ma))
    print("# tools/kernel_diff.py  A = %s  B = %s" % (a_lib, b_lib))
    print("# %d kernels in A, %d in B; only in A: %s; only in B: %s" % (len(ma), len(mb), only_a or "none", only_b or "none"))
    bad += len(only_a) + len(only_b)
    print("%-8s %-8s %-9s %-9s %-13s %-5s %-9s %s" % ("VGPRs", "SGPRs", "scratch", "LDS", "instructions", "waves", "identical", "kernel"))
    pair = lambda x, y: str(x) if x == y else "%d->%d" % (x, y)
    same = 0
    for k in sorted(set(ma) & set(mb)):
        x, y = ma[k], mb[k]
        ident = ba[k] == bb[k]
        same += ident
        wa, wb = waves(x["vgpr_count"]), waves(y["vgpr_count"])
        broke = x["private_segment_fixed_size"] != y["private_segment_fixed_size"] or x["group_segment_fixed_size"] != y["group_segment_fixed_size"] or wa != wb
        bad += broke
        print("%-8s %-8s %-9s %-9s %-13s %-5s %-9s %s%s" % (pair(x["vgpr_count"], y["vgpr_count"]), pair(x["sgpr_count"], y["sgpr_count"]),
              pair(x["private_segment_fixed_size"], y["private_segment_fixed_size"]), pair(x["group_segment_fixed_size"], y["group_segment_fixed_size"]),
              pair(len(ba[k]), len(bb[k])), pair(wa, wb), "yes" if ident else "NO", k, "   <-- scratch / LDS / waves differ" if broke else ""))
    print("# identical: %d of %d; scratch, LDS and waves per SIMD %s" % (same, len(set(ma) & set(mb)), "equal everywhere" if not bad else "DIFFER (or the symbol sets do)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
