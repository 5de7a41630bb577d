#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds of the kernel library (a refactor must not change what the compiler emits).

    python tools/isa_table.py BEFORE_OBJ_DIR AFTER_OBJ_DIR      # the build/obj directories cistgcn_amd/build.py leaves behind

Every object is unbundled, disassembled and split at its kernel symbols.  A kernel is `identical` when its instruction stream (mnemonics
and operands, addresses and comments stripped) is the same text in both builds; otherwise the line gives VGPRs, SGPRs, scratch bytes, LDS
bytes (the kernel's metadata note) and code bytes before -> after.  Needs hipcc's LLVM tools; no GPU."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def device_code(obj, tmp):
    """the gfx950 code object out of the fat binary section of a host object"""
    fat, co = os.path.join(tmp, os.path.basename(obj) + ".fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co], check=True)
    return co


def kernels(co):
    """{kernel symbol: (instruction lines, code bytes, {vgpr, sgpr, scratch, lds})}"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for block in notes.split("\n  - .")[1:]:
        f = dict(re.findall(r"\n    \.(\w+):\s+(\S+)", "\n    ." + block))
        if f.get("symbol", "").endswith(".kd"):
            meta[f["symbol"][:-3]] = dict(vgpr=int(f.get("vgpr_count", -1)), agpr=int(f.get("agpr_count", 0)), sgpr=int(f.get("sgpr_count", -1)),
                                   scratch=int(f.get("private_segment_fixed_size", -1)), lds=int(f.get("group_segment_fixed_size", -1)))
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, name, first = {}, None, None
    for line in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            name = m.group(2) if m.group(2) in meta else None       # anything else: a device function that was not inlined
            if name:
                out[name] = [[], 0, meta[name]]
                first = None
            continue
        m = re.match(r"^\s+(.*?)\s*//\s*([0-9A-F]+):", line)
        if m and name in out:
            text = re.sub(r"\s+", " ", m.group(1))
            addr = int(m.group(2), 16)
            if first is None:
                first = addr
            out[name][0].append((text, addr - first))
    for rec in out.values():                                # the padding behind the last instruction up to the next kernel is not code
        while rec[0] and rec[0][-1][0].split()[0] in ("s_nop", "s_code_end"):
            rec[0].pop()
        rec[1] = rec[0][-1][1] + 4 if rec[0] else 0          # up to the start of the last instruction + its first dword
        rec[0] = [t for t, _ in rec[0]]
    return out


def table(before_dir, after_dir):
    lines, same, differ = [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        ta, tb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        os.makedirs(ta), os.makedirs(tb)
        for obj in sorted(glob.glob(os.path.join(after_dir, "*.o"))):
            base = os.path.basename(obj)
            prev = os.path.join(before_dir, base)
            new = kernels(device_code(obj, tb))
            old = kernels(device_code(prev, ta)) if os.path.exists(prev) else {}
            lines.append("%s: %d kernels" % (base, len(new)))
            for k in sorted(set(old) | set(new)):
                short = k
                if shutil.which("c++filt"):
                    short = re.sub(r"\(.*\)$", "", subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip() or k)
                if k not in old or k not in new:
                    lines.append("  %-90s only %s" % (short, "after" if k in new else "before"))
                    differ += 1
                    continue
                (ia, ba, ma), (ib, bb, mb) = old[k], new[k]
                if ia == ib and ma == mb:
                    lines.append("  %-90s identical  (vgpr %d agpr %d sgpr %d scratch %d lds %d, %d code bytes)" % (short, mb["vgpr"], mb["agpr"], mb["sgpr"], mb["scratch"], mb["lds"], bb))
                    same += 1
                else:
                    lines.append("  %-90s differs    vgpr %d -> %d, agpr %d -> %d, sgpr %d -> %d, scratch %d -> %d, lds %d -> %d, code bytes %d -> %d, instructions %d -> %d"
                                 % (short, ma["vgpr"], mb["vgpr"], ma["agpr"], mb["agpr"], ma["sgpr"], mb["sgpr"], ma["scratch"], mb["scratch"], ma["lds"], mb["lds"], ba, bb, len(ia), len(ib)))
                    differ += 1
    lines.append("%d kernels identical, %d differ" % (same, differ))
    return lines


if __name__ == "__main__":
    print("\n".join(table(sys.argv[1], sys.argv[2])))
