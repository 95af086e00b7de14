#!/usr/bin/env python3
"""Is the device code of two builds of the library the same?  For every object of kvazaar_amd/build.py's units in two object directories: the gfx950 code object is
extracted, and per kernel symbol the disassembled instruction stream (branches are relative: the text does not depend on where the kernel lies), the kernel
descriptor (its 64 bytes but for the entry offset, which says where the kernel lies) and the resources of the metadata note (VGPRs, AGPRs,
SGPRs, scratch, LDS, kernarg bytes) are compared.  One line per kernel; exit status 1 when a kernel differs or the sets of kernel symbols do.

usage: tools/isa_compare.py <parent obj dir> <obj dir> [> profiles/<name>_isa_compare.txt]   (no GPU needed)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size", ".vgpr_spill_count", ".sgpr_spill_count")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, **kw).stdout


def kernels(obj):
    """{kernel symbol: (instruction count, digest of the instruction stream, descriptor bytes, resources)} of the object's gfx950 code object"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "unit.o")
        os.symlink(os.path.abspath(obj), tmp)
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", tmp, cwd=d)
        for co in sorted(os.path.join(d, f) for f in os.listdir(d) if "gfx950" in f):
            notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).decode()
            res = {}
            for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + notes.split("amdhsa.kernels:", 1)[-1])[1:]:
                entry = "    .agpr_count:" + entry
                name = re.search(r"\.name:\s+(\S+)", entry).group(1)
                res[name] = {k: int(m.group(1)) for k in RESOURCES for m in [re.search(re.escape(k) + r":\s+(\d+)", entry)] if m}
            sections = run(os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co).decode()
            at = {m.group(1): (int(m.group(2), 16), int(m.group(3), 16)) for m in re.finditer(r"\]\s+(\.\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", sections)}  # name -> (address, file offset)
            image = open(co, "rb").read()
            kd = {}
            for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+OBJECT\s+\S+\s+\S+\s+\d+\s+(\S+)\.kd$", run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co).decode(), re.M):
                addr, size = int(m.group(1), 16), int(m.group(2))
                raw = image[addr - at[".rodata"][0] + at[".rodata"][1]:][:size]
                kd[m.group(3)] = raw[:16] + bytes(8) + raw[24:]  # without kernel_code_entry_byte_offset: where the object's layout put the code
            dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co).decode()
            for m in re.finditer(r"\n[0-9a-f]+ <([^>]+)>:\n(.*?)(?=\n[0-9a-f]+ <[^>]+>:\n|\Z)", dis, re.S):
                if m.group(1) not in kd:
                    continue  # (a label inside a kernel, a device function kept out of line)
                insts = [re.sub(r"\s*//.*$", "", line).strip() for line in m.group(2).splitlines() if line.strip()]
                while insts and insts[-1] in ("s_code_end", "s_nop 0"):  # the padding behind a kernel: how much depends on what follows it in the object
                    insts.pop()
                out[m.group(1)] = (len(insts), hashlib.sha256("\n".join(insts).encode()).hexdigest()[:16], kd[m.group(1)], res.get(m.group(1)))
            assert set(kd) <= set(out) and set(kd) == set(res), (obj, sorted(set(kd) ^ set(res)))
    return out


def main():
    from kvazaar_amd.build import UNITS
    a_dir, b_dir = sys.argv[1:3]
    bad = new = 0
    for unit, _, _ in UNITS:
        new_unit = not os.path.exists(os.path.join(a_dir, unit + ".o"))  # a translation unit the change adds: its kernels are listed, the parent has nothing to hold them against
        a, b = ({} if new_unit else kernels(os.path.join(a_dir, unit + ".o"))), kernels(os.path.join(b_dir, unit + ".o"))
        for name in sorted(set(a) | set(b)):
            if new_unit:
                verdict = "NEW UNIT"
            elif name not in a or name not in b:
                verdict = "ONLY IN THE " + ("PARENT" if name in a else "CHANGE")
            else:
                same = [a[name][1] == b[name][1] and a[name][0] == b[name][0], a[name][2] == b[name][2], a[name][3] == b[name][3]]
                verdict = "identical" if all(same) else "DIFFERS in " + ", ".join(w for w, s in zip(("instructions", "descriptor", "resources"), same) if not s)
            n, digest, _, r = (b if name in b else a)[name]
            bad += verdict not in ("identical", "NEW UNIT")
            new += verdict == "NEW UNIT"
            print(f"{unit} {name}: {verdict} -- {n} instructions sha256 {digest}, VGPRs {r['.vgpr_count']} AGPRs {r.get('.agpr_count', 0)} SGPRs {r['.sgpr_count']} scratch {r['.private_segment_fixed_size']} B "
                  f"LDS {r['.group_segment_fixed_size']} B")
    print(f"{('ALL KERNELS OF THE PARENT IDENTICAL' if new else 'ALL KERNELS IDENTICAL') if not bad else str(bad) + ' KERNELS DIFFER'} ({len(UNITS)} objects{', ' + str(new) + ' kernels in new units' if new else ''})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
