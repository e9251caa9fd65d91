#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libvdiff_hip.so (CPU only).

    python tools/isa_diff.py OLD/libvdiff_hip.so NEW/libvdiff_hip.so [--show N]

A refactor that moves kernels between translation units must leave every kernel's code as it
was.  This tool unbundles the device code objects of both libraries (objcopy of .hip_fatbin,
then clang-offload-bundler per bundle, as tests/test_kernel_resources.py does), disassembles
them with llvm-objdump and reports

  * the kernels present in only one build, and any kernel a build holds more than once,
  * for each kernel in both, whether the instruction streams are equal,
  * for each kernel in both, its metadata: VGPRs, AGPRs, SGPRs, LDS bytes
    (group_segment_fixed_size), scratch bytes (private_segment_fixed_size) and the VGPR / SGPR
    spill counts, and whether they are equal.

It diffs and summarises; it does not look for particular instructions.

What is normalised away, and nothing else — only what depends on where a kernel or a global
sits inside its code object:

  1. objdump's trailing comment of each line: the instruction's absolute address, its encoding
     words, and the `<symbol+offset>` label objdump prints for a branch target.  The
     instruction text that is compared is the full decoding of those words; a branch's operand
     is printed as a pc-relative word count and is compared as it stands.
  2. the literals of a pc-relative address formation: after `s_getpc_b64 s[N:N+1]`, the
     constant operand of the `s_add_u32 sN, sN, <lit>` and `s_addc_u32 sN+1, sN+1, <lit>` that
     add the distance from this instruction to a global (they become `<pcrel>`).
  3. a trailing `...` after a kernel's last instruction: objdump's mark for the zero fill up
     to the next symbol's alignment, present or not according to what follows the kernel.

Exit status 0 when the kernel sets, every stream and every metadata row are equal, else 1.
"""
from __future__ import annotations

import argparse
import difflib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count")


def code_objects(lib: Path, tmp: Path):
    fat = tmp / "fatbin"
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", str(lib), str(tmp / "junk.so")],
                   check=True, capture_output=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)] + [len(blob)]
    targets = sorted(set(re.findall(rb"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob)))
    if len(starts) < 2 or not targets:
        sys.exit(f"{lib}: no uncompressed hipv4 offload bundle in .hip_fatbin")
    target = f"hipv4-amdgcn-amd-amdhsa--{targets[0].decode()}"
    for i in range(len(starts) - 1):
        chunk, co = tmp / f"b{i}", tmp / f"b{i}.co"
        chunk.write_bytes(blob[starts[i]:starts[i + 1]])
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={chunk}",
                        f"--targets={target}", f"--output={co}"], check=True, capture_output=True)
        yield co


def metadata(co: Path):
    """{kernel: {field: value}} from the amdhsa.kernels note."""
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                           text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        if re.match(r"\s{2}- \.", line):  # a new kernel entry
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"\s{4}\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            out[m.group(2)] = cur
        elif m.group(1) in META:
            cur[m.group(1)] = int(m.group(2))
    return out


def normalise(lines):
    """The instruction texts of one kernel under the normalisation of the module docstring."""
    out, pc = [], {}  # pc: scalar register -> True while its pc-relative add is still to come
    for line in lines:
        ins = line.split("//")[0].strip()
        if not ins:
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            pc = {f"s{m.group(1)}": True, f"s{m.group(2)}": True}
        else:
            m = re.match(r"(s_add_u32|s_addc_u32) (s\d+), (s\d+), (\S+)$", ins)
            if m and m.group(2) == m.group(3) and pc.pop(m.group(2), False):
                ins = f"{m.group(1)} {m.group(2)}, {m.group(3)}, <pcrel>"
        out.append(ins)
    while out and out[-1] == "...":
        out.pop()
    return out


def kernels(lib: Path):
    """({kernel: (instructions, metadata)}, [names held more than once]) of one library."""
    out, dup = {}, []
    with tempfile.TemporaryDirectory() as t:
        for co in code_objects(lib, Path(t)):
            meta = metadata(co)
            asm = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], check=True, capture_output=True,
                                 text=True).stdout
            body, name = {}, None
            for line in asm.splitlines():
                m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    body[name] = []
                elif name and line.startswith("\t"):
                    body[name].append(line)
            for k, md in meta.items():
                if k in out:
                    dup.append(k)
                out[k] = (normalise(body.get(k, [])), md)
    return out, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--show", type=int, default=20, help="diff lines printed per differing kernel")
    a = ap.parse_args()
    for tool in ("clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not (LLVM / tool).exists():
            sys.exit(f"{tool} not in {LLVM}")
    if shutil.which("objcopy") is None:
        sys.exit("objcopy not found")
    (old, dup_old), (new, dup_new) = kernels(a.old), kernels(a.new)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = sorted(set(old) & set(new))
    print(f"kernels: old {len(old)}, new {len(new)}, in both {len(both)}")
    for title, names in (("only in old", only_old), ("only in new", only_new), ("more than once in old", dup_old),
                         ("more than once in new", dup_new)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
    ndiff = nmeta = 0
    print(f"\n{'kernel':<96} {'instr':>6} {'vgpr':>4} {'agpr':>4} {'sgpr':>4} {'lds':>6} {'scratch':>7} {'spill':>5}  "
          "code meta")
    for k in both:
        (io, mo), (inw, mn) = old[k], new[k]
        same_i, same_m = io == inw and len(io) > 0, mo == mn
        ndiff += not same_i
        nmeta += not same_m
        print(f"{k[:96]:<96} {len(inw):>6} {mn.get('vgpr_count', 0):>4} {mn.get('agpr_count', 0):>4} "
              f"{mn.get('sgpr_count', 0):>4} {mn.get('group_segment_fixed_size', 0):>6} "
              f"{mn.get('private_segment_fixed_size', 0):>7} "
              f"{mn.get('vgpr_spill_count', 0) + mn.get('sgpr_spill_count', 0):>5}  "
              f"{'same' if same_i else 'DIFF'} {'same' if same_m else 'DIFF'}")
        if not same_m:
            print(f"    old metadata: {mo}\n    new metadata: {mn}")
        if not same_i:
            for line in list(difflib.unified_diff(io, inw, "old", "new", lineterm="", n=1))[:a.show]:
                print(f"    {line}")
    print(f"\ninstruction streams differing: {ndiff} of {len(both)}; metadata differing: {nmeta} of {len(both)}")
    ok = not (only_old or only_new or dup_old or dup_new or ndiff or nmeta)
    print("EQUAL" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
