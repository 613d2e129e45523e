#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libfeanet_hip.so:  compare_code_objects.py OLD.so NEW.so

For a change that is meant to touch only host code (or to remove a compile-time switch's untaken branch) the
device code of every kernel must come out unchanged.  The two libraries pass when
  - their sets of device function symbols are equal (a name that several translation units define, such as the
    internal-linkage k_norm_final, counts once per definition),
  - every function's disassembly is equal (addresses and the trailing `//` encoding comments stripped), and
  - every kernel's metadata note is equal: VGPR / SGPR / AGPR counts, spill counts, LDS, scratch, kernarg size,
    wavefront size and max flat workgroup size.
Whole-file equality is not asked for: a code object embeds its source file's name.  Exit status 0 when all
three hold, 1 with the offending names otherwise.  CPU only; needs llvm-objdump and llvm-readobj of the ROCm
install (LLVM_BIN overrides their directory)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
ARCH = os.environ.get("FEANET_ARCH", "gfx950")
META = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size", "wavefront_size",
        "max_flat_workgroup_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=cwd).stdout


def functions(co):
    """[(symbol, disassembly text)] of one code object"""
    out, name = [], None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"(?:[0-9a-fA-F]+ )?<(\S+)>:$", line)
        if m:
            name = m.group(1)
            out.append((name, []))
        elif name and line.strip() and line.strip() != "...":  # ("...": zero padding up to the next function)
            out[-1][1].append(line.split("//")[0].strip())
    return [(n, "\n".join(t)) for n, t in out]


def kernels(co):
    """[(kernel name, {field: value})] from the AMDGPU metadata note of one code object"""
    out, indent, cur = [], None, None
    for line in run(f"{LLVM}/llvm-readobj", "--notes", co).splitlines():
        if line.startswith("amdhsa.kernels:"):
            indent = None
            cur = None
            continue
        m = re.match(r"( *)(- )?\.(\w+):\s*(\S*)", line)
        if not m:
            if line and not line.startswith(" "):
                cur = None
            continue
        col = len(m.group(1)) + (2 if m.group(2) else 0)
        if m.group(2) and (indent is None or col == indent):  # a new entry of the kernels list
            indent = col
            cur = {}
            out.append(cur)
        if cur is not None and col == indent:
            cur[m.group(3)] = m.group(4)
    return [(k["name"], {f: k.get(f) for f in META}) for k in out if "name" in k]


def load(so):
    """({symbol: sorted disassemblies}, {kernel: sorted metadata}) over every code object of the library"""
    funcs, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(so, os.path.join(tmp, "lib.so"))
        run(f"{LLVM}/llvm-objdump", "--offloading", "lib.so", cwd=tmp)
        cos = sorted(f for f in os.listdir(tmp) if f.startswith("lib.so.") and ARCH in f)
        for co in cos:
            for n, t in functions(os.path.join(tmp, co)):
                funcs.setdefault(n, []).append(t)
            for n, k in kernels(os.path.join(tmp, co)):
                meta.setdefault(n, []).append(sorted(k.items()))
    for d in (funcs, meta):
        for v in d.values():
            v.sort()
    return funcs, meta, len(cos)


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    (fo, mo, no), (fn, mn, nn) = load(argv[1]), load(argv[2])
    bad = []
    for what, a, b in (("function", fo, fn), ("kernel note", mo, mn)):
        for n in sorted(set(a) | set(b)):
            ca, cb = len(a.get(n, ())), len(b.get(n, ()))
            if ca != cb:
                bad.append(f"{what} {n}: {ca} definition(s) in OLD, {cb} in NEW")
    bad += [f"disassembly differs: {n}" for n in sorted(set(fo) & set(fn)) if len(fo[n]) == len(fn[n]) and fo[n] != fn[n]]
    for n in sorted(set(mo) & set(mn)):
        if len(mo[n]) == len(mn[n]) and mo[n] != mn[n]:
            diff = sorted({k for x, y in zip(mo[n], mn[n]) for (k, v), (_, w) in zip(x, y) if v != w})
            bad.append(f"metadata differs: {n}: {', '.join(diff)}")
    if not fo or not mo or no != nn:
        bad.append(f"code objects: {no} in OLD with {len(fo)} functions, {nn} in NEW with {len(fn)}")
    for b in bad:
        print(b)
    nf, nk = sum(map(len, fn.values())), sum(map(len, mn.values()))
    print(f"{'DIFFERENT' if bad else 'IDENTICAL'}: {nn} {ARCH} code objects, {nf} functions, {nk} kernels"
          f" (disassembly and metadata){': ' + str(len(bad)) + ' difference(s)' if bad else ''}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
