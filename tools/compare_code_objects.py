#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libfeanet_hip.so:
    compare_code_objects.py [--allow renamed,rescheduled] OLD.so NEW.so

For a change that is meant to touch only host code (or to remove a compile-time switch's untaken branch) the
device code of every kernel must come out unchanged.  The two libraries pass when
  - their sets of device function symbols are equal (a name that several translation units define, such as the
    internal-linkage k_norm_final, counts once per definition),
  - every function's disassembly is equal (addresses and the trailing `//` encoding comments stripped), and
  - every kernel's metadata note is equal: VGPR / SGPR / AGPR counts, spill counts, LDS, scratch, kernarg size,
    wavefront size and max flat workgroup size.
Whole-file equality is not asked for: a code object embeds its source file's name.

A change that moves device source text (a helper extracted from several kernels) does not always reproduce the
register allocation and the schedule, so every function gets one of four classes:
  identical    disassembly equal line for line
  renamed      equal line for line once every vector, scalar and accumulator register operand (v12, s[4:5],
               a3) is replaced by its class letter (a single register and a range fold to the same letter: the
               mnemonic carries the operand width, so a width change still shows)
  rescheduled  equal instruction count and equal multiset of lines after that replacement
  changed      anything else
Symbol sets and metadata must be equal whatever the class.  Exit status 0 when every function is identical;
with --allow, also when every non-identical function is of an allowed class (their names are printed class by
class).  1 with the offending names otherwise.  CPU only; needs llvm-objdump and llvm-readobj of the ROCm
install (LLVM_BIN overrides their directory)."""
import argparse
import collections
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


CLASSES = ("identical", "renamed", "rescheduled", "changed")
_REG = re.compile(r"\b([vsa])(?:\d+|\[\d+:\d+\])(?![\w\[])")


def classify(old, new):
    """class of one function from its two disassembly texts"""
    if old == new:
        return "identical"
    a, b = (_REG.sub(r"\1", t).split("\n") for t in (old, new))
    if a == b:
        return "renamed"
    if len(a) == len(b) and collections.Counter(a) == collections.Counter(b):
        return "rescheduled"
    return "changed"


def parse_functions(text):
    """[(symbol, disassembly text)] from llvm-objdump -d --no-show-raw-insn --no-leading-addr output"""
    out, name = [], None
    for line in text.splitlines():
        m = re.match(r"(?:[0-9a-fA-F]+ )?<(\S+)>:$", line)
        if m:
            name = m.group(1)
            out.append((name, []))
        elif name and line.strip() and line.strip() != "...":  # ("...": zero padding up to the next function)
            out[-1][1].append(line.split("//")[0].strip())
    return [(n, "\n".join(t)) for n, t in out]


def functions(co):
    return parse_functions(run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co))


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


def compare(old, new, allow=()):
    """(report lines, exit status) for two (functions, kernel notes, code object count) triples as load() returns"""
    (fo, mo, no), (fn, mn, nn) = old, new
    bad = []
    for what, a, b in (("function", fo, fn), ("kernel note", mo, mn)):
        for n in sorted(set(a) | set(b)):
            ca, cb = len(a.get(n, ())), len(b.get(n, ()))
            if ca != cb:
                bad.append(f"{what} {n}: {ca} definition(s) in OLD, {cb} in NEW")
    # a name with several definitions takes the worst class of its (sorted) pairs
    names = {c: [] for c in CLASSES}
    for n in sorted(set(fo) & set(fn)):
        if len(fo[n]) == len(fn[n]):
            names[max((classify(a, b) for a, b in zip(fo[n], fn[n])), key=CLASSES.index)].append(n)
    for n in sorted(set(mo) & set(mn)):
        if len(mo[n]) == len(mn[n]) and mo[n] != mn[n]:
            diff = sorted({k for x, y in zip(mo[n], mn[n]) for (k, v), (_, w) in zip(x, y) if v != w})
            bad.append(f"metadata differs: {n}: {', '.join(diff)}")
    if not fo or not mo or no != nn:
        bad.append(f"code objects: {no} in OLD with {len(fo)} functions, {nn} in NEW with {len(fn)}")
    for c in CLASSES[1:]:
        if c not in allow:
            bad += [f"disassembly differs ({c}): {n}" for n in names[c]]
    out = list(bad)
    for c in CLASSES[1:]:
        if c in allow and names[c]:
            out.append(f"{c}: {len(names[c])}")
            out += [f"  {n}" for n in names[c]]
    nf, nk = sum(map(len, fn.values())), sum(map(len, mn.values()))
    same = not bad and not any(names[c] for c in CLASSES[1:])
    counts = ", ".join(f"{len(names[c])} {c}" for c in CLASSES)
    out.append(f"{'IDENTICAL' if same else 'DIFFERENT' if bad else 'ALLOWED'}: {nn} {ARCH} code objects, {nf} functions"
               f" ({counts}), {nk} kernels (disassembly and metadata)"
               f"{': ' + str(len(bad)) + ' difference(s)' if bad else ''}")
    return out, 1 if bad else 0


def allowed(value):
    """--allow's value: a comma-separated subset of renamed, rescheduled"""
    allow = tuple(c for c in value.split(",") if c)
    if not allow or any(c not in CLASSES[1:3] for c in allow):
        raise argparse.ArgumentTypeError("takes renamed, rescheduled or both")
    return allow


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--allow", type=allowed, default=(), metavar="renamed,rescheduled")
    ap.add_argument("old")
    ap.add_argument("new")
    a = ap.parse_args(argv[1:])  # (a usage error exits with status 2)
    out, status = compare(load(a.old), load(a.new), a.allow)
    for line in out:
        print(line)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
