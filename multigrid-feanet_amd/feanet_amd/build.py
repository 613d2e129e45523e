"""Build libfeanet_hip.so (gfx950) in-tree with hipcc.

The library is plain HIP C++ behind a C ABI (include/feanet_hip.h); it is loaded with ctypes
after `import torch`, so it binds to the HIP runtime torch already loaded (same soname).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(HERE, "libfeanet_hip.so")
SOURCES = ["generic_ops.hip", "framed_ops.hip", "coarse_tail.hip", "hnet_ops.hip", "mid_ops.hip", "setup_ops.hip",
           "dd_ops.hip", "hjac_tail.hip", "hmid_ops.hip", "pcg_ops.hip", "fmg_ops.hip", "phase_ops.hip",
           "flux_ops.hip", "energy_ops.hip", "periodic_ops.hip", "coef_ops.hip"]
ARCH = os.environ.get("FEANET_ARCH", "gfx950")


def sources():
    return [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(INCLUDE, h) for h in ("feanet_hip.h", "feanet_fmg.h", "feanet_phase.h", "feanet_flux.h",
                                                "feanet_energy.h", "feanet_periodic.h", "feanet_coef.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, out=None, defines=()):
    """out / defines: A/B variant libraries for tools/ (run a script against one with tools/lab/with_lib.py).
    Each source compiles to its own object in parallel (no device code crosses translation units),
    then one link step."""
    if out is None and not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    target = out or LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = target + ".objs"
    os.makedirs(objdir, exist_ok=True)
    # -ffp-contract=on: a*b+c is fused only within one source expression, so a value recomputed
    # at a different call site (task-edge rows, edge lanes) rounds identically -> results are
    # independent of rows-per-task and batch size (bitwise)
    flags = [f"--offload-arch={ARCH}", "-O3", "-ffp-contract=on", "-std=c++17", "-fPIC", "-Wno-pass-failed",
             *[f"-D{d}" for d in defines], f"-I{INCLUDE}", f"-I{CSRC}"]
    objs = []
    cmds = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        cmds.append([hipcc, *flags, "-c", src, "-o", obj])
    if verbose:
        print("[feanet_amd.build]", " ".join(cmds[0][:-4]), "-c <each of", len(cmds), "sources>", file=sys.stderr)
    jobs = max(1, min(len(cmds), int(os.environ.get("MAX_JOBS", os.cpu_count() or 4))))
    with ThreadPoolExecutor(jobs) as ex:
        for c, r in zip(cmds, ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds)):
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise subprocess.CalledProcessError(r.returncode, c)
    subprocess.run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-o", target + ".tmp"], check=True)
    os.replace(target + ".tmp", target)
    return target


if __name__ == "__main__":
    defs = [a[2:] for a in sys.argv[1:] if a.startswith("-D")]
    outs = [a[6:] for a in sys.argv[1:] if a.startswith("--out=")]
    print(build(force="--force" in sys.argv, out=outs[0] if outs else None, defines=defs))
