#!/usr/bin/env python3
"""Timing of the coefficient-field torus kernels (include/feanet_coef.h) next to their pattern counterparts
(include/feanet_periodic.h) on the MI355X.  Not a test; writes a text report.  In one process:

  (a) each fea_coef_* kernel at 4096 x 4096 nodes, one sample, fp64 and fp32, as time and TB/s on the algorithmic
      bytes, next to the fea_per_* kernel of the same role on the same buffers and to fea_pcg_dot on a framed field of
      the same size as the yardstick; the ratio coef / pattern next to the ratio of their algorithmic bytes;
  (b) a whole effective_conductivity_field on a 2048^2 six-disc image written as a field, next to
      effective_conductivity(bc="periodic") on that image (solver set-up, solve at rtol 1e-10, energy route).

No ratio is fixed in advance.  From the bytes alone a sweep should cost 32/25 (fp64) or 16/13 (fp32) of the pattern
sweep, an apply 24/17 or 12/9.

Usage: python tools/coef_timing.py [--out profiles/coef/coef_timing.txt] [--n 4096] [--hn 2048]
Times are a host clock around `reps` back-to-back launches that end in a device synchronise; median of 9 such runs.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multigrid-feanet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flux_timing import per_launch, six_discs, synced  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def ok(rc):
    if rc != 0:
        raise RuntimeError(f"a fea_* call returned {rc}")


def kernel_rows(n):
    from feanet_amd import _lib
    from feanet_amd.coef import CoefPeriodicPCGSolver
    from feanet_amd.periodic import PeriodicPCGSolver
    from feanet_amd.solver import MultigridSolver
    lib = _lib.lib()
    img = six_discs(n)
    field = np.where(img != 0, 20.0, 1.0)
    nodes = n * n
    say(f"(a) {n} x {n} torus nodes, one sample, six-disc image as a pattern map and as a field; bytes are algorithmic")
    for T, suf, esz in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        p = PeriodicPCGSolver(n, phase=torch.from_numpy(img).cuda(), dtype=T, batch=1, graph=False)
        c = CoefPeriodicPCGSolver(n, coef=field, dtype=T, batch=1, graph=False)
        L0, L1, C0 = p.levels[0], p.levels[1], c.levels[0]
        for buf in (L0.f, L0.a, L0.b, L1.a):
            buf.copy_(torch.randn(buf.shape, dtype=T, device="cuda"))
        g = (1, L0.m, L0.n, L0.ld, L0.bs)
        pid, ktab, omd, part = L0.pid.data_ptr(), p.ktab.data_ptr(), p.omd.data_ptr(), p.part.data_ptr()
        k, ldk = C0.k.data_ptr(), C0.ldk
        a, f, b, f1 = L0.a.data_ptr(), L0.f.data_ptr(), L0.b.data_ptr(), L1.f.data_ptr()
        per = lambda name: getattr(lib, f"fea_per_{name}_{suf}")
        coef = lambda name: getattr(lib, f"fea_coef_{name}_{suf}")
        mg = MultigridSolver(n, dtype=T, graph=False)
        F0 = mg.levels[0]
        N = n + 1
        kparts = torch.empty(int(lib.fea_pcg_parts(N, N, esz)), dtype=torch.float64, device="cuda")
        dot = getattr(lib, f"fea_pcg_dot_{suf}")
        med, lo, hi = per_launch(lambda: ok(dot(F0.a.data_ptr(), F0.f.data_ptr(), kparts.data_ptr(), 1, N, N, F0.ld,
                                                F0.bs, None)))
        yard = 2 * esz * N * N / med / 1e12
        say(f"    {suf} fea_pcg_dot ({N}^2 framed nodes)  {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f}) "
            f"{2 * esz:2d} B/node  {yard:.2f} TB/s   (yardstick)")
        om = 2.0 / 3.0
        rows = [
            ("sweep", lambda: ok(coef("sweep")(a, f, b, k, ldk, om, *g, None)), 4 * esz,
             lambda: ok(per("sweep")(a, f, b, pid, L0.ldp, ktab, omd, *g, None)), 3 * esz + 1),
            ("sweep from zero", lambda: ok(coef("sweep")(None, f, b, k, ldk, om, *g, None)), 3 * esz,
             lambda: ok(per("sweep")(None, f, b, pid, L0.ldp, ktab, omd, *g, None)), 2 * esz + 1),
            ("residual_restrict", lambda: ok(coef("residual_restrict")(a, f, f1, k, ldk, *g, L1.ld, L1.bs, None)),
             3 * esz + esz / 4,
             lambda: ok(per("residual_restrict")(a, f, f1, pid, L0.ldp, ktab, *g, L1.ld, L1.bs, None)),
             2 * esz + 1 + esz / 4),
            ("apply with partials", lambda: ok(coef("apply")(a, b, part, k, ldk, *g, None)), 3 * esz,
             lambda: ok(per("apply")(a, b, part, pid, L0.ldp, ktab, *g, None)), 2 * esz + 1),
            ("apply", lambda: ok(coef("apply")(a, b, None, k, ldk, *g, None)), 3 * esz,
             lambda: ok(per("apply")(a, b, None, pid, L0.ldp, ktab, *g, None)), 2 * esz + 1)]
        for name, ccall, cb, pcall, pb in rows:
            tp = per_launch(pcall)[0]
            med, lo, hi = per_launch(ccall)
            rate = cb * nodes / med / 1e12
            say(f"    {suf} fea_coef_{name:20s} {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  "
                f"{cb:5.1f} B/node  {rate:.2f} TB/s  {rate / yard:.2f} of the yardstick;  fea_per_ {tp * 1e6:8.1f} us "
                f"({pb:4.1f} B/node): coef / pattern {med / tp:.2f}, bytes {cb / pb:.2f}")
        C1 = c.levels[1]
        for rule, rname in enumerate(("arithmetic", "harmonic", "geometric")):
            med = per_launch(lambda: ok(coef("coarsen")(k, ldk, C1.k.data_ptr(), C1.ldk, n, n, rule, None)))[0]
            say(f"    {suf} fea_coef_coarsen {rname:10s} {med * 1e6:8.1f} us  "
                f"{1.25 * esz * nodes / med / 1e12:.2f} TB/s on {1.25 * esz:.1f} B/element")
        del p, c, mg, L0, L1, C0, C1, F0
        torch.cuda.empty_cache()


def homogenization(hn):
    from feanet_amd.coef import effective_conductivity_field
    from feanet_amd.homogenize import effective_conductivity
    prop = (1, 20)
    img = six_discs(hn)
    field = np.where(img != 0, float(prop[1]), float(prop[0]))
    say(f"(b) {hn}^2 six discs, prop {prop}, fp64, route energy without the sensitivity field, rtol 1e-10, set-up "
        "included")
    runs = {"effective_conductivity_field (geometric)": lambda: effective_conductivity_field(
                field, route="energy", fields=False, rtol=1e-10),
            "effective_conductivity_field (arithmetic)": lambda: effective_conductivity_field(
                field, route="energy", fields=False, rtol=1e-10, coarsen="arithmetic"),
            "effective_conductivity(bc='periodic')": lambda: effective_conductivity(
                img, prop=prop, bc="periodic", route="energy", fields=False, rtol=1e-10)}
    res = {}
    for name, run in runs.items():
        run()
        ts = [synced(run) for _ in range(5)]
        t = float(np.median([x[0] for x in ts]))
        r = ts[-1][1]
        res[name] = t
        say(f"    {name:42s} {t * 1e3:8.2f} ms, iterations {r.iterations.tolist()}, flags {r.flags.tolist()}, "
            f"K_eff = {np.array2string(r.K_eff, precision=8).replace(chr(10), '')}")
    names = list(runs)
    say(f"    field (geometric) / pattern: {res[names[0]] / res[names[2]]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hn", type=int, default=2048)
    args = ap.parse_args()
    kernel_rows(args.n)
    homogenization(args.hn)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
