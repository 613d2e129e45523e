#!/usr/bin/env python3
"""Timing of the element flux kernel (include/feanet_flux.h) and of effective_conductivity on the MI355X.  Not a
test; writes a text report.  In one process:

  (a) fea_flux alone at 4097^2 nodes, fp64 and fp32, sums only and with the fields, as time and TB/s on the
      algorithmic bytes (fp64: 8 + 1 B per node for the sums, + 16 B with the fields; fp32: 4 + 1 and + 8), next to
      fea_pcg_dot (16 B per fp64 node) and fea_mg_sweep (24 B) in the same run as yardsticks;
  (b) effective_conductivity on 2048^2 elements, six discs, prop = (1, 20): total time, iterations, and the share
      spent in flux().

Usage: python tools/flux_timing.py [--out profiles/flux/flux_timing.txt] [--n 4096] [--hn 2048]
Times are a host clock around `reps` back-to-back launches that end in a device synchronise; median of 9 such runs.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multigrid-feanet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def six_discs(n, seed=0):
    """six discs at seeded random places, radii 0.05 n .. 0.14 n (the image of tests/phase_ref.py)"""
    y, x = np.mgrid[0:n, 0:n] + 0.5
    rng = np.random.default_rng([seed, n, n])
    img = np.zeros((n, n), bool)
    for _ in range(6):
        cx, cy = rng.uniform(0.15, 0.85) * n, rng.uniform(0.15, 0.85) * n
        r = rng.uniform(0.05, 0.14) * n
        img |= (x - cx) ** 2 + (y - cy) ** 2 < r * r
    return img.astype(np.uint8)


def synced(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def per_launch(fn, reps=20, runs=9):
    """median, min, max seconds per call of fn over `runs` timings of `reps` back-to-back calls"""
    for _ in range(3):
        fn()
    ts = [synced(lambda: [fn() for _ in range(reps)])[0] / reps for _ in range(runs)]
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hn", type=int, default=2048)
    args = ap.parse_args()
    from feanet_amd import _lib, flux as fxm
    from feanet_amd.homogenize import effective_conductivity, load_cases
    from feanet_amd.pcg import PCGSolver
    from feanet_amd.solver import MultigridSolver
    n = args.n
    N = n + 1
    nodes = N * N
    img = torch.from_numpy(six_discs(n)).cuda()
    say(f"(a) {N}^2 nodes, one sample, six-disc image ({float(img.float().mean()):.3f} phase 1); bytes are algorithmic")
    lib = _lib.lib()
    for T, suf, esz in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        s = MultigridSolver(n, problem="interface", dtype=T, phase=img, graph=False)
        L0 = s.levels[0]
        L0.a.copy_(torch.randn(L0.a.numel(), dtype=T, device="cuda"))
        L0.f.copy_(torch.randn(L0.a.numel(), dtype=T, device="cuda"))
        per = int(lib.fea_flux_parts(N, N, esz))
        part = torch.empty(5 * per, dtype=torch.float64, device="cuda")
        vec = 16 // esz
        ldq = -(-n // vec) * vec
        q = torch.empty((1, 2, n, ldq), dtype=T, device="cuda")
        fn = getattr(lib, f"fea_flux_{suf}")

        def flux(qp, ph):
            rc = fn(L0.a.data_ptr(), ph, n, 1.0, 20.0, 2.0 / n, qp, ldq, n * ldq, 2 * n * ldq, part.data_ptr(), 1, N, N,
                    L0.ld, L0.bs, None)
            assert rc == 0
        rows = [("flux sums only, image", lambda: flux(None, img.data_ptr()), esz + 1),
                ("flux sums only, no image", lambda: flux(None, None), esz),
                ("flux with fields, image", lambda: flux(q.data_ptr(), img.data_ptr()), esz + 1 + 2 * esz),
                ("flux with fields, no image", lambda: flux(q.data_ptr(), None), esz + 2 * esz)]
        kparts = torch.empty(int(lib.fea_pcg_parts(N, N, esz)), dtype=torch.float64, device="cuda")
        dot = getattr(lib, f"fea_pcg_dot_{suf}")
        sweep = getattr(lib, f"fea_mg_sweep_{suf}")
        rows.append(("fea_pcg_dot", lambda: dot(L0.a.data_ptr(), L0.f.data_ptr(), kparts.data_ptr(), 1, N, N, L0.ld,
                                               L0.bs, None), 2 * esz))
        rows.append(("fea_mg_sweep (two-material)",
                     lambda: sweep(L0.a.data_ptr(), L0.f.data_ptr(), L0.b.data_ptr(), L0.pid.data_ptr(),
                                   s.ktab.data_ptr(), s.omd.data_ptr(), s.ntab, 1, N, N, L0.ld, L0.bs, None),
                     3 * esz))
        for name, call, bpn in rows:
            med, lo, hi = per_launch(call)
            say(f"    {suf} {name:30s} {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  {bpn:2d} B/node  "
                f"{bpn * nodes / med / 1e12:.2f} TB/s")
        t_final = per_launch(lambda: lib.fea_flux_final(part.data_ptr(), per, kparts.data_ptr(), 1, None))[0]
        say(f"    {suf} fea_flux_final ({per} partials per quantity) {t_final * 1e6:.1f} us")
        del s, L0, q, part
        torch.cuda.empty_cache()

    hn = args.hn
    himg = six_discs(hn)
    say(f"(b) effective_conductivity, {hn}^2 elements, six discs, prop (1, 20), fp64 PCG, rtol 1e-10")
    for rep in range(2):
        t, res = synced(lambda: effective_conductivity(himg, prop=(1, 20), max_iters=200))
        say(f"    call {rep + 1}: {t * 1e3:.1f} ms in all (constructor, two load cases, flux), iterations "
            f"{res.iterations.tolist()}, flags {res.flags.tolist()}, Hill defect {res.hill_defect.max():.2e}")
        say(f"        K_eff = {np.array2string(res.K_eff, precision=8).replace(chr(10), '')}")
    s = PCGSolver(hn, problem="interface", batch=2, prop=(1, 20), phase=himg, coarsen="stiff")
    u0 = load_cases(hn, hn, 2.0, torch.float64, s.device)
    bc = u0.clone()
    bc[..., 1:-1, 1:-1] = 0
    t_solve, _ = synced(lambda: s.solve(u0=u0, f=torch.zeros_like(u0), rtol=1e-10, max_iters=200, bc_value=bc))
    t_solve, _ = synced(lambda: s.solve(u0=u0, f=torch.zeros_like(u0), rtol=1e-10, max_iters=200, bc_value=bc))
    tf = [synced(lambda: s.flux(fields=False))[0] for _ in range(9)]
    tq = [synced(lambda: s.flux(fields=True))[0] for _ in range(9)]
    say(f"    on a built solver: solve {t_solve * 1e3:.2f} ms ({s.iterations.tolist()} iterations), flux(fields=False) "
        f"{np.median(tf) * 1e3:.3f} ms = {np.median(tf) / (t_solve + np.median(tf)) * 100:.2f} % of solve + flux; "
        f"flux(fields=True) {np.median(tq) * 1e3:.3f} ms")
    assert fxm.NSUMS == 5
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
