#!/usr/bin/env python3
"""Timing of the torus kernels (include/feanet_periodic.h) and of the periodic homogenization on the MI355X.  Not a
test; writes a text report.  In one process:

  (a) each fea_per_* kernel at 4096 x 4096 nodes, one sample, six-disc image, fp64 and fp32, as time and TB/s on the
      algorithmic bytes, next to fea_pcg_dot on a framed field of the same size in the same run as the yardstick;
  (b) one periodic PCG iteration (the V(1, 1) cycle, the projections, the Krylov updates) on 2048^2 elements, two load
      cases, as the time of a replayed block of check_every iterations divided by their number, next to one iteration
      of the Dirichlet PCGSolver measured the same way;
  (c) a full effective_conductivity(bc="periodic") on 2048^2 six discs (solver set-up, solve at rtol 1e-10, both
      routes' evaluation), next to bc="dirichlet" in the same run.

No ratio is fixed in advance: this first version launches every level's kernels one by one, and the record is what a
later fusion is judged against.

Usage: python tools/periodic_timing.py [--out profiles/periodic/periodic_timing.txt] [--n 4096] [--hn 2048]
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
    from feanet_amd.periodic import PeriodicPCGSolver
    from feanet_amd.solver import MultigridSolver
    lib = _lib.lib()
    img = torch.from_numpy(six_discs(n)).cuda()
    nodes = n * n
    say(f"(a) {n} x {n} torus nodes, one sample, six-disc image ({float(img.float().mean()):.3f} phase 1); bytes are "
        "algorithmic")
    for T, suf, esz in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        s = PeriodicPCGSolver(n, phase=img, dtype=T, batch=1, graph=False)
        L0, L1 = s.levels[0], s.levels[1]
        for buf in (L0.f, L0.a, L0.b, L1.a):
            buf.copy_(torch.randn(buf.shape, dtype=T, device="cuda"))
        g = (1, L0.m, L0.n, L0.ld, L0.bs)
        pid, ktab, omd, part = L0.pid.data_ptr(), s.ktab.data_ptr(), s.omd.data_ptr(), s.part.data_ptr()
        fn = lambda name: getattr(lib, f"fea_per_{name}_{suf}")
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
        rows = [
            ("sweep", lambda: ok(fn("sweep")(L0.a.data_ptr(), L0.f.data_ptr(), L0.b.data_ptr(), pid, L0.ldp, ktab, omd,
                                             *g, None)), 3 * esz + 1),
            ("sweep from zero", lambda: ok(fn("sweep")(None, L0.f.data_ptr(), L0.b.data_ptr(), pid, L0.ldp, ktab, omd,
                                                       *g, None)), 2 * esz + 1),
            ("residual_restrict", lambda: ok(fn("residual_restrict")(L0.a.data_ptr(), L0.f.data_ptr(), L1.f.data_ptr(),
                                                                     pid, L0.ldp, ktab, *g, L1.ld, L1.bs, None)),
             2 * esz + 1 + esz / 4),
            ("prolong_add", lambda: ok(fn("prolong_add")(L1.a.data_ptr(), L0.b.data_ptr(), *g, L1.ld, L1.bs, None)),
             2 * esz + esz / 4),
            ("apply with partials", lambda: ok(fn("apply")(L0.a.data_ptr(), L0.b.data_ptr(), part, pid, L0.ldp, ktab,
                                                           *g, None)), 2 * esz + 1),
            ("apply", lambda: ok(fn("apply")(L0.a.data_ptr(), L0.b.data_ptr(), None, pid, L0.ldp, ktab, *g, None)),
             2 * esz + 1),
            ("reduce a . b", lambda: ok(fn("reduce")(L0.a.data_ptr(), L0.f.data_ptr(), part, *g, None)), 2 * esz),
            ("reduce sum a", lambda: ok(fn("reduce")(L0.a.data_ptr(), None, part, *g, None)), esz)]
        for name, call, bpn in rows:
            med, lo, hi = per_launch(call)
            rate = bpn * nodes / med / 1e12
            say(f"    {suf} fea_per_{name:22s} {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  "
                f"{bpn:5.1f} B/node  {rate:.2f} TB/s   {rate / yard:.2f} of the yardstick")
        t_final = per_launch(lambda: lib.fea_per_final(part, s.per, s.sums.data_ptr(), 2, None))[0]
        say(f"    {suf} fea_per_final ({s.per} partials per quantity, 2 quantities) {t_final * 1e6:.1f} us")
        del s, mg, L0, L1, F0
        torch.cuda.empty_cache()


def iteration_and_homogenization(hn):
    from feanet_amd.homogenize import effective_conductivity, load_cases
    from feanet_amd.pcg import PCGSolver
    from feanet_amd.periodic import PeriodicPCGSolver
    prop = (1, 20)
    img = six_discs(hn)
    say(f"(b) one PCG iteration, {hn}^2 elements, six discs, prop {prop}, fp64, two load cases, replayed graph blocks")
    p = PeriodicPCGSolver(hn, phase=img, prop=prop, batch=2)
    p.solve(rtol=1e-10)
    nb = p.check_every
    block = lambda: p._graphs.run(("iterate", nb, p.hist.data_ptr()), lambda: [p._iteration() for _ in range(nb)])

    def timed_block(prepare, fn):
        ts = []
        for _ in range(9):
            prepare()
            ts.append(synced(fn)[0])
        return float(np.median(ts))
    t_p = timed_block(lambda: p.k.fill_(1), block) / nb
    launches = 2 * p.nu * (len(p.levels) - 1) + p.coarse_sweeps + 2 * (len(p.levels) - 1) + 2 * 4
    say(f"    periodic:  {t_p * 1e6:8.1f} us per iteration ({len(p.levels)} levels, {launches} fea_per_* launches and "
        f"the torch updates; solve took {p.iterations.tolist()} iterations)")
    d = PCGSolver(hn, problem="interface", batch=2, prop=prop, phase=img, coarsen="stiff")
    u0 = load_cases(hn, hn, 2.0, torch.float64, d.device)
    bc = u0.clone()
    bc[..., 1:-1, 1:-1] = 0
    zero = torch.zeros_like(u0)
    d.solve(u0=u0, f=zero, rtol=1e-10, max_iters=200, bc_value=bc)
    its_d = d.iterations.tolist()
    d.load(u0, rtol=0.0)
    d.iterate(nb)
    t_d = timed_block(lambda: d.load(u0, rtol=0.0), lambda: d.iterate(nb)) / nb
    say(f"    dirichlet: {t_d * 1e6:8.1f} us per iteration (PCGSolver, the joined cycle; solve took {its_d} "
        "iterations)")
    say(f"    periodic / dirichlet per iteration: {t_p / t_d:.2f}")
    del p, d
    torch.cuda.empty_cache()
    say(f"(c) effective_conductivity on {hn}^2 six discs, route energy without the sensitivity field, rtol 1e-10, "
        "set-up included")
    res = {}
    for bc_name in ("periodic", "dirichlet"):
        run = lambda: effective_conductivity(img, prop=prop, bc=bc_name, route="energy", fields=False, rtol=1e-10)
        run()
        ts = [synced(run) for _ in range(5)]
        t = float(np.median([x[0] for x in ts]))
        r = ts[-1][1]
        res[bc_name] = t
        say(f"    bc={bc_name:9s} {t * 1e3:8.2f} ms, iterations {r.iterations.tolist()}, flags {r.flags.tolist()}, "
            f"K_eff = {np.array2string(r.K_eff, precision=8).replace(chr(10), '')}, route gap {r.route_gap:.2e}")
    say(f"    periodic / dirichlet: {res['periodic'] / res['dirichlet']:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hn", type=int, default=2048)
    args = ap.parse_args()
    kernel_rows(args.n)
    iteration_and_homogenization(args.hn)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
