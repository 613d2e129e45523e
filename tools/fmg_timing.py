#!/usr/bin/env python3
"""Timing of the full-multigrid start (MultigridSolver.fmg, include/feanet_fmg.h) on the MI355X.  Not a test; writes
a text report.  At 4097^2 fp64 Poisson and 2049^2 fp64 two-material, in one process:

  (a) each new kernel alone on the finest level — fea_fmg_prolong (cubic and bilinear, u = NULL), fea_fmg_restrict,
      fea_fmg_boundary — next to fea_mg_prolong_add on the same buffers (the yardstick with the same stores);
  (b) fmg(1) and fmg(2) under graph replay next to the joined V-cycle, and the phases of fmg(1) launched eagerly
      one by one: the restriction chain, the base cycles, every level's launches — those below the coarse tail and
      the base cycles summed on a line of their own;
  (c) the number of plain V-cycles from a zero guess whose error against a converged iterate matches fmg(1)'s, and
      their time.

Usage: python tools/fmg_timing.py [--out profiles/fmg/fmg_timing.txt] [--cases poisson:4096,interface:2048]
Times are device events around repeated launches or graph replays.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multigrid-feanet_amd"))

import torch  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def event_time(fn, reps, warm=3):
    """Mean seconds per call of fn over `reps` back-to-back calls (device events)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def problem_fields(n, problem):
    """(F, bc): the smooth model problem of DESIGN §14 for Poisson (source and exact Dirichlet data on [-1, 1]^2),
    F = ones with zero Dirichlet data for the two-material problem."""
    N = n + 1
    T = torch.float64
    if problem == "interface":
        return torch.ones((1, 1, N, N), dtype=T, device="cuda"), None
    x = torch.linspace(-1.0, 1.0, N, dtype=T, device="cuda")
    y, x = torch.meshgrid(x, x, indexing="ij")
    s = torch.sin(math.pi * x) * torch.sin(math.pi * y)
    u = s + x * y + 1 + (x * x - y * y) / 2
    bc = torch.zeros_like(u)
    bc[0], bc[-1], bc[:, 0], bc[:, -1] = u[0], u[-1], u[:, 0], u[:, -1]
    return (2 * math.pi ** 2 * s).reshape(1, 1, N, N), bc.reshape(1, 1, N, N)


def part_a(s):
    from feanet_amd import _lib
    T = s.dtype
    L0, L1 = s.levels[0], s.levels[1]
    nodes = L0.H * L0.W
    geom = dict(**L0.geom_kw(), **s._coarse_pitch(0))
    recs = {
        "fea_fmg_prolong cubic, u NULL (10 B)": (10, _lib.launch("fmg_prolong", u=None, ec=L1.a.data_ptr(),
                                                                 out=L0.b.data_ptr(), order=3, **geom)),
        "fea_fmg_prolong bilinear, u NULL (10 B)": (10, _lib.launch("fmg_prolong", u=None, ec=L1.a.data_ptr(),
                                                                    out=L0.b.data_ptr(), order=1, **geom)),
        "fea_fmg_prolong cubic, out = u + I (18 B)": (18, _lib.launch("fmg_prolong", u=L0.a.data_ptr(),
                                                                      ec=L1.a.data_ptr(), out=L0.b.data_ptr(),
                                                                      order=3, **geom)),
        "fea_mg_prolong_add (18 B)": (18, _lib.launch("mg_prolong_add", u=L0.a.data_ptr(), ec=L1.a.data_ptr(),
                                                      out=L0.b.data_ptr(), pidc=s._pid(1), **s._prolongation(),
                                                      **geom)),
        "fea_fmg_restrict (10 B)": (10, _lib.launch("fmg_restrict", f=L0.f.data_ptr(), fc=L1.f.data_ptr(), **geom)),
        "fea_fmg_boundary": (0, s._fmg_boundary(0, "b", s._bc)),
    }
    say(f"(a) kernels alone on the finest level, {L0.H}^2 fp64 {s.problem}, 100 launches each (device events), two "
        "rounds; bytes per fine node in brackets")
    for rnd in range(2):
        for name, (bpn, rec) in recs.items():
            t = event_time(lambda: s._launch([rec]), 100)
            bw = f"{bpn * nodes / t / 1e12:6.2f} TB/s" if bpn else "      -"
            say(f"    round {rnd}  {name:44s} {t * 1e6:8.1f} us  {bw}")


def part_b(s):
    say(f"(b) {s.H}^2 fp64 {s.problem}: graph replays (mean of 20) and the phases of fmg(1) launched eagerly")
    s.load()
    s.vcycle(16)
    s.vcycle(16)
    tv = event_time(lambda: s.vcycle(16), 10) / 16
    say(f"    joined V-cycle                      {tv * 1e6:9.1f} us")
    for cyc in (1, 2):
        t = event_time(lambda: s.fmg(cyc), 20)
        say(f"    fmg({cyc}) under graph replay          {t * 1e6:9.1f} us   = {t / tv:.2f} joined V-cycles")
    prog, _ = s.fmg_program(1)
    t_from = s.tail_from if s.tail_from is not None else s.L
    below = 0.0
    for phase, l, recs in prog:
        t = event_time(lambda: s._launch(recs), 20)
        Lv = s.levels[l]
        say(f"    eager  {phase:8s} level {l:2d} ({Lv.H:5d} x {Lv.W:5d}) {len(recs):3d} launches {t * 1e6:9.1f} us")
        if phase == "base" or (phase == "level" and l >= t_from):
            below += t
    say(f"    eager  base cycles + the levels from the coarse tail down (level >= {t_from}), summed: "
        f"{below * 1e6:9.1f} us")
    n_launch = sum(len(r) for _, _, r in prog)
    say(f"    fmg(1) is {n_launch} launches in one graph; base_cycles = {s.fmg_base_cycles()}")


def part_c(s):
    say(f"(c) {s.H}^2 fp64 {s.problem}: plain V-cycles from the zero guess that match fmg(1)'s error against a "
        "converged iterate")
    s.load()
    r0 = float(s.residual_norm()[0])
    s.vcycle(60)
    ustar = s.solution()
    rstar = float(s.residual_norm()[0])
    s.fmg(1)
    e_fmg = float((s.solution() - ustar).norm())
    r_fmg = float(s.residual_norm()[0])
    say(f"    converged iterate: 60 cycles, ||r|| / ||r0|| = {rstar / r0:.2e}")
    say(f"    fmg(1): ||u - u*|| = {e_fmg:.4e}   ||r|| / ||r0|| = {r_fmg / r0:.3e}")
    s.load()
    k, e = 0, float((s.solution() - ustar).norm())
    say(f"    zero guess: ||u - u*|| = {e:.4e}")
    while e > e_fmg and k < 59:
        s.vcycle(1)
        k += 1
        e = float((s.solution() - ustar).norm())
    say(f"    {k} plain cycles reach ||u - u*|| = {e:.4e}" + ("" if e <= e_fmg else "  (NOT matched within 59)"))

    def run():
        s.load()
        s.vcycle(k)
    def load_only():
        s.load()
    t = event_time(run, 10) - event_time(load_only, 10)
    tf = event_time(lambda: s.fmg(1), 20)
    say(f"    their time (vcycle({k}) as graphs, the load() subtracted) {t * 1e6:9.1f} us   fmg(1) {tf * 1e6:9.1f} us"
        f"   ratio {t / tf:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmg", "fmg_timing.txt"))
    ap.add_argument("--cases", default="poisson:4096,interface:2048")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fmg_timing: needs the MI355X")
    from feanet_amd.solver import MultigridSolver
    say(f"fmg_timing on {torch.cuda.get_device_name(0)}")
    for case in a.cases.split(","):
        problem, n = case.split(":")
        n = int(n)
        s = MultigridSolver(n, problem=problem)
        F, bc = problem_fields(n, problem)
        s.set_rhs(F=F)
        if bc is not None:
            s.set_boundary(bc)
        s.load()
        s.vcycle(2)  # every buffer holds live data
        part_a(s)
        part_b(s)
        part_c(s)
        say()
        del s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
