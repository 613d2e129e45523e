#!/usr/bin/env python3
"""Timing of the multigrid-preconditioned CG (feanet_amd.pcg) on the MI355X.  Not a test; writes a text report.

  (a) each Krylov kernel alone at 4097^2 fp64: time and achieved TB/s on its algorithmic bytes, next to
      fea_mg_sweep timed in the same run on the same buffers;
  (b) one PCG iteration against one joined V-cycle, at 4097^2 Poisson and at 2049^2 two-material;
  (c) time to 1e-8 ||r0||: MultigridSolver.solve against PCGSolver.solve on the 2049^2 two-material problem with
      F = ones, at prop = (1, 20) and at prop = (1, 1000) (where the stationary iteration diverges).
  Each part also times the mixed solver (dtype=float64, precond_dtype=float32) in the same run: (a) the four f64f32
  kernels next to their fp64 siblings, (b) the mixed iteration next to the fp64 one, (c) a mixed column.

Usage: python tools/pcg_timing.py [--out profiles/pcg/pcg_timing.txt] [--parts abc] [--n-kernel 4096]
(the report with the mixed columns is kept as profiles/pcg/pcg_mixed_timing.txt)
Times are device events around repeated launches (kernels, iterations) or a host clock around a synchronised solve.
"""
import argparse
import os
import sys
import time

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


def part_a(n):
    from feanet_amd import _lib
    from feanet_amd.pcg import PCGSolver, STEP_RZ, BETA, ALPHA
    T = torch.float64
    s = PCGSolver(n, dtype=T, graph=False)
    mg, L0 = s.mg, s.mg.levels[0]
    N = n + 1
    g = torch.Generator(device="cuda").manual_seed(0)
    s.set_rhs(f=torch.randn((1, 1, N, N), dtype=T, device="cuda", generator=g))
    s.load(torch.randn((1, 1, N, N), dtype=T, device="cuda", generator=g))
    s.iterate(2)  # every buffer holds live data; z is known
    torch.cuda.synchronize()
    z = L0.buf(s._zname).data_ptr()
    geom, ka, part, sc = L0.geom(), s._kargs(), s.part.data_ptr(), s.sc.data_ptr()
    s.sc[:, BETA] = 0.3
    s.sc[:, ALPHA] = 1e-3
    stream = None
    nodes = N * N
    calls = {
        "fea_mg_sweep (24 B)": (24, lambda: _lib.call("mg_sweep", T, L0.a.data_ptr(), L0.f.data_ptr(), L0.b.data_ptr(),
                                                      ka[0], ka[1], mg.omd.data_ptr(), ka[2], *geom, stream)),
        "fea_pcg_residual (24 B)": (24, lambda: _lib.call("pcg_residual", T, s.x.data_ptr(), s.b.data_ptr(),
                                                          L0.b.data_ptr(), *ka, part, *geom, stream)),
        "fea_pcg_dot (16 B)": (16, lambda: _lib.call("pcg_dot", T, s.r.data_ptr(), z, part, *geom, stream)),
        "fea_pcg_direction (24 B)": (24, lambda: _lib.call("pcg_direction", T, z, s.p[0].data_ptr(),
                                                           s.p[1].data_ptr(), *ka, sc, part, *geom, stream)),
        "fea_pcg_update (40 B)": (40, lambda: _lib.call("pcg_update", T, s.p[1].data_ptr(), s.x.data_ptr(),
                                                        s.r.data_ptr(), *ka, sc, part, *geom, stream)),
        "fea_pcg_scalar_step": (0, lambda: _lib.call_raw("pcg_scalar_step", part, s.per, sc, s.hist.data_ptr(),
                                                         s.hist.shape[0], 1, STEP_RZ, stream)),
    }
    say(f"(a) Krylov kernels alone, {N}^2 fp64 Poisson, 200 launches each (device events), two rounds")
    for rnd in range(2):
        for name, (bpn, fn) in calls.items():
            t = event_time(fn, 200)
            bw = f"{bpn * nodes / t / 1e12:6.2f} TB/s" if bpn else "      -"
            say(f"    round {rnd}  {name:28s} {t * 1e6:8.1f} us  {bw}")
    del s
    torch.cuda.empty_cache()
    part_a_mixed(n)


def part_a_mixed(n):
    """The four f64f32 kernels alone on a mixed solver's own buffers, same size and launch count."""
    from feanet_amd import _lib
    from feanet_amd.pcg import PCGSolver, BETA, ALPHA
    T = torch.float64
    s = PCGSolver(n, dtype=T, precond_dtype=torch.float32, graph=False)
    N = n + 1
    g = torch.Generator(device="cuda").manual_seed(0)
    s.set_rhs(f=torch.randn((1, 1, N, N), dtype=T, device="cuda", generator=g))
    s.load(torch.randn((1, 1, N, N), dtype=T, device="cuda", generator=g))
    s.iterate(2)
    torch.cuda.synchronize()
    z = s.mg.levels[0].buf(s._zname).data_ptr()
    geom, ka, part, sc, sb = s.L0.geom() + s._g32(), s._kargs(), s.part.data_ptr(), s.sc.data_ptr(), s.sb.data_ptr()
    r32 = s._pf.data_ptr()
    s.sc[:, BETA] = 0.3
    s.sc[:, ALPHA] = 1e-3
    stream = None
    nodes = N * N
    calls = {
        "fea_pcg_narrow_f64f32 (12 B)": (12, lambda: _lib.call_raw("pcg_narrow_f64f32", s.r.data_ptr(), r32, sc, sb,
                                                                   *geom, stream)),
        "fea_pcg_dot_f64f32 (12 B)": (12, lambda: _lib.call_raw("pcg_dot_f64f32", s.r.data_ptr(), z, part, *geom,
                                                                stream)),
        "fea_pcg_direction_f64f32 (20 B)": (20, lambda: _lib.call_raw("pcg_direction_f64f32", z, s.p[0].data_ptr(),
                                                                      s.p[1].data_ptr(), *ka, sc, part, *geom, stream)),
        "fea_pcg_update_f64f32 (44 B)": (44, lambda: _lib.call_raw("pcg_update_f64f32", s.p[1].data_ptr(),
                                                                   s.x.data_ptr(), s.r.data_ptr(), r32, *ka, sc, sb,
                                                                   part, *geom, stream)),
    }
    say(f"(a, mixed) f64f32 kernels alone, {N}^2 Poisson, fp64 Krylov fields + fp32 preconditioner frame, 200 "
        "launches each, two rounds")
    for rnd in range(2):
        for name, (bpn, fn) in calls.items():
            t = event_time(fn, 200)
            say(f"    round {rnd}  {name:32s} {t * 1e6:8.1f} us  {bpn * nodes / t / 1e12:6.2f} TB/s")
    del s
    torch.cuda.empty_cache()


def iteration_time(s):
    """Mean / min / max seconds of one iteration over 10 graph-replayed windows of 16 (3 more to warm up)."""
    ts = []
    for i in range(13):
        s.load()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.iterate(16)
        b.record()
        torch.cuda.synchronize()
        if i >= 3:  # the first windows run eagerly and capture the graphs
            ts.append(a.elapsed_time(b) * 1e-3 / 16)
    return sum(ts) / len(ts), min(ts), max(ts)


def precond_time(s):
    """The preconditioner's launch plan alone (eager launches back to back, device events): its share of an iteration."""
    plan = s.mg._plan("a")[0]
    return event_time(lambda: s.mg._launch(plan), 50)


def part_b():
    from feanet_amd.pcg import PCGSolver, DONE
    from feanet_amd.solver import MultigridSolver
    say("(b) one PCG iteration against one joined V-cycle (fp64; graphs; mean over 10 windows of 16)")
    for n, problem in ((4096, "poisson"), (2048, "interface")):
        N = n + 1
        g = torch.Generator(device="cuda").manual_seed(1)
        f = torch.randn((1, 1, N, N), dtype=torch.float64, device="cuda", generator=g)
        mg = MultigridSolver(n, problem=problem)
        mg.set_rhs(f=f)
        mg.load()
        mg.vcycle(16)
        mg.vcycle(16)
        tv = event_time(lambda: mg.vcycle(16), 10) / 16
        del mg
        torch.cuda.empty_cache()
        s = PCGSolver(n, problem=problem)
        s.set_rhs(f=f)
        tp, lo, hi = iteration_time(s)
        frozen = int((s.sc[:, DONE] != 0).sum().item())
        nl = len(s.mg._plan("a")[0])
        tc = precond_time(s)
        say(f"    {N}^2 {problem:9s}: V-cycle {tv * 1e6:8.1f} us   PCG iteration {tp * 1e6:8.1f} us  "
            f"(min {lo * 1e6:.1f}, max {hi * 1e6:.1f}; ratio {tp / tv:.2f}; {nl} preconditioner + 6 Krylov "
            f"launches; frozen samples at the end: {frozen}); its zero-start fp64 cycle alone {tc * 1e6:.1f} us")
        del s
        torch.cuda.empty_cache()
        s = PCGSolver(n, problem=problem, precond_dtype=torch.float32)
        s.set_rhs(f=f)
        tm, lo, hi = iteration_time(s)
        frozen = int((s.sc[:, DONE] != 0).sum().item())
        nl = len(s.mg._plan("a")[0])
        tcm = precond_time(s)
        say(f"    {N}^2 {problem:9s}: mixed (fp32 preconditioner) iteration {tm * 1e6:8.1f} us  "
            f"(min {lo * 1e6:.1f}, max {hi * 1e6:.1f}; {tm / tp:.2f} of the fp64 iteration; {nl} preconditioner + 6 "
            f"Krylov launches; frozen samples at the end: {frozen}); its zero-start fp32 cycle alone {tcm * 1e6:.1f} us")
        del s
        torch.cuda.empty_cache()


def part_c():
    from feanet_amd.pcg import PCGSolver
    from feanet_amd.solver import MultigridSolver
    n, N = 2048, 2049
    say(f"(c) time to 1e-8 ||r0||, {N}^2 two-material fp64, F = ones (host clock around a synchronised solve; "
        "second of two runs)")
    F = torch.ones((1, 1, N, N), dtype=torch.float64, device="cuda")
    for prop in ((1, 20), (1, 1000)):
        mg = MultigridSolver(n, problem="interface", prop=prop)
        mg.set_rhs(F=F)
        mg.load()
        r0 = float(mg.residual_norm()[0])
        cap = 200 if prop == (1, 20) else 60
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, vh = mg.solve(F=F, eps=1e-8 * r0, max_cycles=cap)
            torch.cuda.synchronize()
            tv = time.perf_counter() - t0
        ok = bool(vh[-1][0] <= 1e-8 * r0)
        say(f"    prop={prop}: ||r0|| = {r0:.4e}")
        say(f"      MultigridSolver.solve: {'converged' if ok else 'FAILED'} after {len(vh) - 1} cycles, "
            f"||r|| / ||r0|| = {vh[-1][0] / r0:.3e}, {tv * 1e3:.2f} ms")
        del mg
        torch.cuda.empty_cache()
        for label, pd in (("PCGSolver.solve:      ", None), ("PCGSolver mixed f64f32:", torch.float32)):
            s = PCGSolver(n, problem="interface", prop=prop, precond_dtype=pd)
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, ph = s.solve(F=F, rtol=1e-8, max_iters=200)
                torch.cuda.synchronize()
                tp = time.perf_counter() - t0
            true = float(s.residual_norm()[0])
            say(f"      {label} flag {int(s.flags[0])} after {int(s.iterations[0])} iterations "
                f"(check_every {s.check_every}), ||r|| / ||r0|| = {ph[-1][0] / ph[0][0]:.3e} (true residual "
                f"{true / ph[0][0]:.3e}), {tp * 1e3:.2f} ms")
            del s
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg", "pcg_timing.txt"))
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--n-kernel", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pcg_timing: needs the MI355X")
    say(f"pcg_timing on {torch.cuda.get_device_name(0)}")
    if "a" in a.parts:
        part_a(a.n_kernel)
    if "b" in a.parts:
        part_b()
    if "c" in a.parts:
        part_c()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
