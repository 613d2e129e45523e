#!/usr/bin/env python3
"""Timing of the energy-form kernel (include/feanet_energy.h) and of the two routes of effective_conductivity on the
MI355X.  Not a test; writes a text report.  In one process:

  (a) fea_energy alone at 4097^2 nodes, fp64 and fp32, with and without the densities, with and without the image, as
      time and TB/s on the algorithmic bytes (two fields read: 2 * sizeof(T) per node, + 1 with the image, + 3 *
      sizeof(T) with the densities), next to fea_flux with fields and fea_pcg_dot in the same run as yardsticks, and
      whether each fea_energy row lies inside the band of TB/s the yardsticks reach;
  (b) effective_conductivity's two load cases on 2048^2 elements, six discs, prop = (1, 20), fp64 PCG on one built
      solver: iterations and solve time at rtol = 1e-10 with K_eff by both routes, then the energy route down a ladder
      of looser rtol, and the loosest rung whose K_E agrees with the 1e-10 run to 1e-9 relative.

Usage: python tools/energy_timing.py [--out profiles/energy/energy_timing.txt] [--n 4096] [--hn 2048]
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
LADDER = (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3)
AGREE = 1e-9


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def kernel_rows(n):
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    N = n + 1
    nodes = N * N
    img = torch.from_numpy(six_discs(n)).cuda()
    say(f"(a) {N}^2 nodes, one pair, six-disc image ({float(img.float().mean()):.3f} phase 1); bytes are algorithmic")
    lib = _lib.lib()
    for T, suf, esz in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        s = MultigridSolver(n, problem="interface", dtype=T, phase=img, graph=False)
        L0 = s.levels[0]
        L0.a.copy_(torch.randn(L0.a.numel(), dtype=T, device="cuda"))
        L0.f.copy_(torch.randn(L0.a.numel(), dtype=T, device="cuda"))
        per = int(lib.fea_energy_parts(N, N, esz))
        part = torch.empty(6 * per, dtype=torch.float64, device="cuda")
        sums = torch.empty(6, dtype=torch.float64, device="cuda")
        vec = 16 // esz
        ldd = -(-n // vec) * vec
        dens = torch.empty((1, 3, n, ldd), dtype=T, device="cuda")
        efn, ffn = getattr(lib, f"fea_energy_{suf}"), getattr(lib, f"fea_flux_{suf}")
        dot = getattr(lib, f"fea_pcg_dot_{suf}")
        kparts = torch.empty(int(lib.fea_pcg_parts(N, N, esz)), dtype=torch.float64, device="cuda")

        def energy(dp, ph):
            rc = efn(L0.a.data_ptr(), L0.f.data_ptr(), ph, n, dp, ldd, n * ldd, 3 * n * ldd, part.data_ptr(), 1, N, N,
                     L0.ld, L0.bs, L0.bs, None)
            assert rc == 0

        def flux():
            rc = ffn(L0.a.data_ptr(), img.data_ptr(), n, 1.0, 20.0, 2.0 / n, dens.data_ptr(), ldd, n * ldd, 2 * n * ldd,
                     part.data_ptr(), 1, N, N, L0.ld, L0.bs, None)
            assert rc == 0
        yard = [("fea_flux with fields, image", flux, esz + 1 + 2 * esz),
                ("fea_pcg_dot", lambda: dot(L0.a.data_ptr(), L0.f.data_ptr(), kparts.data_ptr(), 1, N, N, L0.ld, L0.bs,
                                            None), 2 * esz)]
        rows = [("energy sums only, image", lambda: energy(None, img.data_ptr()), 2 * esz + 1),
                ("energy sums only, no image", lambda: energy(None, None), 2 * esz),
                ("energy with densities, image", lambda: energy(dens.data_ptr(), img.data_ptr()), 5 * esz + 1),
                ("energy with densities, no image", lambda: energy(dens.data_ptr(), None), 5 * esz)]
        band = []
        for name, call, bpn in yard:
            med, lo, hi = per_launch(call)
            band.append(bpn * nodes / med / 1e12)
            say(f"    {suf} {name:32s} {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  {bpn:2d} B/node  "
                f"{band[-1]:.2f} TB/s   (yardstick)")
        for name, call, bpn in rows:
            med, lo, hi = per_launch(call)
            rate = bpn * nodes / med / 1e12
            where = "inside" if min(band) <= rate <= max(band) else ("above" if rate > max(band) else "BELOW")
            say(f"    {suf} {name:32s} {med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  {bpn:2d} B/node  "
                f"{rate:.2f} TB/s   {where} the yardsticks' band {min(band):.2f} .. {max(band):.2f}")
        t_final = per_launch(lambda: lib.fea_energy_final(part.data_ptr(), per, sums.data_ptr(), 1, None))[0]
        say(f"    {suf} fea_energy_final ({per} partials per quantity) {t_final * 1e6:.1f} us")
        del s, L0, dens, part
        torch.cuda.empty_cache()


def routes(hn):
    from feanet_amd.flux import coefficients
    from feanet_amd.homogenize import load_cases
    from feanet_amd.pcg import PCGSolver
    prop = (1, 20)
    say(f"(b) two load cases, {hn}^2 elements, six discs, prop {prop}, fp64 PCG on one built solver")
    s = PCGSolver(hn, problem="interface", batch=2, prop=prop, phase=six_discs(hn), coarsen="stiff")
    u0 = load_cases(hn, hn, 2.0, torch.float64, s.device)
    bc = u0.clone()
    bc[..., 1:-1, 1:-1] = 0
    zero = torch.zeros_like(u0)
    vol = hn * hn * (2.0 / hn) ** 2
    k0, k1 = coefficients(prop)

    def run(rtol):
        solve = lambda: s.solve(u0=u0, f=zero, rtol=rtol, max_iters=200, bc_value=bc)
        solve()
        t = float(np.median([synced(solve)[0] for _ in range(5)]))
        A = s.energy_forms(fields=False).A[0].cpu().numpy()
        K_E = (k0 * A[0] + k1 * A[1])[np.array([[0, 1], [1, 2]])] / vol
        K_flux = -s.flux(fields=False).mean_flux.cpu().numpy().T
        return t, s.iterations.tolist(), s.flags.tolist(), K_E, K_flux
    t, its, flags, K_ref, K_flux = run(1e-10)
    tE = [synced(lambda: s.energy_forms(fields=False))[0] for _ in range(9)]
    tF = [synced(lambda: s.flux(fields=False))[0] for _ in range(9)]
    scale = np.abs(K_ref).max()
    say(f"    rtol 1e-10: iterations {its}, flags {flags}, solve {t * 1e3:.2f} ms; energy_forms(fields=False) "
        f"{np.median(tE) * 1e3:.3f} ms, flux(fields=False) {np.median(tF) * 1e3:.3f} ms")
    say(f"        K_E    = {np.array2string(K_ref, precision=10).replace(chr(10), '')}")
    say(f"        K_flux = {np.array2string(K_flux, precision=10).replace(chr(10), '')}")
    say(f"        route gap max|K_E - sym(K_flux)| / max|K_E| = "
        f"{np.abs(K_ref - 0.5 * (K_flux + K_flux.T)).max() / scale:.2e}, flux-route asymmetry "
        f"{abs(K_flux[0, 1] - K_flux[1, 0]) / scale:.2e}")
    loosest = None
    for rtol in LADDER:
        t_r, its_r, flags_r, K_E, K_f = run(rtol)
        eE, eF = np.abs(K_E - K_ref).max() / scale, np.abs(K_f - K_flux).max() / scale
        ok = eE <= AGREE and flags_r == [1, 1]
        say(f"    rtol {rtol:.0e}: iterations {its_r}, solve {t_r * 1e3:.2f} ms ({t_r / t:.2f} of the 1e-10 solve); "
            f"K_E off by {eE:.2e}, flux route off by {eF:.2e}, min diag(K_E - K_E(1e-10)) "
            f"{np.diag(K_E - K_ref).min():+.2e}{'' if ok else '   (K_E beyond ' + format(AGREE, '.0e') + ')'}")
        if ok and (loosest is None or loosest[0] * 10.5 > rtol):
            loosest = (rtol, its_r, t_r)
    if loosest is None:
        say(f"    no rung of the ladder keeps K_E within {AGREE:.0e} of the 1e-10 run")
    else:
        say(f"    loosest rtol with K_E within {AGREE:.0e} relative of the 1e-10 run: {loosest[0]:.0e} "
            f"(iterations {loosest[1]}, solve {loosest[2] * 1e3:.2f} ms = {loosest[2] / t:.2f} of the 1e-10 solve)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hn", type=int, default=2048)
    args = ap.parse_args()
    kernel_rows(args.n)
    routes(args.hn)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
