#!/usr/bin/env python3
"""Timing of the two-material set-up from an element phase image (include/feanet_phase.h, MultigridSolver(phase=...))
on the MI355X.  Not a test; writes a text report.  At 2048^2 elements (2049^2 nodes, 11 levels), in one process:

  (a) the hierarchy's set-up — every level's image (fea_phase_coarsen) and pattern map (fea_phase_pattern_map) —
      from a device-resident image, next to the numpy path of feanet_amd.mesh_setup on the host and the
      host-to-device copy of the image alone; the two give the same bytes (asserted);
  (b) the constructors MultigridSolver(phase=image) and MultigridSolver(shape=0), each built twice, in alternating
      order (the first constructor of a process also loads the library's code objects);
  (c) the joined fp64 V-cycle on a six-disc image next to the reference's centred disc (shape=0, BASELINE C3's
      geometry), alternating the two solvers; the kernels are the same, only the pattern maps differ.

Usage: python tools/phase_timing.py [--out profiles/phase/phase_timing.txt] [--n 2048]
Times are a host clock around work that ends in a device synchronise.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--cycles", type=int, default=512)
    args = ap.parse_args()
    from feanet_amd import mesh_setup as ms
    from feanet_amd.solver import MultigridSolver
    n = args.n
    L = int(np.log2(n))
    img = six_discs(n)
    say(f"{n}^2 elements, {L} levels, six discs: {img.mean():.3f} of the elements phase 1")

    # (a)
    dev = torch.from_numpy(img).cuda()

    def device_setup():
        return [ms.phase_pattern_map_device(p) for p in ms.phase_hierarchy_device(dev, L, (1, 20), "majority")]

    def host_setup():
        return [ms.phase_pattern_map(p) for p in ms.phase_hierarchy(img, L, (1, 20), "majority")]
    for _ in range(3):
        device_setup()
    td = [synced(device_setup)[0] for _ in range(20)]
    th = []
    for _ in range(5):
        t = time.perf_counter()
        host_setup()
        th.append(time.perf_counter() - t)
    tup = [synced(lambda: torch.from_numpy(img).cuda())[0] for _ in range(5)]
    for a, b in zip(device_setup(), host_setup()):
        assert np.array_equal(a.cpu().numpy(), b)
    say(f"(a) images + pattern maps of all levels: device {np.median(td) * 1e3:.3f} ms (min {min(td) * 1e3:.3f}, max "
        f"{max(td) * 1e3:.3f}; {2 * L - 1} launches), numpy {np.median(th) * 1e3:.1f} ms (min {min(th) * 1e3:.1f}); "
        f"host-to-device copy of the image {np.median(tup) * 1e3:.3f} ms")

    # (b)
    solvers = {}
    for rep in range(2):
        for name in (("phase", "shape0") if rep == 0 else ("shape0", "phase")):
            kw = dict(phase=dev) if name == "phase" else dict(shape=0)
            t, s = synced(lambda: MultigridSolver(n, problem="interface", **kw))
            solvers[name] = s
            say(f"(b) constructor {name:7s} (round {rep + 1}): {t * 1e3:.1f} ms")
    for name, s in solvers.items():
        say(f"    {name}: {int((s.fine_pid != 0).sum())} finest nodes with a pattern other than 0; launches "
            f"{[r[0] for r in s._plan('a')[0]]}")

    # (c)
    K = args.cycles
    f = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 1, n + 1, n + 1))).cuda()
    res = {name: [] for name in solvers}
    for s in solvers.values():
        s.set_rhs(f=f)
        for _ in range(2):
            s.load()
            s.vcycle(K)
    for _ in range(7):
        for name, s in solvers.items():
            s.load()
            res[name].append(synced(lambda: s.vcycle(K))[0] / K * 1e6)
    for name, v in res.items():
        say(f"(c) joined V-cycle {n + 1}^2 fp64 {name:7s}: median {np.median(v):.2f} us of {K}-cycle calls "
            f"{[round(x, 2) for x in v]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
