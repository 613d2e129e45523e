"""numpy side of the energy-form tests (test_energy_host.py, test_gpu_energy.py); a helper, not a test, in the role of
flux_ref.py, on which it builds.

The element expression d(u, v) of include/feanet_energy.h evaluated in a chosen dtype, its fp64 value with the absolute
companion of generic_ref.py, the six per-phase sums in the kernel's order, and the energy-route homogenisation on
flux_ref's dense solves: K_E, dK_dprop and the flux route's K_eff from the same fields, of the exact solution, of a
perturbed one, or of the iterates of phase_ref.numpy_pcg.

Grid axes: index 0 is the row direction (coordinate r h), index 1 the column direction (c h)."""
import functools

import numpy as np

import flux_ref as fx

NSUMS = 6
NAMES = ("uu", "uv", "vv")


def energy_parts(H, W, esz):
    """fea_flux's task rule: strips over node columns 1 .. W-1, row tasks of the height ONE sample gets"""
    return fx.flux_parts(H, W, esz)


# ----------------------------------------------------------------------------- the element expression
def diffs(u):
    a, b, c, d = fx.corners(u)
    return (b - a) + (d - c), (c - a) + (d - b), (a - b) - (c - d)


def d_of(x, y, quarter, sixth):
    return (x[0] * y[0] + x[1] * y[1]) * quarter + (x[2] * y[2]) * sixth


def element_values(u, v, dt, wide=False):
    """d(u,u), d(u,v), d(v,v) with every operation rounded to dt (no fused multiply-add).  wide: the same inputs and
    constants (u, v and 1/6 as dt values) widened, every operation in fp64 — the exact reference of the dt kernel.
    u, v [B, H, W].  -> dict of [B, He, We] arrays uu, uv, vv"""
    ct = np.float64 if wide else dt
    x, y = diffs(np.asarray(u, dt).astype(ct)), diffs(np.asarray(v, dt).astype(ct))
    quarter, sixth = ct(0.25), ct(dt(1.0 / 6.0))
    return dict(uu=d_of(x, x, quarter, sixth), uv=d_of(x, y, quarter, sixth), vv=d_of(y, y, quarter, sixth))


def companions(u, v, dt):
    """The absolute companions S (generic_ref.py: every factor by its absolute value, every subtraction an addition)
    of the three element values, in fp64: sc, sr and w each become s4 = |a| + |b| + |c| + |d|."""
    su = sum(fx.corners(np.abs(np.asarray(u, np.float64))))
    sv = sum(fx.corners(np.abs(np.asarray(v, np.float64))))
    c = 2 * 0.25 + float(dt(1.0 / 6.0))
    return dict(uu=c * su * su, uv=c * su * sv, vv=c * sv * sv)


def sums_of(vals, phase):
    """[B, 6] float64 sums in the kernel's order: uu over phase 0, uu over phase 1, uv, vv likewise"""
    B = vals["uu"].shape[0]
    p1 = np.zeros(vals["uu"].shape[-2:], bool) if phase is None else np.asarray(phase) != 0
    out = []
    for n in NAMES:
        x = np.asarray(vals[n], np.float64)
        out += [np.where(~p1, x, 0.0).reshape(B, -1).sum(1), np.where(p1, x, 0.0).reshape(B, -1).sum(1)]
    return np.stack(out, 1)


# ----------------------------------------------------------------------------- the energy route, dense
def forms_of_pair(u, phase):
    """A [2 phases, 2, 2] in fp64 of the two load-case fields u [2, H, W]: A_p[i, j] = sum over phase p of d(u_i, u_j)"""
    s = sums_of(element_values(u[0:1], u[1:2], np.float64), phase)[0]
    return np.array([[[s[p], s[2 + p]], [s[2 + p], s[4 + p]]] for p in (0, 1)])


def routes(u, phase, k0, k1, size=2.0):
    """Both routes on the same two fields u [2, H, W]: dict K_E, dK [2, 2, 2] (= A_p / |V|), K_flux, gap"""
    m, n = np.shape(phase)
    h = size / n
    vol = m * n * h * h
    dK = forms_of_pair(u, phase) / vol
    K_E = k0 * dK[0] + k1 * dK[1]
    s = fx.sums_of(fx.element_values(u, phase, k0, k1, h, np.float64))
    K_flux = -(s[:, 0:2] / (m * n)).T
    gap = np.abs(K_E - 0.5 * (K_flux + K_flux.T)).max() / np.abs(K_E).max()
    return dict(K_E=K_E, dK=dK, K_flux=K_flux, gap=gap)


def coefficients(prop, exact):
    return (float(prop[0]), float(prop[1])) if exact else (float(np.float32(prop[0])), float(np.float32(prop[1])))


def stiffness(phase, prop, exact):
    return fx.assemble_exact(phase, prop) if exact else fx.assemble_table(phase, prop)


def homogenize(phase, prop, size=2.0, exact=False):
    """The dense pipeline of flux_ref.homogenize with both routes: dict u, K_E, dK, K_flux, gap"""
    phase = np.asarray(phase, np.uint8)
    m, n = phase.shape
    u = fx.dirichlet_solve(stiffness(phase, prop, exact), fx.load_cases(m, n, size))
    return dict(u=u, **routes(u, phase, *coefficients(prop, exact), size))


@functools.lru_cache(maxsize=None)
def homogenize_image(name, m, n, prop, size=2.0, exact=False):
    """homogenize() on a study image of phase_ref.py by name (cached: the references are shared and never changed)"""
    import phase_ref as pr
    return homogenize(pr.image(name, m, n), prop, size, exact)


def central_difference(phase, prop, rel=1e-4, exact=True, step=None):
    """(K_eff(k1 + s) - K_eff(k1 - s)) / (step taken) of both routes, s = rel k1 (or the absolute `step`), by dense
    solves; with the float32 table the step taken is the difference of the float32-rounded coefficients"""
    s = step if step is not None else rel * prop[1]
    hi = homogenize(phase, (prop[0], prop[1] + s), exact=exact)
    lo = homogenize(phase, (prop[0], prop[1] - s), exact=exact)
    taken = coefficients((prop[0], prop[1] + s), exact)[1] - coefficients((prop[0], prop[1] - s), exact)[1]
    return (hi["K_E"] - lo["K_E"]) / taken, (hi["K_flux"] - lo["K_flux"]) / taken


def interior_perturbation(m, n, seed):
    """[2, m+1, n+1] standard normal on the interior nodes, zero on the boundary"""
    dv = np.zeros((2, m + 1, n + 1))
    dv[:, 1:-1, 1:-1] = np.random.default_rng(seed).standard_normal((2, m - 1, n - 1))
    return dv


def pcg_iterates(phase, prop, rtol, coarsen="stiff", size=2.0, mixed=False, max_iters=200):
    """The two load cases solved by phase_ref.numpy_pcg from the linear fields, stopped at ||r|| <= rtol ||r0|| per
    sample as the device solver does -> (u [2, H, W], iterations [2])"""
    import phase_ref as pr
    phase = np.asarray(phase, np.uint8)
    m, n = phase.shape
    L = pr.default_levels(m, n)
    mg = pr.oracle(phase, L, np.float64, prop, coarsen)
    mg32 = pr.oracle(phase, L, np.float32, prop, coarsen) if mixed else None
    x0 = fx.load_cases(m, n, size)
    xs, _, its = pr.numpy_pcg(mg, x0, np.zeros_like(x0), max_iters, np.float64, rtol=rtol, mg32=mg32)
    return (xs[-1] if xs else x0), its
