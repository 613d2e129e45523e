"""Effective conductivity of a two-material element phase image.

Two load cases on one image, as one batch of two samples: f = 0 and the linear field u = r h (sample 0) or u = c h
(sample 1) as Dirichlet data on the boundary, i.e. a unit mean gradient G_j = e_j.  With <q> the element mean of the
flux, K_eff[:, j] = -<q>_j.  The linear field is also the initial guess, so a homogeneous image starts with r0 = 0
and the conjugate gradient freezes it in its INIT step.

Grid axes: index 0 is the row direction, index 1 the column direction.
"""
from collections import namedtuple

import numpy as np
import torch

HomogenizationResult = namedtuple("HomogenizationResult",
                                  "K_eff mean_flux mean_grad energy hill_defect iterations flags converged")
HomogenizationResult.__doc__ = """K_eff: [2, 2] float64 host array.  mean_flux, mean_grad: [2 load cases, 2 components].
energy: [2], u^T K u of each load case.  hill_defect: [2], |energy_j + He We h^2 G_j . <q>_j| / energy_j (Hill's
identity).  iterations, flags: per load case (flags: 1 converged, 2 breakdown, 0 stopped at max_iters).  converged: all
flags are 1."""


def load_cases(m, n, size, dtype, device):
    """[2, 1, m+1, n+1]: u = r h and u = c h, h = size / n."""
    h = size / n
    r = torch.arange(m + 1, dtype=torch.float64, device=device) * h
    c = torch.arange(n + 1, dtype=torch.float64, device=device) * h
    u = torch.stack([r[:, None].expand(m + 1, n + 1), c[None, :].expand(m + 1, n + 1)])
    return u.reshape(2, 1, m + 1, n + 1).to(dtype).contiguous()


def effective_conductivity(phase, prop=(1, 20), size=2.0, dtype=torch.float64, method="pcg", rtol=1e-10,
                           max_iters=200, coarsen="stiff", device=None, **solver_kw):
    """K_eff of the [m, n] element phase image `phase` (host or device; 0 -> prop[0], 1 -> prop[1]) on the rectangle of
    width `size` (h = size / n).  method "pcg": PCGSolver (solver_kw e.g. precond_dtype=torch.float32); "mg":
    MultigridSolver's stationary cycles (all samples run until the slowest is done; a sample whose ||r0|| is at the
    rounding level of the residual counts as solved).  Every sample stops at ||r|| <= rtol ||r0||.  Raises
    RuntimeError if a sample broke down; samples that did not converge in max_iters are reported in flags / converged, not hidden."""
    from .pcg import PCGSolver
    from .solver import MultigridSolver
    if method not in ("pcg", "mg"):
        raise ValueError(f"effective_conductivity: unknown method {method!r} ('pcg' or 'mg')")
    if len(phase.shape) != 2:
        raise ValueError(f"effective_conductivity: phase must be [rows, n], got shape {tuple(phase.shape)}")
    m, n = (int(v) for v in phase.shape)
    h = size / n
    cls = PCGSolver if method == "pcg" else MultigridSolver
    s = cls(n, rows=m, problem="interface", dtype=dtype, device=device, batch=2, size=size, prop=prop, phase=phase,
            coarsen=coarsen, **solver_kw)
    u0 = load_cases(m, n, size, dtype, s.device)
    zero = torch.zeros_like(u0)
    bc = u0.clone()  # the Dirichlet data: load() forms u0 * geo + bc, so bc is zero on the interior nodes
    bc[..., 1:-1, 1:-1] = 0
    if method == "pcg":
        s.solve(u0=u0, f=zero, rtol=rtol, max_iters=max_iters, bc_value=bc)
        flags, iters = s.flags.copy(), s.iterations.copy()
    else:
        s.set_boundary(bc)
        s.set_rhs(f=zero)
        s.load(u0)
        r0 = s.residual_norm().cpu().numpy()
        # the stationary iteration stops on the TRUE residual, which cannot fall below its own rounding: an entry of
        # K u is a sum of 9 products w u, so its error is within 2 (9 + 2) u_T sum |w| |u| (the field bound), and
        # sum |w| <= 2 * 16 kmax / 6.  A sample that starts at that level (a homogeneous image) is already solved.
        u_t = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
        kmax = float(max(np.float32(prop[0]), np.float32(prop[1])))
        floor = 22 * u_t * (32.0 * kmax / 6.0) * float(u0.abs().max()) * np.sqrt((m - 1) * (n - 1))
        thresh = np.maximum(rtol * r0, floor)
        iters = np.zeros(2, np.int64)
        rn = r0
        if (r0 > thresh).any():
            _, hist = s.solve(u0=u0, eps=float(thresh.min()), max_cycles=max_iters)
            iters[:] = len(hist) - 1
            rn = np.asarray(hist[-1])
        flags = np.where(~np.isfinite(rn), 2, np.where(rn <= thresh, 1, 0)).astype(np.int64)
    if (flags == 2).any():
        raise RuntimeError(f"effective_conductivity: the solve broke down (flags {flags.tolist()}); contrast "
                           f"{prop}, method {method!r}")
    res = s.flux(fields=False)
    mean_flux = res.mean_flux.cpu().numpy()
    mean_grad = res.mean_grad.cpu().numpy()
    energy = res.energy.cpu().numpy()
    G = np.eye(2)
    hill = np.abs(energy + m * n * h * h * (G * mean_flux).sum(1)) / energy
    return HomogenizationResult(-mean_flux.T.copy(), mean_flux, mean_grad, energy, hill, iters, flags,
                                bool((flags == 1).all()))
