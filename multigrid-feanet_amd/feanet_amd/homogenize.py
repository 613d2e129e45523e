"""Effective conductivity of a two-material element phase image.

Two load cases on one image, as one batch of two samples: f = 0 and the linear field u = r h (sample 0) or u = c h
(sample 1) as Dirichlet data on the boundary, i.e. a unit mean gradient G_j = e_j.  With <q> the element mean of the
flux, K_eff[:, j] = -<q>_j.  The linear field is also the initial guess, so a homogeneous image starts with r0 = 0
and the conjugate gradient freezes it in its INIT step.

route="energy"  evaluates the same two solved fields through the energy form instead:
K_E[i, j] = a(u_i, u_j) / |V| with a(u, v) = sum_e k_e u_e^T Ke v_e.  It is symmetric by construction, its error is
quadratic in the error of the iterate (one-sided on the diagonal), and its derivative with respect to the coefficient
of a phase, or of one element, needs no further solve.

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


EnergyHomogenizationResult = namedtuple(
    "EnergyHomogenizationResult", "K_eff dK_dprop sensitivity K_eff_flux route_gap iterations flags converged")
EnergyHomogenizationResult.__doc__ = """K_eff: [2, 2] float64 host array, (k0 A_0 + k1 A_1) / |V| with k0, k1 the
float32-rounded prop and |V| = m n h^2; exactly symmetric.  dK_dprop: [2 phases, 2, 2], A_p / |V|, the derivative of
K_eff with respect to prop[p].  sensitivity: device tensor [3, m, n] in the solver's dtype, the derivative of
K_eff[0, 0], K_eff[0, 1], K_eff[1, 1] with respect to each element's own coefficient (the element density / |V|), or
None (fields=False).  K_eff_flux: the flux route's tensor from the same solve; route_gap: max|K_eff -
sym(K_eff_flux)| / max|K_eff|.  iterations, flags, converged: as in HomogenizationResult."""


def load_cases(m, n, size, dtype, device):
    """[2, 1, m+1, n+1]: u = r h and u = c h, h = size / n."""
    h = size / n
    r = torch.arange(m + 1, dtype=torch.float64, device=device) * h
    c = torch.arange(n + 1, dtype=torch.float64, device=device) * h
    u = torch.stack([r[:, None].expand(m + 1, n + 1), c[None, :].expand(m + 1, n + 1)])
    return u.reshape(2, 1, m + 1, n + 1).to(dtype).contiguous()


def effective_conductivity(phase, prop=(1, 20), size=2.0, dtype=torch.float64, method="pcg", rtol=1e-10,
                           max_iters=200, coarsen="stiff", device=None, route="flux", fields=True, bc="dirichlet",
                           **solver_kw):
    """K_eff of the [m, n] element phase image `phase` (host or device; 0 -> prop[0], 1 -> prop[1]) on the rectangle of
    width `size` (h = size / n).  method "pcg": PCGSolver (solver_kw e.g. precond_dtype=torch.float32); "mg":
    MultigridSolver's stationary cycles (all samples run until the slowest is done; a sample whose ||r0|| is at the
    rounding level of the residual counts as solved).  Every sample stops at ||r|| <= rtol ||r0||.  Raises
    RuntimeError if a sample broke down; samples that did not converge in max_iters are reported in flags / converged, not hidden.
    route "flux": K_eff[:, j] = -<q>_j, a HomogenizationResult.  route "energy": K_eff from the energy form of the same
    two fields with its derivatives, an EnergyHomogenizationResult (fields=False: without the element sensitivity).
    bc "dirichlet": the linear fields as Dirichlet data (KUBC, an upper bound).  bc "periodic" (DESIGN §18): the image
    is a periodic cell, u = X_j + chi_j with a periodic fluctuation chi_j solved by PeriodicPCGSolver (solver_kw: nu,
    coarse_sweeps, omega, graph, check_every) and evaluated on the unwrapped field; both routes, the same result
    tuples; method "mg" and precond_dtype are not offered there."""
    if bc not in ("dirichlet", "periodic"):
        raise ValueError(f"effective_conductivity: unknown bc {bc!r} ('dirichlet' or 'periodic')")
    if bc == "periodic":
        return _periodic(phase, prop, size, dtype, method, rtol, max_iters, coarsen, device, route, fields, solver_kw)
    from .pcg import PCGSolver
    from .solver import MultigridSolver
    if method not in ("pcg", "mg"):
        raise ValueError(f"effective_conductivity: unknown method {method!r} ('pcg' or 'mg')")
    if route not in ("flux", "energy"):
        raise ValueError(f"effective_conductivity: unknown route {route!r} ('flux' or 'energy')")
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
    return _evaluate(s, m, n, h, prop, route, fields, iters, flags)


def _periodic(phase, prop, size, dtype, method, rtol, max_iters, coarsen, device, route, fields, solver_kw):
    """effective_conductivity(bc="periodic")"""
    from .periodic import PeriodicPCGSolver
    if method != "pcg":
        raise ValueError(f"effective_conductivity: bc='periodic' has no method {method!r} (conjugate gradients only)")
    if "precond_dtype" in solver_kw:
        raise ValueError("effective_conductivity: bc='periodic' has no mixed precision (precond_dtype)")
    if route not in ("flux", "energy"):
        raise ValueError(f"effective_conductivity: unknown route {route!r} ('flux' or 'energy')")
    if len(phase.shape) != 2:
        raise ValueError(f"effective_conductivity: phase must be [rows, n], got shape {tuple(phase.shape)}")
    m, n = (int(v) for v in phase.shape)
    s = PeriodicPCGSolver(n, rows=m, phase=phase, prop=prop, size=size, dtype=dtype, batch=2, coarsen=coarsen,
                          device=device, **solver_kw)
    s.solve(rtol=rtol, max_iters=max_iters)
    if (s.flags == 2).any():
        raise RuntimeError(f"effective_conductivity: the solve broke down (flags {s.flags.tolist()}); contrast "
                           f"{prop}, bc 'periodic'")
    return _evaluate(s, m, n, size / n, prop, route, fields, s.iterations, s.flags)


def _evaluate(s, m, n, h, prop, route, fields, iters, flags):
    """Both result tuples from a solver that holds the two solved load cases (its flux / energy_forms methods)."""
    res = s.flux(fields=False)
    if route == "energy":
        from .flux import coefficients
        forms = s.energy_forms(pair=(0, 1), fields=fields)
        vol = m * n * h * h
        A = forms.A[0].cpu().numpy()
        dK = np.stack([np.array([[a[0], a[1]], [a[1], a[2]]]) for a in A]) / vol
        k0, k1 = coefficients(prop)
        K_E = k0 * dK[0] + k1 * dK[1]
        K_flux = -res.mean_flux.cpu().numpy().T.copy()
        gap = float(np.abs(K_E - 0.5 * (K_flux + K_flux.T)).max() / np.abs(K_E).max())
        sens = None if forms.density is None else forms.density[0] / vol
        return EnergyHomogenizationResult(K_E, dK, sens, K_flux, gap, iters, flags, bool((flags == 1).all()))
    mean_flux = res.mean_flux.cpu().numpy()
    mean_grad = res.mean_grad.cpu().numpy()
    energy = res.energy.cpu().numpy()
    G = np.eye(2)
    hill = np.abs(energy + m * n * h * h * (G * mean_flux).sum(1)) / energy
    return HomogenizationResult(-mean_flux.T.copy(), mean_flux, mean_grad, energy, hill, iters, flags,
                                bool((flags == 1).all()))


class _EffectiveConductivity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prop, phase, kw):
        res = effective_conductivity(phase, prop=tuple(float(p) for p in prop.detach().cpu()), route="energy",
                                     fields=False, **kw)
        if not res.converged:
            raise RuntimeError(f"effective_conductivity_torch: the solve did not converge (flags {res.flags.tolist()})")
        ctx.dK = torch.from_numpy(res.dK_dprop)
        return torch.from_numpy(res.K_eff).to(prop.device)

    @staticmethod
    def backward(ctx, grad):
        dK = ctx.dK.to(grad.device)
        return (dK * grad.to(dK.dtype)).sum((1, 2)), None, None


def effective_conductivity_torch(phase, prop_tensor, **kw):
    """The energy route's K_eff ([2, 2] float64, on prop_tensor's device) as a differentiable function of the two
    coefficients prop_tensor ([2], any float dtype, host or device): backward contracts the incoming gradient with
    dK_dprop, dK_eff / dprop[p] = A_p / |V| (no further solve), and returns it in float64 cast by autograd to
    prop_tensor's dtype.  The solver rounds prop to float32, so value and derivative are taken AT the float32-rounded
    prop: a change of prop below its float32 spacing changes neither.  kw: effective_conductivity's (size, dtype,
    method, rtol, ...).  The derivative is exact only for a converged solve (stationarity), so an unconverged one
    raises."""
    if prop_tensor.shape != (2,):
        raise ValueError("effective_conductivity_torch: prop_tensor must have shape [2], got "
                         f"{tuple(prop_tensor.shape)}")
    return _EffectiveConductivity.apply(prop_tensor, phase, kw)
