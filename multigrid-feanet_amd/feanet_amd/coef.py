"""Periodic homogenization of an element coefficient field.

The [m, n] field k holds one positive coefficient per element of the periodic cell of feanet_amd.periodic: a grey-scale
image, a density field k = kmin + rho^p (kmax - kmin), a random medium, any number of phases.  CoefPeriodicPCGSolver is
PeriodicPCGSolver on the matrix-free torus kernels of include/feanet_coef.h (csrc/coef_ops.hip), which read k where the
two-material kernels read a pattern map and a stencil table; prolongation, the reductions, the projection, the
iteration and the unwrapping are inherited.  The operator's rows sum to zero exactly, the projection stays because the
right-hand side is mean-free only to rounding.  The coarse fields are 2 x 2 block means of the finer one.

The solved fields are evaluated by the existing flux and energy kernels with a unit coefficient; the sums weighted by
k come from fea_per_reduce on the element fields, which have the torus layout of k.
"""
import numpy as np
import torch

from . import _lib
from .flux import EnergyForms, FluxResult
from .homogenize import EnergyHomogenizationResult, HomogenizationResult
from .periodic import PeriodicPCGSolver

RULES = {"arithmetic": 0, "harmonic": 1, "geometric": 2}  # FEA_COEF_ARITHMETIC, _HARMONIC, _GEOMETRIC


def check_field(k):
    """The coefficient field as a float64 tensor (on the device it came from; a host array becomes a host tensor).
    ValueError unless it is [m, n] with m, n >= 2 and every value is finite and positive."""
    t = k.detach() if torch.is_tensor(k) else torch.as_tensor(np.asarray(k))
    if t.dim() != 2:
        raise ValueError(f"feanet_amd.coef: the coefficient field must be [rows, n], got shape {tuple(t.shape)}")
    if min(t.shape) < 2:
        raise ValueError(f"feanet_amd.coef: the cell needs at least 2 x 2 elements, got {tuple(t.shape)}")
    if not (t.dtype.is_floating_point or t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
        raise ValueError(f"feanet_amd.coef: the coefficient field must be real numbers, got {t.dtype}")
    t = t.to(torch.float64)
    if not bool(torch.isfinite(t).all()):
        raise ValueError("feanet_amd.coef: the coefficient field has a value that is not finite")
    if not bool((t > 0).all()):
        raise ValueError("feanet_amd.coef: every coefficient must be positive")
    return t


class CoefPeriodicPCGSolver(PeriodicPCGSolver):
    """PeriodicPCGSolver for an [rows, n] element coefficient field `coef` (host or device, any real dtype; rounded to
    the solver's dtype): conjugate gradients on the projected operator, preconditioned by one V(nu, nu) cycle from a
    zero guess (weighted Jacobi omega / d with the node's own diagonal; full weighting and its transpose; coarse_sweeps
    sweeps from zero on the coarsest level).  The coarse field of a level is the mean of each 2 x 2 block of the finer
    one under `coarsen`: "arithmetic", "harmonic" or "geometric" (DESIGN §19 has the iteration counts; no rule wins
    everywhere).  solve(), .x, .flags, .iterations, .history, unwrapped() and precondition() are the base class's."""

    def __init__(self, n, rows=None, coef=None, size=2.0, dtype=torch.float64, batch=2, nu=1, coarse_sweeps=2,
                 coarsen="geometric", omega=2.0 / 3.0, graph=True, check_every=8, device=None):
        if coef is None:
            raise ValueError("CoefPeriodicPCGSolver: give the element coefficient field `coef`")
        if coarsen not in RULES:
            raise ValueError(f"CoefPeriodicPCGSolver: unknown coarsen {coarsen!r} ({', '.join(RULES)})")
        field = check_field(coef)
        self._common(n, rows, "coef", field.shape, size, dtype, batch, nu, coarse_sweeps, omega, graph, check_every,
                     device)
        self.coarsen = coarsen
        self.prop = None  # there are no two materials here
        k0 = field.to(self.device).to(dtype)
        if not bool((torch.isfinite(k0) & (k0 > 0)).all()):
            raise ValueError(f"CoefPeriodicPCGSolver: a coefficient is not positive and finite once rounded to {dtype}")
        self.kmax = float(k0.max())
        F = None
        for L in self.levels:
            L.ldk = L.ld  # the pitch of the element fields of the flux and energy kernels too
            L.k = torch.ones((L.m, L.ldk), dtype=dtype, device=self.device)
            if F is None:
                L.k[:, :self.n] = k0
            else:
                _lib.call("coef_coarsen", dtype, F.k.data_ptr(), F.ldk, L.k.data_ptr(), L.ldk, F.m, F.n,
                          RULES[coarsen], self._stream())
            F = L

    @property
    def coef(self):
        """The field the solver works on: [m, n] in its dtype (the input rounded to it)."""
        return self.levels[0].k[:, :self.n]

    # ------------------------------------------------------------------ launches
    def _field(self, L):
        return dict(k=L.k.data_ptr(), ldk=L.ldk)

    def _sweep(self, L, u, out):
        self._call("coef_sweep", u=None if u is None else u.data_ptr(), f=L.f.data_ptr(), out=out.data_ptr(),
                   **self._field(L), omega=self.omega, B=self.B, **L.geom())

    def _residual_restrict(self, L, C, u):
        self._call("coef_residual_restrict", u=u.data_ptr(), f=L.f.data_ptr(), fc=C.f.data_ptr(), **self._field(L),
                   B=self.B, **L.geom(), ldc=C.ld, bstridec=C.bs)

    def _apply(self, L, p, y, part):
        self._call("coef_apply", p=p.data_ptr(), y=y.data_ptr(), part=part, **self._field(L), B=self.B, **L.geom())

    def load_case_rhs(self):
        """[2, m, n] float64: b_0 = (h / 2) ((k_SW + k_SE) - (k_NW + k_NE)), b_1 = (h / 2) ((k_NE + k_SE) - (k_NW +
        k_SW)) with the four elements of each node, the right-hand sides of the two unit mean gradients."""
        se = self.coef.to(torch.float64)
        sw, ne, nw = torch.roll(se, 1, 1), torch.roll(se, 1, 0), torch.roll(se, (1, 1), (0, 1))
        half = 0.5 * self.h
        return torch.stack([half * ((sw + se) - (nw + ne)), half * ((ne + se) - (nw + sw))]).contiguous()

    # ------------------------------------------------------------------ evaluation
    def _weighted_sum(self, ptr):
        """sum over the elements of k times the [m, ld] element field at device address `ptr`: a float64 scalar"""
        L0 = self.levels[0]
        self._call("per_reduce", a=ptr, b=L0.k.data_ptr(), part=self.part.data_ptr(), B=1, **L0.geom())
        self._final(1)
        return self.sums[0].clone()

    def _forms(self, framed, geom, pair, who):
        """(the three sums of k d over the elements, the densities [1, 3, m, n]) of samples pair[0], pair[1]"""
        from . import flux as fx
        forms = fx.pair_forms(framed.data_ptr(), self.dtype, self.device, self.B, geom, pair, None, True, who)
        d = forms.density
        step = d.stride(1) * d.element_size()
        return torch.stack([self._weighted_sum(d.data_ptr() + q * step) for q in range(3)]), d

    def flux(self, fields=True):
        """Element fluxes q = -k grad u, their means, the mean gradient and the energy of the unwrapped field, as
        PeriodicPCGSolver.flux; no host synchronisation."""
        from . import flux as fx
        framed, geom = self._framed()
        res = fx.flux_framed(framed.data_ptr(), self.dtype, self.device, *geom, phase=None, k0=1.0, k1=1.0, h=self.h,
                             fields=True)
        q = res.q
        esz = q.element_size()
        qs = torch.stack([torch.stack([self._weighted_sum(q.data_ptr() + (b * q.stride(0) + c * q.stride(1)) * esz)
                                       for c in range(2)]) for b in range(self.B)])
        energy = torch.stack([self._forms(framed, geom, (b, b), "CoefPeriodicPCGSolver.flux")[0][0]
                              for b in range(self.B)])
        sums = torch.cat([qs, res.sums[:, 2:4], energy[:, None]], 1)
        count = torch.full((), float(self.m * self.n), dtype=torch.float64, device=self.device)
        return FluxResult(q * self.coef if fields else None, qs / count, res.mean_grad, energy, sums)

    def energy_forms(self, pair=(0, 1), fields=True):
        """The energy forms between samples pair[0] and pair[1] of the unwrapped field: EnergyForms.A is [1, 1, 3], the
        sums over the elements of k d(u,u), k d(u,v), k d(v,v) (there are no phases to split by); density is
        [1, 3, m, n], the three d per element without the coefficient: the derivative of the sums with respect to each
        element's own coefficient.  No host synchronisation."""
        framed, geom = self._framed()
        A, d = self._forms(framed, geom, pair, "CoefPeriodicPCGSolver.energy_forms")
        return EnergyForms(A.reshape(1, 1, 3), d if fields else None)


def effective_conductivity_field(k, size=2.0, dtype=torch.float64, rtol=1e-10, max_iters=200, coarsen="geometric",
                                 route="flux", fields=True, device=None, **solver_kw):
    """K_eff of the periodic cell whose element (R, C) has the coefficient k[R, C] (host or device, [m, n], positive
    and finite; rounded to `dtype`), on the rectangle of width `size` (h = size / n): u = X_j + chi_j with the
    periodic fluctuation chi_j solved by CoefPeriodicPCGSolver (solver_kw: nu, coarse_sweeps, omega, graph,
    check_every) to ||r|| <= rtol ||r0||.  route "flux": K_eff[:, j] = -<q>_j, a HomogenizationResult.  route "energy":
    K_eff = sum_e k_e d(e) / |V|, exactly symmetric, an EnergyHomogenizationResult whose dK_dprop is None (there is no
    prop) and whose sensitivity [3, m, n] is the derivative of K_eff[0, 0], K_eff[0, 1], K_eff[1, 1] with respect to
    each element's own coefficient (fields=False: None).  Raises RuntimeError if a sample broke down; samples that did
    not converge in max_iters are reported in flags / converged, not hidden."""
    if route not in ("flux", "energy"):
        raise ValueError(f"effective_conductivity_field: unknown route {route!r} ('flux' or 'energy')")
    field = check_field(k)
    m, n = (int(v) for v in field.shape)
    s = CoefPeriodicPCGSolver(n, rows=m, coef=field, size=size, dtype=dtype, batch=2, coarsen=coarsen, device=device,
                              **solver_kw)
    s.solve(rtol=rtol, max_iters=max_iters)
    iters, flags = s.iterations, s.flags
    if (flags == 2).any():
        raise RuntimeError(f"effective_conductivity_field: the solve broke down (flags {flags.tolist()})")
    h = size / n
    vol = m * n * h * h
    res = s.flux(fields=False)
    mean_flux = res.mean_flux.cpu().numpy()
    if route == "energy":
        forms = s.energy_forms(pair=(0, 1), fields=fields)
        a = forms.A[0, 0].cpu().numpy() / vol
        K_E = np.array([[a[0], a[1]], [a[1], a[2]]])
        K_flux = -mean_flux.T.copy()
        gap = float(np.abs(K_E - 0.5 * (K_flux + K_flux.T)).max() / np.abs(K_E).max())
        sens = None if forms.density is None else forms.density[0] / vol
        return EnergyHomogenizationResult(K_E, None, sens, K_flux, gap, iters, flags, bool((flags == 1).all()))
    mean_grad = res.mean_grad.cpu().numpy()
    energy = res.energy.cpu().numpy()
    hill = np.abs(energy + vol * (np.eye(2) * mean_flux).sum(1)) / energy
    return HomogenizationResult(-mean_flux.T.copy(), mean_flux, mean_grad, energy, hill, iters, flags,
                                bool((flags == 1).all()))


class _FieldConductivity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, kw):
        res = effective_conductivity_field(k.detach(), route="energy", fields=True, **kw)
        if not res.converged:
            raise RuntimeError("effective_conductivity_field_torch: the solve did not converge (flags "
                               f"{res.flags.tolist()})")
        ctx.sens = res.sensitivity.to(torch.float64)
        return torch.from_numpy(res.K_eff).to(k.device)

    @staticmethod
    def backward(ctx, grad):
        s = ctx.sens
        g = grad.to(device=s.device, dtype=s.dtype)
        out = g[0, 0] * s[0] + (g[0, 1] + g[1, 0]) * s[1] + g[1, 1] * s[2]
        return out.to(grad.device), None


def effective_conductivity_field_torch(k_tensor, **kw):
    """The energy route's K_eff ([2, 2] float64, on k_tensor's device) as a differentiable function of the whole
    coefficient field k_tensor ([m, n], any float dtype, host or device): backward returns
    g00 s00 + (g01 + g10) s01 + g11 s11 with g the incoming gradient and s the sensitivity fields, the gradient with
    respect to every element's coefficient at once, with no further solve.  The solver rounds the field to its dtype
    (kw dtype, float64 by default), so value and derivative are taken AT the field rounded to that dtype: a change of
    an element below that spacing changes neither.  kw: effective_conductivity_field's (size, dtype, rtol, coarsen,
    ...), without route and fields.  The derivative is exact only for a converged solve (stationarity), so an
    unconverged one raises."""
    if k_tensor.dim() != 2:
        raise ValueError("effective_conductivity_field_torch: k_tensor must be [rows, n], got shape "
                         f"{tuple(k_tensor.shape)}")
    if "route" in kw or "fields" in kw:
        raise ValueError("effective_conductivity_field_torch: the route is 'energy' with fields; give neither")
    return _FieldConductivity.apply(k_tensor, kw)
