"""Periodic homogenization: a two-material element phase image as a periodic cell.

The [m, n] image is a torus of m x n nodes, node (r, c) the upper-left node of element (r, c), every index modulo
(m, n).  PeriodicPCGSolver solves K chi = b for the periodic fluctuation chi by conjugate gradients preconditioned with
one V(nu, nu) cycle of the torus kernels (include/feanet_periodic.h, csrc/periodic_ops.hip).  K is singular (constants)
and the float32 stencil table's rows sum to zero only to about 1e-7, so the iteration runs on the projected operator
P K P, P = I - 1 1^T / (m n) per sample: b, z = M r and K p each have their own mean subtracted.  The solved fields are
evaluated by the existing flux and energy kernels on the unwrapped field U = chi + X on (m + 1) x (n + 1) nodes.

Per-sample scalars stay on the device; the vector updates are torch elementwise operations driven by [B, 1, 1] device
tensors; a sample that is done or has broken down stops moving.  Blocks of iterations replay through graphs.GraphCache
as one linear chain on one stream.
"""
import numpy as np
import torch

from . import _lib, mesh_setup as ms, ops
from .graphs import GraphCache

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]  # tap t -> (dr, dc)


def wrapped_pattern_map(phase):
    """uint8 [m, n] pattern ids of the torus nodes of a uint8 [m, n] phase tensor (any device): interface_pattern_map's
    code e1 + 2 e2 + 4 e3 + 8 e4 with wrapped indices, e1 = (r-1, c), e2 = (r-1, c-1), e3 = (r, c-1), e4 = (r, c)."""
    ph = phase.to(torch.int64)
    code = torch.roll(ph, 1, 0) + 2 * torch.roll(ph, (1, 1), (0, 1)) + 4 * torch.roll(ph, 1, 1) + 8 * ph
    return torch.from_numpy(ms._BITS_TO_ID).to(ph.device)[code]


def load_table(ktab, h):
    """bt [16, 2] float64: bt[p][j] = -h sum_t w_t d_j(t), w_t = ktab[p][8 - t] the weight of tap t = (dr, dc) of a node
    of pattern p (the own-row form), d_0 = dr, d_1 = dc: the right-hand side of load case j at such a node."""
    k = np.asarray(ktab, np.float64).reshape(-1, 9)
    bt = np.zeros((k.shape[0], 2))
    for t, (dr, dc) in enumerate(TAPS):
        bt[:, 0] += k[:, 8 - t] * dr
        bt[:, 1] += k[:, 8 - t] * dc
    return -h * bt


def coarse_shapes(m, n):
    """The level shapes: halved while both extents are even and the smaller one exceeds 2."""
    out = [(m, n)]
    while m % 2 == 0 and n % 2 == 0 and min(m, n) > 2:
        m, n = m // 2, n // 2
        out.append((m, n))
    return out


def solved_floor(kmax, h, m, n, dtype):
    """||P b|| at or below which a sample starts solved: the rounding level of a residual of fields of size h of an
    operator whose largest coefficient is kmax (effective_conductivity's floor with h for max|u0|)."""
    u_t = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    return 22 * u_t * (32.0 * kmax / 6.0) * h * np.sqrt(m * n)


class _TorusLevel:
    """The geometry and the f / a / b buffers of one level; the solver that owns it attaches its operator's data
    (PeriodicPCGSolver: image, pid, ldp; feanet_amd.coef: k, ldk)."""

    def __init__(self, m, n, B, dtype, device):
        self.m, self.n = int(m), int(n)
        self.esz = 4 if dtype == torch.float32 else 8
        vec = 16 // self.esz
        self.ld = -(-self.n // vec) * vec
        self.bs = self.m * self.ld
        self.f, self.a, self.b = (torch.zeros((B, self.m, self.ld), dtype=dtype, device=device) for _ in range(3))

    def geom(self):
        return dict(m=self.m, n=self.n, ld=self.ld, bstride=self.bs)


class PeriodicPCGSolver:
    """Conjugate gradients on the periodic cell of an [rows, n] element phase image, preconditioned by one V(nu, nu)
    cycle from a zero guess (weighted Jacobi, omega / d per pattern; full-weighting restriction and its transpose;
    coarse_sweeps sweeps from zero on the coarsest level; the coarse images by mesh_setup.coarsen_phase's rule
    `coarsen`).  solve() leaves .x ([B, 1, m, n], mean-free), .iterations, .flags (1 converged, 2 breakdown, 0 stopped)
    and .history (list of per-sample residual norms, entry 0 the initial one)."""

    def __init__(self, n, rows=None, phase=None, prop=(1, 20), size=2.0, dtype=torch.float64, batch=2, nu=1,
                 coarse_sweeps=2, coarsen="stiff", omega=2.0 / 3.0, graph=True, check_every=8, device=None):
        if phase is None:
            raise ValueError("PeriodicPCGSolver: give the element phase image `phase`")
        if len(phase.shape) != 2:
            raise ValueError(f"PeriodicPCGSolver: phase must be [rows, n], got shape {tuple(phase.shape)}")
        self._common(n, rows, "phase", phase.shape, size, dtype, batch, nu, coarse_sweeps, omega, graph, check_every,
                     device)
        self.prop = tuple(prop)
        self.kmax = float(max(np.float32(prop[0]), np.float32(prop[1])))
        npdt = np.float32 if dtype == torch.float32 else np.float64
        ktab = ms.stencil_table(self.prop)
        self.ktab_np = ktab
        self.ktab = torch.from_numpy(ktab.reshape(16, 9).astype(npdt)).to(self.device)
        self.omd = torch.from_numpy(ms.omega_over_d(ktab, omega, npdt)).to(self.device)
        self.bt = torch.from_numpy(load_table(ktab, self.h)).to(self.device)
        img = ms._phase_tensor(phase, self.device)
        k = ms.phase_min_count(self.prop, coarsen)
        for i, L in enumerate(self.levels):
            if i:
                img = ms.coarsen_phase_device(img, k)
            assert tuple(img.shape) == (L.m, L.n)
            L.image, L.ldp = img, -(-L.n // 16) * 16
            L.pid = torch.zeros((L.m, L.ldp), dtype=torch.uint8, device=self.device)
            L.pid[:, :L.n] = wrapped_pattern_map(img)

    def _common(self, n, rows, what, shape, size, dtype, batch, nu, coarse_sweeps, omega, graph, check_every, device):
        """What every solver on the torus layout checks and holds: the cell against the [rows, n] input `what` of
        shape `shape`, the device, the library, the scalars, the levels without their operator, the Krylov fields,
        the partial sums and the per-sample scalars."""
        name = type(self).__name__
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name}: unsupported dtype {dtype} (float32/float64 only)")
        m = int(n if rows is None else rows)
        n = int(n)
        if tuple(int(v) for v in shape) != (m, n):
            raise ValueError(f"{name}: {what} is {tuple(shape)}, the cell has {m} x {n} elements")
        if int(nu) < 1 or int(coarse_sweeps) < 1 or int(batch) < 1 or int(check_every) < 1:
            raise ValueError(f"{name}: nu, coarse_sweeps, batch and check_every must be at least 1")
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name} needs the MI355X (there is no CPU fallback for the HIP path)")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _lib.lib()
        self.m, self.n, self.B, self.dtype = m, n, int(batch), dtype
        self.size, self.h, self.omega = float(size), float(size) / n, float(omega)
        self.nu, self.coarse_sweeps = int(nu), int(coarse_sweeps)
        self.use_graph, self.check_every = bool(graph), int(check_every)
        self.levels = [_TorusLevel(lm, ln, self.B, dtype, self.device) for lm, ln in coarse_shapes(m, n)]
        L0 = self.levels[0]
        self.r = L0.f  # the preconditioner's right-hand side buffer is the residual
        self._x, self.p, self.y = (torch.zeros_like(L0.f) for _ in range(3))
        self.per = int(_lib.lib().fea_per_parts(m, n, L0.esz))
        f64 = dict(dtype=torch.float64, device=self.device)
        self.part = torch.zeros(2 * self.B * self.per, **f64)
        self.sums = torch.zeros(2 * self.B, **f64)
        self.rz_old, self.rn, self.rr0, self.thresh = (torch.zeros(self.B, **f64) for _ in range(4))
        self.flag = torch.zeros(self.B, dtype=torch.int64, device=self.device)
        self.iters = torch.zeros(self.B, dtype=torch.int64, device=self.device)
        self.k = torch.zeros(1, dtype=torch.int64, device=self.device)  # the history row the next iteration writes
        self.hist = torch.zeros((201, self.B), **f64)
        self._graphs = GraphCache(self.device)
        self._load_cases = False
        self.flags = self.iterations = self.history = None

    # ------------------------------------------------------------------ launches
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, name, **kw):
        rec = _lib.launch(name, **kw)
        _lib.call(rec[0], self.dtype, *rec[1], self._stream())

    # the three launches of the operator: what a solver on another operator (feanet_amd.coef) replaces
    def _stencil(self, L):
        return dict(pid=L.pid.data_ptr(), ldp=L.ldp, ktab=self.ktab.data_ptr())

    def _sweep(self, L, u, out):
        self._call("per_sweep", u=None if u is None else u.data_ptr(), f=L.f.data_ptr(), out=out.data_ptr(),
                   **self._stencil(L), omd=self.omd.data_ptr(), B=self.B, **L.geom())

    def _residual_restrict(self, L, C, u):
        """C.f = R (L.f - K u)"""
        self._call("per_residual_restrict", u=u.data_ptr(), f=L.f.data_ptr(), fc=C.f.data_ptr(), **self._stencil(L),
                   B=self.B, **L.geom(), ldc=C.ld, bstridec=C.bs)

    def _sweeps(self, L, u, count):
        """count sweeps from u (None: the zero guess), ping-pong between L.a and L.b -> the buffer of the result"""
        for _ in range(count):
            out = L.b if u is L.a else L.a
            self._sweep(L, u, out)
            u = out
        return u

    def _cycle(self, l=0):
        """One V(nu, nu) cycle from a zero guess on level l's right-hand side L.f; the buffer that holds the result."""
        L = self.levels[l]
        if l == len(self.levels) - 1:
            return self._sweeps(L, None, self.coarse_sweeps)
        C = self.levels[l + 1]
        u = self._sweeps(L, None, self.nu)
        self._residual_restrict(L, C, u)
        ec = self._cycle(l + 1)
        self._call("per_prolong_add", ec=ec.data_ptr(), u=u.data_ptr(), B=self.B, **L.geom(), ldc=C.ld, bstridec=C.bs)
        return self._sweeps(L, u, self.nu)

    def _final(self, count):
        _lib.call_raw("per_final", self.part.data_ptr(), self.per, self.sums.data_ptr(), count, self._stream())

    def _reduce(self, a, b=None):
        """[B] float64: a . b per sample, or the sum of a (a view of a buffer the next reduction overwrites)"""
        L0 = self.levels[0]
        self._call("per_reduce", a=a.data_ptr(), b=None if b is None else b.data_ptr(), part=self.part.data_ptr(),
                   B=self.B, **L0.geom())
        self._final(self.B)
        return self.sums[:self.B]

    def _project(self, v, total=None):
        """v -= mean(v) per sample (total: the sums of v, if they are known)"""
        s = self._reduce(v) if total is None else total
        v.sub_((s / float(self.m * self.n)).to(self.dtype)[:, None, None])

    def _apply(self, L, p, y, part):
        self._call("per_apply", p=p.data_ptr(), y=y.data_ptr(), part=part, **self._stencil(L), B=self.B, **L.geom())

    def apply(self, p, y, sums=False):
        """y = K p on torus buffers; sums: also (p . y, sum y) per sample as a [B, 2] float64 view."""
        self._apply(self.levels[0], p, y, self.part.data_ptr() if sums else None)
        if sums:
            self._final(2 * self.B)
            return self.sums.view(self.B, 2)

    def precondition(self, r):
        """z = M r ([B, m, n] or [B, 1, m, n] in, [B, m, n] out), the unprojected cycle (for tests and tools)."""
        L0 = self.levels[0]
        L0.f[..., :self.n] = r.reshape(self.B, self.m, self.n).to(self.dtype)
        return self._cycle()[..., :self.n].clone()

    # ------------------------------------------------------------------ iteration
    def _iteration(self):
        T = self.dtype
        col = lambda s: s.to(T)[:, None, None]
        z = self._cycle()
        self._project(z)
        rz = self._reduce(self.r, z).clone()
        active = self.flag == 0
        beta = rz / self.rz_old  # rz_old is +inf before the first iteration: beta = 0
        self.p.copy_(torch.where(active[:, None, None], z + col(beta) * self.p, self.p))
        s2 = self.apply(self.p, self.y, sums=True)
        pAp, sy = s2[:, 0].clone(), s2[:, 1].clone()
        self._project(self.y, sy)
        bad = ~(torch.isfinite(pAp) & (pAp > 0))
        self.flag.copy_(torch.where(active & bad, 2, self.flag))
        active = active & ~bad
        a3 = active[:, None, None]
        alpha = col(rz / pAp)
        self._x.copy_(torch.where(a3, self._x + alpha * self.p, self._x))
        self.r.copy_(torch.where(a3, self.r - alpha * self.y, self.r))
        rn = torch.sqrt(self._reduce(self.r, self.r))
        self.rn.copy_(torch.where(active, rn, self.rn))
        self.rz_old.copy_(torch.where(active, rz, self.rz_old))
        self.iters.add_(active.to(torch.int64))
        self.hist.index_copy_(0, self.k, self.rn[None])
        self.k.add_(1)
        self.flag.copy_(torch.where(active & (rn <= self.thresh), 1, self.flag))

    def load_case_rhs(self):
        """[2, m, n] float64: b_j = bt[pid][:, j], the right-hand sides of the two unit mean gradients."""
        L0 = self.levels[0]
        return self.bt[L0.pid[:, :self.n].long()].permute(2, 0, 1).contiguous()

    def solve(self, b=None, rtol=1e-10, max_iters=200):
        """Solve P K P x = P b per sample until ||r|| <= rtol ||P b||, breakdown or max_iters.  b None: the two load
        cases (batch 2); else [B, 1, m, n] or [B, m, n].  A sample whose ||P b|| is at the rounding level of a residual
        (solved_floor) starts solved, with 0 iterations.  Returns x [B, 1, m, n].  The host reads the flags every
        check_every iterations and at no other time."""
        m, n, B = self.m, self.n, self.B
        if b is None:
            if B != 2:
                raise ValueError("PeriodicPCGSolver.solve: the load cases need batch=2")
            b = self.load_case_rhs()
            self._load_cases = True
        else:
            ops.require_hip(b, "b")
            if b.numel() != B * m * n or tuple(b.shape[-2:]) != (m, n):
                raise ValueError(f"PeriodicPCGSolver.solve: b must be [{B}, 1, {m}, {n}]")
            self._load_cases = False
        if max_iters + 1 > self.hist.shape[0]:
            self.hist = torch.zeros((max_iters + 1, B), dtype=torch.float64, device=self.device)
            self._graphs.clear()
        self.r.zero_()
        self.r[..., :n] = b.reshape(B, m, n).to(self.dtype)
        self._project(self.r)
        self._x.zero_()
        self.p.zero_()
        self.hist.zero_()
        self.rr0.copy_(torch.sqrt(self._reduce(self.r, self.r)))
        self.rn.copy_(self.rr0)
        self.thresh.copy_(self.rr0 * float(rtol))
        self.flag.copy_((self.rr0 <= solved_floor(self.kmax, self.h, m, n, self.dtype)).to(torch.int64))
        self.rz_old.fill_(float("inf"))
        self.iters.zero_()
        self.hist[0] = self.rr0
        self.k.fill_(1)
        it = 0
        while it < max_iters:
            nb = min(self.check_every, max_iters - it)
            if bool((self.flag != 0).all().item()):
                break
            self._graphs.run(("iterate", nb, self.hist.data_ptr()),
                             lambda: [self._iteration() for _ in range(nb)], self.use_graph)
            it += nb
        self._project(self._x)
        self.flags = self.flag.cpu().numpy().copy()
        self.iterations = self.iters.cpu().numpy().copy()
        h = self.hist[:int(self.iterations.max()) + 1].cpu().numpy()
        self.history = [row.copy() for row in h]
        return self.x

    @property
    def x(self):
        """The current iterate as a contiguous [B, 1, m, n] tensor."""
        return self._x[..., :self.n].reshape(self.B, 1, self.m, self.n).contiguous()

    # ------------------------------------------------------------------ evaluation
    def unwrapped(self):
        """U [B, 1, m+1, n+1]: the periodic extension of x, plus the linear fields of homogenize.load_cases if the last
        solve took the load cases (sample j: the unit mean gradient e_j)."""
        m, n = self.m, self.n
        ri = torch.arange(m + 1, device=self.device) % m
        ci = torch.arange(n + 1, device=self.device) % n
        U = self.x[:, :, ri][:, :, :, ci].contiguous()
        if self._load_cases:
            from .homogenize import load_cases
            U = U + load_cases(m, n, self.size, self.dtype, self.device)
        return U

    def _framed(self):
        """(the framed copy of the unwrapped field, its geometry (B, H, W, ld, bstride))"""
        from . import flux as fx
        framed, *geom = fx._framed_copy(self.unwrapped(), "u")
        return framed, tuple(geom)

    def flux(self, fields=True):
        """Element fluxes, their means, the mean gradient and the energy of the unwrapped field, as
        MultigridSolver.flux; no host synchronisation."""
        from . import flux as fx
        framed, geom = self._framed()
        k0, k1 = fx.coefficients(self.prop)
        return fx.flux_framed(framed.data_ptr(), self.dtype, self.device, *geom, phase=self.levels[0].image, k0=k0,
                              k1=k1, h=self.h, fields=fields)

    def energy_forms(self, pair=(0, 1), fields=True):
        """The energy forms between samples pair[0] and pair[1] of the unwrapped field, as
        MultigridSolver.energy_forms; no host synchronisation."""
        from . import flux as fx
        framed, geom = self._framed()
        return fx.pair_forms(framed.data_ptr(), self.dtype, self.device, self.B, geom, pair, self.levels[0].image,
                             fields, "PeriodicPCGSolver.energy_forms")
