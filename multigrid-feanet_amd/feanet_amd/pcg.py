"""PCGSolver: conjugate gradients preconditioned by one V-cycle, resident on one MI355X.

The stationary iteration of MultigridSolver needs the V-cycle's error propagator to contract; with rediscretised
coarse operators and two Jacobi sweeps as the coarse solve it stops doing so once the two-material contrast leaves
the reference's prop=(1, 20).  The same V(nu, nu) cycle from a zero guess is a symmetric positive definite operator
M (symmetric smoother, R = P^T, positive semi-definite coarse term), so it can precondition CG, which converges
whatever the contraction number of the stationary iteration.

One iteration (all on the device, nothing read by the host):

    z = M r                      MultigridSolver(zero_start=True): its right-hand side buffer IS r, its end iterate IS z
    rz = r.z                     fea_pcg_dot        + fea_pcg_scalar_step(RZ):  beta = rz / rz_prev
    p' = z + beta p              fea_pcg_direction  + fea_pcg_scalar_step(PAP): alpha = rz / p'.Kp'
    x += alpha p', r -= alpha Kp'  fea_pcg_update   + fea_pcg_scalar_step(RR):  ||r||, done flag, history row

p ping-pongs between two buffers (the direction kernel rebuilds p' on its halos from z and p).  A sample freezes
(alpha = beta = 0, x and r stop moving, history rows repeat) once ||r|| <= its threshold or on a breakdown
(pAp <= 0 or non-finite, r.z non-finite), so its result depends neither on the other samples nor on how often the
host looks at the flags.  Blocks of iterations are replayed as HIP graphs.

Mixed precision (dtype=float64, precond_dtype=float32): the recurrences above stay in fp64 — they fix the attainable
accuracy — while M, which only has to be a good approximate inverse, is an fp32 hierarchy at half the bytes.  x, b, r
and the two p are the only fp64 fields; the fp64f32 kernels hand the preconditioner float(r s_b) in its fp32 frame
and read its fp32 end iterate.  s_b is one power of two per sample, fixed by load() so that ||r0|| s_b is in [1, 2):
the fp32 cycle sees O(1) data however far r has been reduced and whatever the units of b, and CG is invariant to it
(z, r.z and alpha carry the factor; x, r, beta and the history do not).
"""
import numpy as np
import torch

from . import _lib, mesh_setup as ms, ops
from .graphs import GraphCache
from .solver import MultigridSolver, _Level

# scalar block layout and steps: include/feanet_hip.h (FEA_PCG_*)
NSCALARS = 12
RZ, RZ_PREV, PAP, ALPHA, BETA, RNORM, DONE, ITERS, EPS, RTOL, THRESH, ROW = range(NSCALARS)
CONVERGED, BREAKDOWN = 1, 2
STEP_INIT, STEP_RZ, STEP_PAP, STEP_RR = range(4)
_KRYLOV = ("pcg_residual", "pcg_dot", "pcg_direction", "pcg_update")  # launched in the solver's dtype


class PCGSolver:
    """Multigrid-preconditioned conjugate gradients for MultigridSolver's problems (one GPU).

    Args as MultigridSolver (n, levels, problem, dtype, batch, omega, size, prop, shape, rows, R, P, w, and the
    element phase image phase / coarsen / phase_levels of the two-material problem, with its limits: two phases, one
    image for the whole batch), and
        nu: pre- and post-sweeps of the preconditioning V(nu, nu) cycle (equal, so the cycle is symmetric).
        graph: replay blocks of iterations as HIP graphs.
        check_every: solve() reads the samples' done flags every this many iterations, and at no other time.
        precond_dtype: dtype of the preconditioning hierarchy.  None or dtype: the whole solver in dtype.
            dtype=float64 with precond_dtype=float32: fp64 conjugate gradients around an fp32 V-cycle (five fp64
            fine-level fields, no fp64 coarse level).  A preconditioner wider than the solve is refused.

    Rejected with ValueError, because the preconditioner would not be symmetric: compat schedules, the learned
    smoother, and R / P tables that are not one kernel repeated with R == P (per-pattern learned tables pick the
    kernel by fine-node pattern in R and coarse-node pattern in P, so P != R^T).  The ratios w may be any positive
    pair.
    """

    GRAPH_ITERS = 8    # iterations per captured HIP graph
    HIST_ROWS = 1024   # history rows kept on the device (grown by solve(max_iters=...))

    def __init__(self, n, levels=None, problem="poisson", dtype=torch.float64, device=None, batch=1,
                 omega=2.0 / 3.0, size=2.0, prop=(1, 20), shape=0, rows=None, R=None, P=None, w=(1.0, 1.0), nu=1,
                 graph=True, check_every=8, smoother="jac", compat=None, precond_dtype=None, phase=None,
                 coarsen="majority", phase_levels=None):
        pdt = dtype if precond_dtype is None else precond_dtype
        for name, d in (("dtype", dtype), ("precond_dtype", pdt)):
            if d not in (torch.float32, torch.float64):
                raise TypeError(f"PCGSolver: {name} must be torch.float32 or torch.float64, got {d!r}")
        if pdt == torch.float64 and dtype == torch.float32:
            raise ValueError("PCGSolver: precond_dtype=float64 is wider than dtype=float32; the preconditioner may be "
                             "narrower than the solve, not wider")
        if compat is not None:
            raise ValueError("PCGSolver: compat schedules are not symmetric V-cycles")
        if smoother != "jac":
            raise ValueError(f"PCGSolver: smoother={smoother!r} is not symmetric; only 'jac' can precondition CG")
        if int(nu) < 1:
            raise ValueError("PCGSolver: nu >= 1 (without smoothing the V-cycle is only semi-definite)")
        if int(check_every) < 1:
            raise ValueError("PCGSolver: check_every >= 1")
        lin = ms.linear_transfer_kernel() / np.float32(4.0)
        tabs = [lin[None] if t is None else np.asarray(torch.as_tensor(t).detach().cpu().float().numpy(), np.float32)
                for t in (R, P)]
        Rk, Pk = (t.reshape(-1, 3, 3) for t in tabs)
        if not ((Rk == Rk[:1]).all() and (Pk == Pk[:1]).all() and np.array_equal(Rk[0], Pk[0])):
            raise ValueError("PCGSolver: R and P must be one 3x3 kernel, the same for both (P = R^T); per-pattern "
                             "tables make the V-cycle non-symmetric")
        wl = [float(v) for v in (w.detach().cpu().tolist() if torch.is_tensor(w) else w)]
        if not (wl[0] > 0 and wl[1] > 0):
            raise ValueError("PCGSolver: the ratios w must be positive")
        self.mg = MultigridSolver(n, levels=levels, problem=problem, dtype=pdt, device=device, batch=batch,
                                  omega=omega, size=size, prop=prop, shape=shape, R=R, P=P, w=w, nu1=int(nu),
                                  nu2=int(nu), graph=False, rows=rows, zero_start=True, smoother="jac", phase=phase,
                                  coarsen=coarsen, phase_levels=phase_levels)
        mg = self.mg
        self.device, self.dtype, self.B = mg.device, dtype, mg.B
        self.mixed = pdt != dtype
        self.use_graph = bool(graph)
        self.check_every = int(check_every)
        self._pf = mg.levels[0].f  # the preconditioner's right-hand side buffer
        self._bc = None  # mixed precision: the Dirichlet values in fp64 (else the preconditioner holds them)
        if self.mixed:
            # the Krylov fields' own fp64 frame: its three fields are r, x and b, and its pattern map and stencil
            # table are kapply<double>'s (pattern windows hold byte offsets of sizeof(T) table rows)
            if mg.phase_images is not None:  # the same fine image, on the device
                self.L0 = L0 = _Level(mg.m, mg.n, self.B, dtype, self.device, pid_phase=mg.phase_images[0])
            else:
                self.L0 = L0 = _Level(mg.m, mg.n, self.B, dtype, self.device,
                                      pid_shape=(shape, size) if problem == "interface" else None)
            self.ktab = torch.from_numpy(mg.ktab_np.reshape(-1, 9).astype(np.float64)).to(self.device)
            self.r, self.x, self.b = L0.f, L0.a, L0.b
            p0, p1 = (torch.zeros_like(L0.a) for _ in range(2))
            self.sb = torch.ones(self.B, dtype=torch.float64, device=self.device)  # per-sample scale s_b
        else:
            self.L0 = L0 = mg.levels[0]
            self.ktab = mg.ktab
            self.r = L0.f  # the preconditioner's right-hand side buffer is the residual
            self.x, self.b, p0, p1 = (torch.zeros_like(L0.a) for _ in range(4))
        self.p = (p0, p1)
        self._parity = 0  # the next iteration reads p[_parity] and writes p[1 - _parity]
        self._zname = None
        self.per = int(_lib.lib().fea_pcg_parts(L0.H, L0.W, L0.esz))
        self.part = torch.zeros(self.B * self.per, dtype=torch.float64, device=self.device)
        self.sc = torch.zeros((self.B, NSCALARS), dtype=torch.float64, device=self.device)
        self.hist = torch.zeros((self.HIST_ROWS, self.B), dtype=torch.float64, device=self.device)
        self._graphs = GraphCache(self.device)
        self._loaded = False
        self.flags = None        # after solve(): per-sample 1 converged, 2 breakdown, 0 still running
        self.iterations = None   # after solve(): per-sample iterations that moved x

    # ------------------------------------------------------------------ problem data
    @property
    def H(self):
        return self.mg.H

    @property
    def W(self):
        return self.mg.W

    def set_rhs(self, f=None, F=None):
        """The assembled right-hand side f, or the nodal source F (FNet applied on the device)."""
        if (f is None) == (F is None):
            raise ValueError("PCGSolver.set_rhs: give exactly one of f (assembled) or F (source)")
        if F is not None:
            f = ops.conv3x3(self._check_field(F, "F"), torch.from_numpy(self.mg.mass))
        self._pack(self._check_field(f, "f"), self.b, reset=False)
        self._loaded = False

    def set_boundary(self, bc_value=None, geometry_idx=None):
        """Dirichlet data of the fine level (square geometry only, as MultigridSolver); used by the next load()."""
        if not self.mixed:
            self.mg.set_boundary(bc_value, geometry_idx)
            return
        self.mg.set_boundary(None, geometry_idx)  # refuses any geometry but the square; the values stay in fp64 here
        self._bc = None if bc_value is None else self._check_field(bc_value, "boundary_value")

    def _check_field(self, x, name):
        """x as a contiguous [B, 1, H, W] tensor of the solver's dtype (never through the preconditioner's)."""
        if not self.mixed:
            return self.mg._check_field(x, name)
        ops.require_hip(x, name)
        x = x.to(self.dtype)
        H, W = self.H, self.W
        if x.numel() == H * W:
            x = x.reshape(1, 1, H, W).expand(self.B, 1, H, W)
        if tuple(x.shape[-2:]) != (H, W) or x.numel() != self.B * H * W:
            raise ValueError(f"PCGSolver: {name} must be [{self.B}, 1, {H}, {W}]")
        return x.reshape(self.B, 1, H, W).contiguous()

    def _pack(self, x, dst, bc=None, reset=True):
        """x (None: zeros) -> framed dst in the solver's dtype; reset: x*geo + bc, else a raw copy."""
        bp, bs = (None, 0) if bc is None else (bc.data_ptr(), self.H * self.W)
        _lib.call("mg_pack", self.dtype, None if x is None else x.data_ptr(), dst.data_ptr(), None,
                  0 if reset else -1, bp, bs, *self.L0.geom(), self._stream())

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _kargs(self):
        L0 = self.L0
        return (None if L0.pid is None else L0.pid.data_ptr(), self.ktab.data_ptr(), self.mg.ntab)

    def _stencil(self):
        pid, ktab, ntab = self._kargs()
        return dict(pid=pid, ktab=ktab, ntab=ntab)

    def _geom(self):
        """The Krylov fields' frame by parameter name; mixed precision: with the preconditioner's fp32 level-0 frame."""
        g = self.L0.geom_kw()
        if self.mixed:
            g["ld32"], g["bstride32"] = self._g32()
        return g

    def _g32(self):
        """(ld, bstride) of the preconditioner's fp32 level-0 frame (mixed precision)."""
        P0 = self.mg.levels[0]
        return (P0.ld, P0.bs)

    def _scalar(self, step):
        return _lib.launch("pcg_scalar_step", part=self.part.data_ptr(), per=self.per, scalars=self.sc.data_ptr(),
                           hist=self.hist.data_ptr(), hist_rows=self.hist.shape[0], B=self.B, step=step)

    def _launch(self, launches):
        stream = self._stream()
        for name, args in launches:
            if name == "pcg_scalar_step" or name.endswith("_f64f32"):
                _lib.call_raw(name, *args, stream)
            else:  # the preconditioner's plan runs in its own dtype
                _lib.call(name, self.dtype if name in _KRYLOV else self.mg.dtype, *args, stream)

    def load(self, u0=None, eps=0.0, rtol=None):
        """Start from u0 (reset_boundary applied: u*geo + bc): r = b - K x, history row 0 = ||r0||.  Samples stop at
        ||r|| <= rtol * ||r0|| if rtol is given, else at ||r|| <= eps."""
        mg, L0 = self.mg, self.L0
        if u0 is not None:
            u0 = self._check_field(u0, "u0")
        self._pack(u0, self.x, bc=self._bc if self.mixed else mg._bc)
        self.p[0].zero_()
        self.p[1].zero_()
        self.sc.zero_()
        self.sc[:, EPS] = float(eps)
        self.sc[:, RTOL] = -1.0 if rtol is None else float(rtol)
        self._parity = 0
        self._launch([_lib.launch("pcg_residual", x=self.x.data_ptr(), f=self.b.data_ptr(), r=self.r.data_ptr(),
                                  part=self.part.data_ptr(), **self._stencil(), **L0.geom_kw()),
                      self._scalar(STEP_INIT)])
        if self.mixed:  # fixes s_b from ||r0|| and hands the preconditioner float(r0 s_b)
            self._launch([_lib.launch("pcg_narrow_f64f32", r=self.r.data_ptr(), r32=self._pf.data_ptr(),
                                      scalars=self.sc.data_ptr(), sb=self.sb.data_ptr(), **self._geom())])
        self._loaded = True

    # ------------------------------------------------------------------ iteration
    def _iteration(self, q):
        """Launches of one iteration reading p[q], writing p[1 - q]."""
        mg, P0 = self.mg, self.mg.levels[0]
        plan, end = mg._plan("a")  # from a zero guess: the plan does not depend on the start buffer
        if self._zname is None:
            self._zname = end
        assert end == self._zname and P0.buf(end).data_ptr() != self._pf.data_ptr(), "the preconditioner's output moved"
        z = P0.buf(end).data_ptr()
        launch, g, st = _lib.launch, self._geom(), self._stencil()
        part, sc, r, x = self.part.data_ptr(), self.sc.data_ptr(), self.r.data_ptr(), self.x.data_ptr()
        pin, pout = self.p[q].data_ptr(), self.p[1 - q].data_ptr()
        if self.mixed:
            return list(plan) + [
                launch("pcg_dot_f64f32", r=r, z32=z, part=part, **g), self._scalar(STEP_RZ),
                launch("pcg_direction_f64f32", z32=z, p_in=pin, p_out=pout, scalars=sc, part=part, **st, **g),
                self._scalar(STEP_PAP),
                launch("pcg_update_f64f32", p=pout, x=x, r=r, r32=self._pf.data_ptr(), scalars=sc,
                       sb=self.sb.data_ptr(), part=part, **st, **g),
                self._scalar(STEP_RR)]
        return list(plan) + [
            launch("pcg_dot", r=r, z=z, part=part, **g), self._scalar(STEP_RZ),
            launch("pcg_direction", z=z, p_in=pin, p_out=pout, scalars=sc, part=part, **st, **g),
            self._scalar(STEP_PAP),
            launch("pcg_update", p=pout, x=x, r=r, scalars=sc, part=part, **st, **g), self._scalar(STEP_RR)]

    def krylov_launches_per_iteration(self):
        return 6

    def _run_block(self, q, nb):
        """nb iterations from parity q: eager, then captured, then replayed (GraphCache)."""
        self._graphs.run((q, nb, self.hist.data_ptr()),
                         lambda: self._launch([rec for i in range(nb) for rec in self._iteration((q + i) % 2)]),
                         self.use_graph)

    def iterate(self, k=1):
        """k iterations on the resident state (asynchronous; no host sync)."""
        if not self._loaded:
            raise RuntimeError("PCGSolver.iterate: call load() (after set_rhs) first")
        while k > 0:
            nb = min(k, self.GRAPH_ITERS)
            self._run_block(self._parity, nb)
            self._parity = (self._parity + nb) % 2
            k -= nb

    def solution(self):
        """Current iterate as a contiguous [B, 1, H, W] tensor."""
        L0 = self.L0
        out = torch.empty((self.B, 1, self.H, self.W), dtype=self.dtype, device=self.device)
        _lib.call("mg_unpack", self.dtype, self.x.data_ptr(), out.data_ptr(), *L0.geom(), self._stream())
        return out

    def flux(self, fields=True):
        """Element fluxes, their means, the mean gradient and the energy of the current iterate x (mixed precision:
        the fp64 x), as MultigridSolver.flux; no host synchronisation."""
        from . import flux as fx
        img, k0, k1 = self.mg.flux_image()
        return fx.flux_framed(self.x.data_ptr(), self.dtype, self.device, *self.L0.geom(), phase=img, k0=k0, k1=k1,
                              h=self.mg.size / self.mg.n, fields=fields)

    def energy_forms(self, pair=(0, 1), fields=True):
        """The energy forms between samples pair[0] and pair[1] of the current iterate x (mixed precision: the fp64
        x), as MultigridSolver.energy_forms; no host synchronisation."""
        from . import flux as fx
        return fx.pair_forms(self.x.data_ptr(), self.dtype, self.device, self.B, self.L0.geom(), pair,
                             self.mg.flux_image()[0], fields, "PCGSolver.energy_forms")

    def residual_norm(self):
        """Per-sample true residual ||(b - K x)[1:-1, 1:-1]||_2 (float64 device tensor [B]), recomputed from x."""
        mg, L0 = self.mg, self.L0
        _lib.call("mg_residual_norm", self.dtype, self.x.data_ptr(), self.b.data_ptr(), *self._kargs(),
                  mg.norm_out.data_ptr(), mg.ws.data_ptr(), *L0.geom(), 0, 0, 0, 0, self._stream())
        return mg.norm_out.clone()

    def scalars(self):
        """The per-sample scalar blocks ([B, 12] float64, host copy; synchronises)."""
        return self.sc.cpu().numpy()

    def history(self):
        """Recurrence residual norms so far: list of per-sample arrays, entry 0 the initial residual, up to the
        last iteration that moved any sample (synchronises)."""
        sc = self.scalars()
        rows = min(int(sc[:, ITERS].max()) + 1, self.hist.shape[0])
        h = self.hist[:rows].cpu().numpy()
        return [h[i].copy() for i in range(rows)]

    def solve(self, u0=None, f=None, F=None, eps=1e-6, rtol=None, max_iters=100, bc_value=None):
        """Iterate until every sample is frozen (converged: ||r_b|| <= eps, or <= rtol * ||r0_b|| if rtol is given;
        or broken down) or max_iters.  Returns (u [B, 1, H, W], history as MultigridSolver.solve: a list of
        per-sample arrays, first entry the initial residual).  self.flags / self.iterations hold the per-sample
        outcome.  The host reads the done flags every check_every iterations and at no other time."""
        if bc_value is not None:
            self.set_boundary(bc_value)
        if f is not None or F is not None:
            self.set_rhs(f=f, F=F)
        if max_iters + 1 > self.hist.shape[0]:
            self.hist = torch.zeros((max_iters + 1, self.B), dtype=torch.float64, device=self.device)
            self._graphs.clear()
        self.load(u0, eps=eps, rtol=rtol)
        it = 0
        while it < max_iters:
            k = min(self.check_every, max_iters - it)
            self.iterate(k)
            it += k
            if bool((self.sc[:, DONE] != 0).all().item()):
                break
        sc = self.scalars()
        self.flags = sc[:, DONE].astype(np.int64)
        self.iterations = sc[:, ITERS].astype(np.int64)
        return self.solution(), self.history()
