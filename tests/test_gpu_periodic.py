"""The periodic cell on the device: every fea_per_* kernel against the numpy oracle of periodic_ref.py
within the absolute-companion bound of generic_ref.py, their write footprint and batch independence, the V-cycle, the
projected conjugate gradient, and effective_conductivity(bc="periodic") against dense solves on the same table.

The kernel tests use the random_elements image, prop (1, 20), B = 3, pad columns (and the pattern map's pad bytes)
pre-filled with NaN (0xff)."""
import functools

import numpy as np
import pytest
import torch

import periodic_ref as pf
import phase_ref as pr

pytestmark = pytest.mark.gpu

# (6, 258): a second strip in fp32 too (256 columns), so lane 63 loads its right neighbour
EVEN = [(2, 2), (4, 6), (6, 10), (12, 16), (20, 66), (32, 130), (6, 258)]
SUFS = ["f64", "f32"]
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
PROP = (1, 20)
B = 3
RTOL = 1e-10
# the smallest m at n = 16 for which fea_per_parts shows more than one row task (the same for both types: one strip)
M_TASKS = next(m for m in range(2, 64) if pf.parts(m, 16, 8) > 1 and pf.parts(m, 16, 4) > 1)
SHAPES = EVEN + [(5, 7), (M_TASKS, 16)]


# ----------------------------------------------------------------------------- torus buffers
class Torus:
    """The level's operands on the device: NaN in every pad column, 0xff in the pattern map's pad bytes."""

    def __init__(self, m, n, suf):
        from feanet_amd import mesh_setup as ms
        self.m, self.n, self.suf, self.T = m, n, suf, DT[suf]
        esz = 4 if suf == "f32" else 8
        vec = 16 // esz
        self.esz, self.ld = esz, -(-n // vec) * vec
        self.bs = m * self.ld
        self.ldp = -(-n // 16) * 16
        self.img = pr.image("random_elements", m, n)
        self.pid_np = pf.wrapped_map(self.img)
        pid = np.full((m, self.ldp), 255, np.uint8)
        pid[:, :n] = self.pid_np
        self.pid = torch.from_numpy(pid).cuda()
        ktab = ms.stencil_table(PROP).reshape(16, 9)
        self.ktab_np = ktab.astype(np.float64)
        self.omd_np = ms.omega_over_d(ktab.reshape(16, 3, 3), pf.OMEGA, NP[suf])
        self.ktab = torch.from_numpy(ktab.astype(NP[suf])).cuda()
        self.omd = torch.from_numpy(self.omd_np).cuda()
        self.per = pf.parts(m, n, esz)

    def field(self, seed, nb=B, m=None, n=None, ld=None):
        """(host values as T widened to fp64 [nb, m, n], device buffer [nb, m, ld] with NaN pads)"""
        m, n, ld = m or self.m, n or self.n, ld or self.ld
        x = np.random.default_rng([seed, m, n]).standard_normal((nb, m, n)).astype(NP[self.suf])
        return x.astype(np.float64), self.buffer(x, ld)

    def buffer(self, x, ld=None):
        nb, m, n = x.shape
        buf = torch.full((nb, m, ld or self.ld), float("nan"), dtype=self.T, device="cuda")
        buf[..., :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda().to(self.T)
        return buf

    def empty(self, nb=B, m=None, ld=None):
        return torch.full((nb, m or self.m, ld or self.ld), float("nan"), dtype=self.T, device="cuda")

    def geom(self):
        return dict(m=self.m, n=self.n, ld=self.ld, bstride=self.bs)

    def stencil(self):
        return dict(pid=self.pid.data_ptr(), ldp=self.ldp, ktab=self.ktab.data_ptr())

    def coarse(self):
        vec = 16 // self.esz
        mc, nc = self.m // 2, self.n // 2
        ldc = -(-nc // vec) * vec
        return mc, nc, ldc, mc * ldc


def call(name, T, **kw):
    from feanet_amd import _lib
    rec = _lib.launch(name, **kw)
    _lib.call(rec[0], T, *rec[1], torch.cuda.current_stream().cuda_stream)


def final(part, per, count):
    from feanet_amd import _lib
    sums = torch.zeros(count, dtype=torch.float64, device="cuda")
    _lib.call_raw("per_final", part.data_ptr(), per, sums.data_ptr(), count, torch.cuda.current_stream().cuda_stream)
    return sums.cpu().numpy()


def footprint(buf, n):
    """the valid part as fp64 numpy, after checking that it is finite and every pad is still NaN"""
    h = buf.cpu().numpy()
    assert np.isnan(h[..., n:]).all(), "a pad column was written"
    assert np.isfinite(h[..., :n]).all(), "a node was not written, or a pad value was read"
    return h[..., :n].astype(np.float64)


def check(op, suf, got, ref, S, terms):
    bound = 2 * terms * U[suf] * S
    err = np.abs(got - ref)
    worst = (err / np.maximum(bound, np.finfo(np.float64).tiny)).max()
    print(f"{op} {suf} {got.shape}: worst |got - ref| / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{op} {suf}: {worst:.3f} bounds"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ----------------------------------------------------------------------------- kernels
def run_sweep(t, u, f, nb=B, out=None):
    out = t.empty(nb) if out is None else out
    call("per_sweep", t.T, u=None if u is None else u.data_ptr(), f=f.data_ptr(), out=out.data_ptr(), **t.stencil(),
         omd=t.omd.data_ptr(), B=nb, **t.geom())
    return out


def run_apply(t, p, nb=B, part=True):
    y = t.empty(nb)
    pt = torch.full((2 * nb * t.per,), float("nan"), dtype=torch.float64, device="cuda") if part else None
    call("per_apply", t.T, p=p.data_ptr(), y=y.data_ptr(), part=None if pt is None else pt.data_ptr(), **t.stencil(),
         B=nb, **t.geom())
    return y, pt


def run_reduce(t, a, b, nb=B):
    pt = torch.full((nb * t.per,), float("nan"), dtype=torch.float64, device="cuda")
    call("per_reduce", t.T, a=a.data_ptr(), b=None if b is None else b.data_ptr(), part=pt.data_ptr(), B=nb, **t.geom())
    return pt


def run_restrict(t, u, f, nb=B):
    mc, nc, ldc, bsc = t.coarse()
    fc = t.empty(nb, mc, ldc)
    call("per_residual_restrict", t.T, u=None if u is None else u.data_ptr(), f=f.data_ptr(), fc=fc.data_ptr(),
         **t.stencil(), B=nb, **t.geom(), ldc=ldc, bstridec=bsc)
    return fc


def run_prolong(t, ec, u, nb=B):
    mc, nc, ldc, bsc = t.coarse()
    call("per_prolong_add", t.T, ec=ec.data_ptr(), u=u.data_ptr(), B=nb, **t.geom(), ldc=ldc, bstridec=bsc)
    return u


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", SHAPES)
def test_apply_and_reduce(m, n, suf):
    """y = K p within 2 (9 + 2) u_T S; the partials of p . y, of sum y and of the reduce kernel against fp64 sums of
    the device's own values, within the rounding of N double additions and one product; sample b of the B = 3 call
    equals its own B = 1 call bit for bit, partial sums included."""
    t = Torus(m, n, suf)
    ph, pd = t.field(1)
    y, part = run_apply(t, pd)
    got = footprint(y, n)
    check("apply", suf, got, pf.apply_own(ph, t.pid_np, t.ktab_np), pf.apply_own(ph, t.pid_np, t.ktab_np, True), 9 + 2)
    assert np.isnan(footprint(pd, n)).sum() == 0
    y2, none = run_apply(t, pd, part=False)
    assert none is None and torch.equal(y2[..., :n], y[..., :n])
    N = m * n
    sums = final(part, t.per, 2 * B).reshape(B, 2)
    assert np.isfinite(part.cpu().numpy()).all()
    flat = lambda a: a.reshape(B, -1)
    assert (np.abs(sums[:, 0] - flat(ph * got).sum(1)) <= (N + 2) * 2.0 ** -53 * flat(np.abs(ph * got)).sum(1)).all()
    assert (np.abs(sums[:, 1] - flat(got).sum(1)) <= (N + 2) * 2.0 ** -53 * flat(np.abs(got)).sum(1)).all()
    qh, qd = t.field(2)
    for b_h, b_d in ((qh, qd), (None, None)):
        pt = run_reduce(t, pd, b_d)
        terms = ph * qh if b_h is not None else ph
        s = final(pt, t.per, B)
        assert (np.abs(s - flat(terms).sum(1)) <= (N + 2) * 2.0 ** -53 * flat(np.abs(terms)).sum(1)).all()
        for b in range(B):
            one = run_reduce(t, pd[b:b + 1].clone(), None if b_d is None else b_d[b:b + 1].clone(), nb=1)
            assert torch.equal(one, pt[b * t.per:(b + 1) * t.per])
    for b in range(B):
        y1, p1 = run_apply(t, pd[b:b + 1].clone(), nb=1)
        assert np.array_equal(bits(y1[..., :n].cpu().numpy()), bits(y[b:b + 1, :, :n].cpu().numpy()))
        assert torch.equal(p1, part[2 * b * t.per:2 * (b + 1) * t.per])


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", SHAPES)
def test_sweep(m, n, suf):
    """out = u + omd (f - K u): S = |omd| (|f| + S_K) + |u|, the residual's 9 + 2 terms and two more; the zero guess;
    B = 1 inside a B = 3 buffer leaves the other samples alone; batch independence."""
    t = Torus(m, n, suf)
    uh, ud = t.field(3)
    fh, fd = t.field(4)
    omd = t.omd_np.astype(np.float64)[t.pid_np]
    out = run_sweep(t, ud, fd)
    ref = omd * (fh - pf.apply_own(uh, t.pid_np, t.ktab_np)) + uh
    S = np.abs(omd) * (np.abs(fh) + pf.apply_own(uh, t.pid_np, t.ktab_np, True)) + np.abs(uh)
    check("sweep", suf, footprint(out, n), ref, S, 9 + 4)
    zero = run_sweep(t, None, fd)
    check("zero sweep", suf, footprint(zero, n), omd * fh, np.abs(omd * fh), 9 + 4)
    keep = torch.full_like(out, 7.0)
    run_sweep(t, ud, fd, nb=1, out=keep)
    assert torch.equal(keep[0, :, :n], out[0, :, :n]) and (keep[1:] == 7.0).all() and (keep[0, :, n:] == 7.0).all()
    for b in range(1, B):
        one = run_sweep(t, ud[b:b + 1].clone(), fd[b:b + 1].clone(), nb=1)
        assert np.array_equal(bits(one[..., :n].cpu().numpy()), bits(out[b:b + 1, :, :n].cpu().numpy()))


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", EVEN)
def test_residual_restrict_and_prolong(m, n, suf):
    """fc = R (f - K u): S = R (|f| + S_K), 9 + 2 terms of the residual and 9 of the restriction; u += R^T ec:
    S = |u| + R^T |ec|, at most four additions, the weight and the sum."""
    t = Torus(m, n, suf)
    mc, nc, ldc, bsc = t.coarse()
    uh, ud = t.field(5)
    fh, fd = t.field(6)
    fc = run_restrict(t, ud, fd)
    ref = pf.restrict(fh - pf.apply_own(uh, t.pid_np, t.ktab_np))
    S = pf.restrict(np.abs(fh) + pf.apply_own(uh, t.pid_np, t.ktab_np, True))
    check("residual_restrict", suf, footprint(fc, nc), ref, S, 9 + 9 + 2)
    fz = run_restrict(t, None, fd)
    check("zero residual_restrict", suf, footprint(fz, nc), pf.restrict(fh), pf.restrict(fh, True), 9 + 9 + 2)
    for b in range(B):
        one = run_restrict(t, ud[b:b + 1].clone(), fd[b:b + 1].clone(), nb=1)
        assert np.array_equal(bits(one[..., :nc].cpu().numpy()), bits(fc[b:b + 1, :, :nc].cpu().numpy()))
    eh, ed = t.field(7, m=mc, n=nc, ld=ldc)
    before = ud.clone()
    run_prolong(t, ed, ud)
    check("prolong_add", suf, footprint(ud, n), uh + pf.prolong(eh), np.abs(uh) + pf.prolong(eh, True), 4 + 2)
    keep = before.clone()
    run_prolong(t, ed, keep, nb=1)
    assert torch.equal(keep[0, :, :n], ud[0, :, :n]) and torch.equal(keep[1:, :, :n], before[1:, :, :n])


def test_argument_checks():
    """an odd extent in residual_restrict / prolong_add, out == u, a short pitch: FEA_EINVAL, nothing is launched"""
    from feanet_amd import effective_conductivity
    t = Torus(12, 16, "f64")
    _, ud = t.field(1)
    _, fd = t.field(2)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        call("per_residual_restrict", t.T, u=ud.data_ptr(), f=fd.data_ptr(), fc=t.empty().data_ptr(), **t.stencil(),
             B=B, m=11, n=16, ld=t.ld, bstride=t.bs, ldc=8, bstridec=t.bs)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        call("per_prolong_add", t.T, ec=fd.data_ptr(), u=ud.data_ptr(), B=B, m=12, n=15, ld=t.ld, bstride=t.bs, ldc=8,
             bstridec=t.bs)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        run_sweep(t, ud, fd, out=ud)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        call("per_apply", t.T, p=ud.data_ptr(), y=fd.data_ptr(), part=None, **t.stencil(), B=B, m=12, n=16, ld=15,
             bstride=t.bs)
    img = pr.six_discs(12, 16)
    with pytest.raises(ValueError, match="method"):
        effective_conductivity(img, bc="periodic", method="mg")
    with pytest.raises(ValueError, match="precond_dtype"):
        effective_conductivity(img, bc="periodic", precond_dtype=torch.float32)
    with pytest.raises(ValueError, match=r"\[rows, n\]"):
        effective_conductivity(np.zeros((2, 12, 16), np.uint8), bc="periodic")
    with pytest.raises(ValueError, match="unknown bc"):
        effective_conductivity(img, bc="neumann")


# ----------------------------------------------------------------------------- the cycle
@pytest.mark.parametrize("m, n", [(12, 16), (20, 66), (64, 64)])
def test_cycle_against_the_oracle(m, n):
    """M r in fp64 against the oracle's.  The allowance is 16 times the difference between the oracle run in float64
    and in np.longdouble, measured here on the CPU (the kernels fuse and reorder sums); DESIGN §18 records both."""
    from feanet_amd import PeriodicPCGSolver
    img = pr.image("random_elements", m, n)
    r = pf.mean_free(np.random.default_rng([11, m, n]).standard_normal((2, m, n)))
    ref = pf.Oracle(img, PROP).cycle(r)
    wide = pf.Oracle(img, PROP, dt=np.longdouble).cycle(r.astype(np.longdouble))
    measured = float(np.abs(ref - wide).max())
    s = PeriodicPCGSolver(n, rows=m, phase=img, prop=PROP, batch=2)
    got = s.precondition(torch.from_numpy(r).cuda()).cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"cycle {m} x {n}: |device - oracle| = {err:.3e}, oracle float64 vs longdouble {measured:.3e}, "
          f"max|M r| = {np.abs(ref).max():.3e}, levels {[(L.m, L.n) for L in s.levels]}")
    assert [(L.m, L.n) for L in s.levels] == [p.shape for p in pf.Oracle(img, PROP).pids]
    assert measured > 0 and err <= 16 * measured


# ----------------------------------------------------------------------------- solves
@functools.lru_cache(maxsize=None)
def dense(name, m, n, prop):
    return pf.homogenize_image(name, m, n, prop)


def both_routes(img, prop, **kw):
    from feanet_amd import effective_conductivity
    e = effective_conductivity(img, prop=prop, bc="periodic", route="energy", rtol=RTOL, **kw)
    f = effective_conductivity(img, prop=prop, bc="periodic", route="flux", rtol=RTOL, **kw)
    return e, f


@pytest.mark.parametrize("name, m, n, prop", [("six_discs", 32, 48, (1, 20)), ("offcentre_disc", 64, 64, (1, 1000))])
def test_solve_against_the_dense_reference(name, m, n, prop):
    """K_eff of both routes within 100 rtol max|K| of the dense reference on the same table; all flags 1; at most the
    oracle's iterations plus 2; mean_grad is the identity; route_gap within the dense pipeline's own defect."""
    img = pr.image(name, m, n)
    ref = dense(name, m, n, prop)
    _, its, flags, _ = pf.Oracle(img, prop, coarsen="stiff").pcg(rtol=RTOL)
    e, f = both_routes(img, prop, coarsen="stiff")
    scale = np.abs(ref["K_E"]).max()
    print(f"{name} {m} x {n} {prop}: iterations {e.iterations} (oracle {its}), |K_E - dense| = "
          f"{np.abs(e.K_eff - ref['K_E']).max():.2e}, |K_flux - dense| = {np.abs(f.K_eff - ref['K_flux']).max():.2e}, "
          f"route gap {e.route_gap:.3e} (dense {ref['gap']:.3e})")
    assert (flags == 1).all() and (e.flags == 1).all() and (f.flags == 1).all() and e.converged and f.converged
    assert (e.iterations <= its + 2).all() and np.array_equal(e.iterations, f.iterations)
    assert np.abs(e.K_eff - ref["K_E"]).max() <= 100 * RTOL * scale
    assert np.abs(f.K_eff - ref["K_flux"]).max() <= 100 * RTOL * scale
    assert np.array_equal(e.K_eff_flux, f.K_eff) and e.K_eff[0, 1] == e.K_eff[1, 0]
    assert np.abs(f.mean_grad - np.eye(2)).max() <= 1e-12
    assert abs(e.route_gap - ref["gap"]) <= 2 * 100 * RTOL
    assert e.sensitivity.shape == (3, m, n) and e.sensitivity.dtype == torch.float64


def test_laminate_on_the_device():
    """stripes 12 x 16 (1, 20): diag(arithmetic mean, harmonic mean) = diag(10.5, 2 / 1.05); the row load case starts
    solved; the Dirichlet bound on the same image is far above."""
    from feanet_amd import effective_conductivity
    img = pr.stripes(12, 16)
    e, f = both_routes(img, (1, 20))
    K = e.K_eff
    assert abs(K[0, 0] - 10.5) <= 1e-8 and abs(K[1, 1] - 2 / 1.05) <= 1e-8
    assert max(abs(K[0, 1]), abs(K[1, 0])) <= 1e-8 * np.abs(K).max()
    # the flux route carries the float32 table's Hill defect, 7.2e-7 on K[1, 1] here, in the dense pipeline as well
    # (DESIGN §18): it is held to that pipeline's value instead, and to the laminate within the defect
    ref = dense("stripes", 12, 16, (1, 20))
    assert np.abs(f.K_eff - ref["K_flux"]).max() <= 100 * RTOL * np.abs(ref["K_flux"]).max()
    assert np.abs(f.K_eff - np.diag([10.5, 2 / 1.05])).max() <= 2 * ref["gap"] * 10.5
    assert e.iterations[0] == 0 and e.iterations[1] > 0 and (e.flags == 1).all()
    d = effective_conductivity(img, prop=(1, 20), bc="dirichlet", route="energy", rtol=RTOL)
    assert d.K_eff[1, 1] > 7
    assert np.array_equal(d.K_eff, effective_conductivity(img, prop=(1, 20), route="energy", rtol=RTOL).K_eff)


def test_roll_invariance():
    """the cell is a torus: K_eff of the image rolled by (3, 5) elements is K_eff of the image, within 100 rtol"""
    from feanet_amd import effective_conductivity
    img = pr.six_discs(32, 48)
    a = effective_conductivity(img, bc="periodic", route="energy", rtol=RTOL)
    b = effective_conductivity(np.roll(img, (3, 5), (0, 1)), bc="periodic", route="energy", rtol=RTOL)
    assert a.converged and b.converged
    assert np.abs(a.K_eff - b.K_eff).max() <= 100 * RTOL * np.abs(a.K_eff).max()
    assert np.abs(a.K_eff_flux - b.K_eff_flux).max() <= 100 * RTOL * np.abs(a.K_eff).max()


def test_graph_replay_and_reloading_give_the_same_bits():
    """graph=True (eager block, captured block, replays) and graph=False; a second right-hand side loaded into a used
    solver and the same right-hand side in a fresh one."""
    from feanet_amd import PeriodicPCGSolver
    m, n = 20, 66
    img = pr.six_discs(m, n)
    kw = dict(rows=m, phase=img, prop=PROP, batch=2)
    g = PeriodicPCGSolver(n, graph=True, **kw)
    e = PeriodicPCGSolver(n, graph=False, **kw)
    xg, xe = g.solve(rtol=RTOL), e.solve(rtol=RTOL)
    assert len(g._graphs) >= 1 and len(e._graphs) == 0 and g.iterations.min() > 16
    assert torch.equal(xg, xe) and np.array_equal(g.iterations, e.iterations) and (g.flags == 1).all()
    assert np.array_equal(np.array(g.history), np.array(e.history))
    b2 = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 1, m, n))).cuda()
    x2 = g.solve(b2, rtol=RTOL)
    fresh = PeriodicPCGSolver(n, graph=True, **kw)
    assert torch.equal(x2, fresh.solve(b2, rtol=RTOL)) and np.array_equal(g.iterations, fresh.iterations)
    assert abs(float(x2.sum())) <= 1e-10 * float(x2.abs().sum())
    # a frozen sample does not depend on its neighbour: sample 0 next to a zero right-hand side (solved at once)
    b3 = b2.clone()
    b3[1] = 0
    x3 = fresh.solve(b3, rtol=RTOL)
    assert torch.equal(x3[0], x2[0]) and fresh.iterations[1] == 0 and fresh.flags[1] == 1 and (x3[1] == 0).all()


def test_fp32_solve():
    """fp32, six_discs 32 x 48, rtol 1e-5: the K_eff error against the dense reference is allowed four times that of
    the float32 numpy oracle's iterates, measured here on the CPU (DESIGN §18 records it)."""
    from feanet_amd import effective_conductivity
    m, n = 32, 48
    img = pr.six_discs(m, n)
    ref = dense("six_discs", m, n, PROP)
    x, its, flags, _ = pf.Oracle(img, PROP, dt=np.float32).pcg(rtol=1e-5)
    o = pf.routes_of(x, img, PROP)
    measured = max(np.abs(o["K_E"] - ref["K_E"]).max(), np.abs(o["K_flux"] - ref["K_flux"]).max())
    e = effective_conductivity(img, prop=PROP, bc="periodic", route="energy", dtype=torch.float32, rtol=1e-5)
    err = max(np.abs(e.K_eff - ref["K_E"]).max(), np.abs(e.K_eff_flux - ref["K_flux"]).max())
    print(f"fp32: device error {err:.3e}, float32 oracle error {measured:.3e}, iterations {e.iterations} "
          f"(oracle {its})")
    assert (flags == 1).all() and e.converged and (e.iterations <= its + 2).all()
    assert err <= 4 * measured


def test_effective_conductivity_torch_backward_periodic():
    """Backward against central differences in k1, 20 +/- 0.25, six discs at 32 x 32, as test_gpu_energy.py does for
    the Dirichlet problem: the truncation of the difference measured with dense CPU solves on the same table, allowed
    twice, plus the solves' 100 rtol terms."""
    from feanet_amd import effective_conductivity_torch
    m = n = 32
    img = pr.six_discs(m, n)
    ref = dense("six_discs", m, n, PROP)
    hi_d, lo_d = pf.homogenize(img, (1, 20.25)), pf.homogenize(img, (1, 19.75))
    trunc = np.abs((hi_d["K_E"] - lo_d["K_E"]) / 0.5 - ref["dK"][1]).max()
    tol = 2 * trunc + 2 * 100 * RTOL * np.abs(ref["K_E"]).max() / 0.5 + 100 * RTOL * np.abs(ref["dK"][1]).max()
    prop = torch.tensor([1.0, 20.0], dtype=torch.float64, device="cuda", requires_grad=True)
    K = effective_conductivity_torch(img, prop, rtol=RTOL, bc="periodic")
    assert K.shape == (2, 2) and K.is_cuda and K.requires_grad
    assert np.abs(K.detach().cpu().numpy() - ref["K_E"]).max() <= 100 * RTOL * np.abs(ref["K_E"]).max()
    hi = effective_conductivity_torch(img, torch.tensor([1.0, 20.25]), rtol=RTOL, bc="periodic")
    lo = effective_conductivity_torch(img, torch.tensor([1.0, 19.75]), rtol=RTOL, bc="periodic")
    quotient = ((hi - lo) / 0.5).numpy()
    for i, j in ((0, 0), (0, 1), (1, 1)):
        g, = torch.autograd.grad(K[i, j], prop, retain_graph=True)
        g = g.cpu().numpy()
        print(f"dK[{i}, {j}] / dprop = {g}, difference quotient in k1 {quotient[i, j]:.9e} (truncation {trunc:.2e}, "
              f"allowed {tol:.2e})")
        assert abs(g[1] - quotient[i, j]) <= tol
        assert abs(g[0] - ref["dK"][0][i, j]) <= 100 * RTOL * np.abs(ref["dK"][0]).max()
