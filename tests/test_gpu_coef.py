"""Element coefficient fields on the device: every fea_coef_* kernel against the numpy oracle of
coef_ref.py within the absolute-companion bound, their write footprint and batch independence, and
effective_conductivity_field / CoefPeriodicPCGSolver against dense solves.

The kernel tests use a lognormal field (sigma 1, rounded to the kernel's type), B = 3, the pad columns of every field
and of k pre-filled with NaN.

The bounds.  |got - ref64| <= 2 (ops + 2) u_T S, ref64 the fixed expression evaluated in fp64 at the values the kernel
reads, S the same expression with every value replaced by its absolute value and every subtraction by an addition,
ops the number of rounded operations on the longest path from an input to the result (each contributes a factor
(1 + delta), |delta| <= u_T; the factor 2 and the + 2 absorb the second-order terms and a fused multiply-add's
different but never larger rounding, as in §18):
  apply   a difference (1), (d + d) (2), + 2 d (3; the doubling is exact), k * t (4), the pair sum (5), the sum of the
          pairs (6), the constant 1/6 rounded to T (7), the product with it (8):                       ops = 8
  sweep   the residual f - K u (8 + 1 = 9); the weight: k + k (1), the sum of the pairs (2), the constant 2/3 (3), the
          product with it (4), omega rounded to T (5), the division (6); w * r multiplies the two paths
          (9 + 6 + 1 = 16), + u (17), and one more for a division that is within one ulp instead of half:  ops = 18
  restrict  the residual (9), nine weighted terms accumulated (exact weights, 9 additions):             ops = 18
"""
import numpy as np
import pytest
import torch

import coef_ref as cf
import periodic_ref as pf
import phase_ref as pr

pytestmark = pytest.mark.gpu

SUFS = ["f64", "f32"]
DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
ESZ = {"f32": 4, "f64": 8}
B = 3
RTOL = 1e-10
# the smallest m at n = 16 for which fea_per_parts shows more than one row task (the same for both types: one strip)
M_TASKS = next(m for m in range(2, 64) if pf.parts(m, 16, 8) > 1 and pf.parts(m, 16, 4) > 1)
EVEN = [(2, 2), (4, 6), (6, 10), (12, 16), (20, 66), (32, 130), (6, 258)]
SHAPES = EVEN + [(5, 7), (M_TASKS, 16)]
WORST = {}


# ----------------------------------------------------------------------------- torus buffers
class Cell:
    """The level's operands on the device: NaN in every pad column of the fields and of k."""

    def __init__(self, m, n, suf):
        self.m, self.n, self.suf, self.T = m, n, suf, DT[suf]
        vec = 16 // ESZ[suf]
        self.esz, self.ld = ESZ[suf], -(-n // vec) * vec
        self.bs = m * self.ld
        self.k_np = cf.lognormal(m, n, 1.0).astype(NP[suf])
        self.k64 = self.k_np.astype(np.float64)
        self.k = self.buffer(self.k_np[None])[0]
        self.per = pf.parts(m, n, self.esz)

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

    def coef(self):
        return dict(k=self.k.data_ptr(), ldk=self.ld)

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


def check(op, suf, got, ref, S, ops):
    bound = 2 * (ops + 2) * U[suf] * S
    err = np.abs(got - ref)
    worst = (err / np.maximum(bound, np.finfo(np.float64).tiny)).max()
    WORST[op, suf] = max(WORST.get((op, suf), 0.0), worst)
    print(f"{op} {suf} {got.shape}: worst |got - ref| / bound = {worst:.3f} (so far {WORST[op, suf]:.3f})")
    assert (err <= bound).all(), f"{op} {suf}: {worst:.3f} bounds"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b, n):
    return np.array_equal(bits(a[..., :n].cpu().numpy()), bits(b[..., :n].cpu().numpy()))


# ----------------------------------------------------------------------------- kernels
def run_sweep(t, u, f, nb=B, out=None, omega=cf.OMEGA):
    out = t.empty(nb) if out is None else out
    call("coef_sweep", t.T, u=None if u is None else u.data_ptr(), f=f.data_ptr(), out=out.data_ptr(), **t.coef(),
         omega=omega, B=nb, **t.geom())
    return out


def run_apply(t, p, nb=B, part=True):
    y = t.empty(nb)
    pt = torch.full((2 * nb * t.per,), float("nan"), dtype=torch.float64, device="cuda") if part else None
    call("coef_apply", t.T, p=p.data_ptr(), y=y.data_ptr(), part=None if pt is None else pt.data_ptr(), **t.coef(),
         B=nb, **t.geom())
    return y, pt


def run_restrict(t, u, f, nb=B, fc=None):
    mc, nc, ldc, bsc = t.coarse()
    fc = t.empty(nb, mc, ldc) if fc is None else fc
    call("coef_residual_restrict", t.T, u=None if u is None else u.data_ptr(), f=f.data_ptr(), fc=fc.data_ptr(),
         **t.coef(), B=nb, **t.geom(), ldc=ldc, bstridec=bsc)
    return fc


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", SHAPES)
def test_apply(m, n, suf):
    """y = K p within 2 (8 + 2) u_T S; K 1 = 0 exactly; the partials of p . y and of sum y against fp64 sums of the
    device's own values, within the rounding of N double additions and one product; sample b of the B = 3 call equals
    its own B = 1 call bit for bit, partial sums included; only the m x n nodes are written."""
    t = Cell(m, n, suf)
    ph, pd = t.field(1)
    y, part = run_apply(t, pd)
    got = footprint(y, n)
    check("apply", suf, got, cf.apply_diff(ph, t.k64), cf.apply_diff(ph, t.k64, absolute=True), cf.OPS_APPLY)
    ones = t.buffer(np.full((B, m, n), -3.7, NP[suf]))
    assert (footprint(run_apply(t, ones, part=False)[0], n) == 0.0).all()
    y2, none = run_apply(t, pd, part=False)
    assert none is None and torch.equal(y2[..., :n], y[..., :n])
    N = m * n
    sums = final(part, t.per, 2 * B).reshape(B, 2)
    assert np.isfinite(part.cpu().numpy()).all()
    flat = lambda a: a.reshape(B, -1)
    assert (np.abs(sums[:, 0] - flat(ph * got).sum(1)) <= (N + 2) * 2.0 ** -53 * flat(np.abs(ph * got)).sum(1)).all()
    assert (np.abs(sums[:, 1] - flat(got).sum(1)) <= (N + 2) * 2.0 ** -53 * flat(np.abs(got)).sum(1)).all()
    for b in range(B):
        y1, p1 = run_apply(t, pd[b:b + 1].clone(), nb=1)
        assert same_bits(y1, y[b:b + 1], n)
        assert torch.equal(p1, part[2 * b * t.per:2 * (b + 1) * t.per])
    keep = torch.full_like(y, 7.0)
    call("coef_apply", t.T, p=pd.data_ptr(), y=keep.data_ptr(), part=None, **t.coef(), B=1, **t.geom())
    assert torch.equal(keep[0, :, :n], y[0, :, :n]) and (keep[1:] == 7.0).all() and (keep[0, :, n:] == 7.0).all()


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", SHAPES)
def test_sweep(m, n, suf):
    """out = u + (omega / d) (f - K u) within 2 (18 + 2) u_T S, S = |w| (|f| + S_K) + |u|; the zero guess; another
    omega; B = 1 inside a B = 3 buffer of sentinels leaves everything else alone; batch independence."""
    t = Cell(m, n, suf)
    uh, ud = t.field(3)
    fh, fd = t.field(4)
    out = run_sweep(t, ud, fd)
    om = float(NP[suf](cf.OMEGA))
    check("sweep", suf, footprint(out, n), cf.sweep(uh, fh, t.k64, om), cf.sweep_companion(uh, fh, t.k64, om),
          cf.OPS_SWEEP)
    zero = run_sweep(t, None, fd)
    check("zero sweep", suf, footprint(zero, n), cf.sweep(None, fh, t.k64, om), cf.sweep_companion(None, fh, t.k64, om),
          cf.OPS_SWEEP)
    other = run_sweep(t, ud, fd, omega=0.5)
    check("sweep", suf, footprint(other, n), cf.sweep(uh, fh, t.k64, 0.5), cf.sweep_companion(uh, fh, t.k64, 0.5),
          cf.OPS_SWEEP)
    keep = torch.full_like(out, 7.0)
    run_sweep(t, ud, fd, nb=1, out=keep)
    assert torch.equal(keep[0, :, :n], out[0, :, :n]) and (keep[1:] == 7.0).all() and (keep[0, :, n:] == 7.0).all()
    for b in range(1, B):
        one = run_sweep(t, ud[b:b + 1].clone(), fd[b:b + 1].clone(), nb=1)
        assert same_bits(one, out[b:b + 1], n)
        one = run_sweep(t, None, fd[b:b + 1].clone(), nb=1)
        assert same_bits(one, zero[b:b + 1], n)


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", EVEN)
def test_residual_restrict(m, n, suf):
    """fc = R (f - K u) within 2 (18 + 2) u_T S, S = R (|f| + S_K); the zero guess; the residual is the apply kernel's
    (R applied to f - y of the device's own y, within the restriction's own rounding); batch independence; B = 1 inside
    a buffer of sentinels."""
    t = Cell(m, n, suf)
    mc, nc, ldc, bsc = t.coarse()
    uh, ud = t.field(5)
    fh, fd = t.field(6)
    fc = run_restrict(t, ud, fd)
    ref = pf.restrict(fh - cf.apply_diff(uh, t.k64))
    S = pf.restrict(np.abs(fh) + cf.apply_diff(uh, t.k64, absolute=True))
    got = footprint(fc, nc)
    check("residual_restrict", suf, got, ref, S, cf.OPS_RESTRICT)
    fz = run_restrict(t, None, fd)
    check("zero residual_restrict", suf, footprint(fz, nc), pf.restrict(fh), pf.restrict(fh, True), cf.OPS_RESTRICT)
    y = footprint(run_apply(t, ud, part=False)[0], n)
    res = (fh - y).astype(NP[suf]).astype(np.float64)   # the residual as the kernel holds it: one rounded subtraction
    assert (np.abs(got - pf.restrict(res)) <= 2 * (9 + 2) * U[suf] * pf.restrict(res, True)).all()
    for b in range(B):
        one = run_restrict(t, ud[b:b + 1].clone(), fd[b:b + 1].clone(), nb=1)
        assert same_bits(one, fc[b:b + 1], nc)
    keep = torch.full_like(fc, 7.0)
    run_restrict(t, ud, fd, nb=1, fc=keep)
    assert torch.equal(keep[0, :, :nc], fc[0, :, :nc]) and (keep[1:] == 7.0).all() and (keep[0, :, nc:] == 7.0).all()


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("m, n", EVEN)
def test_coarsen(m, n, suf):
    """fea_coef_coarsen against numpy: the arithmetic mean bit for bit, the harmonic and the geometric mean (computed in
    double, rounded once) within 4 u_T of the value; only the (m / 2) x (n / 2) elements are written."""
    t = Cell(m, n, suf)
    mc, nc, ldc, _ = t.coarse()
    for rule in cf.RULES:
        kc = torch.full((mc, ldc), float("nan"), dtype=t.T, device="cuda")
        call("coef_coarsen", t.T, k=t.k.data_ptr(), ldk=t.ld, kc=kc.data_ptr(), ldkc=ldc, m=m, n=n,
             rule=cf.RULES.index(rule))
        got = kc.cpu().numpy()
        assert np.isnan(got[:, nc:]).all()
        ref = cf.coarsen(t.k_np, rule, NP[suf])
        if rule == "arithmetic":
            assert np.array_equal(bits(got[:, :nc]), bits(ref))
        else:
            err = np.abs(got[:, :nc].astype(np.float64) - ref.astype(np.float64)) / ref.astype(np.float64)
            print(f"coarsen {rule} {suf} {m} x {n}: worst relative difference {err.max() / U[suf]:.2f} u_T")
            assert (err <= 4 * U[suf]).all()


def test_argument_checks():
    """an odd extent in residual_restrict and coarsen, out == u, a short pitch, m = 1, a null field: FEA_EINVAL, nothing
    is launched; the host layer's own refusals"""
    from feanet_amd import CoefPeriodicPCGSolver, effective_conductivity_field, effective_conductivity_field_torch
    t = Cell(12, 16, "f64")
    _, ud = t.field(1)
    _, fd = t.field(2)
    bad = pytest.raises(RuntimeError, match="invalid arguments")
    with bad:
        call("coef_residual_restrict", t.T, u=ud.data_ptr(), f=fd.data_ptr(), fc=t.empty().data_ptr(), **t.coef(),
             B=B, m=11, n=16, ld=t.ld, bstride=t.bs, ldc=8, bstridec=t.bs)
    with bad:
        call("coef_coarsen", t.T, k=t.k.data_ptr(), ldk=t.ld, kc=t.empty().data_ptr(), ldkc=8, m=12, n=15, rule=0)
    with bad:
        run_sweep(t, ud, fd, out=ud)
    with bad:
        run_sweep(t, ud, fd, out=fd)
    with bad:
        call("coef_apply", t.T, p=ud.data_ptr(), y=fd.data_ptr(), part=None, **t.coef(), B=B, m=12, n=16, ld=15,
             bstride=t.bs)
    with bad:
        call("coef_apply", t.T, p=ud.data_ptr(), y=fd.data_ptr(), part=None, **t.coef(), B=B, m=1, n=16, ld=t.ld,
             bstride=t.bs)
    with bad:
        call("coef_apply", t.T, p=ud.data_ptr(), y=fd.data_ptr(), part=None, k=None, ldk=t.ld, B=B, **t.geom())
    k = cf.lognormal(12, 16)
    with pytest.raises(ValueError, match="positive"):
        effective_conductivity_field(np.where(k > 1, k, 0.0))
    with pytest.raises(ValueError, match="positive"):
        CoefPeriodicPCGSolver(16, rows=12, coef=-k)
    with pytest.raises(ValueError, match="positive"):
        CoefPeriodicPCGSolver(16, rows=12, coef=np.where(k > 1, k, 1e-60), dtype=torch.float32)  # 0 once rounded
    with pytest.raises(ValueError, match="coarsen"):
        CoefPeriodicPCGSolver(16, rows=12, coef=k, coarsen="stiff")
    with pytest.raises(ValueError, match="12 x 16"):
        CoefPeriodicPCGSolver(16, rows=12, coef=k.T)
    with pytest.raises(ValueError, match="route"):
        effective_conductivity_field_torch(torch.from_numpy(k), route="flux")


# ----------------------------------------------------------------------------- solves
def effective_conductivity_field(*a, **kw):
    from feanet_amd import effective_conductivity_field as fn
    return fn(*a, **kw)


def both_routes(k, **kw):
    e = effective_conductivity_field(k, route="energy", rtol=RTOL, **kw)
    f = effective_conductivity_field(k, route="flux", rtol=RTOL, **kw)
    return e, f


def test_laminate_on_the_device():
    """columns of width 4 with the values 1, 3, 20, 7.5 at 12 x 16, energy route: diag(7.875, 2.6373626...) within
    100 rtol max|K|; the row load case starts solved"""
    e = effective_conductivity_field(cf.laminate(), route="energy", rtol=RTOL)
    v = np.array([1.0, 3.0, 20.0, 7.5])
    want = np.diag([v.mean(), 1.0 / (1.0 / v).mean()])
    print(f"laminate: K_E = {e.K_eff.tolist()}, iterations {e.iterations}")
    assert e.converged and (e.flags == 1).all() and e.iterations[0] == 0 and e.iterations[1] > 0
    assert np.abs(e.K_eff - want).max() <= 100 * RTOL * 7.875
    assert e.K_eff[0, 1] == e.K_eff[1, 0] and e.dK_dprop is None


def test_lognormal_solve_against_the_dense_reference():
    """lognormal, sigma 1, seed 0, 32 x 48: K_eff of both routes within 100 rtol max|K| of the dense reference; all
    flags 1; at most the numpy oracle's iterations plus 2 (test_coef_host.py checks that the oracle converges well
    inside max_iters); mean_grad is the identity; Hill's identity."""
    m, n = 32, 48
    k = cf.lognormal(m, n, 1.0, 0)
    ref = cf.homogenize_lognormal(m, n)
    _, its, flags, _ = cf.Oracle(k).pcg(rtol=RTOL)
    e, f = both_routes(k)
    scale = np.abs(ref["K_E"]).max()
    print(f"lognormal {m} x {n}: iterations {e.iterations} (oracle {its}), |K_E - dense| = "
          f"{np.abs(e.K_eff - ref['K_E']).max():.2e}, |K_flux - dense| = {np.abs(f.K_eff - ref['K_flux']).max():.2e}, "
          f"route gap {e.route_gap:.3e} (dense {ref['gap']:.3e}), hill {f.hill_defect}")
    assert (flags == 1).all() and (e.flags == 1).all() and (f.flags == 1).all() and e.converged and f.converged
    assert (e.iterations <= its + 2).all() and np.array_equal(e.iterations, f.iterations)
    assert np.abs(e.K_eff - ref["K_E"]).max() <= 100 * RTOL * scale
    assert np.abs(f.K_eff - ref["K_flux"]).max() <= 100 * RTOL * scale
    assert np.array_equal(e.K_eff_flux, f.K_eff) and e.K_eff[0, 1] == e.K_eff[1, 0]
    assert np.abs(f.mean_grad - np.eye(2)).max() <= 1e-12
    assert (f.hill_defect <= 2 * 100 * RTOL).all()
    assert e.sensitivity.shape == (3, m, n) and e.sensitivity.dtype == torch.float64 and e.dK_dprop is None
    assert effective_conductivity_field(k, route="energy", rtol=RTOL, fields=False).sensitivity is None


def test_image_as_a_field_against_the_exact_two_material_reference():
    """the 0/1 six_discs image at 32 x 48 with prop (1, 20) written as a field: periodic_ref.homogenize(exact=True),
    both routes, within 100 rtol max|K|; every coarsening rule reaches the same K_eff"""
    m, n = 32, 48
    img = pr.six_discs(m, n)
    ref = pf.homogenize(img, (1, 20), exact=True)
    k = cf.from_image(img, (1, 20))
    scale = np.abs(ref["K_E"]).max()
    e, f = both_routes(k)
    print(f"six_discs as a field: iterations {e.iterations}, |K_E - exact| = {np.abs(e.K_eff - ref['K_E']).max():.2e}")
    assert e.converged and f.converged
    assert np.abs(e.K_eff - ref["K_E"]).max() <= 100 * RTOL * scale
    assert np.abs(f.K_eff - ref["K_flux"]).max() <= 100 * RTOL * scale
    for rule in ("arithmetic", "harmonic"):
        r = effective_conductivity_field(k, route="energy", rtol=RTOL, coarsen=rule)
        assert r.converged and np.abs(r.K_eff - ref["K_E"]).max() <= 100 * RTOL * scale


def test_sensitivity_field():
    """the sensitivity [3, m, n] of the lognormal solve against the dense one; the yardstick is the fp64 numpy oracle's
    own distance from the dense field at the same rtol (3.1e-12 at max|sens| 8.0e-3), the device is allowed
    four times that"""
    m, n = 32, 48
    k = cf.lognormal(m, n, 1.0, 0)
    ref = cf.homogenize_lognormal(m, n)["sens"]
    x, _, flags, _ = cf.Oracle(k).pcg(rtol=RTOL)
    yard = np.abs(cf.routes_of(x, k)["sens"] - ref).max()
    e = effective_conductivity_field(k, route="energy", rtol=RTOL)
    err = np.abs(e.sensitivity.cpu().numpy() - ref).max()
    print(f"sensitivity: |device - dense| = {err:.3e}, oracle {yard:.3e}, max|sens| = {np.abs(ref).max():.3e}")
    assert (flags == 1).all() and yard > 0 and err <= 4 * yard


def test_effective_conductivity_field_torch_backward():
    """Backward against central differences in two elements at 16 x 16 (k_e +/- 0.1 k_e): the truncation of the
    difference measured with dense CPU solves, allowed twice, plus the solves' 100 rtol terms: the formula of
    test_effective_conductivity_torch_backward_periodic."""
    from feanet_amd import effective_conductivity_field_torch
    m = n = 16
    k = cf.lognormal(m, n, 1.0, 1)
    ref = cf.homogenize(k)
    comps = ((0, 0), (0, 1), (1, 1))
    kt = torch.tensor(k, dtype=torch.float64, device="cuda", requires_grad=True)
    K = effective_conductivity_field_torch(kt, rtol=RTOL)
    assert K.shape == (2, 2) and K.is_cuda and K.requires_grad
    assert np.abs(K.detach().cpu().numpy() - ref["K_E"]).max() <= 100 * RTOL * np.abs(ref["K_E"]).max()
    grads = [torch.autograd.grad(K[i, j], kt, retain_graph=True)[0].cpu().numpy() for i, j in comps]
    assert all(g.shape == (m, n) for g in grads)
    for R, C in ((3, 5), (12, 0)):
        step = 0.1 * k[R, C]
        hi, lo = k.copy(), k.copy()
        hi[R, C] += step
        lo[R, C] -= step
        taken = hi[R, C] - lo[R, C]
        qd = (cf.dense_k_eff(hi) - cf.dense_k_eff(lo)) / taken
        trunc = max(abs(qd[i, j] - ref["sens"][q, R, C]) for q, (i, j) in enumerate(comps))
        tol = 2 * trunc + 2 * 100 * RTOL * np.abs(ref["K_E"]).max() / taken + 100 * RTOL * np.abs(ref["sens"]).max()
        Kh = effective_conductivity_field_torch(torch.from_numpy(hi), rtol=RTOL)
        Kl = effective_conductivity_field_torch(torch.from_numpy(lo), rtol=RTOL)
        assert not Kh.is_cuda and not Kh.requires_grad
        quotient = ((Kh - Kl) / taken).numpy()
        for q, (i, j) in enumerate(comps):
            print(f"dK[{i}, {j}] / dk[{R}, {C}] = {grads[q][R, C]:.9e}, difference quotient {quotient[i, j]:.9e} "
                  f"(truncation {trunc:.2e}, allowed {tol:.2e})")
            assert abs(grads[q][R, C] - quotient[i, j]) <= tol
    # g00 s00 + (g01 + g10) s01 + g11 s11 for a full incoming gradient
    g = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64, device="cuda")
    full, = torch.autograd.grad(K, kt, grad_outputs=g)
    want = 1.0 * grads[0] + 5.0 * grads[1] + 4.0 * grads[2]
    assert np.abs(full.cpu().numpy() - want).max() <= 1e-14 * np.abs(want).max()
    with pytest.raises(RuntimeError, match="did not converge"):
        effective_conductivity_field_torch(kt, rtol=RTOL, max_iters=2)


def test_roll_invariance():
    """the cell is a torus: K_eff of the field rolled by (3, 5) elements is K_eff of the field, within 100 rtol"""
    k = cf.lognormal(32, 48, 1.0, 0)
    a = effective_conductivity_field(k, route="energy", rtol=RTOL)
    b = effective_conductivity_field(np.roll(k, (3, 5), (0, 1)), route="energy", rtol=RTOL)
    assert a.converged and b.converged
    assert np.abs(a.K_eff - b.K_eff).max() <= 100 * RTOL * np.abs(a.K_eff).max()
    assert np.abs(a.K_eff_flux - b.K_eff_flux).max() <= 100 * RTOL * np.abs(a.K_eff).max()


def test_graph_replay_and_reloading_give_the_same_bits():
    """graph=True (eager block, captured block, replays) and graph=False; a second right-hand side loaded into a used
    solver and the same right-hand side in a fresh one; the cycle against the oracle's."""
    from feanet_amd import CoefPeriodicPCGSolver
    m, n = 20, 66
    k = cf.lognormal(m, n, 1.0)
    kw = dict(rows=m, coef=k, batch=2)
    g = CoefPeriodicPCGSolver(n, graph=True, **kw)
    e = CoefPeriodicPCGSolver(n, graph=False, **kw)
    xg, xe = g.solve(rtol=RTOL), e.solve(rtol=RTOL)
    assert len(g._graphs) >= 1 and len(e._graphs) == 0 and g.iterations.min() > 16
    assert torch.equal(xg, xe) and np.array_equal(g.iterations, e.iterations) and (g.flags == 1).all()
    assert np.array_equal(np.array(g.history), np.array(e.history))
    b2 = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 1, m, n))).cuda()
    x2 = g.solve(b2, rtol=RTOL)
    fresh = CoefPeriodicPCGSolver(n, graph=True, **kw)
    assert torch.equal(x2, fresh.solve(b2, rtol=RTOL)) and np.array_equal(g.iterations, fresh.iterations)
    assert abs(float(x2.sum())) <= 1e-10 * float(x2.abs().sum())
    # the levels are the oracle's, and so is the right-hand side of the load cases
    o = cf.Oracle(k)
    assert [(L.m, L.n) for L in g.levels] == [x.shape for x in o.ks]
    for L, kl in zip(g.levels[1:], o.ks[1:]):
        assert np.abs(L.k[:, :L.n].cpu().numpy() - kl).max() <= 4 * U["f64"] * kl.max()
    assert np.abs(g.load_case_rhs().cpu().numpy() - o.rhs()).max() == 0.0


def test_fp32_solve():
    """fp32, lognormal 32 x 48, rtol 1e-5: the K_eff error against the dense reference is allowed four times that of
    the float32 numpy oracle's iterates, measured here on the CPU (DESIGN §19 records it)."""
    m, n = 32, 48
    k = cf.lognormal(m, n, 1.0, 0)
    ref = cf.homogenize_lognormal(m, n)
    x, its, flags, _ = cf.Oracle(k, dt=np.float32).pcg(rtol=1e-5)
    o = cf.routes_of(x, k.astype(np.float32).astype(np.float64))
    measured = max(np.abs(o["K_E"] - ref["K_E"]).max(), np.abs(o["K_flux"] - ref["K_flux"]).max())
    e = effective_conductivity_field(k, route="energy", dtype=torch.float32, rtol=1e-5)
    err = max(np.abs(e.K_eff - ref["K_E"]).max(), np.abs(e.K_eff_flux - ref["K_flux"]).max())
    print(f"fp32: device error {err:.3e}, float32 oracle error {measured:.3e}, iterations {e.iterations} "
          f"(oracle {its})")
    assert (flags == 1).all() and e.converged and (e.iterations <= its + 2).all()
    assert e.sensitivity.dtype == torch.float32
    assert err <= 4 * measured
