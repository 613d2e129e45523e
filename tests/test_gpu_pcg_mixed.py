"""GPU parity of the mixed-precision Krylov kernels (fea_pcg_*_f64f32) and of PCGSolver(dtype=float64,
precond_dtype=float32) against numpy: fp64 recurrences around OracleMultigrid(float32).step(0, float32(r s_b)).

Tolerances are the project's.  The fp64 outputs of the kernels: fields 1e-12 relative to max(1, max|expected|),
reduced scalars rtol 1e-12 (test_gpu_pcg.py's kernel test); the narrowed residual is float32(r s_b) bit for bit.  The
solver's preconditioner differs from the oracle's at fp32 rounding, so iterates and histories are held to
test_iterate_vs_numpy's fp32 bounds: the iterate after the first iteration within 2e-5, histories rtol 2e-3 with a
floor of 1e-6 of the initial residual.  Attainable accuracy: the numpy model reaches a true residual of at most
1.2e-12 ||r0|| at rtol = 1e-12; ten times that is the cap."""
import numpy as np
import pytest
import torch

from oracle import feanet_oracle as orc

pytestmark = pytest.mark.gpu

T64, T32 = torch.float64, torch.float32
RZ, RZ_PREV, PAP, ALPHA, BETA, RNORM, DONE, ITERS, EPS, RTOL, THRESH, ROW = range(12)
INIT, STEP_RZ, STEP_PAP, STEP_RR = range(4)


def close(out, ref, what, tol=1e-12):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{what}: scaled max err {err:.3e}")
    assert err <= tol, f"{what}: scaled max err {err:.3e} > {tol}"


def dot64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).reshape(a.shape[0], -1).sum(1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def scale_of(rn):
    """s_b of the specification: 2^-floor(log2 ||r0||); 1 for a zero or non-finite norm."""
    rn = np.asarray(rn, np.float64)
    ok = np.isfinite(rn) & (rn > 0)
    return np.where(ok, 2.0 ** -np.floor(np.log2(np.where(ok, rn, 1.0))), 1.0)


@pytest.fixture(params=[False, True], ids=["cached", "nt"])
def nt(request, monkeypatch):
    """FEANET_NT_BYTES=0 selects the nontemporal-store instantiations that otherwise run only on fields > 64 MiB."""
    if request.param:
        monkeypatch.setenv("FEANET_NT_BYTES", "0")
    return request.param


class Fields:
    """fp64 framed level-0 buffers next to fp32 ones of the same nodes (the solver's level allocator, both dtypes),
    with numpy I/O, and the numpy operator."""

    def __init__(self, n, B, problem, m=None, prop=(1, 20)):
        from feanet_amd import _lib, mesh_setup as ms
        from feanet_amd.solver import _Level
        m = n if m is None else m
        self.H, self.W, self.B = m + 1, n + 1, B
        self.ktab = ms.stencil_table(prop if problem == "interface" else None)
        if problem == "interface":
            full = ms.interface_pattern_map(n + 1)
            if m > n:      # a tall grid: the square's map repeated down the rows (any map of valid ids is a problem)
                full = full[np.arange(m + 1) % (n + 1)]
            r0 = max(n - m, 0) // 2
            self.pid_np = np.ascontiguousarray(full[r0:r0 + m + 1])
        else:
            self.pid_np = np.zeros((self.H, self.W), np.uint8)
        dev = torch.device("cuda")
        self.L = _Level(m, n, B, T64, dev, self.pid_np if problem == "interface" else None)
        self.L32 = _Level(m, n, B, T32, dev)
        self.kt = torch.from_numpy(self.ktab.reshape(-1, 9).astype(np.float64)).cuda()
        self.ntab = self.ktab.shape[0]
        self.geo = np.zeros((self.H, self.W))
        self.geo[1:-1, 1:-1] = 1
        self.per = int(_lib.lib().fea_pcg_parts(self.H, self.W, 8))
        self.part = torch.zeros(B * self.per, dtype=T64, device="cuda")
        self.sc = torch.zeros((B, 12), dtype=T64, device="cuda")
        self.sb = torch.full((B,), 7.0, dtype=T64, device="cuda")
        self.hist = torch.zeros((4, B), dtype=T64, device="cuda")
        self.bufs = {"z32": self.L32.a, "r32": self.L32.f}

    def lev(self, name):
        return self.L32 if name.endswith("32") else self.L

    def buf(self, name):
        if name not in self.bufs:
            self.bufs[name] = torch.zeros_like(self.L.a)
        return self.bufs[name]

    def put(self, name, arr):
        t = self.buf(name)
        self.lev(name).view(t).copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(t.dtype))

    def get(self, name):
        return self.lev(name).view(self.buf(name)).cpu().numpy()

    def raw(self, name):
        return self.buf(name).cpu().numpy()

    def framed32(self, arr):
        """The whole raw fp32 buffer that holds arr on its nodes and zeros everywhere else."""
        t = torch.zeros_like(self.L32.f)
        self.L32.view(t).copy_(torch.from_numpy(np.ascontiguousarray(arr, np.float32)))
        return t.cpu().numpy()

    def ptr(self, name):
        return self.buf(name).data_ptr()

    def kargs(self):
        return (None if self.L.pid is None else self.L.pid.data_ptr(), self.kt.data_ptr(), self.ntab)

    def geom(self):
        return self.L.geom() + (self.L32.ld, self.L32.bs)

    def rand(self, rng, dt=np.float64, interior=True):
        a = rng.standard_normal((self.B, self.H, self.W)).astype(dt)
        return np.where(self.geo != 0, a, dt(0)) if interior else a  # +0 outside (a * geo would leave -0 there)

    def K(self, v):
        return orc.knet_apply(np.asarray(v, np.float64), self.pid_np, self.ktab) * self.geo

    def sums(self):
        return self.part.view(self.B, self.per).sum(1).cpu().numpy()

    def step(self, step):
        from feanet_amd import _lib
        _lib.call_raw("pcg_scalar_step", self.part.data_ptr(), self.per, self.sc.data_ptr(), self.hist.data_ptr(),
                      self.hist.shape[0], self.B, step, None)
        return self.sc.cpu().numpy()


# (n, rows, B): 256 crosses the fp64 strip edge (128 columns); 512 crosses the fp32 frame's strip width (256), so four
# fp64 strips index one fp32 row; (160, 24) is a rectangle
SIZES = [(2, None, 1), (4, None, 3), (16, None, 3), (128, None, 1), (256, None, 3), (160, 24, 2), (512, None, 1),
         (32, 4096, 2), (32, 16384, 1), (32, 65536, 1)]
# the tall one-strip shapes and the row-task height they must reach (every other size runs 2-row tasks)
TALL = {(32, 4096): 2, (32, 16384): 8, (32, 65536): 32}


@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("n,m,B", SIZES, ids=lambda v: str(v))
def test_kernels_vs_numpy(problem, n, m, B, nt):
    """Each mixed kernel on seeded random framed inputs: fp64 fields and reduced sums against numpy on the widened
    inputs, the narrowed residual bit for bit, and not one element of the fp32 buffer written outside the interior."""
    from feanet_amd import _lib
    rng = np.random.default_rng(1000 * n + B)
    fr = Fields(n, B, problem, m=m)
    g = fr.geom()
    if (n, m) in TALL:
        from test_gpu_pcg import task_height
        assert task_height(fr.H, fr.W, 8) == TALL[(n, m)]
    cr = lambda name, *a: _lib.call_raw(name, *a, None)

    # --- narrow: s_b from the sample's RNORM (whatever its magnitude), r32 = float32(r s_b) on the interior
    r = fr.rand(rng)
    fr.put("r", r)
    rn = np.sqrt(dot64(r, r)) * np.array([1.0, 2.0 ** -37.3, 2.0 ** 50.6])[:B]
    fr.sc[:, RNORM] = torch.from_numpy(rn).cuda()
    cr("pcg_narrow_f64f32", fr.ptr("r"), fr.ptr("r32"), fr.sc.data_ptr(), fr.sb.data_ptr(), *g)
    sb = fr.sb.cpu().numpy()
    assert same_bits(sb, scale_of(rn)), (sb, scale_of(rn))
    assert ((rn * sb >= 1) & (rn * sb < 2)).all()
    assert same_bits(fr.get("r"), r), "r modified"
    assert same_bits(fr.raw("r32"), fr.framed32((r * sb[:, None, None]).astype(np.float32))), "narrow"

    # --- dot: partials of r . widen(z32)
    z = fr.rand(rng, np.float32)
    fr.put("z32", z)
    cr("pcg_dot_f64f32", fr.ptr("r"), fr.ptr("z32"), fr.part.data_ptr(), *g)
    np.testing.assert_allclose(fr.sums(), dot64(r, z), rtol=1e-12)

    # --- direction: p_out = widen(z32) + beta p_in, inputs untouched, partials of p_out . K p_out
    p = fr.rand(rng)
    beta = 0.37
    fr.put("p", p)
    fr.buf("q").zero_()
    fr.sc[:, BETA] = beta
    fr.sc[:, RZ] = 2.5
    cr("pcg_direction_f64f32", fr.ptr("z32"), fr.ptr("p"), fr.ptr("q"), *fr.kargs(), fr.sc.data_ptr(),
       fr.part.data_ptr(), *g)
    q = fr.get("q")
    q_ref = z.astype(np.float64) + beta * p
    close(q, q_ref, "direction")
    assert same_bits(fr.get("p"), p), "p_in modified"
    assert same_bits(fr.raw("z32"), fr.framed32(z)), "z32 modified"
    assert (q[:, 0] == 0).all() and (q[:, -1] == 0).all() and (q[:, :, 0] == 0).all() and (q[:, :, -1] == 0).all()
    pAp = dot64(q_ref, fr.K(q_ref))
    np.testing.assert_allclose(fr.sums(), pAp, rtol=1e-12)
    sc = fr.step(STEP_PAP)
    np.testing.assert_allclose(sc[:, ALPHA], 2.5 / pAp, rtol=1e-12)

    # --- update: x += alpha p, r -= alpha K p in fp64, r32 = float32(r_new s_b); a frozen sample is left alone
    alpha = 0.61
    fr.sc[:, ALPHA] = alpha
    x = fr.rand(rng, interior=False)
    fr.put("x", x)
    cr("pcg_update_f64f32", fr.ptr("q"), fr.ptr("x"), fr.ptr("r"), fr.ptr("r32"), *fr.kargs(), fr.sc.data_ptr(),
       fr.sb.data_ptr(), fr.part.data_ptr(), *g)
    x_ref = x + alpha * q * fr.geo
    r_new = r - alpha * fr.K(q)
    close(fr.get("x"), x_ref, "update x")
    close(fr.get("r"), r_new, "update r")
    assert same_bits(fr.get("q"), q)
    np.testing.assert_allclose(fr.sums(), dot64(r_new, r_new), rtol=1e-12)
    x1, r1, s1 = fr.get("x"), fr.get("r"), fr.sums()
    assert same_bits(fr.raw("r32"), fr.framed32((r1 * sb[:, None, None]).astype(np.float32))), "update r32"
    assert same_bits(fr.sb.cpu().numpy(), sb), "the update changed s_b"
    n1 = fr.raw("r32")
    fr.sc[:, DONE] = 1
    cr("pcg_update_f64f32", fr.ptr("q"), fr.ptr("x"), fr.ptr("r"), fr.ptr("r32"), *fr.kargs(), fr.sc.data_ptr(),
       fr.sb.data_ptr(), fr.part.data_ptr(), *g)
    assert same_bits(fr.get("x"), x1) and same_bits(fr.get("r"), r1), "a frozen sample moved"
    assert same_bits(fr.raw("r32"), n1), "a frozen sample's r32 moved"
    assert same_bits(fr.sums(), s1), "a frozen sample's r.r is not the same bits"


def test_scale_of_extreme_norms():
    """s_b for a zero, a non-finite and far-out norms: 1, 1, and the exact power of two."""
    from feanet_amd import _lib
    fr = Fields(4, 3, "poisson")
    for rn in ([0.0, np.inf, np.nan], [2.0 ** -140 * 1.7, 2.0 ** 140 * 1.2, 1.0], [3e-300, 7e300, 1.9999999]):
        fr.sc[:, RNORM] = torch.tensor(rn, dtype=T64).cuda()
        _lib.call_raw("pcg_narrow_f64f32", fr.ptr("r"), fr.ptr("r32"), fr.sc.data_ptr(), fr.sb.data_ptr(), *fr.geom(),
                      None)
        assert same_bits(fr.sb.cpu().numpy(), scale_of(rn)), rn


# ----------------------------------------------------------------------------- numpy mixed PCG
def oracle(n, problem, dt, prop=(1, 20)):
    from feanet_amd import mesh_setup as ms
    pids = {(n >> l) + 1: ms.interface_pattern_map((n >> l) + 1) for l in range(int(np.log2(n)))}
    return orc.OracleMultigrid(n, problem, dt, prop=prop, pids=pids if problem == "interface" else None)


def numpy_mixed_pcg(n, problem, x0, f, iters, prop=(1, 20), eps=0.0, rtol=None):
    """fp64 CG on K (boundary rows / columns zeroed) preconditioned by the fp32 oracle cycle on float32(r s_b); the
    per-sample freeze of the device.  Returns iterates after each iteration, the history, iteration counts, s_b."""
    lv = oracle(n, problem, np.float64, prop).levels[0]
    m32 = oracle(n, problem, np.float32, prop)
    geo = np.zeros((lv.H, lv.W))
    geo[1:-1, 1:-1] = 1
    x = np.asarray(x0, np.float64).copy()
    B = x.shape[0]
    r = (np.asarray(f, np.float64) - lv.K(x)) * geo
    p = np.zeros_like(x)
    hist = [np.sqrt(dot64(r, r))]
    sb = scale_of(hist[0])
    thresh = rtol * hist[0] if rtol is not None else np.full(B, eps)
    done = hist[0] <= thresh
    iters_b = np.zeros(B, np.int64)
    rz_prev = np.ones(B)
    xs = []
    for it in range(iters):
        r32 = (r * sb[:, None, None]).astype(np.float32)
        z = np.asarray(m32.step(np.zeros_like(r32), r32), np.float64)
        rz = dot64(r, z)
        beta = np.where(done | (it == 0), 0.0, rz / rz_prev)
        p = z + beta[:, None, None] * p
        Kp = lv.K(p) * geo
        pAp = dot64(p, Kp)
        alpha = np.where(done, 0.0, rz / np.where(done, 1.0, pAp))[:, None, None]
        x = x + alpha * p
        r = r - alpha * Kp
        rz_prev = np.where(done, rz_prev, rz)
        hist.append(np.sqrt(dot64(r, r)))
        iters_b += ~done
        done = done | (hist[-1] <= thresh)
        xs.append(x.copy())
        if done.all():
            break
    return xs, hist, iters_b, sb


def mixed(n, **kw):
    from feanet_amd import PCGSolver
    return PCGSolver(n, dtype=T64, precond_dtype=T32, **kw)


@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("n,B", [(16, 1), (16, 3), (64, 1), (64, 3)])
def test_iterate_vs_numpy(problem, n, B):
    """iterate(k), k = 1, 3, 8, against the numpy mixed PCG; (16, 3) carries a random u0 and nonzero Dirichlet data.
    After one Poisson iteration the Dirichlet values and b are checked at 1e-10 through solution() and
    residual_norm(): any of them rounded through fp32 would be off by 1e-8."""
    N = n + 1
    rng = np.random.default_rng(7 * n + B)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((B, N, N))
    full = (n, B) == (16, 3)
    u0 = rng.standard_normal((B, N, N)) if full else np.zeros((B, N, N))
    bc = rng.random((B, N, N)) * (1 - geo) if full else np.zeros((B, N, N))
    xs, hist, _, sb = numpy_mixed_pcg(n, problem, u0 * geo + bc, f, 8)
    s = mixed(n, problem=problem, batch=B)
    # five fp64 fine-level fields and no fp64 hierarchy
    assert s.dtype == T64 and s.mg.dtype == T32 and all(Lv.f.dtype == T32 for Lv in s.mg.levels)
    assert all(t.dtype == T64 for t in (s.x, s.b, s.r) + s.p) and len({t.data_ptr() for t in (s.x, s.b, s.r) + s.p}) == 5
    cu = lambda a: torch.from_numpy(a).cuda().reshape(B, 1, N, N)
    s.set_boundary(cu(bc))
    s.set_rhs(f=cu(f))
    s.load(cu(u0))
    assert same_bits(s.sb.cpu().numpy(), sb)
    done = 0
    for k in (1, 3, 8):
        s.iterate(k - done)
        done = k
        got = s.solution().cpu().numpy()[:, 0]
        ref = xs[k - 1]
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        print(f"k={k}: iterate scaled err {err:.3e}")
        if k == 1:
            assert err < 2e-5, f"k={k}: {err:.3e}"
            if problem == "poisson":
                bnd = (1 - geo).astype(bool)
                assert np.abs(got[:, bnd] - bc[:, bnd]).max() <= 1e-10, "Dirichlet values rounded"
                lv = oracle(n, problem, np.float64).levels[0]
                true = np.sqrt(dot64((f - lv.K(got)) * geo, (f - lv.K(got)) * geo))
                np.testing.assert_allclose(s.residual_norm().cpu().numpy(), true, rtol=1e-10)
        h = np.array(s.history())
        assert h.shape == (k + 1, B)
        print("history rel err", np.abs(h - np.array(hist[:k + 1])) / np.array(hist[:k + 1]))
        np.testing.assert_allclose(h, np.array(hist[:k + 1]), rtol=2e-3, atol=1e-6 * hist[0].max())
    sc = s.scalars()
    assert (sc[:, ITERS] == 8).all() and (sc[:, DONE] == 0).all() and (sc[:, ROW] == 9).all()


def test_F_is_assembled_in_fp64():
    """set_rhs(F=...) of the mixed solver stores bitwise the fp64 solver's b."""
    from feanet_amd import PCGSolver
    n, N = 16, 17
    F = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 1, N, N))).cuda()
    a, b = mixed(n), PCGSolver(n)
    a.set_rhs(F=F)
    b.set_rhs(F=F)
    assert torch.equal(a.L0.view(a.b), b.L0.view(b.b))


@pytest.mark.parametrize("prop", [(1, 20), (1, 1000)], ids=["c20", "c1000"])
def test_attainable_accuracy(prop):
    """rtol = 1e-12 on the two-material problem: converges to fp64's accuracy (true residual <= 1e-11 ||r0||) in the
    numpy model's iteration count (+-1) and within 2 of the all-fp64 solver's."""
    from feanet_amd import PCGSolver
    n, N = 64, 65
    rng = np.random.default_rng(64)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((1, N, N)) * geo
    ft = torch.from_numpy(f).cuda().reshape(1, 1, N, N)
    _, rh, it_ref, _ = numpy_mixed_pcg(n, "interface", np.zeros((1, N, N)), f, 100, prop=prop, rtol=1e-12)
    s = mixed(n, problem="interface", prop=prop)
    u, hist = s.solve(f=ft, rtol=1e-12, max_iters=100)
    true = float(s.residual_norm()[0])
    d = PCGSolver(n, problem="interface", prop=prop)
    d.solve(f=ft, rtol=1e-12, max_iters=100)
    print(f"prop={prop}: mixed {s.iterations} numpy {it_ref} fp64 {d.iterations}; recurrence "
          f"{hist[-1][0] / hist[0][0]:.3e} true {true / hist[0][0]:.3e} (numpy {rh[-1][0] / rh[0][0]:.3e})")
    assert s.flags[0] == 1 and d.flags[0] == 1
    assert true <= 1e-11 * hist[0][0], f"true residual {true / hist[0][0]:.3e} ||r0||"
    assert abs(int(s.iterations[0]) - int(it_ref[0])) <= 1
    assert abs(int(s.iterations[0]) - int(d.iterations[0])) <= 2
    assert torch.isfinite(u).all()


def test_scale_equivariance():
    """b, b 2^140 and b 2^-140: the same iterations, and solution and history bitwise the unscaled ones times the
    power of two (without s_b the fp32 cycle overflows on the first and stalls on the second)."""
    n, N = 64, 65
    rng = np.random.default_rng(140)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((1, 1, N, N)) * geo
    out = {}
    for e in (0, 140, -140):
        s = mixed(n)
        u, hist = s.solve(f=torch.from_numpy(f * 2.0 ** e).cuda(), rtol=1e-10, max_iters=60)
        out[e] = (u.cpu().numpy(), np.array(hist), int(s.iterations[0]), int(s.flags[0]), float(s.sb[0]))
        print(f"2^{e}: {out[e][2]} iterations, flag {out[e][3]}, last {out[e][1][-1, 0] / out[e][1][0, 0]:.3e}")
    u0, h0, it0, fl0, sb0 = out[0]
    assert fl0 == 1 and np.isfinite(u0).all()
    for e in (140, -140):
        u, h, it, fl, sb = out[e]
        assert it == it0 and fl == 1
        assert sb == sb0 * 2.0 ** -e
        assert same_bits(u, u0 * 2.0 ** e), f"2^{e}: solution"
        assert same_bits(h, h0 * 2.0 ** e), f"2^{e}: history"


def test_freeze_and_batch_independence():
    """An easy sample, a hard one and an all-zero right-hand side in one batch: every sample's result and history
    are bitwise those of its own B = 1 mixed solve, whatever check_every; the zero sample freezes in INIT with
    s_b = 1."""
    n, N, B = 32, 33, 3
    rng = np.random.default_rng(33)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((B, N, N)) * geo
    f[0] *= 1e-4   # easy: reaches the absolute eps in few iterations
    f[2] = 0.0
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1, 1, N, N)
    runs = {}
    for ce in (1, 5):
        s = mixed(n, problem="interface", batch=B, check_every=ce)
        u, hist = s.solve(f=cu(f), eps=1e-7, max_iters=60)
        runs[ce] = (u.cpu().numpy(), np.array(hist), s.iterations.copy(), s.flags.copy(), s.sb.cpu().numpy())
    u, hist, iters, flags, sb = runs[1]
    print("iterations", iters, "flags", flags, "s_b", sb)
    for a, b in zip(runs[1], runs[5]):
        assert np.array_equal(a, b), "result depends on check_every"
    assert (flags == 1).all() and iters[2] == 0 and 0 < iters[0] < iters[1]
    assert sb[2] == 1.0 and same_bits(sb, scale_of(hist[0]))
    assert np.isfinite(u).all() and (u[2] == 0).all() and (hist[:, 2] == 0).all()
    assert hist.shape[0] == iters.max() + 1
    for b in range(B):
        s1 = mixed(n, problem="interface", batch=1, check_every=3)
        u1, h1 = s1.solve(f=cu(f[b:b + 1]), eps=1e-7, max_iters=60)
        h1 = np.array(h1)[:, 0]
        assert s1.iterations[0] == iters[b]
        assert same_bits(u1.cpu().numpy()[0], u[b]), f"sample {b}: iterate differs from its B = 1 solve"
        assert same_bits(h1, hist[:len(h1), b]), f"sample {b}: history differs from its B = 1 solve"
        assert (hist[len(h1):, b] == h1[-1]).all(), f"sample {b}: frozen history rows do not repeat"


def test_graph_replay_matches_eager():
    n, N, B = 128, 129, 2
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((B, 1, N, N))).cuda()
    out = []
    for graph in (False, True):
        s = mixed(n, problem="interface", batch=B, graph=graph)
        s.set_rhs(f=f)
        for _ in range(3):  # graph=True: eager the first time, captured the second, replayed the third
            s.load()
            s.iterate(6)
            out.append((s.solution().cpu().numpy(), np.array(s.history())))
        assert bool(s._graphs) == graph
    for u, h in out[1:]:
        assert same_bits(u, out[0][0]) and same_bits(h, out[0][1])


@pytest.mark.parametrize("T", [T32, T64], ids=["f32", "f64"])
def test_default_path_unchanged(T):
    """precond_dtype=None and precond_dtype=dtype are the solver constructed without the argument, bit for bit."""
    from feanet_amd import PCGSolver
    n, N, B = 32, 33, 2
    f = torch.from_numpy(np.random.default_rng(9).standard_normal((B, 1, N, N))).to(T).cuda()
    out = []
    for kw in ({}, {"precond_dtype": None}, {"precond_dtype": T}):
        s = PCGSolver(n, problem="interface", dtype=T, batch=B, **kw)
        assert not s.mixed and s.mg.dtype == T and s.r is s.mg.levels[0].f
        u, h = s.solve(f=f, rtol=1e-5, max_iters=30)
        out.append((u.cpu().numpy(), np.array(h), s.scalars()))
    for o in out[1:]:
        assert all(same_bits(a, b) for a, b in zip(o, out[0]))


def test_bad_dtype_pairs_raise():
    from feanet_amd import PCGSolver
    with pytest.raises(ValueError, match="wider"):
        PCGSolver(16, dtype=T32, precond_dtype=T64)
    with pytest.raises(TypeError):
        PCGSolver(16, dtype=T64, precond_dtype=torch.float16)
    with pytest.raises(TypeError):
        PCGSolver(16, dtype=torch.int32)
