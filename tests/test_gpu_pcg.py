"""GPU parity of the Krylov kernels (fea_pcg_*) and of PCGSolver against a numpy conjugate gradient built from
oracle pieces: Level.K with boundary rows and columns zeroed as the operator, OracleMultigrid.step(0, r) as the
preconditioner, dot products summed in float64.

Tolerances are the project's: fields 1e-12 (fp64) / 5e-6 (fp32) relative to max(1, max|expected|) and reduced
scalars rtol 1e-12 / 1e-5 (test_gpu_mg.py's kernel tests); iterates 1e-10 scaled in fp64 (test_full_size_vs_oracle;
fp32 iterates of two implementations drift apart by cond(K) eps32, so as in test_vcycle_vs_oracle they are compared
after the first iteration only, at its 2e-5, and through the history afterwards); histories rtol 1e-9 / 2e-3 with
test_vcycle_vs_oracle's absolute floor of 1e-12 / 1e-6 of the initial residual."""
import numpy as np
import pytest
import torch

from oracle import feanet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 5e-6, torch.float64: 1e-12}
STOL = {torch.float32: 1e-5, torch.float64: 1e-12}
RZ, RZ_PREV, PAP, ALPHA, BETA, RNORM, DONE, ITERS, EPS, RTOL, THRESH, ROW = range(12)
INIT, STEP_RZ, STEP_PAP, STEP_RR = range(4)


def npdt(T):
    return np.float32 if T == torch.float32 else np.float64


def close(out, ref, T, what):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{what}: scaled max err {err:.3e}")
    assert err <= TOL[T], f"{what}: scaled max err {err:.3e} > {TOL[T]}"


@pytest.fixture(params=[False, True], ids=["cached", "nt"])
def nt(request, monkeypatch):
    """FEANET_NT_BYTES=0 selects the nontemporal-store instantiations that otherwise run only on fields > 64 MiB."""
    if request.param:
        monkeypatch.setenv("FEANET_NT_BYTES", "0")
    return request.param


class Fields:
    """Framed level-0 buffers (the solver's level allocator) with numpy I/O, and the numpy operator."""

    def __init__(self, n, B, T, problem, m=None, prop=(1, 20)):
        from feanet_amd import _lib, mesh_setup as ms
        from feanet_amd.solver import _Level
        m = n if m is None else m
        self.H, self.W, self.B, self.T = m + 1, n + 1, B, T
        self.ktab = ms.stencil_table(prop if problem == "interface" else None)
        if problem == "interface":
            # a rectangle is a window of the square's map around the inclusion, as a domain-decomposed rank's
            full = ms.interface_pattern_map(n + 1)
            if m > n:      # a tall grid: the square's map repeated down the rows (any map of valid ids is a problem)
                full = full[np.arange(m + 1) % (n + 1)]
            r0 = max(n - m, 0) // 2
            self.pid_np = np.ascontiguousarray(full[r0:r0 + m + 1])
        else:
            self.pid_np = np.zeros((self.H, self.W), np.uint8)
        self.L = _Level(m, n, B, T, torch.device("cuda"), self.pid_np if problem == "interface" else None)
        self.kt = torch.from_numpy(self.ktab.reshape(-1, 9).astype(npdt(T))).cuda()
        self.ntab = self.ktab.shape[0]
        self.geo = np.zeros((self.H, self.W))
        self.geo[1:-1, 1:-1] = 1
        self.per = int(_lib.lib().fea_pcg_parts(self.H, self.W, 4 if T == torch.float32 else 8))
        self.part = torch.zeros(B * self.per, dtype=torch.float64, device="cuda")
        self.sc = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
        self.hist = torch.zeros((4, B), dtype=torch.float64, device="cuda")
        self.bufs = {}

    def buf(self, name):
        if name not in self.bufs:
            self.bufs[name] = torch.zeros_like(self.L.a)
        return self.bufs[name]

    def put(self, name, arr):
        self.L.view(self.buf(name)).copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(self.T))

    def get(self, name):
        return self.L.view(self.buf(name)).cpu().numpy()

    def ptr(self, name):
        return self.buf(name).data_ptr()

    def kargs(self):
        return (None if self.L.pid is None else self.L.pid.data_ptr(), self.kt.data_ptr(), self.ntab)

    def rand(self, rng, interior=True):
        a = rng.standard_normal((self.B, self.H, self.W)).astype(npdt(self.T))
        return a * self.geo.astype(a.dtype) if interior else a

    def K(self, v):  # float64, interior rows only
        return orc.knet_apply(np.asarray(v, np.float64), self.pid_np, self.ktab) * self.geo

    def sums(self):
        return self.part.view(self.B, self.per).sum(1).cpu().numpy()

    def step(self, step):
        from feanet_amd import _lib
        _lib.call_raw("pcg_scalar_step", self.part.data_ptr(), self.per, self.sc.data_ptr(), self.hist.data_ptr(),
                      self.hist.shape[0], self.B, step, None)
        return self.sc.cpu().numpy()


def dot64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).reshape(a.shape[0], -1).sum(1)


SIZES = [(2, None, 1), (4, None, 3), (16, None, 3), (128, None, 1), (256, None, 3), (160, 24, 2),
         (32, 4096, 2), (32, 16384, 1), (32, 65536, 1)]
# the tall one-strip shapes and the row-task height they must reach (every other size runs 2-row tasks)
TALL = {(32, 4096): 2, (32, 16384): 8, (32, 65536): 32}


def task_height(H, W, esz):
    """the rows per task behind fea_pcg_parts on a one-strip grid: the only height with that many row tasks"""
    from feanet_amd import _lib
    per = int(_lib.lib().fea_pcg_parts(H, W, esz))
    hs = [rb for rb in (2, 4, 8, 16, 32) if -(-(H - 2) // rb) == per]
    assert len(hs) == 1, (H, W, per)
    return hs[0]


# (T, n, rows, B); 512 is the fp32 two-strip size (fp64 crosses its strip edge at 256)
KERNEL_CASES = [(T, n, m, B) for T in (torch.float32, torch.float64) for n, m, B in SIZES] + \
    [(torch.float32, 512, None, 1)]


@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("T,n,m,B", KERNEL_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_kernels_vs_numpy(T, problem, n, m, B, nt):
    """Each Krylov kernel on seeded random framed inputs: fields and reduced scalars against numpy.  A strip is 128
    columns in fp64 and 256 in fp32, so the sizes cross a strip edge and the row-task edges; (160, 24) is a
    rectangle."""
    from feanet_amd import _lib
    rng = np.random.default_rng(1000 * n + B)
    fr = Fields(n, B, T, problem, m=m)
    g = fr.L.geom()
    if (n, m) in TALL:
        assert task_height(fr.H, fr.W, 4 if T == torch.float32 else 8) == TALL[(n, m)]

    # --- residual: r = f - K x inside, 0 on the boundary; also with r aliasing f
    x, f = fr.rand(rng, interior=False), fr.rand(rng, interior=False)
    fr.put("x", x)
    fr.put("f", f)
    fr.put("r", np.full_like(x, 7.0))
    _lib.call("pcg_residual", T, fr.ptr("x"), fr.ptr("f"), fr.ptr("r"), *fr.kargs(), fr.part.data_ptr(), *g, None)
    r_ref = (f.astype(np.float64) - orc.knet_apply(x.astype(np.float64), fr.pid_np, fr.ktab)) * fr.geo
    r = fr.get("r")
    close(r, r_ref, T, "residual")
    assert (r[:, 0] == 0).all() and (r[:, -1] == 0).all() and (r[:, :, 0] == 0).all() and (r[:, :, -1] == 0).all()
    assert np.array_equal(fr.get("x"), x) and np.array_equal(fr.get("f"), f)
    np.testing.assert_allclose(fr.sums(), dot64(r_ref, r_ref), rtol=STOL[T])
    fr.sc.zero_()
    fr.sc[:, RTOL] = 0.5
    sc = fr.step(INIT)
    np.testing.assert_allclose(sc[:, RNORM], np.sqrt(dot64(r_ref, r_ref)), rtol=STOL[T])
    np.testing.assert_allclose(sc[:, THRESH], 0.5 * sc[:, RNORM], rtol=1e-15)
    assert (sc[:, DONE] == 0).all() and (sc[:, ROW] == 1).all()
    assert np.array_equal(fr.hist[0].cpu().numpy(), sc[:, RNORM])
    _lib.call("pcg_residual", T, fr.ptr("x"), fr.ptr("f"), fr.ptr("f"), *fr.kargs(), fr.part.data_ptr(), *g, None)
    assert np.array_equal(fr.get("f"), r), "r aliasing f"

    # --- dot
    z = fr.rand(rng)
    fr.put("z", z)
    _lib.call("pcg_dot", T, fr.ptr("r"), fr.ptr("z"), fr.part.data_ptr(), *g, None)
    np.testing.assert_allclose(fr.sums(), dot64(r, z), rtol=STOL[T])

    # --- direction: p_out = z + beta p_in, p_in untouched, partials of p_out . K p_out
    p = fr.rand(rng)
    beta = 0.37
    fr.put("p", p)
    fr.buf("q").zero_()
    fr.sc[:, BETA] = beta
    fr.sc[:, RZ] = 2.5
    _lib.call("pcg_direction", T, fr.ptr("z"), fr.ptr("p"), fr.ptr("q"), *fr.kargs(), fr.sc.data_ptr(),
              fr.part.data_ptr(), *g, None)
    q = fr.get("q")
    q_ref = z.astype(np.float64) + float(npdt(T)(beta)) * p.astype(np.float64)
    close(q, q_ref, T, "direction")
    assert np.array_equal(fr.get("p"), p), "p_in modified"
    assert np.array_equal(fr.get("z"), z)
    assert (q[:, 0] == 0).all() and (q[:, -1] == 0).all() and (q[:, :, 0] == 0).all() and (q[:, :, -1] == 0).all()
    pAp = dot64(q_ref, fr.K(q_ref))
    np.testing.assert_allclose(fr.sums(), pAp, rtol=STOL[T])
    sc = fr.step(STEP_PAP)
    np.testing.assert_allclose(sc[:, ALPHA], 2.5 / pAp, rtol=STOL[T])

    # --- update: x += alpha p, r -= alpha K p (in place), partials of the new r.r; a frozen sample is left alone
    alpha = 0.61
    fr.sc[:, ALPHA] = alpha
    x_in, r_in = fr.get("x"), fr.get("r")
    _lib.call("pcg_update", T, fr.ptr("q"), fr.ptr("x"), fr.ptr("r"), *fr.kargs(), fr.sc.data_ptr(),
              fr.part.data_ptr(), *g, None)
    a = float(npdt(T)(alpha))
    x_ref = x_in.astype(np.float64) + a * q.astype(np.float64) * fr.geo
    r_new = r_in.astype(np.float64) - a * fr.K(q)
    close(fr.get("x"), x_ref, T, "update x")
    close(fr.get("r"), r_new, T, "update r")
    assert np.array_equal(fr.get("q"), q)
    np.testing.assert_allclose(fr.sums(), dot64(r_new, r_new), rtol=STOL[T])
    x1, r1, s1 = fr.get("x"), fr.get("r"), fr.sums()
    fr.sc[:, DONE] = 1
    _lib.call("pcg_update", T, fr.ptr("q"), fr.ptr("x"), fr.ptr("r"), *fr.kargs(), fr.sc.data_ptr(),
              fr.part.data_ptr(), *g, None)
    assert np.array_equal(fr.get("x"), x1) and np.array_equal(fr.get("r"), r1), "a frozen sample moved"
    assert np.array_equal(fr.sums(), s1), "a frozen sample's r.r is not the same bits"


# ----------------------------------------------------------------------------- numpy PCG
def numpy_pcg(mg_o, x0, f, iters, dt, eps=0.0, rtol=None):
    """CG on K (boundary rows / columns zeroed) preconditioned by OracleMultigrid.step(0, r); per-sample freeze as
    the device's.  Returns iterates after each iteration, the history and the per-sample iteration counts."""
    lv = mg_o.levels[0]
    geo = np.zeros((lv.H, lv.W), dt)
    geo[1:-1, 1:-1] = 1
    x = np.asarray(x0, dt).copy()
    B = x.shape[0]
    r = ((np.asarray(f, dt) - lv.K(x)) * geo).astype(dt)
    p = np.zeros_like(x)
    hist = [np.sqrt(dot64(r, r))]
    thresh = rtol * hist[0] if rtol is not None else np.full(B, eps)
    done = hist[0] <= thresh
    iters_b = np.zeros(B, np.int64)
    rz_prev = np.ones(B)
    xs = []
    for it in range(iters):
        z = np.asarray(mg_o.step(np.zeros_like(r), r), dt)
        rz = dot64(r, z)
        beta = np.where(done | (it == 0), 0.0, rz / rz_prev)
        p = (z + beta.astype(dt)[:, None, None] * p).astype(dt)
        Kp = (lv.K(p) * geo).astype(dt)
        pAp = dot64(p, Kp)
        alpha = np.where(done, 0.0, rz / np.where(done, 1.0, pAp)).astype(dt)[:, None, None]
        x = (x + alpha * p).astype(dt)
        r = (r - alpha * Kp).astype(dt)
        rz_prev = np.where(done, rz_prev, rz)
        hist.append(np.sqrt(dot64(r, r)))
        iters_b += ~done
        done = done | (hist[-1] <= thresh)
        xs.append(x.copy())
        if done.all():
            break
    return xs, hist, iters_b


def oracle(n, problem, dt, prop=(1, 20)):
    from feanet_amd import mesh_setup as ms
    pids = {(n >> l) + 1: ms.interface_pattern_map((n >> l) + 1) for l in range(int(np.log2(n)))}
    return orc.OracleMultigrid(n, problem, dt, prop=prop, pids=pids if problem == "interface" else None)


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("n,B", [(16, 1), (16, 3), (64, 1), (64, 3)])
def test_iterate_vs_numpy(T, problem, n, B):
    """PCGSolver.iterate(k), k = 1, 3, 8, against the numpy PCG; (16, 3) carries nonzero Dirichlet data."""
    from feanet_amd import PCGSolver
    dt = npdt(T)
    N = n + 1
    rng = np.random.default_rng(7 * n + B)
    geo, _ = orc.square_geometry(N, dt)
    f = rng.standard_normal((B, N, N)).astype(dt)
    u0 = rng.standard_normal((B, N, N)).astype(dt)
    bc = (rng.random((B, N, N)) * (1 - geo)).astype(dt) if (n, B) == (16, 3) else np.zeros((B, N, N), dt)
    xs, hist, _ = numpy_pcg(oracle(n, problem, dt), u0 * geo + bc, f, 8, dt)
    s = PCGSolver(n, problem=problem, dtype=T, batch=B)
    cu = lambda a: torch.from_numpy(a).cuda().reshape(B, 1, N, N)
    s.set_boundary(cu(bc))
    s.set_rhs(f=cu(f))
    s.load(cu(u0))
    done = 0
    for k in (1, 3, 8):
        s.iterate(k - done)
        done = k
        got = s.solution().cpu().numpy()[:, 0]
        ref = xs[k - 1]
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        print(f"k={k}: iterate scaled err {err:.3e}")
        if T == torch.float64:
            assert err < 1e-10, f"k={k}: {err:.3e}"
        elif k == 1:
            assert err < 2e-5, f"k={k}: {err:.3e}"
        h = np.array(s.history())
        assert h.shape == (k + 1, B)
        r0 = hist[0].max()
        print("history rel err", np.abs(h - np.array(hist[:k + 1])) / np.array(hist[:k + 1]))
        np.testing.assert_allclose(h, np.array(hist[:k + 1]), rtol=1e-9 if T == torch.float64 else 2e-3,
                                   atol=(1e-12 if T == torch.float64 else 1e-6) * r0)
    sc = s.scalars()
    assert (sc[:, ITERS] == 8).all() and (sc[:, DONE] == 0).all() and (sc[:, ROW] == 9).all()


def test_high_contrast():
    """prop = (1, 1000): the stationary V-cycle iteration diverges, the same cycle as a CG preconditioner converges,
    in the numpy PCG's iteration count."""
    from feanet_amd import MultigridSolver, PCGSolver
    n, N = 64, 65
    rng = np.random.default_rng(64)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((1, N, N)) * geo
    ft = torch.from_numpy(f).cuda().reshape(1, 1, N, N)
    mg = MultigridSolver(n, problem="interface", prop=(1, 1000))
    _, vh = mg.solve(f=ft, eps=0.0, max_cycles=30)
    print("V-cycle residuals", vh[0][0], vh[-1][0])
    assert vh[-1][0] > vh[0][0], "the stationary iteration was expected to diverge at contrast 1000"
    _, rh, it_ref = numpy_pcg(oracle(n, "interface", np.float64, prop=(1, 1000)), np.zeros((1, N, N)), f, 100,
                              np.float64, rtol=1e-8)
    s = PCGSolver(n, problem="interface", prop=(1, 1000))
    u, hist = s.solve(f=ft, rtol=1e-8, max_iters=100)
    print("PCG iterations", s.iterations, "numpy", it_ref, "last", hist[-1], "true", s.residual_norm().cpu().numpy())
    assert s.flags[0] == 1 and hist[-1][0] <= 1e-8 * hist[0][0]
    assert abs(int(s.iterations[0]) - int(it_ref[0])) <= 1
    assert len(hist) == s.iterations[0] + 1
    np.testing.assert_allclose(s.residual_norm().cpu().numpy(), hist[-1], rtol=1e-3)
    assert torch.isfinite(u).all()


def test_freeze_and_batch_independence():
    """An easy sample, a hard one and an all-zero right-hand side in one batch: every sample's result and history
    are bitwise those of its own B = 1 solve, whatever check_every; the zero sample freezes at once."""
    from feanet_amd import PCGSolver
    n, N, B = 32, 33, 3
    rng = np.random.default_rng(33)
    geo, _ = orc.square_geometry(N, np.float64)
    f = rng.standard_normal((B, N, N)) * geo
    f[0] *= 1e-4   # easy: reaches the absolute eps in few iterations
    f[2] = 0.0
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1, 1, N, N)
    runs = {}
    for ce in (1, 5):
        s = PCGSolver(n, problem="interface", batch=B, check_every=ce)
        u, hist = s.solve(f=cu(f), eps=1e-7, max_iters=60)
        runs[ce] = (u.cpu().numpy(), np.array(hist), s.iterations.copy(), s.flags.copy())
    u, hist, iters, flags = runs[1]
    print("iterations", iters, "flags", flags)
    for a, b in zip(runs[1], runs[5]):
        assert np.array_equal(a, b), "result depends on check_every"
    assert (flags == 1).all() and iters[2] == 0 and 0 < iters[0] < iters[1]
    assert np.isfinite(u).all() and (u[2] == 0).all() and hist[0, 2] == 0 and (hist[:, 2] == 0).all()
    assert hist.shape[0] == iters.max() + 1
    for b in range(B):
        s1 = PCGSolver(n, problem="interface", batch=1, check_every=3)
        u1, h1 = s1.solve(f=cu(f[b:b + 1]), eps=1e-7, max_iters=60)
        h1 = np.array(h1)[:, 0]
        assert s1.iterations[0] == iters[b]
        assert np.array_equal(u1.cpu().numpy()[0], u[b]), f"sample {b}: iterate differs from its B = 1 solve"
        assert np.array_equal(h1, hist[:len(h1), b]), f"sample {b}: history differs from its B = 1 solve"
        assert (hist[len(h1):, b] == h1[-1]).all(), f"sample {b}: frozen history rows do not repeat"


def test_graph_replay_matches_eager():
    from feanet_amd import PCGSolver
    n, N, B = 128, 129, 2
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((B, 1, N, N))).cuda()
    out = []
    for graph in (False, True):
        s = PCGSolver(n, problem="interface", batch=B, graph=graph)
        s.set_rhs(f=f)
        for _ in range(3):  # graph=True: eager the first time, captured the second, replayed the third
            s.load()
            s.iterate(6)
            out.append((s.solution().cpu().numpy(), np.array(s.history())))
        assert bool(s._graphs) == graph
    for u, h in out[1:]:
        assert np.array_equal(u, out[0][0]) and np.array_equal(h, out[0][1])


def test_constructor_rejects_nonsymmetric_preconditioners():
    from feanet_amd import PCGSolver
    with pytest.raises(ValueError):
        PCGSolver(32, smoother="hjac")
    with pytest.raises(ValueError):
        PCGSolver(32, compat="mm_interface_q2")
    rng = np.random.default_rng(0)
    R = rng.standard_normal((16, 3, 3)).astype(np.float32)
    with pytest.raises(ValueError):
        PCGSolver(32, problem="interface", R=R, P=R + 0.1)
    with pytest.raises(ValueError):
        PCGSolver(32, problem="interface", R=R, P=R)  # per-pattern tables: P != R^T even when the tables are equal
    k = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32) / 4
    PCGSolver(32, problem="interface", R=k, P=k, w=(0.9, 1.1))
