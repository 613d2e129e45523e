"""GPU parity of the framed multigrid kernels (fea_mg_*) and of the MultigridSolver V-cycle.

Level kernels are compared with the CPU oracle on seeded inputs at sizes that cross every strip
and row-task edge (N = 3 .. 1025, batches 1 and 3, Poisson and two-material, fp32 and fp64);
V-cycles are compared with the oracle's MultiGrid.Step and with the reference's own recorded
residual histories (golden fixtures); at the benchmark size 4097^2 fp64 the checks are
size-independent properties (convergence factor, exact scaling, batch independence).
Tolerances: fp64 1e-12, fp32 5e-6, relative to max(1, max|expected|)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import feanet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 5e-6, torch.float64: 1e-12}
# two-material pattern maps made by the ORACLE's own element / node loops (tests/golden/make_c3_maps.py; the
# CPU suite re-checks them against the loop): the oracle side of the 1025^2 cases uses these instead of
# re-running the O(N^2) Python loops
_MAPS = {}


def oracle_maps():
    if not _MAPS:
        import os
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_pattern_maps.npz"))
        _MAPS.update({int(k[4:]): d[k] for k in d.files if k.startswith("pid_")})
    return _MAPS


def npdt(T):
    return np.float32 if T == torch.float32 else np.float64


def close(out, ref, T, what):
    out = np.asarray(out, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    assert err <= TOL[T], f"{what}: scaled max err {err:.3e} > {TOL[T]}"


class Frame:
    """A framed level (via the solver's level allocator) with numpy I/O for tests."""

    def __init__(self, n, B, T, problem, m=None):
        from feanet_amd.solver import _Level
        from feanet_amd import mesh_setup as ms
        m = n if m is None else m
        self.N = n + 1
        self.H, self.W = m + 1, n + 1
        if problem == "interface":
            self.pid_np = oracle_maps().get(self.N) if self.N == self.H else None
            if self.pid_np is None:
                self.pid_np = ms.interface_pattern_map(self.N)
            if self.H != self.N:  # a rectangle: the centred row crop of the square's map (as test_gpu_pcg.py)
                r0 = (self.N - self.H) // 2
                self.pid_np = np.ascontiguousarray(self.pid_np[r0:r0 + self.H])
        else:
            self.pid_np = np.zeros((self.H, self.W), np.uint8)
        self.L = _Level(m, n, B, T, torch.device("cuda"), self.pid_np if problem == "interface" else None)
        self.T = T

    def put(self, name, arr):
        self.L.view(self.L.buf(name)).copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(self.T))

    def get(self, name):
        return self.L.view(self.L.buf(name)).cpu().numpy()

    def args(self):
        return self.L.geom()

    def pid(self):
        return None if self.L.pid is None else self.L.pid.data_ptr()


def tables(problem, T, learned=False):
    from feanet_amd import mesh_setup as ms
    ktab = ms.stencil_table((1, 20) if problem == "interface" else None)
    omd = ms.omega_over_d(ktab, 2 / 3., npdt(T))
    lin = ms.linear_transfer_kernel() / 4
    C = ktab.shape[0]
    rng = np.random.default_rng(5)
    R = np.broadcast_to(lin, (C, 3, 3)).copy()
    P = np.broadcast_to(lin, (C, 3, 3)).copy()
    if learned:  # per-pattern distinct kernels exercise the pattern lookups
        R = (R * (1 + 0.1 * rng.standard_normal((C, 3, 3)))).astype(np.float32)
        P = (P * (1 + 0.1 * rng.standard_normal((C, 3, 3)))).astype(np.float32)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1, 9) if x.ndim == 3 else x).cuda().to(T)
    return ktab, omd, R, P, cuda(ktab), torch.from_numpy(omd).cuda().to(T), cuda(R), cuda(P)


def rand_state(rng, B, N, T, bc_scale=1.0):
    hw = (N, N) if np.isscalar(N) else tuple(N)
    u = rng.standard_normal((B,) + hw).astype(npdt(T))
    f = rng.standard_normal((B,) + hw).astype(npdt(T))
    return u, f


SIZES = [(2, 1), (4, 3), (8, 1), (16, 3), (128, 1), (256, 3), (1024, 1)]


@pytest.fixture(params=[False, True], ids=["cached", "nt"])
def nt(request, monkeypatch):
    """nt: FEANET_NT_BYTES=0 forces the nontemporal instantiations of the level kernels (stores past the
    caches; the cycle join's nontemporal iterate loads) that otherwise only run on levels > 64 MiB, i.e.
    only at sizes too large for the oracle (the 4097^2 metric configuration)."""
    if request.param:
        monkeypatch.setenv("FEANET_NT_BYTES", "0")
    return request.param


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("n,B", SIZES)
def test_mg_sweep(T, problem, n, B, nt):
    from feanet_amd import _lib
    rng = np.random.default_rng(n + B)
    fr = Frame(n, B, T, problem)
    ktab, omd, _, _, kt, om, _, _ = tables(problem, T)
    u, f = rand_state(rng, B, fr.N, T)
    fr.put("a", u)
    fr.put("f", f)
    fr.put("b", u * 0 + 7.0)  # sentinel: boundary of the output must stay untouched
    nt = ktab.shape[0]
    _lib.call("mg_sweep", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), kt.data_ptr(),
              om.data_ptr(), nt, *fr.args(), None)
    out = fr.get("b")
    geo, _ = orc.square_geometry(fr.N, npdt(T))
    bc = u * (1 - geo)  # boundary values live in the field
    ref = orc.jacobi_sweep(u, f, fr.pid_np, ktab, geo, bc)
    close(out[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, "sweep interior")
    assert (out[:, 0, :] == 7).all() and (out[:, -1, :] == 7).all() and (out[:, :, 0] == 7).all() and \
        (out[:, :, -1] == 7).all(), "boundary written"
    # zero initial guess: out = omd * f inside
    _lib.call("mg_sweep", T, None, fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), kt.data_ptr(), om.data_ptr(), nt,
              *fr.args(), None)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], (omd[fr.pid_np.astype(np.int64)] * f)[:, 1:-1, 1:-1], T, "zero sweep")
    # residual norm
    ws = torch.zeros(_lib.norm_workspace_bytes(B, fr.H, fr.W) // 8 + 1, dtype=torch.float64, device="cuda")
    res = torch.zeros(B, dtype=torch.float64, device="cuda")
    _lib.call("mg_residual_norm", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.pid(), kt.data_ptr(), nt, res.data_ptr(),
              ws.data_ptr(), *fr.args(), 0, 0, 0, 0, None)
    np.testing.assert_allclose(res.cpu().numpy(), orc.interior_norm(f - orc.knet_apply(u, fr.pid_np, ktab)),
                               rtol=1e-5 if T == torch.float32 else 1e-12)


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem,learned", [("poisson", False), ("interface", False), ("interface", True)])
@pytest.mark.parametrize("n,B", SIZES[1:])
def test_mg_transfer(T, problem, learned, n, B, nt):
    from feanet_amd import _lib
    rng = np.random.default_rng(3 * n + B)
    fr = Frame(n, B, T, problem)
    co = Frame(n // 2, B, T, problem)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned)
    nt = ktab.shape[0]
    u, f = rand_state(rng, B, fr.N, T)
    fr.put("a", u)
    fr.put("f", f)
    w0, w1 = 1.25, 0.75
    # residual + restriction
    _lib.call("mg_residual_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), None, co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, w0, *fr.args(), co.L.ld, co.L.bs, None)
    ref = orc.restrict(f - orc.knet_apply(u, fr.pid_np, ktab), fr.pid_np, R, w0)
    close(co.get("f"), ref, T, "residual+restrict")
    # fused pre-sweep + residual + restriction: u' = J(u, f) stored, fc = R(f - K u')
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_sweep_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(),
              fr.pid(), kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, w0, *fr.args(), co.L.ld, co.L.bs,
              None, None, None, None)
    geo, _ = orc.square_geometry(fr.N, npdt(T))
    up = orc.jacobi_sweep(u, f, fr.pid_np, ktab, geo, u * (1 - geo))
    outb = fr.get("b")
    close(outb[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1], T, "fused sweep u'")
    assert (outb[:, 0, :] == 7).all() and (outb[:, :, 0] == 7).all() and (outb[:, :, -1] == 7).all()
    close(co.get("f"), orc.restrict(f - orc.knet_apply(up, fr.pid_np, ktab), fr.pid_np, R, w0), T, "fused RR")
    # zero-guess sweep fused: v = omd*f written, restriction of f - K v
    fr.put("b", u * 0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, w0, *fr.args(), co.L.ld, co.L.bs, None)
    geo, _ = orc.square_geometry(fr.N, npdt(T))
    v = omd[fr.pid_np.astype(np.int64)] * f * geo
    close(fr.get("b"), v, T, "zero-guess v")
    close(co.get("f"), orc.restrict(f - orc.knet_apply(v, fr.pid_np, ktab), fr.pid_np, R, w0), T, "zero RR")
    # prolongation + correction + sweep
    e = rng.standard_normal((B, co.N, co.N)).astype(npdt(T))
    e[:, 0, :] = e[:, -1, :] = e[:, :, 0] = e[:, :, -1] = 0
    co.put("a", e)
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_prolong_sweep", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(),
              fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, w1, *fr.args(), co.L.ld,
              co.L.bs, None)
    x = u + orc.prolong(e, co.pid_np, P, w1)
    bc = u * (1 - geo)
    ref = orc.jacobi_sweep(x, f, fr.pid_np, ktab, geo, bc)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, "prolong+sweep")
    assert (out[:, 0, :] == 7).all() and (out[:, :, -1] == 7).all()
    # recompute mode: RR without storing v, then prolong+sweep with u = NULL (v = omd*f recomputed)
    # is bitwise the stored-v pair
    fr.put("a", u * 0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), fr.L.a.data_ptr(), co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, w0, *fr.args(), co.L.ld, co.L.bs, None)
    fc_stored = co.get("f")
    _lib.call("mg_prolong_sweep", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(),
              fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, w1, *fr.args(), co.L.ld,
              co.L.bs, None)
    ps_stored = fr.get("b")
    co.put("f", fc_stored * 0 + 3.0)
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), None, co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, w0, *fr.args(), co.L.ld, co.L.bs, None)
    assert (fr.get("b") == 7).all(), "v written although v_out = NULL"
    assert np.array_equal(co.get("f")[:, 1:-1, 1:-1], fc_stored[:, 1:-1, 1:-1])
    _lib.call("mg_prolong_sweep", T, None, co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(),
              fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, w1, *fr.args(), co.L.ld,
              co.L.bs, None)
    out = fr.get("b")
    assert np.array_equal(out[:, 1:-1, 1:-1], ps_stored[:, 1:-1, 1:-1]), "recomputed iterate differs"
    assert (out[:, 0, :] == 7).all() and (out[:, :, -1] == 7).all()
    fr.put("a", u)
    _lib.call("mg_prolong_add", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.b.data_ptr(), co.pid(), pt.data_ptr(),
              nt, w1, *fr.args(), co.L.ld, co.L.bs, None)
    close(fr.get("b")[:, 1:-1, 1:-1], x[:, 1:-1, 1:-1], T, "prolong+add")


# ----------------------------------------------------------------------------- V-cycles
@pytest.mark.parametrize("tail,fuse", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("n,L", [(64, None), (128, 4), (32, 1), (32, 2), (256, None), (1024, None)])
def test_vcycle_vs_oracle(T, problem, n, L, tail, fuse, nt):
    from feanet_amd.solver import MultigridSolver
    B = 2
    N = n + 1
    bc, u0, f, geo, r0, vs, refs = _oracle_cycles(T, problem, n, L, B)
    s = MultigridSolver(n, levels=L, problem=problem, dtype=T, batch=B, coarse_tail=tail, fuse=fuse)
    if tail and s.L > 1 and n <= 256:
        assert s.tail_from is not None
    s.set_boundary(torch.from_numpy(bc).cuda().reshape(B, 1, N, N))
    s.set_rhs(f=torch.from_numpy(f).cuda().reshape(B, 1, N, N))
    s.load(torch.from_numpy(u0).cuda().reshape(B, 1, N, N))
    for k in range(4):
        s.vcycle()
        v = vs[k]
        got = s.solution().cpu().numpy()[:, 0]
        if T == torch.float64 or k == 0:
            # fp64: every cycle; fp32: the first cycle (later iterates differ by cond(K)*eps32 ~ 1e-4
            # between any two fp32 implementations, so fp32 is compared through the residual below)
            err = np.abs(got - v).max() / max(1.0, np.abs(v).max())
            assert err < (1e-10 if T == torch.float64 else 2e-5), f"cycle {k}: {err:.3e}"
        res = s.residual_norm().cpu().numpy()
        tol = 1e-9 if T == torch.float64 else 2e-3
        np.testing.assert_allclose(res, refs[k], rtol=tol, atol=(1e-12 if T == torch.float64 else 1e-6) * r0.max())


_ORACLE_CYCLES = {}


def _oracle_cycles(T, problem, n, L, B):
    """Seeded problem (random Dirichlet data, iterate, rhs) and the oracle's first four MultiGrid.Step
    iterates and residual norms; cached across the kernel-variant parametrisations that share them."""
    key = (T, problem, n, L, B)
    if key not in _ORACLE_CYCLES:
        rng = np.random.default_rng(n)
        N = n + 1
        mg_o = orc.OracleMultigrid(n, problem, npdt(T), levels=L,
                                   pids=oracle_maps() if problem == "interface" else None)
        geo, _ = orc.square_geometry(N, npdt(T))
        bc = (rng.random((B, N, N)) * (1 - geo)).astype(npdt(T))
        mg_o.set_boundary(geo, bc)
        u0 = rng.standard_normal((B, N, N)).astype(npdt(T))
        f = rng.standard_normal((B, N, N)).astype(npdt(T))
        v = u0 * geo + bc
        r0 = orc.interior_norm(f - mg_o.levels[0].K(v))
        vs, refs = [], []
        for _ in range(4):
            v = mg_o.step(v, f)
            vs.append(v)
            refs.append(orc.interior_norm(f - mg_o.levels[0].K(v)))
        _ORACLE_CYCLES[key] = (bc, u0, f, geo, r0, vs, refs)
    return _ORACLE_CYCLES[key]


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("problem,n,B", [("poisson", 64, 2), ("poisson", 256, 1), ("poisson", 1024, 1),
                                         ("interface", 128, 2), ("interface", 256, 1)])
def test_joined_vcycles_vs_oracle(T, problem, n, B, nt):
    """vcycle(k) with joined cycle boundaries (fea_mg_cycle_join on the finest level, graph-replayed
    blocks) against k oracle MultiGrid.Step cycles, with random Dirichlet data; cached and
    nontemporal kernel instantiations.  fp64 to 1e-10 of max|u|; fp32 residual norms to 2e-3."""
    from feanet_amd.solver import MultigridSolver
    rng = np.random.default_rng(7 * n + B)
    N = n + 1
    mg_o = orc.OracleMultigrid(n, problem, npdt(T))
    geo, _ = orc.square_geometry(N, npdt(T))
    bc = (rng.random((B, N, N)) * (1 - geo)).astype(npdt(T))
    mg_o.set_boundary(geo, bc)
    u0 = rng.standard_normal((B, N, N)).astype(npdt(T))
    f = rng.standard_normal((B, N, N)).astype(npdt(T))
    s = MultigridSolver(n, problem=problem, dtype=T, batch=B)
    s.set_boundary(torch.from_numpy(bc).cuda().reshape(B, 1, N, N))
    s.set_rhs(f=torch.from_numpy(f).cuda().reshape(B, 1, N, N))
    v = u0 * geo + bc
    for k in ((2, 3) if T == torch.float64 else (2,)):
        s.load(torch.from_numpy(u0).cuda().reshape(B, 1, N, N))
        s.vcycle(k)
        ref = v
        for _ in range(k):
            ref = mg_o.step(ref, f)
        got = s.solution().cpu().numpy()[:, 0]
        if T == torch.float64:
            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
            assert err < 1e-10, f"k={k}: {err:.3e}"
        else:  # two fp32 implementations' iterates drift apart by cond(K) eps32: compare residuals
            np.testing.assert_allclose(s.residual_norm().cpu().numpy(), orc.interior_norm(f - mg_o.levels[0].K(ref)),
                                       rtol=2e-3)


def test_full_size_vs_oracle():
    """The metric configuration itself: 4097^2 fp64 Poisson, seeded rhs and random Dirichlet data,
    one V-cycle (fea_mg_sweep_restrict / prolongation kernels) and then three joined V-cycles
    (fea_mg_cycle_join, nontemporal loads and stores: every level-0 field is > 64 MiB) against the
    oracle's MultiGrid.Step (M-FEANet-mg_test.ipynb:27346-27372), 1e-10 of max|u| (~1.5 s per oracle
    cycle on the host)."""
    from feanet_amd.solver import MultigridSolver
    n = 4096
    N = n + 1
    rng = np.random.default_rng(4097)
    f = rng.standard_normal((1, N, N))
    geo, _ = orc.square_geometry(N, np.float64)
    bc = rng.random((1, N, N)) * (1 - geo)
    mg_o = orc.OracleMultigrid(n, "poisson", np.float64)
    mg_o.set_boundary(geo, bc)
    s = MultigridSolver(n, dtype=torch.float64)
    assert s.levels[0].f.numel() * 8 > 64 << 20  # the nontemporal instantiations run
    s.set_boundary(torch.from_numpy(bc).cuda().reshape(1, 1, N, N))
    s.set_rhs(f=torch.from_numpy(f).cuda().reshape(1, 1, N, N))
    s.load()
    v = bc.copy()
    r0 = float(mg_o.residual_norm(v, f)[0])
    s.vcycle()
    v = mg_o.step(v, f)
    got = s.solution().cpu().numpy()[:, 0]
    err = np.abs(got - v).max() / np.abs(v).max()
    assert err < 1e-10, f"first cycle: {err:.3e}"
    s.vcycle(3)
    for _ in range(3):
        v = mg_o.step(v, f)
    got = s.solution().cpu().numpy()[:, 0]
    err = np.abs(got - v).max() / np.abs(v).max()
    assert err < 1e-10, f"joined cycles 2-4: {err:.3e}"
    res = float(s.residual_norm()[0])
    ref = float(mg_o.residual_norm(v, f)[0])
    assert abs(res - ref) <= 1e-9 * ref + 1e-12 * r0, (res, ref)


def test_vcycle_graph_replay_matches_eager():
    from feanet_amd.solver import MultigridSolver
    n, B = 256, 2
    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    out = []
    for graph in (False, True):
        s = MultigridSolver(n, dtype=torch.float64, batch=B, graph=graph)
        s.set_rhs(f=f)
        s.load()
        s.vcycle(5)
        out.append(s.solution())
    assert torch.equal(out[0], out[1])


def test_mg_test_isopoisson_golden(gold):
    """mg_test MultiGrid.Step (jac) on the reference's IsoPoisson 33^2 samples: same cycle count and
    residual history as the reference's own run, solution within 2e-5 of the dataset direct solve."""
    from feanet_amd.solver import MultigridSolver
    g = gold("mg_test_isopoisson33.npz")
    for k in range(3):
        s = MultigridSolver(32, dtype=torch.float32)
        s.set_boundary(torch.from_numpy(g["boundary_value"][k]).float().cuda())
        u, hist = s.solve(F=torch.from_numpy(g["rhs"][k]).float().cuda(), eps=5e-5, max_cycles=60)
        hist = np.array([h[0] for h in hist])
        ref = g[f"jac_hist_{k}"]
        assert len(hist) == len(ref)
        np.testing.assert_allclose(hist[:6], ref[:6], rtol=2e-4, atol=1e-6 * ref[0])
        assert np.abs(u.cpu().numpy()[0, 0] - g["u"][k]).max() < 2e-5


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_mg_test_synth65_golden(gold, dt):
    from feanet_amd.solver import MultigridSolver
    g = gold("mg_test_synth65.npz")
    T = torch.float32 if dt == "f32" else torch.float64
    for L in (6, 3):
        s = MultigridSolver(64, levels=L, dtype=T)
        s.set_boundary(torch.from_numpy(g[f"{dt}_bc"]).cuda())
        eps = 1e-9 if dt == "f64" else 5e-6
        u, hist = s.solve(F=torch.from_numpy(g[f"{dt}_F"]).cuda(), eps=eps, max_cycles=(39 if L == 6 else 24))
        hist = np.array([h[0] for h in hist])
        ref = g[f"{dt}_L{L}_hist"]
        assert abs(len(hist) - len(ref)) <= (0 if dt == "f64" else 1)
        np.testing.assert_allclose(hist[:10], ref[:10], rtol=1e-9 if dt == "f64" else 5e-4,
                                   atol=(1e-12 if dt == "f64" else 1e-6) * ref[0])


def test_mm_interface_golden(gold):
    """MM_Interface_error.ipynb: two-material 65^2, f = FNet(1), Q2 schedule -> 14 V-cycles, and the
    residual history the notebook itself recorded."""
    from feanet_amd.solver import MultigridSolver
    g = gold("mm_interface65.npz")
    rec = gold("recorded_outputs.npz")
    s = MultigridSolver(64, problem="interface", dtype=torch.float32, compat="mm_interface_q2")
    s.set_rhs(F=torch.ones(1, 1, 65, 65, device="cuda"))
    s.load()
    hist = []
    while (not hist or hist[-1] > 5e-5) and len(hist) < 40:
        s.vcycle()
        hist.append(float(s.residual_norm()[0]))
    assert len(hist) == 14
    # fp32 histories of two implementations agree to ~1e-3 relative (rounding differs per op order)
    np.testing.assert_allclose(hist[:8], g["hist"][:8], rtol=3e-3, atol=1e-5 * g["hist"][0])
    np.testing.assert_allclose(hist[:6], rec["mm_interface_res"][:6], rtol=3e-3)


def test_multigrid_py_learned_golden(gold):
    """FEANet/multigrid.py MultiGrid.iterate with the shipped learned R/P ratios (BASELINE config 3
    operators) at 65^2: 12 cycles like the reference; linear R/P: 13 cycles."""
    from feanet_amd.solver import MultigridSolver
    g = gold("multigrid_py_iface65.npz")
    for tag, ncyc in (("linear", 13), ("learned", 12)):
        s = MultigridSolver(64, problem="interface", dtype=torch.float32, R=g[f"{tag}_rtab"], P=g[f"{tag}_ptab"],
                            w=tuple(g[f"{tag}_w"]))
        u, hist = s.solve(f=torch.from_numpy(g["f"]).cuda(), eps=5e-5, max_cycles=40)
        hist = np.array([h[0] for h in hist])
        assert len(hist) - 1 == ncyc == len(g[f"{tag}_hist"]) - 1
        np.testing.assert_allclose(hist[:8], g[f"{tag}_hist"][:8], rtol=3e-3, atol=1e-5 * hist[0])


def test_mm_convergence_golden(gold):
    """MM_Model_convergence.ipynb V(nu1,nu2) histories (rec_V_cycle) at n = 16, 32, 64.
    With nu1 = 0 the reference applies K to the un-reset random initial guess in the first
    cycle; the solver resets the iterate on load, so there the asymptotic factor is compared."""
    from feanet_amd.solver import MultigridSolver
    g = gold("mm_convergence.npz")
    for n in (16, 32, 64):
        for nu in ((1, 1), (0, 1), (1, 0), (2, 1), (1, 2), (2, 2), (0, 2), (2, 0)):
            key = f"n{n}_v{nu[0]}{nu[1]}"
            ref = g[key + "_hist"]
            s = MultigridSolver(n, dtype=torch.float32, nu1=nu[0], nu2=nu[1])
            s.set_rhs(f=torch.zeros(1, 1, n + 1, n + 1, device="cuda"))
            s.load(torch.from_numpy(g[key + "_init"]).cuda().reshape(1, 1, n + 1, n + 1))
            hist = []
            for _ in range(6):
                s.vcycle()
                hist.append(float(s.residual_norm()[0]))
            if nu[0] >= 1:
                np.testing.assert_allclose(hist, ref[:6], rtol=2e-3, atol=1e-6 * ref[0], err_msg=key)
            else:
                q, qr = hist[5] / hist[4], ref[5] / ref[4]
                assert abs(q - qr) < 0.02 * qr + 1e-3, (key, q, qr)
    rec = gold("recorded_outputs.npz")["mm_vnu_q_n64"]  # factors the notebook printed at n = 64
    assert 0.24 < rec[3] < 0.27


# ----------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def big():
    from feanet_amd.solver import MultigridSolver
    s = MultigridSolver(4096, dtype=torch.float64)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    f = torch.randn(1, 1, 4097, 4097, device="cuda", dtype=torch.float64, generator=g)
    s.set_rhs(f=f)
    return s, f


def test_full_size_convergence(big):
    """4097^2 fp64 Poisson: V(1,1) contraction ~0.26 (MM_Model_convergence.ipynb:265-268 records
    0.2590-0.2632 for n = 64..512) and the relative residual falls below 1e-6 within 12 cycles."""
    s, f = big
    s.load()
    r = [float(s.residual_norm()[0])]
    for _ in range(12):
        s.vcycle()
        r.append(float(s.residual_norm()[0]))
    q = r[-1] / r[-2]
    assert 0.15 < q < 0.32, r
    assert r[-1] / r[0] < 1e-6, r


def test_full_size_exact_scaling(big):
    """The V-cycle is linear in (u0, f): scaling both by 2 scales every intermediate exactly."""
    from feanet_amd.solver import MultigridSolver
    s, f = big
    s.load()
    s.vcycle(2)
    a = s.solution()
    s2 = MultigridSolver(4096, dtype=torch.float64)
    s2.set_rhs(f=2 * f)
    s2.load()
    s2.vcycle(2)
    assert torch.equal(2 * a, s2.solution())


def test_batch_independence():
    from feanet_amd.solver import MultigridSolver
    n = 1024
    rng = np.random.default_rng(3)
    f = torch.from_numpy(rng.standard_normal((3, 1, n + 1, n + 1))).cuda()
    sb = MultigridSolver(n, dtype=torch.float64, batch=3)
    sb.set_rhs(f=f)
    sb.load()
    sb.vcycle(3)
    ub = sb.solution()
    for b in range(3):
        s1 = MultigridSolver(n, dtype=torch.float64, batch=1)
        s1.set_rhs(f=f[b:b + 1])
        s1.load()
        s1.vcycle(3)
        assert torch.equal(s1.solution()[0], ub[b])


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("Nt,nlev", [(5, 2), (9, 3), (17, 3), (33, 5), (65, 6), (65, 2)])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nu", [(1, 1), (2, 1), (0, 2), (1, 0)])
def test_coarse_tail_kernel(T, problem, Nt, nlev, B, nu):
    """fea_mg_coarse_tail against the restatement of its sub-cycle with oracle operators."""
    from feanet_amd import _lib, mesh_setup as ms
    from test_schedule import tail_oracle
    n = (Nt - 1) << 1  # a parent level above the tail (unused, only to build the hierarchy)
    L = nlev + 1
    mg = orc.OracleMultigrid(n, problem, npdt(T), levels=L)
    rng = np.random.default_rng(Nt + nlev + B)
    f = rng.standard_normal((B, Nt, Nt)).astype(npdt(T))
    f[:, 0, :] = f[:, -1, :] = f[:, :, 0] = f[:, :, -1] = 0
    ref = tail_oracle(mg, 1, f, None, B, nu1=nu[0], nu2=nu[1], q2=False)
    fr = Frame(Nt - 1, B, T, problem)
    fr.put("f", f)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T)
    pidl = None
    if problem == "interface":
        maps = [ms.interface_pattern_map(((Nt - 1) >> k) + 1).reshape(-1) for k in range(nlev)]
        pidl = torch.from_numpy(np.concatenate(maps)).cuda()
    _lib.call("mg_coarse_tail", T, fr.L.f.data_ptr(), fr.L.a.data_ptr(), Nt, Nt, nlev, fr.L.ld, fr.L.bs,
              None if pidl is None else pidl.data_ptr(), kt.data_ptr(), om.data_ptr(), ktab.shape[0], rt.data_ptr(),
              pt.data_ptr(), 1.0, 1.0, nu[0], nu[1], 0, B, None)
    got = fr.get("a")
    close(got, ref, T, f"tail Nt={Nt} nlev={nlev} B={B} nu={nu}")


# ----------------------------------------------------------------------------- rectangles (H != W)
# (65536, 32, 1) and (4096, 32, 8): one strip and >= 2048 row tasks, so the task height is 32 and 16 rows (every
# other shape of the list runs at 2; tests/footprint.py ties the heights in between to these bitwise)
RECT = [(8, 16, 1), (64, 16, 2), (16, 256, 1), (512, 128, 1), (6, 10, 3), (65536, 32, 1), (4096, 32, 8)]


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("m,n,B", RECT)
def test_mg_rect_kernels(T, m, n, B):
    """Every framed kernel on an (m+1) x (n+1) grid (rows != columns: the local slabs of the
    domain-decomposed path) against the oracle; the residual norm over a row range."""
    from feanet_amd import _lib
    rng = np.random.default_rng(7 * m + n)
    fr = Frame(n, B, T, "poisson", m=m)
    co = Frame(n // 2, B, T, "poisson", m=m // 2)
    ktab, omd, R, P, kt, om, rt, pt = tables("poisson", T)
    H, W = fr.H, fr.W
    u, f = rand_state(rng, B, (H, W), T)
    geo, _ = orc.square_geometry((H, W), npdt(T))
    fr.put("a", u)
    fr.put("f", f)
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_sweep", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), None, kt.data_ptr(),
              om.data_ptr(), 1, *fr.args(), None)
    up = orc.jacobi_sweep(u, f, fr.pid_np, ktab, geo, u * (1 - geo))
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1], T, "rect sweep")
    assert (out[:, 0, :] == 7).all() and (out[:, -1, :] == 7).all() and (out[:, :, -1] == 7).all()
    w0, w1 = 1.25, 0.75
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_sweep_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(),
              None, kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), 1, w0, *fr.args(), co.L.ld, co.L.bs, None, None,
              None, None)
    close(fr.get("b")[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1], T, "rect fused sweep")
    close(co.get("f"), orc.restrict(f - orc.knet_apply(up, fr.pid_np, ktab), fr.pid_np, R, w0), T, "rect SR")
    _lib.call("mg_residual_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), None, co.L.f.data_ptr(), None,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), 1, w0, *fr.args(), co.L.ld, co.L.bs, None)
    close(co.get("f"), orc.restrict(f - orc.knet_apply(u, fr.pid_np, ktab), fr.pid_np, R, w0), T, "rect RR")
    fr.put("b", u * 0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(), None,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), 1, w0, *fr.args(), co.L.ld, co.L.bs, None)
    v = omd[0] * f * geo
    close(fr.get("b"), v, T, "rect zero-guess v")
    close(co.get("f"), orc.restrict(f - orc.knet_apply(v, fr.pid_np, ktab), fr.pid_np, R, w0), T, "rect zero RR")
    e = rng.standard_normal((B, co.H, co.W)).astype(npdt(T))
    e[:, 0, :] = e[:, -1, :] = e[:, :, 0] = e[:, :, -1] = 0
    co.put("a", e)
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_prolong_sweep", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(),
              None, None, kt.data_ptr(), om.data_ptr(), 1, pt.data_ptr(), 1, w1, *fr.args(), co.L.ld, co.L.bs, None)
    x = u + orc.prolong(e, co.pid_np, P, w1)
    ref = orc.jacobi_sweep(x, f, fr.pid_np, ktab, geo, u * (1 - geo))
    close(fr.get("b")[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, "rect prolong+sweep")
    # residual norm over all interior rows and over a row range
    ws = torch.zeros(_lib.norm_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.float64, device="cuda")
    res = torch.zeros(B, dtype=torch.float64, device="cuda")
    r = f - orc.knet_apply(u, fr.pid_np, ktab)
    for lo, hi in ((0, 0), (1, H - 1), (2, max(2, H // 2)), (H // 2, H - 1), (3, 3)):
        for clo, chi in ((0, 0), (1, W - 1), (2, max(2, W // 2)), (W // 3, W - 1)):
            _lib.call("mg_residual_norm", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), None, kt.data_ptr(), 1,
                      res.data_ptr(), ws.data_ptr(), *fr.args(), lo, hi, clo, chi, None)
            a, b = (1, H - 1) if (lo, hi) == (0, 0) else (lo, hi)
            c, d = (1, W - 1) if (clo, chi) == (0, 0) else (clo, chi)
            ref = np.sqrt((r[:, a:b, c:d].astype(np.float64) ** 2).sum(axis=(1, 2)))
            np.testing.assert_allclose(res.cpu().numpy(), ref, rtol=1e-5 if T == torch.float32 else 1e-12,
                                       err_msg=f"norm rows {lo}:{hi} cols {clo}:{chi}")


# Widths that are not 2^k + 1.  321: three fp64 / two fp32 strips, the last one partial and ending in mid-wave
# (the row's last vector in lane 31 / 15); 323 = 3 (mod 4): one valid element in the fp32 tail vector.
ODD_WIDTHS = [(33, 321, 2), (35, 323, 3)]


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("H,W,B", ODD_WIDTHS)
def test_mg_kernels_odd_widths(T, problem, H, W, B, nt):
    """The value comparisons of test_mg_sweep / test_mg_transfer / test_mg_rect_kernels against the oracle at
    33 x 321 and 35 x 323, Poisson and two-material (distinct per-pattern R / P), same tolerances: mg_sweep (both
    modes), mg_residual_restrict (three modes), mg_sweep_restrict, mg_prolong_sweep, mg_prolong_add, and
    mg_residual_norm over row and column ranges."""
    from feanet_amd import _lib
    rng = np.random.default_rng(H + W + B)
    fr = Frame(W - 1, B, T, problem, m=H - 1)
    co = Frame((W - 1) // 2, B, T, problem, m=(H - 1) // 2)
    assert fr.pid_np.shape == (H, W) and co.pid_np.shape == (co.H, co.W)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=(problem == "interface"))
    ntab = ktab.shape[0]
    u, f = rand_state(rng, B, (H, W), T)
    geo, _ = orc.square_geometry((H, W), npdt(T))
    pid = fr.pid_np.astype(np.int64)
    w0, w1 = 1.25, 0.75
    fr.put("a", u)
    fr.put("f", f)

    def untouched(out, what):
        assert (out[:, 0, :] == 7).all() and (out[:, -1, :] == 7).all() and (out[:, :, 0] == 7).all() and \
            (out[:, :, -1] == 7).all(), f"{what}: boundary written"
    # sweep, with an iterate and from a zero guess
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_sweep", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), kt.data_ptr(),
              om.data_ptr(), ntab, *fr.args(), None)
    up = orc.jacobi_sweep(u, f, fr.pid_np, ktab, geo, u * (1 - geo))
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1], T, "sweep")
    untouched(out, "sweep")
    _lib.call("mg_sweep", T, None, fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), kt.data_ptr(), om.data_ptr(), ntab,
              *fr.args(), None)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], (omd[pid] * f)[:, 1:-1, 1:-1], T, "zero sweep")
    untouched(out, "zero sweep")
    # residual + restriction of a stored iterate
    _lib.call("mg_residual_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), None, co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(), ntab, w0, *fr.args(), co.L.ld, co.L.bs, None)
    close(co.get("f"), orc.restrict(f - orc.knet_apply(u, fr.pid_np, ktab), fr.pid_np, R, w0), T, "RR")
    # fused pre-sweep + residual + restriction
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_sweep_restrict", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(),
              fr.pid(), kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(), ntab, w0, *fr.args(), co.L.ld, co.L.bs,
              None, None, None, None)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], up[:, 1:-1, 1:-1], T, "fused sweep u'")
    untouched(out, "fused sweep")
    close(co.get("f"), orc.restrict(f - orc.knet_apply(up, fr.pid_np, ktab), fr.pid_np, R, w0), T, "fused RR")
    # zero guess, v stored; then v not stored
    v = omd[pid] * f * geo
    fc_ref = orc.restrict(f - orc.knet_apply(v, fr.pid_np, ktab), fr.pid_np, R, w0)
    fr.put("b", u * 0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), fr.L.b.data_ptr(), co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(), ntab, w0, *fr.args(), co.L.ld, co.L.bs, None)
    close(fr.get("b"), v, T, "zero-guess v")
    close(co.get("f"), fc_ref, T, "zero RR")
    fr.put("b", u * 0 + 7.0)
    co.put("f", fc_ref * 0)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), None, co.L.f.data_ptr(), fr.pid(),
              kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(), ntab, w0, *fr.args(), co.L.ld, co.L.bs, None)
    assert (fr.get("b") == 7).all(), "v written although v_out = NULL"
    close(co.get("f"), fc_ref, T, "zero RR, v not stored")
    # prolongation + correction, with and without the post-sweep
    e = rng.standard_normal((B, co.H, co.W)).astype(npdt(T))
    e[:, 0, :] = e[:, -1, :] = e[:, :, 0] = e[:, :, -1] = 0
    co.put("a", e)
    x = u + orc.prolong(e, co.pid_np, P, w1)
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_prolong_sweep", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(),
              fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), ntab, pt.data_ptr(), ntab, w1, *fr.args(), co.L.ld,
              co.L.bs, None)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], orc.jacobi_sweep(x, f, fr.pid_np, ktab, geo, u * (1 - geo))[:, 1:-1, 1:-1], T,
          "prolong+sweep")
    untouched(out, "prolong+sweep")
    fr.put("b", u * 0 + 7.0)
    _lib.call("mg_prolong_add", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.b.data_ptr(), co.pid(), pt.data_ptr(),
              ntab, w1, *fr.args(), co.L.ld, co.L.bs, None)
    out = fr.get("b")
    close(out[:, 1:-1, 1:-1], x[:, 1:-1, 1:-1], T, "prolong+add")
    untouched(out, "prolong+add")
    # residual norm over row and column ranges
    ws = torch.zeros(_lib.norm_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.float64, device="cuda")
    res = torch.zeros(B, dtype=torch.float64, device="cuda")
    r = f - orc.knet_apply(u, fr.pid_np, ktab)
    for lo, hi in ((0, 0), (1, H - 1), (2, H // 2), (H // 2, H - 1), (3, 3)):
        for clo, chi in ((0, 0), (1, W - 1), (2, W // 2), (W // 3, W - 1), (W - 2, W - 1)):
            _lib.call("mg_residual_norm", T, fr.L.a.data_ptr(), fr.L.f.data_ptr(), fr.pid(), kt.data_ptr(), ntab,
                      res.data_ptr(), ws.data_ptr(), *fr.args(), lo, hi, clo, chi, None)
            a, b = (1, H - 1) if (lo, hi) == (0, 0) else (lo, hi)
            c, d = (1, W - 1) if (clo, chi) == (0, 0) else (clo, chi)
            ref = np.sqrt((r[:, a:b, c:d].astype(np.float64) ** 2).sum(axis=(1, 2)))
            np.testing.assert_allclose(res.cpu().numpy(), ref, rtol=1e-5 if T == torch.float32 else 1e-12,
                                       err_msg=f"norm rows {lo}:{hi} cols {clo}:{chi}")


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("m,n,tail", [(256, 128, True), (128, 256, True), (64, 128, False), (1024, 512, True)])
def test_vcycle_rect_vs_oracle(T, m, n, tail):
    """MultigridSolver(rows=m) on a rectangle against the oracle's V-cycle on the same grid."""
    from feanet_amd.solver import MultigridSolver
    rng = np.random.default_rng(m + n)
    B = 2
    H, W = m + 1, n + 1
    s = MultigridSolver(n, rows=m, dtype=T, batch=B, coarse_tail=tail)
    mg_o = orc.OracleMultigrid(n, "poisson", npdt(T), levels=s.L, rows=m)
    assert s.L == mg_o.L
    if tail:
        assert s.tail_from is not None
    u0 = rng.standard_normal((B, H, W)).astype(npdt(T))
    f = rng.standard_normal((B, H, W)).astype(npdt(T))
    geo, _ = orc.square_geometry((H, W), npdt(T))
    s.set_rhs(f=torch.from_numpy(f).cuda().reshape(B, 1, H, W))
    s.load(torch.from_numpy(u0).cuda().reshape(B, 1, H, W))
    v = u0 * geo
    r0 = orc.interior_norm(f - mg_o.levels[0].K(v))
    for k in range(3):
        s.vcycle()
        v = mg_o.step(v, f)
        got = s.solution().cpu().numpy()[:, 0]
        if T == torch.float64 or k == 0:
            err = np.abs(got - v).max() / max(1.0, np.abs(v).max())
            assert err < (1e-10 if T == torch.float64 else 2e-5), f"cycle {k}: {err:.3e}"
        np.testing.assert_allclose(s.residual_norm().cpu().numpy(), orc.interior_norm(f - mg_o.levels[0].K(v)),
                                   rtol=1e-9 if T == torch.float64 else 2e-3,
                                   atol=(1e-12 if T == torch.float64 else 1e-6) * r0.max())


# ----------------------------------------------------------------------------- cycle join
@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("problem,n,m,B", [("poisson", 256, None, 1), ("poisson", 1024, None, 2),
                                           ("poisson", 128, 512, 1), ("interface", 256, None, 2),
                                           ("poisson", 4, None, 1), ("poisson", 64, 8, 3)])
@pytest.mark.parametrize("k", [2, 3, 6])
def test_cycle_join_bitwise(T, problem, n, m, B, k, nt):
    """vcycle(k) with the finest level's cycle boundaries joined (fea_mg_cycle_join) is bitwise the
    unjoined sequence of k V-cycles; the graph-replayed second call as well."""
    from feanet_amd.solver import MultigridSolver
    rows = m if m is not None else n
    rng = np.random.default_rng(n + rows + k)
    f = torch.from_numpy(rng.standard_normal((B, 1, rows + 1, n + 1))).cuda().to(T)
    u0 = torch.from_numpy(rng.standard_normal((B, 1, rows + 1, n + 1))).cuda().to(T)
    out = []
    for join in (False, True):
        kw = dict(rows=m) if m is not None else {}
        s = MultigridSolver(n, problem=problem, dtype=T, batch=B, join_cycles=join, **kw)
        s.set_rhs(f=f)
        s.load(u0)
        s.vcycle(k)
        a = s.solution()
        s.vcycle(k)   # second call: segments replayed as graphs
        out.append((a, s.solution()))
    assert torch.equal(out[0][0], out[1][0]), (out[0][0] - out[1][0]).abs().max().item()
    assert torch.equal(out[0][1], out[1][1])


def test_cycle_join_bitwise_full_size():
    """At 4097^2 fp64 the finest fields exceed the nontemporal threshold (64 MiB): the join then streams
    u with nontemporal loads and stores u' nontemporally; still bitwise the unjoined cycles."""
    from feanet_amd.solver import MultigridSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    f = torch.randn(1, 1, 4097, 4097, device="cuda", dtype=torch.float64, generator=g)
    out = []
    for join in (False, True):
        s = MultigridSolver(4096, dtype=torch.float64, join_cycles=join)
        s.set_rhs(f=f)
        s.load()
        s.vcycle(3)
        out.append(s.solution())
        del s
    assert torch.equal(out[0], out[1])


def test_cycle_join_kernel_direct(nt):
    """fea_mg_cycle_join against fea_mg_prolong_sweep + fea_mg_sweep_restrict on random data, including
    boundary nodes that are not zero (Dirichlet data) and a coarse correction with a nonzero ring."""
    from feanet_amd import _lib
    for T in (torch.float64, torch.float32):
        # (4096, 32, 16): the join's power-of-two path (B >= kJoinBatchPow2) at 32-row tasks
        for (m, n, B, problem) in ((256, 256, 2, "poisson"), (130, 514, 1, "poisson"), (64, 64, 1, "interface"),
                                   (4096, 32, 16, "poisson")):
            fr = Frame(n, B, T, problem, m=m)
            co = Frame(n // 2, B, T, problem, m=m // 2)
            ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=(problem == "interface"))
            nt = ktab.shape[0]
            rng = np.random.default_rng(m + n)
            u, f = rand_state(rng, B, (fr.H, fr.W), T)
            e = rng.standard_normal((B, co.H, co.W)).astype(npdt(T))
            e[:, 0] = e[:, -1] = 0
            e[:, :, 0] = e[:, :, -1] = 0
            for name in ("a", "b"):
                fr.put(name, u)
            fr.put("f", f)
            co.put("a", e)
            args_ps = (fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), co.pid(),
                       kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, 0.75) + fr.args() + (co.L.ld, co.L.bs)
            _lib.call("mg_prolong_sweep", T, *args_ps, None)
            # SR from b into a zero-initialised buffer with the same boundary
            tmp = fr.L.a.clone()
            _lib.call("mg_sweep_restrict", T, fr.L.b.data_ptr(), fr.L.f.data_ptr(), tmp.data_ptr(), co.L.f.data_ptr(),
                      fr.pid(), kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, 1.25, *fr.args(), co.L.ld,
                      co.L.bs, None, None, None, None)
            ref_u, ref_f = fr.L.view(tmp).clone(), co.get("f").copy()
            co.put("f", np.zeros_like(ref_f))
            out = fr.L.a.clone()
            fr.put("b", u)
            _lib.call("mg_cycle_join", T, fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr(), out.data_ptr(),
                      co.L.f.data_ptr(), fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt,
                      rt.data_ptr(), nt, 0.75, 1.25, *fr.args(), co.L.ld, co.L.bs, None, None, None, None)
            got_u = fr.L.view(out)
            assert torch.equal(got_u, ref_u), (T, m, n, (got_u - ref_u).abs().max().item())
            got_f = co.get("f")
            assert np.array_equal(got_f[:, 1:-1, 1:-1], ref_f[:, 1:-1, 1:-1]), (T, m, n)


# ----------------------------------------------------------------------------- solve loop
@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("problem,n,B", [("poisson", 256, 1), ("poisson", 1024, 2), ("interface", 128, 2)])
def test_solve_joined_matches_per_cycle_loop(T, problem, n, B):
    """solve(): the device-resident loop (norms fused into the cycle join, host checks per block,
    recomputed last post-smooth, re-run from a snapshot when a block overshoots) gives the per-cycle
    driver loop's result: same number of cycles, bitwise the same iterate, norms to 1e-12 (fp64)."""
    from feanet_amd.solver import MultigridSolver
    rng = np.random.default_rng(n + B)
    N = n + 1
    f = torch.from_numpy(rng.standard_normal((B, 1, N, N))).cuda().to(T)
    bc = torch.from_numpy(rng.random((B, 1, N, N))).cuda().to(T)
    ref_s = MultigridSolver(n, problem=problem, dtype=T, batch=B, join_cycles=False)
    s = MultigridSolver(n, problem=problem, dtype=T, batch=B)
    r0 = None
    for rel in (0.5, 1e-2, 1e-4, 1e-6, 1e-9, 0.0):
        for solver in (ref_s, s):
            solver.set_boundary(bc)
        if r0 is None:
            ref_s.set_rhs(f=f)
            ref_s.load()
            r0 = float(ref_s.residual_norm().max())
        eps = rel * r0
        mc = 7 if rel == 0.0 else 60
        ua, ha = ref_s.solve(f=f, eps=eps, max_cycles=mc)
        ub, hb = s.solve(f=f, eps=eps, max_cycles=mc)
        assert len(ha) == len(hb), (rel, eps, len(ha), len(hb), [x.max() for x in ha[-4:]], [x.max() for x in hb[-7:]])
        assert torch.equal(ua, ub), (rel, (ua - ub).abs().max().item())
        np.testing.assert_allclose(np.array(hb), np.array(ha), rtol=1e-11 if T == torch.float64 else 1e-5,
                                   atol=1e-14 * r0)
        # the solver stays usable: one more cycle from the returned state
        s.vcycle()
        ref_s.vcycle()
        assert torch.equal(s.solution(), ref_s.solution())


def test_solve_overshoot_rerun(monkeypatch):
    """A block that overshoots (convergence before its last cycle) is re-run from its start buffer: force
    it with blocks far longer than needed; still the per-cycle loop's cycles, iterate and history."""
    from feanet_amd.solver import MultigridSolver
    n = 256
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((1, 1, n + 1, n + 1))).cuda()
    ref_s = MultigridSolver(n, dtype=torch.float64, join_cycles=False)
    s = MultigridSolver(n, dtype=torch.float64)
    ref_s.set_rhs(f=f)
    ref_s.load()
    r0 = float(ref_s.residual_norm()[0])
    ua, ha = ref_s.solve(f=f, eps=1e-7 * r0)
    monkeypatch.setattr(s, "SOLVE_BLOCK_MAX", 64)
    import math as _m
    real_ceil = _m.ceil
    monkeypatch.setattr("feanet_amd.solver.math.ceil", lambda x: real_ceil(x) + 5)  # predict 5 cycles too many
    ub, hb = s.solve(f=f, eps=1e-7 * r0)
    monkeypatch.setattr("feanet_amd.solver.math.ceil", real_ceil)
    assert any(e[0] == "rerun" for e in s._solve_log), s._solve_log
    assert len(ha) == len(hb)
    assert torch.equal(ua, ub)
    np.testing.assert_allclose(np.array(hb), np.array(ha), rtol=1e-11)


def test_solve_full_size_rate():
    """4097^2 fp64: solve() to a 1e-8 relative residual uses the fused norms (cycle count and history as
    the per-cycle loop) and its cycles run within 10 % of the bench's rate (vcycle(k) of the same count;
    load() and solution(), which solve() also does, timed separately and added).  Best of 5."""
    import time
    from feanet_amd.solver import MultigridSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    f = torch.randn(1, 1, 4097, 4097, device="cuda", dtype=torch.float64, generator=g)
    s = MultigridSolver(4096, dtype=torch.float64)
    s.set_rhs(f=f)
    s.load()
    r0 = float(s.residual_norm()[0])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for _ in range(3):  # warm: eager first, captured second
        u, h = s.solve(eps=1e-8 * r0)
    runs = [timed(lambda: s.solve(eps=1e-8 * r0)) for _ in range(5)]
    t_solve = float(np.min([t for t, _ in runs]))
    u, h = runs[-1][1]
    k = len(h) - 1
    assert 8 <= k <= 20, h
    assert h[-1].max() <= 1e-8 * r0 < h[-2].max()
    for _ in range(3):
        s.load()
        s.vcycle(k)
    t_load, t_cyc, t_sol = [], [], []
    for _ in range(5):
        t_load.append(timed(s.load)[0])
        t_cyc.append(timed(lambda: s.vcycle(k))[0])
        t_sol.append(timed(s.solution)[0])
    t_cyc = float(np.min(t_cyc))
    t_io = float(np.min(t_load) + np.min(t_sol))  # load() + solution(): part of solve(), not of the cycles
    print(f"solve {k} cycles: {t_solve * 1e3:.3f} ms, vcycle({k}) {t_cyc * 1e3:.3f} ms, io {t_io * 1e3:.3f} ms, "
          f"{s._solve_log}, ratios {[round(float(h[i + 1].max() / h[i].max()), 4) for i in range(len(h) - 1)]}")
    s._trace = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve(eps=1e-8 * r0)
    print("solve phases (ms):", [(w, round((t - t0) * 1e3, 3)) if isinstance(t, float) else (w, t)
                                 for w, t in [(e[0], e[1]) if len(e) == 2 else (e[0], e[1:]) for e in s._solve_log]])
    s._trace = False
    # best of 5 each; slack: two host round trips (the block reads of the norm history), which vary by box
    assert t_solve < 1.10 * t_cyc + t_io + 1e-4, (t_solve, t_cyc, t_io)


def test_pipelined_state_semantics():
    """Joinable solvers rest between vcycle() calls in the pipelined state (next pre-smooth done, end
    iterate materialised on demand): solution() / residual_norm() between calls, a new right-hand side
    mid-pipeline and vcycle(1) chains all give the unjoined sequence's iterates bitwise."""
    from feanet_amd.solver import MultigridSolver
    n, B = 256, 2
    rng = np.random.default_rng(21)
    f1 = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    f2 = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    u0 = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    out = []
    for join in (False, True):
        s = MultigridSolver(n, dtype=torch.float64, batch=B, join_cycles=join)
        s.set_rhs(f=f1)
        s.load(u0)
        rec = []
        s.vcycle(1)
        rec.append(s.residual_norm())
        s.vcycle(1)
        s.vcycle(3)
        rec.append(s.solution())
        s.set_rhs(f=f2)  # the pipelined pre-smooth used f1: must be redone with f2
        s.vcycle(2)
        rec.append(s.solution())
        rec.append(s.residual_norm())
        s.vcycle(1)
        rec.append(s.solution())
        out.append(rec)
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what", ["P", "R", "w", "RP"])
def test_set_transfer_keeps_pipelined_iterate(what):
    """set_transfer on a solver resting in the pipelined state (its last end iterate not stored, recomputed with
    the prolongation tables on demand): the iterate the finished cycles produced is kept — solution() after the
    call equals solution() before it, bitwise, whether or not it had been materialised — and the next cycles run
    with the new tables (they equal a solver built with them from that iterate)."""
    from feanet_amd.solver import MultigridSolver
    from feanet_amd import mesh_setup as ms
    n, B = 128, 1
    rng = np.random.default_rng(8)
    f = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    lin = ms.linear_transfer_kernel().reshape(1, 3, 3)
    R2 = lin / 4 * 1.1 if "R" in what else None
    P2 = lin * 0.9 if "P" in what else None
    w2 = (0.9, 1.2) if what == "w" else None
    for peek in (False, True):
        s = MultigridSolver(n, dtype=torch.float64, batch=B)
        s.set_rhs(f=f)
        s.load()
        s.vcycle(2)
        before = s.solution().clone() if peek else None
        if not peek:  # reference value from a twin solver that never changes its tables
            t = MultigridSolver(n, dtype=torch.float64, batch=B)
            t.set_rhs(f=f)
            t.load()
            t.vcycle(2)
            before = t.solution().clone()
        s.set_transfer(R=R2, P=P2, w=w2)
        assert torch.equal(s.solution(), before), (what, peek)
        s.vcycle(2)
        after = s.solution()
        ref = MultigridSolver(n, dtype=torch.float64, batch=B)
        ref.set_transfer(R=R2, P=P2, w=w2)
        ref.set_rhs(f=f)
        ref.load(before)
        ref.vcycle(2)
        assert torch.equal(after, ref.solution()), (what, peek)


def test_step_runs_unjoined_plan(monkeypatch):
    """step() (MultiGrid.Step / iterate, one cycle from a loaded iterate, read at once) launches exactly the
    unjoined plan — no cycle join, no discarded pipelined pre-smooth — also right after a pipelined
    vcycle(k) call; and its result is bitwise the unjoined solver's."""
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    n, B = 128, 2
    rng = np.random.default_rng(5)
    f = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    u0 = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    ref = MultigridSolver(n, dtype=torch.float64, batch=B, join_cycles=False).step(u0, f)
    s = MultigridSolver(n, dtype=torch.float64, batch=B, graph=False)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for warm in (False, True):
        if warm:  # leave the solver in the pipelined state first
            s.set_rhs(f=f)
            s.load(u0)
            s.vcycle(3)
            s.solution()
        names.clear()
        out = s.step(u0, f)
        torch.cuda.synchronize()
        plan = [name for name, _ in s._plan("a")[0]]
        body = [x for x in names if x not in ("mg_pack", "mg_unpack")]
        assert body == plan, (warm, body)
        assert "mg_cycle_join" not in names
        assert names.count("mg_pack") == 3 and names.count("mg_unpack") == 1, names  # f, a, b; the result
        assert torch.equal(out, ref)


def test_set_boundary_takes_effect_at_load():
    """set_boundary(new) followed by solution() / residual_norm() without a load(): the joined solver's
    materialised end iterate carries the iterate buffers' (old) Dirichlet values, as the unjoined solver's."""
    from feanet_amd.solver import MultigridSolver
    n, B = 64, 1
    rng = np.random.default_rng(8)
    N = n + 1
    f = torch.from_numpy(rng.standard_normal((B, 1, N, N))).cuda()
    u0 = torch.from_numpy(rng.standard_normal((B, 1, N, N))).cuda()
    bc1 = torch.zeros(B, 1, N, N, dtype=torch.float64)
    bc1[..., 0, :] = 1.0
    bc2 = torch.zeros_like(bc1)
    bc2[..., :, 0] = -2.0
    out = []
    for join in (False, True):
        s = MultigridSolver(n, dtype=torch.float64, batch=B, join_cycles=join)
        s.set_rhs(f=f)
        s.set_boundary(bc1.cuda())
        s.load(u0)
        s.vcycle(3)
        s.set_boundary(bc2.cuda())
        out.append((s.solution(), s.residual_norm()))
        s.load(u0)  # now bc2
        s.vcycle(2)
        out.append((s.solution(), s.residual_norm()))
    (u_a, r_a), (u_a2, r_a2), (u_b, r_b), (u_b2, r_b2) = out
    assert torch.equal(u_a, u_b) and torch.equal(r_a, r_b)
    assert torch.equal(u_a2, u_b2) and torch.equal(r_a2, r_b2)
    assert torch.equal(u_b[..., 0, 1:-1].cpu(), bc1[..., 0, 1:-1])
    assert torch.equal(u_b2[..., :, 0].cpu(), bc2[..., :, 0])


def test_mg_step_custom_op():
    """torch.ops.feanet.mg_step (the fused V-cycle as a custom op): opcheck-clean, bitwise the solver's own
    cycles, one and several per call."""
    from feanet_amd import torch_ops  # noqa: F401
    from feanet_amd.solver import MultigridSolver
    n, B = 64, 2
    rng = np.random.default_rng(9)
    f = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    u0 = torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda()
    s = MultigridSolver(n, dtype=torch.float64, batch=B)
    ref = MultigridSolver(n, dtype=torch.float64, batch=B, join_cycles=False)
    for cyc in (1, 3):
        got = torch.ops.feanet.mg_step(u0, f, s.handle, cyc)
        ref.set_rhs(f=f)
        ref.load(u0)
        ref.vcycle(cyc)
        assert torch.equal(got, ref.solution())
        torch.library.opcheck(torch.ops.feanet.mg_step, (u0, f, s.handle, cyc),
                              test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    with pytest.raises(RuntimeError, match="no live MultigridSolver"):
        torch.ops.feanet.mg_step(u0, f, 10 ** 9, 1)


def test_multigrid_iterate_grad_mode_fused():
    """FEANet/multigrid.py MultiGrid.iterate under autograd: the fused forward (bitwise the no-grad call)
    with gradients from the recomputed module-level cycle — equal to back-propagating the module path."""
    import FEANet.multigrid as mgm
    lin = torch.asarray([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float32)
    torch.set_default_device("cuda")
    try:
        mg = mgm.MultiGrid(32, lin / 16.0, lin / 4.0, torch.tensor([4.0, 1.0]))
        g = torch.Generator(device="cuda").manual_seed(3)
        f = torch.randn(2, 1, 33, 33, generator=g, device="cuda")
        u = torch.randn(2, 1, 33, 33, generator=g, device="cuda")
        with torch.no_grad():
            v_ng = mg.iterate(u, f)
        v = mg.iterate(u, f)
        assert v.requires_grad and torch.equal(v.detach(), v_ng)
        (v ** 2).sum().backward()
        gR, gP = mg.conv.net.weight.grad.clone(), mg.deconv.net.weight.grad.clone()
        mg.zero_grad()
        vm = mg.iterate_modules(u, f)
        (vm ** 2).sum().backward()
    finally:
        torch.set_default_device("cpu")
    for a, b in ((gR, mg.conv.net.weight.grad), (gP, mg.deconv.net.weight.grad)):
        assert (a - b).abs().max() <= 1e-4 * b.abs().max()


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem,n,m,B", [("poisson", 4, None, 1), ("poisson", 16, None, 2), ("poisson", 128, None, 1),
                                           ("poisson", 1024, None, 1), ("poisson", 256, 64, 2),
                                           ("interface", 32, None, 3), ("interface", 256, None, 1)])
def test_zero_guess_kernel_variants_bitwise(T, problem, n, m, B, monkeypatch):
    """The zero-guess level kernels have two launch forms each: the residual-restriction on overlapped strips
    (k_mg_zero_restrict, when v is not kept) or with per-lane halos (when v is stored); the prolongation +
    sweep of the recomputed iterate omd f on overlapped strips (levels <= FEANET_NT_BYTES / 4) or as
    k_mg_prolong<ZU> (larger levels: FEANET_NT_BYTES=0 makes this level one).  Both pairs are bitwise the
    same, including rows != columns and per-pattern learned R/P."""
    from feanet_amd import _lib
    rng = np.random.default_rng(13 * n + B)
    fr = Frame(n, B, T, problem, m=m)
    co = Frame(n // 2, B, T, problem, m=None if m is None else m // 2)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=problem == "interface")
    nt = ktab.shape[0]
    u, f = rand_state(rng, B, (fr.H, fr.W), T)
    fr.put("f", f)
    e = rng.standard_normal((B, co.H, co.W)).astype(npdt(T))
    e[:, 0, :] = e[:, -1, :] = e[:, :, 0] = e[:, :, -1] = 0

    def run(what, keep_v=False, small_nt=False):
        monkeypatch.delenv("FEANET_NT_BYTES", raising=False)
        if small_nt:
            monkeypatch.setenv("FEANET_NT_BYTES", "0")
        if what == "rr":
            co.put("f", e * 0 + 3.0)
            _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), fr.L.a.data_ptr() if keep_v else None,
                      co.L.f.data_ptr(), fr.pid(), kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, 1.25,
                      *fr.args(), co.L.ld, co.L.bs, None)
            return co.get("f")
        co.put("a", e)
        fr.put("b", u * 0 + 7.0)
        _lib.call("mg_prolong_sweep", T, None, co.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(),
                  co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, 0.75, *fr.args(), co.L.ld,
                  co.L.bs, None)
        return fr.get("b")

    rr = [run("rr", keep_v=True), run("rr")]
    assert np.array_equal(rr[0], rr[1])
    ps = [run("ps", small_nt=True), run("ps")]
    assert np.array_equal(ps[0], ps[1])
    assert (ps[0][:, 0, :] == 7).all() and (ps[0][:, :, -1] == 7).all()


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem,n,m,B", [("poisson", 8, None, 1), ("poisson", 16, None, 3), ("poisson", 64, None, 2),
                                           ("poisson", 256, None, 1), ("poisson", 512, None, 2),
                                           ("poisson", 2048, None, 1), ("poisson", 256, 64, 2),
                                           ("poisson", 64, 512, 1), ("poisson", 488, 120, 1),
                                           ("interface", 32, None, 3), ("interface", 256, None, 1),
                                           ("interface", 1024, None, 1)])
def test_zero_restrict2_bitwise(T, problem, n, m, B):
    """fea_mg_zero_restrict2 (two zero-guess restrictions in one pass) is bitwise the two single-level
    k_mg_zero_restrict launches it replaces — both outputs, every size (strip and task edges, rows != columns,
    one to several strips and row tasks), batch, dtype, and the two-material problem with per-pattern learned
    R; boundary nodes of both outputs are left untouched."""
    from feanet_amd import _lib
    rng = np.random.default_rng(7 * n + B)
    m_ = n if m is None else m
    fr = Frame(n, B, T, problem, m=m)
    c1 = Frame(n // 2, B, T, problem, m=m_ // 2)
    c2 = Frame(n // 4, B, T, problem, m=m_ // 4)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=problem == "interface")
    nt = ktab.shape[0]
    _, f = rand_state(rng, B, (fr.H, fr.W), T)
    fr.put("f", f)
    s1 = np.full((B, c1.H, c1.W), 3.0)
    s2 = np.full((B, c2.H, c2.W), 5.0)
    c1.put("f", s1)
    c2.put("f", s2)
    _lib.call("mg_residual_restrict", T, None, fr.L.f.data_ptr(), None, c1.L.f.data_ptr(), fr.pid(), kt.data_ptr(),
              om.data_ptr(), nt, rt.data_ptr(), nt, 1.25, *fr.args(), c1.L.ld, c1.L.bs, None)
    _lib.call("mg_residual_restrict", T, None, c1.L.f.data_ptr(), None, c2.L.f.data_ptr(), c1.pid(), kt.data_ptr(),
              om.data_ptr(), nt, rt.data_ptr(), nt, 1.25, *c1.args(), c2.L.ld, c2.L.bs, None)
    ref1, ref2 = c1.get("f"), c2.get("f")
    c1.put("f", s1)
    c2.put("f", s2)
    _lib.call("mg_zero_restrict2", T, fr.L.f.data_ptr(), c1.L.f.data_ptr(), c2.L.f.data_ptr(), fr.pid(), c1.pid(),
              kt.data_ptr(), om.data_ptr(), nt, rt.data_ptr(), nt, 1.25, *fr.args(), c1.L.ld, c1.L.bs, c2.L.ld,
              c2.L.bs, None)
    got1, got2 = c1.get("f"), c2.get("f")
    assert np.array_equal(got1, ref1), f"f_l+1: {np.argwhere(got1 != ref1)[:5]}"
    assert np.array_equal(got2, ref2), f"f_l+2: {np.argwhere(got2 != ref2)[:5]}"
    assert (got1[:, 0, :] == 3).all() and (got1[:, :, -1] == 3).all()
    assert (got2[:, -1, :] == 5).all() and (got2[:, :, 0] == 5).all()


def test_solver_pairs_restrictions():
    """The solver's plan at 4097^2 runs levels 1 and 2 as ONE fea_mg_zero_restrict2 launch going down and ONE
    fea_mg_prolong2 launch going up, and the V-cycle with and without the pairing is bitwise the same."""
    from feanet_amd.solver import MultigridSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    f = torch.randn(1, 1, 4097, 4097, dtype=torch.float64, device="cuda", generator=g)
    outs = []
    for pair in (True, False):
        s = MultigridSolver(4096, dtype=torch.float64, pair_levels=pair)
        names = [nm for nm, _ in s._plan("a")[0]]
        assert ("mg_zero_restrict2" in names) == pair and ("mg_prolong2" in names) == pair, names
        s.set_rhs(f=f)
        s.load()
        s.vcycle(3)
        outs.append(s.solution())
    assert torch.equal(outs[0], outs[1])


# bytes_per_vcycle() of tools/plan_dump.py's single-GPU configurations.  The literals are what the positional
# accounting printed (tools/plan_dump.py run on the commit before launch records were read by parameter name), not
# what the code under test gives.
_PINNED_BYTES = {
    "poisson n=1024 fp32": 18655300,
    "poisson n=512 fp32 MID_NODES=300000": 4594736,
    "poisson n=32 fp64 unfused V(2,2), no tail": 141696,
    "poisson n=32 fp64 unfused V(2,0), no tail": 101840,
    "interface n=32 fp64 compat=mm_interface_q2": 147975,
    "poisson n=128 fp64 zero_start": 450600,
    "interface n=128 fp32 B=2, 16-row R/P": 490796,
    "poisson n=256 fp32 B=64": 70584320,
    "hjac n=256 fp32": 2043964,
    "hjac n=512 fp32": 8377420,
    "hjac n=32 fp64 unfused": 80480,
}


def test_bytes_per_vcycle_pinned(monkeypatch):
    """The bench line's byte accounting (MultigridSolver.bytes_per_vcycle / _plan_bytes) on every configuration of
    the plan dumper: the pinned integers, and between them the plans meet every kernel name _plan_bytes has a branch
    for.  Builds solvers only; nothing is launched beyond construction."""
    import inspect
    import os
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tools.plan_dump import single_gpu_cases
    from feanet_amd.solver import MultigridSolver
    cases = single_gpu_cases()
    assert sorted(label for label, _, _ in cases) == sorted(_PINNED_BYTES)
    met = set()
    for label, make, mid_nodes in cases:
        if mid_nodes:  # read when the plan is built
            monkeypatch.setattr(MultigridSolver, "MID_NODES", mid_nodes)
        s = make()
        plan = s._plan("a")[0]
        monkeypatch.undo()
        met.update(name for name, _ in (plan[1:-1] if s._joinable() else plan))  # what _plan_bytes is handed
        got = s.bytes_per_vcycle()
        print(label, got)
        assert got == _PINNED_BYTES[label], label
    branches = set(re.findall(r'"(mg_[a-z0-9_]+)"', inspect.getsource(MultigridSolver._plan_bytes)))
    assert len(branches) == 17 and branches <= met, sorted(branches - met)


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem,n,m,B", [("poisson", 8, None, 1), ("poisson", 16, None, 3), ("poisson", 64, None, 2),
                                           ("poisson", 256, None, 1), ("poisson", 512, None, 2),
                                           ("poisson", 2048, None, 1), ("poisson", 256, 64, 2),
                                           ("poisson", 64, 512, 1), ("poisson", 488, 120, 1),
                                           ("interface", 32, None, 3), ("interface", 256, None, 1),
                                           ("interface", 1024, None, 1)])
def test_prolong2_bitwise(T, problem, n, m, B):
    """fea_mg_prolong2 (two recomputed-iterate prolongations + post-sweeps in one pass) is bitwise the two
    single-level fea_mg_prolong_sweep(u = NULL) launches it replaces, at every size (strip and task edges,
    rows != columns), batch, dtype, and on the two-material problem with per-pattern learned P; the output's
    boundary nodes are left untouched."""
    from feanet_amd import _lib
    rng = np.random.default_rng(11 * n + B)
    m_ = n if m is None else m
    fr = Frame(n, B, T, problem, m=m)
    c1 = Frame(n // 2, B, T, problem, m=m_ // 2)
    c2 = Frame(n // 4, B, T, problem, m=m_ // 4)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=problem == "interface")
    nt = ktab.shape[0]
    _, f0 = rand_state(rng, B, (fr.H, fr.W), T)
    _, f1 = rand_state(rng, B, (c1.H, c1.W), T)
    e2 = rng.standard_normal((B, c2.H, c2.W)).astype(npdt(T))
    e2[:, 0, :] = e2[:, -1, :] = e2[:, :, 0] = e2[:, :, -1] = 0
    fr.put("f", f0)
    c1.put("f", f1)
    c2.put("a", e2)
    c1.put("a", np.zeros((B, c1.H, c1.W)))
    sent = np.full((B, fr.H, fr.W), 7.0)
    fr.put("b", sent)
    _lib.call("mg_prolong_sweep", T, None, c2.L.a.data_ptr(), c1.L.f.data_ptr(), c1.L.a.data_ptr(), c1.pid(), c2.pid(),
              kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, 0.75, *c1.args(), c2.L.ld, c2.L.bs, None)
    _lib.call("mg_prolong_sweep", T, None, c1.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(), c1.pid(),
              kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, 0.75, *fr.args(), c1.L.ld, c1.L.bs, None)
    ref = fr.get("b")
    fr.put("b", sent)
    _lib.call("mg_prolong2", T, c1.L.f.data_ptr(), c2.L.a.data_ptr(), fr.L.f.data_ptr(), fr.L.b.data_ptr(), fr.pid(),
              c1.pid(), c2.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, 0.75, *fr.args(), c1.L.ld,
              c1.L.bs, c2.L.ld, c2.L.bs, None)
    got = fr.get("b")
    assert np.array_equal(got, ref), f"{np.argwhere(got != ref)[:5]}"
    assert (got[:, 0, :] == 7).all() and (got[:, :, -1] == 7).all() and (got[:, -1, :] == 7).all()


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("m,n,B,problem,cut", [(1024, 1024, 1, "poisson", (9, 16, 17)),
                                               (514, 258, 2, "poisson", (3, 4, 5)),
                                               (2048, 1024, 1, "poisson", (33, 64, 65)),
                                               (256, 256, 1, "interface", (5, 8, 9)), (64, 64, 2, "poisson", (1, 2, 1))])
def test_cycle_join_rects_bitwise(T, m, n, B, problem, cut):
    """fea_mg_cycle_join_rects (the join over rectangles: a domain-decomposed rank's four border strips in one
    launch, then its interior in another) covering the grid is bitwise the whole-grid fea_mg_cycle_join, both
    outputs; border strips of `cut` = (coarse rows, left fine columns (even), right fine columns (odd): rectangle
    bounds are odd) and a one-rectangle whole-grid launch."""
    from feanet_amd import _lib
    fr = Frame(n, B, T, problem, m=m)
    co = Frame(n // 2, B, T, problem, m=m // 2)
    ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=(problem == "interface"))
    nt = ktab.shape[0]
    rng = np.random.default_rng(m + n + B)
    u, f = rand_state(rng, B, (fr.H, fr.W), T)
    e = rng.standard_normal((B, co.H, co.W)).astype(npdt(T))
    e[:, 0] = e[:, -1] = e[:, :, 0] = e[:, :, -1] = 0
    fr.put("a", u)
    fr.put("f", f)
    co.put("a", e)
    head = (fr.L.a.data_ptr(), co.L.a.data_ptr(), fr.L.f.data_ptr())
    tail = (fr.pid(), co.pid(), kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(), nt, rt.data_ptr(), nt, 0.75, 1.25,
            *fr.args(), co.L.ld, co.L.bs)
    sent_c = np.full((B, co.H, co.W), 3.0)

    def run(rect_sets):
        out = fr.L.a.clone()
        co.put("f", sent_c)
        for rects in rect_sets:
            if rects is None:
                _lib.call("mg_cycle_join", T, *head, out.data_ptr(), co.L.f.data_ptr(), *tail, None, None, None, None)
            else:
                arr = (ctypes.c_int * (4 * len(rects)))(*[x for r in rects for x in r])
                _lib.call("mg_cycle_join_rects", T, *head, out.data_ptr(), co.L.f.data_ptr(), *tail, len(rects),
                          ctypes.addressof(arr), None)
        torch.cuda.synchronize()
        return fr.L.view(out).clone(), co.get("f").copy()

    Hc, W = co.H, fr.W
    a, cl, cr = cut
    border = [(1, 1 + a, 1, W - 1), (Hc - 1 - a, Hc - 1, 1, W - 1), (1 + a, Hc - 1 - a, 1, 1 + cl),
              (1 + a, Hc - 1 - a, W - 1 - cr, W - 1)]
    interior = [(1 + a, Hc - 1 - a, 1 + cl, W - 1 - cr)]
    ref_u, ref_f = run([None])
    for sets in ([border, interior], [interior, border], [[(1, Hc - 1, 1, W - 1)]]):
        got_u, got_f = run(sets)
        assert torch.equal(got_u, ref_u), (sets, (got_u - ref_u).abs().max().item())
        assert np.array_equal(got_f, ref_f), sets


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,m,nlev,B", [(128, None, 6, 1), (128, None, 6, 3), (128, None, 2, 2), (64, None, 5, 1),
                                        (16, None, 3, 2), (8, None, 2, 1), (128, 64, 2, 1), (64, 128, 3, 2)])
def test_coarse_tail_ext_bitwise(T, n, m, nlev, B):
    """fea_mg_coarse_tail_ext (the level X above the coarse tail restricted into the tail's LDS and prolonged back out
    of it inside the tail's launch) is bitwise the three launches it replaces: the zero-guess
    fea_mg_residual_restrict of X, fea_mg_coarse_tail on the next level, fea_mg_prolong_sweep(u = NULL) of X — at the
    65^2 / 6-level tail of every BASELINE plan (129^2 X) and the general tails (smaller, rows != columns), batches;
    X's boundary nodes are left untouched."""
    from feanet_amd import _lib
    rng = np.random.default_rng(29 * n + B)
    m_ = n if m is None else m
    X = Frame(n, B, T, "poisson", m=m)
    t = Frame(n // 2, B, T, "poisson", m=m_ // 2)
    ktab, omd, R, P, kt, om, rt, pt = tables("poisson", T)
    _, f = rand_state(rng, B, (X.H, X.W), T)
    X.put("f", f)
    sentinel = np.full((B, X.H, X.W), 7.0)
    X.put("a", sentinel)
    X.put("b", sentinel)
    w0, w1 = 1.25, 0.75
    _lib.call("mg_residual_restrict", T, None, X.L.f.data_ptr(), None, t.L.f.data_ptr(), None, kt.data_ptr(),
              om.data_ptr(), 1, rt.data_ptr(), 1, w0, *X.args(), t.L.ld, t.L.bs, None)
    _lib.call("mg_coarse_tail", T, t.L.f.data_ptr(), t.L.a.data_ptr(), t.H, t.W, nlev, t.L.ld, t.L.bs, None,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), pt.data_ptr(), w0, w1, 1, 1, 0, B, None)
    _lib.call("mg_prolong_sweep", T, None, t.L.a.data_ptr(), X.L.f.data_ptr(), X.L.a.data_ptr(), None, None,
              kt.data_ptr(), om.data_ptr(), 1, pt.data_ptr(), 1, w1, *X.args(), t.L.ld, t.L.bs, None)
    ref = X.get("a")
    _lib.call("mg_coarse_tail_ext", T, X.L.f.data_ptr(), X.L.b.data_ptr(), X.H, X.W, X.L.ld, X.L.bs, nlev,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), pt.data_ptr(), w0, w1, B, None)
    got = X.get("b")
    assert np.array_equal(got, ref), f"{np.argwhere(got != ref)[:5]}"
    assert (got[:, 0, :] == 7).all() and (got[:, -1, :] == 7).all() and (got[:, :, 0] == 7).all()
    assert (got[:, :, -1] == 7).all()


@pytest.mark.parametrize("T,n,B", [(torch.float64, 4096, 1), (torch.float64, 1024, 1), (torch.float32, 1024, 4),
                                   (torch.float64, 256, 2)])
def test_solver_tail_ext(T, n, B):
    """The solver's plan runs the level above the 65^2 tail inside the tail's launch (fea_mg_coarse_tail_ext) where
    the level pairing leaves it alone (4097^2: levels 1-2 and 3-4 paired, the 129^2 level 5 extended; 1025^2:
    levels 1-2 paired, level 3), and single / joined V-cycles with and without it are bitwise the same.  (By default
    only batches >= TAIL_EXT_MIN_BATCH take it; forced on here.)"""
    from feanet_amd.solver import MultigridSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    f = torch.randn(B, 1, n + 1, n + 1, dtype=T, device="cuda", generator=g)
    outs = []
    for ext in (True, False):
        s = MultigridSolver(n, dtype=T, batch=B)
        s.TAIL_EXT, s.TAIL_EXT_MIN_BATCH = ext, 1
        names = [nm for nm, _ in s._plan("a")[0]]
        assert ("mg_coarse_tail_ext" in names) == ext and ("mg_coarse_tail" in names) != ext, names
        s.set_rhs(f=f)
        s.load()
        s.vcycle(1)
        one = s.solution()
        s.vcycle(5)
        outs.append((one, s.solution()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_solver_tail_ext_default_by_batch():
    """TAIL_EXT_MIN_BATCH: the batch-1 plan keeps the streaming launches around the tail, a 64-sample plan extends it."""
    from feanet_amd.solver import MultigridSolver
    for B, ext in ((1, False), (64, True)):
        s = MultigridSolver(256, dtype=torch.float32, batch=B)
        names = [nm for nm, _ in s._plan("a")[0]]
        assert ("mg_coarse_tail_ext" in names) == ext, (B, names)
