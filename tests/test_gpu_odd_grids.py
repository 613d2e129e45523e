"""The coarse end of the V-cycle on grids that are not 2^k + 1 nodes wide.

MultigridSolver(n, rows=m) and the C ABI take any grid whose interval counts are divisible by 2^(L-1); the other GPU
files reach the coarse tail, the extended tail, the HJac tail and the multi-level launches almost only at 2^k + 1.
Here: fea_mg_coarse_tail and fea_mg_hjac_tail against the oracle restatements of their sub-cycles
(test_schedule.tail_oracle / hjac_tail_oracle), fea_mg_coarse_tail_ext bitwise against its three launches, and whole
solvers against the oracle's MultiGrid.Step, on level heights 49 / 41 / 45 / 37 (three rows per wave of the fused
tail), even coarsest levels (4, 6, 8, 64 nodes), tails with rows != columns, and a 97-row level above the tail.
tests/test_tail_partition_host.py restates the tail's wave partition and asserts that TAIL_SHAPES and EXT_SHAPES
reach every template body of it.

Tolerances are the project's: a kernel against the oracle TOL (scaled max error 1e-12 fp64, 5e-6 fp32); a solver
against the oracle 1e-10 per cycle in fp64, 2e-5 on the first cycle in fp32 and the residual norms as
test_gpu_mg.test_vcycle_rect_vs_oracle."""
import numpy as np
import pytest
import torch

from oracle import feanet_oracle as orc
from test_gpu_mg import Frame, close, npdt, rand_state, tables

pytestmark = pytest.mark.gpu

W0, W1 = 1.25, 0.75  # restriction / prolongation ratios (the other tail tests only pass 1.0)
NUS = [(1, 1), (2, 1), (0, 2), (1, 0)]  # (1, 1): the fused row-wave path; the others: the general path

# (Ht, Wt, nlev) of fea_mg_coarse_tail.  Rows per wave of the fused path (16 waves): H = 49 / 41 / 45 / 37 -> 3
# (both window parities), 65 / 57 -> 4, 33 / 25 / 21 -> 2, <= 18 -> 1; coarsest levels of 4, 6 and 8 nodes; nlev = 1
# tails, whose only phase is the coarsest one, at 1, 2, 3 and 4 rows per wave and at 64 nodes (the largest even count)
TAIL_SHAPES = [
    (49, 49, 5), (49, 25, 4), (25, 49, 4),
    (41, 57, 4), (57, 41, 4), (45, 45, 3), (37, 37, 3),
    (13, 13, 3), (7, 13, 2), (21, 13, 3),
    (65, 33, 5), (33, 65, 5), (65, 49, 5),
    (4, 4, 1), (6, 8, 1), (64, 64, 1), (65, 65, 1), (49, 3, 1), (25, 33, 1),
]
# (Hx, Wx, nlev) of fea_mg_coarse_tail_ext: level X on top of an ((Hx + 1) / 2) x ((Wx + 1) / 2) tail of nlev levels.
# Fine rows per wave going up: 25 -> 2, 49 -> 4, 97 / 81 / 89 -> 6 (of the compiled 8: the last wave's window is
# clipped in the middle), 113 / 129 -> 8
EXT_SHAPES = [
    (97, 97, 5), (97, 97, 2), (97, 49, 4), (49, 97, 4), (113, 81, 4), (81, 113, 4), (25, 25, 3), (129, 97, 5),
    (89, 73, 3),
]


def level_maps(Ht, Wt, nlev):
    """Two-material pattern maps of an Ht x Wt tail: the level maps of the square of max(Ht, Wt) nodes, cut to a
    window whose offset on the top level is divisible by 2^(nlev-1) (so the window is the same nodes on every level,
    as a domain-decomposed rank's window of the global maps); the whole maps for a square."""
    from feanet_amd import mesh_setup as ms
    S, step = max(Ht, Wt), 1 << (nlev - 1)
    r0, c0 = (S - Ht) // 2 // step * step, (S - Wt) // 2 // step * step
    maps = []
    for k in range(nlev):
        full = ms.interface_pattern_map(((S - 1) >> k) + 1)
        h, w = ((Ht - 1) >> k) + 1, ((Wt - 1) >> k) + 1
        maps.append(np.ascontiguousarray(full[r0 >> k:(r0 >> k) + h, c0 >> k:(c0 >> k) + w]))
    return maps


_HIER = {}


def hierarchy(Ht, Wt, nlev, problem, T):
    """(oracle hierarchy of the tail's levels with w = (W0, W1), device tables, compact pattern maps), cached; the
    two-material problem with learned per-pattern R / P on maps that keep the stiffness table symmetric."""
    key = (Ht, Wt, nlev, problem, T)
    if key not in _HIER:
        from feanet_amd import mesh_setup as ms
        ktab, omd, R, P, kt, om, rt, pt = tables(problem, T, learned=problem == "interface")
        pids = pidl = None
        if problem == "interface":
            maps = level_maps(Ht, Wt, nlev)
            for m in maps:
                assert ms.stencil_mirror_mismatches(ktab, m) == 0
            pids = {m.shape: m for m in maps}
            pidl = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
        mg = orc.OracleMultigrid(Wt - 1, problem, npdt(T), levels=nlev, rows=Ht - 1, rtab=R, ptab=P, w=(W0, W1),
                                 pids=pids)
        assert [(lv.H, lv.W) for lv in mg.levels] == [(((Ht - 1) >> k) + 1, ((Wt - 1) >> k) + 1) for k in range(nlev)]
        _HIER[key] = (mg, (kt, om, ktab.shape[0], rt, pt), pidl)
    return _HIER[key]


def zero_boundary(rng, B, H, W, T):
    f = rng.standard_normal((B, H, W)).astype(npdt(T))
    f[:, 0, :] = f[:, -1, :] = f[:, :, 0] = f[:, :, -1] = 0
    return f


def boundary_keeps(got, val):
    return ((got[:, 0, :] == val).all() and (got[:, -1, :] == val).all() and (got[:, :, 0] == val).all()
            and (got[:, :, -1] == val).all())


# ----------------------------------------------------------------------------- a. fea_mg_coarse_tail
@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("Ht,Wt,nlev", TAIL_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nu", NUS)
def test_coarse_tail_odd_grids(T, problem, Ht, Wt, nlev, B, nu):
    """fea_mg_coarse_tail against the oracle restatement of its sub-cycle: interior to TOL, boundary nodes of the
    output untouched."""
    from feanet_amd import _lib
    from test_schedule import tail_oracle
    mg, (kt, om, ntab, rt, pt), pidl = hierarchy(Ht, Wt, nlev, problem, T)
    rng = np.random.default_rng(1000 * Ht + 10 * Wt + nlev + B)
    f = zero_boundary(rng, B, Ht, Wt, T)
    ref = tail_oracle(mg, 0, f, None, B, nu1=nu[0], nu2=nu[1], q2=False)
    fr = Frame(Wt - 1, B, T, "poisson", m=Ht - 1)
    fr.put("f", f)
    fr.put("a", np.full((B, Ht, Wt), 7.0))
    _lib.call("mg_coarse_tail", T, fr.L.f.data_ptr(), fr.L.a.data_ptr(), Ht, Wt, nlev, fr.L.ld, fr.L.bs,
              None if pidl is None else pidl.data_ptr(), kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(),
              pt.data_ptr(), W0, W1, nu[0], nu[1], 0, B, None)
    got = fr.get("a")
    what = f"tail {Ht}x{Wt} nlev={nlev} B={B} nu={nu} {problem}"
    assert boundary_keeps(got, 7.0), f"{what}: a boundary node was written"
    close(got[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, what)


# ----------------------------------------------------------------------------- b. fea_mg_coarse_tail_ext
@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("Hx,Wx,nlev", EXT_SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_coarse_tail_ext_odd_grids(T, Hx, Wx, nlev, B):
    """fea_mg_coarse_tail_ext is bitwise the three launches it replaces (test_gpu_mg.test_coarse_tail_ext_bitwise)
    where the level above the tail is not 2^k + 1 rows high; X's boundary nodes keep their sentinel and the frame
    around X (padding, ghost rows) holds the reference launches' bytes."""
    from feanet_amd import _lib
    rng = np.random.default_rng(29 * Hx + Wx + B)
    X = Frame(Wx - 1, B, T, "poisson", m=Hx - 1)
    t = Frame((Wx - 1) // 2, B, T, "poisson", m=(Hx - 1) // 2)
    _, _, _, _, kt, om, rt, pt = tables("poisson", T)
    _, f = rand_state(rng, B, (X.H, X.W), T)
    X.put("f", f)
    sentinel = np.full((B, X.H, X.W), 7.0)
    X.put("a", sentinel)
    X.put("b", sentinel)
    _lib.call("mg_residual_restrict", T, None, X.L.f.data_ptr(), None, t.L.f.data_ptr(), None, kt.data_ptr(),
              om.data_ptr(), 1, rt.data_ptr(), 1, W0, *X.args(), t.L.ld, t.L.bs, None)
    _lib.call("mg_coarse_tail", T, t.L.f.data_ptr(), t.L.a.data_ptr(), t.H, t.W, nlev, t.L.ld, t.L.bs, None,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), pt.data_ptr(), W0, W1, 1, 1, 0, B, None)
    _lib.call("mg_prolong_sweep", T, None, t.L.a.data_ptr(), X.L.f.data_ptr(), X.L.a.data_ptr(), None, None,
              kt.data_ptr(), om.data_ptr(), 1, pt.data_ptr(), 1, W1, *X.args(), t.L.ld, t.L.bs, None)
    ref = X.get("a")
    assert boundary_keeps(ref, 7.0) and (ref[:, 1:-1, 1:-1] != 7).any()
    _lib.call("mg_coarse_tail_ext", T, X.L.f.data_ptr(), X.L.b.data_ptr(), X.H, X.W, X.L.ld, X.L.bs, nlev,
              kt.data_ptr(), om.data_ptr(), 1, rt.data_ptr(), pt.data_ptr(), W0, W1, B, None)
    got = X.get("b")
    assert np.array_equal(got, ref), f"{np.argwhere(got != ref)[:5]}"
    assert boundary_keeps(got, 7.0)
    assert torch.equal(X.L.b, X.L.a), "the frame of the output differs"


# ----------------------------------------------------------------------------- c. fea_mg_hjac_tail
HJAC_SHAPES = [(49, 49, 5, (torch.float32,)), (25, 25, 4, (torch.float32, torch.float64)),
               (25, 49, 4, (torch.float32, torch.float64)), (13, 21, 3, (torch.float32, torch.float64))]


@pytest.mark.parametrize("Ht,Wt,nlev,T", [(h, w, k, T) for h, w, k, Ts in HJAC_SHAPES for T in Ts])
@pytest.mark.parametrize("problem", ["poisson", "interface"])
@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("nu", [(1, 1), (2, 1), (0, 1)])
def test_hjac_tail_odd_grids(Ht, Wt, nlev, T, problem, nl, nu):
    """fea_mg_hjac_tail called directly, against the oracle restatement of its sub-cycle (HRelax sweeps)."""
    from feanet_amd import _lib
    from test_schedule import hjac_tail_oracle
    B = 2
    mg, (kt, om, ntab, rt, pt), pidl = hierarchy(Ht, Wt, nlev, problem, T)
    rng = np.random.default_rng(100 * Ht + Wt + nl)
    hw = (0.25 * rng.standard_normal((nl, 3, 3))).astype(np.float32)
    f = zero_boundary(rng, B, Ht, Wt, T)
    mg.nu, mg.hw = nu, hw
    ref = hjac_tail_oracle(mg, 0, f, B)
    hwt = torch.from_numpy(hw.reshape(-1)).cuda().to(T)
    fr = Frame(Wt - 1, B, T, "poisson", m=Ht - 1)
    fr.put("f", f)
    fr.put("a", np.full((B, Ht, Wt), 7.0))
    _lib.call("mg_hjac_tail", T, fr.L.f.data_ptr(), fr.L.a.data_ptr(), Ht, Wt, nlev, fr.L.ld, fr.L.bs,
              None if pidl is None else pidl.data_ptr(), kt.data_ptr(), om.data_ptr(), ntab, rt.data_ptr(),
              pt.data_ptr(), hwt.data_ptr(), nl, W0, W1, nu[0], nu[1], B, None)
    got = fr.get("a")
    what = f"hjac tail {Ht}x{Wt} nlev={nlev} nl={nl} nu={nu} {problem}"
    assert boundary_keeps(got, 7.0), f"{what}: a boundary node was written"
    close(got[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, what)


def plan_names(s):
    return [nm for nm, _ in s._plan("a")[0]]


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,m", [(96, 96), (192, 96)])
def test_hjac_tail_solver_bitwise_odd_grids(T, n, m):
    """test_gpu_hnet.test_hjac_tail_bitwise on 97^2 and 97 x 193 nodes: whole learned-smoother V-cycles with the
    coarse levels in one fea_mg_hjac_tail launch are bitwise the per-level sequence."""
    from feanet_amd.solver import MultigridSolver
    B, nl = 2, 3
    rng = np.random.default_rng(n + m)
    hw = (0.25 * rng.standard_normal((nl, 3, 3))).astype(np.float32)
    f = torch.from_numpy(rng.standard_normal((B, 1, m + 1, n + 1))).to("cuda", T)
    out = []
    for tail in (True, False):
        s = MultigridSolver(n, rows=m, dtype=T, batch=B, smoother="hjac", hnet=hw, coarse_tail=tail)
        assert ("mg_hjac_tail" in plan_names(s)) == tail, plan_names(s)
        if tail:
            assert (s.levels[s.hjac_tail_from].H, s.levels[s.hjac_tail_from].W) == ((49, 49) if n == m else (25, 49))
        s.set_rhs(f=f)
        s.load()
        sols = []
        for _ in range(3):
            s.vcycle()
            sols.append(s.solution())
        out.append(sols)
    for k, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), (k, (a - b).abs().max().item())


# ----------------------------------------------------------------------------- d. whole solvers
_PROBLEMS = {}


def seeded_problem(T, n, m, B, tag="", **okw):
    """A seeded iterate and right-hand side on (m + 1) x (n + 1) nodes and the oracle's iterates and residual norms of
    three MultiGrid.Step cycles from them (cached under `tag`: the solver variants of one grid share them)."""
    key = (T, n, m, B, tag)
    if key not in _PROBLEMS:
        H, W = m + 1, n + 1
        rng = np.random.default_rng(m + n)
        mg = orc.OracleMultigrid(n, dtype=npdt(T), rows=m, **okw)
        u0 = rng.standard_normal((B, H, W)).astype(npdt(T))
        f = rng.standard_normal((B, H, W)).astype(npdt(T))
        geo, _ = orc.square_geometry((H, W), npdt(T))
        v = u0 * geo
        r0 = orc.interior_norm(f - mg.levels[0].K(v))
        vs, rs = [], []
        for _ in range(3):
            v = mg.step(v, f)
            vs.append(v)
            rs.append(orc.interior_norm(f - mg.levels[0].K(v)))
        _PROBLEMS[key] = (u0, f, r0, vs, rs)
    return _PROBLEMS[key]


def run_vs_oracle(s, T, prob):
    """Three single cycles, then vcycle(3) joined from the same start, against the oracle; returns the four iterates
    for bitwise comparisons between solver variants."""
    u0, f, r0, vs, rs = prob
    B, H, W = f.shape
    cu = lambda a: torch.from_numpy(a).cuda().reshape(B, 1, H, W)
    f64 = T == torch.float64
    rtol, atol = (1e-9, 1e-12 * r0.max()) if f64 else (2e-3, 1e-6 * r0.max())
    s.set_rhs(f=cu(f))
    s.load(cu(u0))
    sols = []
    for k in range(3):
        s.vcycle()
        sols.append(s.solution())
        got = sols[-1].cpu().numpy()[:, 0]
        if f64 or k == 0:
            err = np.abs(got - vs[k]).max() / max(1.0, np.abs(vs[k]).max())
            assert err < (1e-10 if f64 else 2e-5), f"cycle {k}: {err:.3e}"
        np.testing.assert_allclose(s.residual_norm().cpu().numpy(), rs[k], rtol=rtol, atol=atol)
    s.load(cu(u0))
    s.vcycle(3)
    sols.append(s.solution())
    if f64:
        got = sols[-1].cpu().numpy()[:, 0]
        err = np.abs(got - vs[2]).max() / max(1.0, np.abs(vs[2]).max())
        assert err < 1e-10, f"vcycle(3): {err:.3e}"
    np.testing.assert_allclose(s.residual_norm().cpu().numpy(), rs[2], rtol=rtol, atol=atol)
    return sols


def levels_of(s):
    return [(Lv.H, Lv.W) for Lv in s.levels]


_SOLS_96 = {}


def solver_96(T, tail):
    """MultigridSolver(96, rows=96) with / without the coarse tail, run against the oracle; its iterates, cached."""
    from feanet_amd.solver import MultigridSolver
    if (T, tail) not in _SOLS_96:
        s = MultigridSolver(96, rows=96, dtype=T, batch=2, coarse_tail=tail)
        assert levels_of(s) == [(k, k) for k in (97, 49, 25, 13, 7, 4)]
        assert ("mg_coarse_tail" in plan_names(s)) == tail and (s.tail_from == 1) == tail
        _SOLS_96[T, tail] = run_vs_oracle(s, T, seeded_problem(T, 96, 96, 2, levels=6))
    return _SOLS_96[T, tail]


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("tail", [True, False])
def test_solver_96_vs_oracle(T, tail):
    """MultigridSolver(96, rows=96): levels 97, 49, 25, 13, 7, 4; the coarse tail is 49^2 with five levels (three
    rows per wave on top, a 4^2 coarsest level).  With and without the tail, against the oracle."""
    solver_96(T, tail)


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
def test_solver_96_tail_on_off_bitwise(T):
    """The 97^2 solver with the coarse tail and with one launch per level op: the same bytes.  (This test found
    the tail summing its prolongation in another order than crow_term of the streaming kernels: 3.6e-15 in fp64 and
    1.4e-6 in fp32 after one cycle, at 2^k + 1 grids as well.)"""
    for a, b in zip(solver_96(T, True), solver_96(T, False)):
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,m,top,tail", [(96, 48, (49, 97), (25, 49)), (80, 112, (113, 81), (57, 41)),
                                          (192, 96, (97, 193), (25, 49))])
def test_solver_rect_odd_grids(T, n, m, top, tail):
    """Rectangles whose levels are not 2^k + 1: 49 x 97 (tail 25 x 49, coarsest 4 x 7), 113 x 81 (tail 57 x 41,
    coarsest 8 x 6) and 97 x 193."""
    from feanet_amd.solver import MultigridSolver
    s = MultigridSolver(n, rows=m, dtype=T, batch=2)
    assert levels_of(s)[0] == top and levels_of(s)[s.tail_from] == tail
    run_vs_oracle(s, T, seeded_problem(T, n, m, 2, levels=s.L))


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
@pytest.mark.parametrize("learned", [False, True])
def test_solver_96_two_material(T, learned):
    """The two-material problem on 97^2 nodes (maps of 97, 49, 25, 13, 7 and 4 nodes a side), with the bilinear and
    with learned per-pattern R / P."""
    from feanet_amd.solver import MultigridSolver
    _, _, R, P, _, _, _, _ = tables("interface", T, learned=learned)
    kw = dict(R=R, P=P) if learned else {}
    s = MultigridSolver(96, rows=96, problem="interface", dtype=T, batch=2, **kw)
    assert s.tail_from == 1 and "mg_coarse_tail" in plan_names(s)
    okw = dict(rtab=R, ptab=P) if learned else {}
    run_vs_oracle(s, T, seeded_problem(T, 96, 96, 2, tag=f"interface {learned}", problem="interface", levels=6, **okw))


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
def test_solver_96_hjac(T):
    """smoother="hjac" on 97^2 nodes against the oracle's Step with every sweep an HRelax (as
    test_gpu_hnet.test_hjac_vcycle_vs_oracle)."""
    from feanet_amd.solver import MultigridSolver
    n, B = 96, 2
    rng = np.random.default_rng(11)
    hw = (0.2 * rng.standard_normal((3, 3, 3))).astype(np.float32)
    mg = orc.OracleMultigrid(n, "poisson", npdt(T), levels=6, rows=n)
    for l in mg.levels:
        l.sweep = (lambda ll, o: (lambda v, ff: (lambda j: j + orc.hnet(j - v, ll.geo, hw))(o(v, ff))))(l, l.sweep)
    f = rng.standard_normal((B, n + 1, n + 1)).astype(npdt(T))
    s = MultigridSolver(n, rows=n, dtype=T, batch=B, smoother="hjac", hnet=hw)
    assert "mg_hjac_tail" in plan_names(s)
    s.set_rhs(f=torch.from_numpy(f).cuda().reshape(B, 1, n + 1, n + 1))
    s.load()
    v = np.zeros((B, n + 1, n + 1), npdt(T))
    for k in range(3):
        s.vcycle()
        v = mg.step(v, f)
        got = s.solution().cpu().numpy()[:, 0]
        if T == torch.float64 or k == 0:
            err = np.abs(got - v).max() / max(1.0, np.abs(v).max())
            assert err < (1e-10 if T == torch.float64 else 2e-5), (k, err)


PLAN_768 = ["mg_sweep_restrict", "mg_zero_restrict2", "mg_residual_restrict", "mg_coarse_tail", "mg_mid_up",
            "mg_prolong_sweep"]
PLAN_768_BOTH = ["mg_sweep_restrict", "mg_mid_down", "mg_coarse_tail", "mg_mid_up", "mg_prolong_sweep"]


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
def test_solver_768(T):
    """MultigridSolver(768, rows=768) takes the shipped default plan on 769^2 nodes: the cycle join on 769^2, the
    register-strip fea_mg_mid_up over 385 / 193 / 97 and a 49^2 five-level tail.  Against the oracle; with both
    three-level switches on the five-launch plan, bitwise the same."""
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    prob = seeded_problem(T, 768, 768, 1, levels=9)
    outs = []
    for both in (False, True):
        s = MultigridSolver(768, rows=768, dtype=T)
        if both:
            s.THREE_LEVEL_DOWN = s.THREE_LEVEL_UP = True
        assert plan_names(s) == (PLAN_768_BOTH if both else PLAN_768), plan_names(s)
        tail = [rec for rec in s._plan("a")[0] if rec[0] == "mg_coarse_tail"][0]
        assert (_lib.arg(tail, "Ht"), _lib.arg(tail, "Wt"), _lib.arg(tail, "nlev")) == (49, 49, 5)
        assert s._joinable()
        outs.append(run_vs_oracle(s, T, prob))
    for a, b in zip(*outs):
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
def test_solver_192_tail_ext(T):
    """MultigridSolver(192, rows=192) with TAIL_EXT_MIN_BATCH = 1 runs the 97^2 level inside the tail's launch
    (fea_mg_coarse_tail_ext), bitwise the plan without it (test_gpu_mg.test_solver_tail_ext)."""
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    B = 2
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    f = torch.randn(B, 1, 193, 193, dtype=T, device="cuda", generator=g)
    outs = []
    for ext in (True, False):
        s = MultigridSolver(192, rows=192, dtype=T, batch=B)
        s.TAIL_EXT, s.TAIL_EXT_MIN_BATCH = ext, 1
        names = plan_names(s)
        assert ("mg_coarse_tail_ext" in names) == ext and ("mg_coarse_tail" in names) != ext, names
        if ext:
            rec = [r for r in s._plan("a")[0] if r[0] == "mg_coarse_tail_ext"][0]
            assert (_lib.arg(rec, "Hx"), _lib.arg(rec, "Wx")) == (97, 97)
        s.set_rhs(f=f)
        s.load()
        s.vcycle(1)
        one = s.solution()
        s.vcycle(5)
        outs.append((one, s.solution()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_pcg_96_tail_on_and_off(monkeypatch):
    """PCGSolver(96, rows=96): the preconditioning V-cycle with its 49^2 tail in one launch and with one launch per
    level op gives the same iteration count and bitwise the same solution."""
    from feanet_amd import pcg
    from feanet_amd.solver import MultigridSolver
    rng = np.random.default_rng(96)
    f = torch.from_numpy(rng.standard_normal((2, 1, 97, 97))).cuda()
    runs = []
    for tail in (True, False):
        monkeypatch.setattr(pcg, "MultigridSolver", lambda *a, _t=tail, **kw: MultigridSolver(*a, coarse_tail=_t, **kw))
        s = pcg.PCGSolver(96, rows=96, batch=2)
        assert (s.mg.tail_from == 1) == tail and ("mg_coarse_tail" in plan_names(s.mg)) == tail
        u, hist = s.solve(f=f, rtol=1e-10, max_iters=60)
        assert (s.flags == 1).all(), s.flags
        runs.append((u, np.array(hist), s.iterations.copy()))
    assert np.array_equal(runs[0][2], runs[1][2]), (runs[0][2], runs[1][2])
    assert torch.equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("T", [torch.float64, torch.float32])
def test_solve_96x48_matches_per_cycle_loop(T):
    """solve(eps) on 49 x 97 nodes: the device-resident joined loop against the per-cycle driver loop, as
    test_gpu_mg.test_solve_joined_matches_per_cycle_loop (same number of cycles, bitwise the same iterate)."""
    from feanet_amd.solver import MultigridSolver
    n, m, B = 96, 48, 2
    rng = np.random.default_rng(n + m + B)
    f = torch.from_numpy(rng.standard_normal((B, 1, m + 1, n + 1))).cuda().to(T)
    bc = torch.from_numpy(rng.random((B, 1, m + 1, n + 1))).cuda().to(T)
    ref_s = MultigridSolver(n, rows=m, dtype=T, batch=B, join_cycles=False)
    s = MultigridSolver(n, rows=m, dtype=T, batch=B)
    r0 = None
    for rel in (1e-2, 1e-6, 0.0):
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
        assert len(ha) == len(hb), (rel, eps, len(ha), len(hb))
        assert torch.equal(ua, ub), (rel, (ua - ub).abs().max().item())
        np.testing.assert_allclose(np.array(hb), np.array(ha), rtol=1e-11 if T == torch.float64 else 1e-5,
                                   atol=1e-14 * r0)
        s.vcycle()
        ref_s.vcycle()
        assert torch.equal(s.solution(), ref_s.solution())
