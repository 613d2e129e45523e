"""Full-multigrid start on the GPU: the three kernels of include/feanet_fmg.h against tests/fmg_ref.py (derived
bound), their write footprint and padding independence (tests/footprint.py's method), fea_fmg_restrict bitwise
against fea_mg_residual_restrict, and MultigridSolver.fmg against the driver composed from the CPU oracle."""
import os
import re

import numpy as np
import pytest
import torch

import fmg_ref as fr
from footprint import C1, C2, Geo, canary
from generic_ref import U

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NP = {"f32": np.float32, "f64": np.float64}
TT = {"f32": torch.float32, "f64": torch.float64}
ESZ = {"f32": 4, "f64": 8}


# ----------------------------------------------------------------------------- raw framed buffers and calls
def coarse_geo(g):
    """The (H+1)/2 x (W+1)/2 level of g; a direction of 2 nodes takes the pitch of 3 (fea_mg_layout starts at 3)."""
    from feanet_amd import _lib
    Hc, Wc = (g.H + 1) // 2, (g.W + 1) // 2
    ld, bs = _lib.mg_layout(max(Hc, 3), max(Wc, 3), g.esz)
    return Geo(Hc, Wc, g.B, g.esz, ld, bs)


def call(name, suf, raws, **scal):
    """fea_<name>_<suf> on copies of the raw host buffers `raws` (operand -> array, None for NULL, or the name of
    the operand it aliases); returns the buffers after the call."""
    from feanet_amd import _lib
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in raws.items() if isinstance(v, np.ndarray)}

    def value(p):
        if p not in raws:
            return scal[p]
        v = raws[p]
        return None if v is None else dev[v if isinstance(v, str) else p].data_ptr()
    names = [p.split()[1] for p in (_lib._FMG.get(name) or _lib._SIGS[name])[:-1]]
    _lib.call(name, TT[suf], *[value(p) for p in names], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dev.items()}


def pitches(g, cg):
    return dict(B=g.B, H=g.H, W=g.W, ld=g.ld, bstride=g.bs, ldc=cg.ld, bstridec=cg.bs)


def nodes_of(g, raw):
    return raw[g.index(np.arange(g.H), np.arange(g.W))]


def draw(rng, *shape):
    """standard normal fp32 values: the f32 and the f64 kernel read the same numbers"""
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def prolong_case(suf, H, W, B, order, mode, seed=0, fill=0.0):
    """One fea_fmg_prolong call; mode "null" (u NULL), "given" or "inplace" (out == u).  Returns (got nodes of out,
    reference, companion S), all [B, H, W] fp64 except got."""
    g = Geo(H, W, B, ESZ[suf])
    cg = coarse_geo(g)
    rng = np.random.default_rng([seed, H, W])
    e = draw(rng, B, cg.H, cg.W)
    u = None if mode == "null" else draw(rng, B, H, W)
    raws = {"ec": cg.framed(e, fill, NP[suf]), "u": None if u is None else g.framed(u, fill, NP[suf]),
            "out": "u" if mode == "inplace" else canary(g.numel, NP[suf], C1)}
    after = call("fmg_prolong", suf, raws, order=order, **pitches(g, cg))
    got = nodes_of(g, after["u" if mode == "inplace" else "out"])
    return got, fr.prolong(u, e, order), fr.prolong(u, e, order, absolute=True)


def check_prolong(suf, got, ref, S, what):
    inner = (slice(None), slice(1, -1), slice(1, -1))
    err = np.abs(got[inner].astype(np.float64) - ref[inner])
    bound = 2 * sum(fr.NM) * U[suf] * S[inner]
    worst = float((err / np.where(bound > 0, bound, 1)).max()) if err.size else 0.0
    print(f"fmg_prolong {suf} {what}: err/bound = {worst:.3g}")
    assert np.all(err <= bound), f"{what}: error is {worst:.3g} times its bound"


# ----------------------------------------------------------------------------- kernels against the reference
SMALL = [3, 5, 7, 9, 17]  # 2, 3, 4, 5, 9 coarse nodes: fallback, overlapping one-sided rows, first central row
EDGES = {"f64": [129, 131, 259], "f32": [257, 259, 515]}  # one strip exactly, two more columns, past two strips


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("order", [1, 3])
def test_prolong_small_grids(suf, order):
    for n in SMALL:
        for mode in ("null", "given", "inplace"):
            got, ref, S = prolong_case(suf, n, n, 1, order, mode)
            check_prolong(suf, got, ref, S, f"{n}x{n} order {order} u {mode}")
    # rectangles: the two directions fall back independently (2 coarse rows, 5 coarse columns and the reverse)
    for H, W in ((3, 9), (9, 3), (5, 17), (7, 5)):
        got, ref, S = prolong_case(suf, H, W, 2, order, "given")
        check_prolong(suf, got, ref, S, f"{H}x{W} order {order}")


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_prolong_strip_edges_and_batch(suf):
    for W in EDGES[suf]:
        for order in (1, 3):
            got, ref, S = prolong_case(suf, 9, W, 1, order, "given")
            check_prolong(suf, got, ref, S, f"9x{W} order {order}")
    for mode in ("null", "given", "inplace"):
        got, ref, S = prolong_case(suf, 17, EDGES[suf][1], 3, 3, mode)
        check_prolong(suf, got, ref, S, f"batch 3, u {mode}")


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_prolong_task_heights_bitwise(suf):
    """4097 x 33: one sample marches 2 rows per task, 16 samples 32 rows per task; every sample of the batch is
    bitwise its own run (the batch holds the single run's sample 16 times)."""
    H, W = 4097, 33
    got1, ref, S = prolong_case(suf, H, W, 1, 3, "given", seed=7)
    check_prolong(suf, got1, ref, S, "4097x33 batch 1")
    g = Geo(H, W, 16, ESZ[suf])
    cg = coarse_geo(g)
    rng = np.random.default_rng([7, H, W])
    e, u = draw(rng, 1, cg.H, cg.W), draw(rng, 1, H, W)
    raws = {"ec": cg.framed(np.repeat(e, 16, 0), 0.0, NP[suf]), "u": g.framed(np.repeat(u, 16, 0), 0.0, NP[suf]),
            "out": canary(g.numel, NP[suf], C1)}
    got16 = nodes_of(g, call("fmg_prolong", suf, raws, order=3, **pitches(g, cg))["out"])
    for b in range(16):
        assert np.array_equal(got16[b, 1:-1, 1:-1], got1[0, 1:-1, 1:-1]), b


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_boundary_values(suf):
    for H, W, B, stride in ((3, 3, 1, 1), (9, 131, 3, 2), (17, 5, 2, 4), (65, 65, 1, 1)):
        g = Geo(H, W, B, ESZ[suf])
        Hf, Wf = (H - 1) * stride + 1, (W - 1) * stride + 1
        bc = draw(np.random.default_rng([H, W, stride]), B, Hf, Wf).astype(NP[suf])
        before = canary(g.numel, NP[suf], C1)
        for src, per in ((bc, Hf * Wf), (bc[:1], 0), (None, 0)):
            raws = {"bc": None if src is None else np.ascontiguousarray(src).ravel(), "dst": before}
            got = nodes_of(g, call("fmg_boundary", suf, raws, bc_bstride=per, stride=stride, B=B, H=H, W=W, ld=g.ld,
                                   bstride=g.bs)["dst"])
            want = nodes_of(g, before).copy()
            samp = np.zeros((B, H, W), NP[suf]) if src is None else np.broadcast_to(src[:, ::stride, ::stride],
                                                                                     (B, H, W))
            for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0),
                       (slice(None), slice(None), -1)):
                want[sl] = samp[sl]
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (H, W, B, stride)


# ----------------------------------------------------------------------------- footprint
def footprint(name, suf, inputs, outputs, scal):
    """tests/footprint.py's two runs.  inputs: operand -> (Geo, nodes) or a plain array (bc); outputs: operand ->
    (Geo, write mask, nodes or None); an output with nodes is in place (its canary is its own content), and an
    input may be the NAME of such an output (out == u).  Asserts (a) - (d) of footprint.py on bytes."""
    dt = NP[suf]
    runs = {}
    for run, fill, byte in (("Z", 0.0, C1), ("P", np.nan, C2)):
        raws = {}
        for k, v in inputs.items():
            raws[k] = v if v is None or isinstance(v, str) else (v[0].framed(v[1], fill, dt) if isinstance(v, tuple)
                                                                 else np.asarray(v, dt))
        for k, (g, mask, nodes) in outputs.items():
            raws[k] = canary(g.numel, dt, byte) if nodes is None else g.framed(nodes, fill, dt)
        after = call(name, suf, raws, **scal)
        for k, v in raws.items():
            if not isinstance(v, np.ndarray):
                continue
            b, a = v.view(np.uint8).reshape(len(v), -1), after[k].view(np.uint8).reshape(len(v), -1)
            same = (a == b).all(axis=1)
            if k in outputs:
                g, mask, _ = outputs[k]
                bad = np.flatnonzero(~same & ~mask)
                assert bad.size == 0, f"(a) {name} {suf} run {run}: {k} written outside its set at {g.where(bad[0])}"
            else:
                assert same.all(), f"(b) {name} {suf} run {run}: input {k} changed"
        runs[run] = (raws, after)
    for k, (g, mask, nodes) in outputs.items():
        z, p = (runs[r][1][k].view(np.uint8).reshape(g.numel, -1)[mask] for r in "ZP")
        diff = np.flatnonzero((z != p).any(axis=1))
        assert diff.size == 0, (f"(c) {name} {suf}: {k} depends on storage that holds no node, first at "
                                f"{g.where(np.flatnonzero(mask)[diff[0]])}")
        zb, pb = (runs[r][0][k].view(np.uint8).reshape(g.numel, -1)[mask] for r in "ZP")
        untouched = (z == zb).all(axis=1) & (p == pb).all(axis=1)
        assert not untouched.any(), f"(d) {name} {suf}: {k} has elements of its write set nothing was stored to"


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_footprint(suf):
    rng = np.random.default_rng(11)
    for H, W, B in ((3, 3, 1), (9, 9, 2), (17, EDGES[suf][1], 2), (67, 5, 3)):
        g = Geo(H, W, B, ESZ[suf])
        cg = coarse_geo(g)
        e, u = draw(rng, B, cg.H, cg.W), draw(rng, B, H, W)
        for order in (1, 3):
            footprint("fmg_prolong", suf, {"u": None, "ec": (cg, e)}, {"out": (g, g.interior(), None)},
                      dict(order=order, **pitches(g, cg)))
            footprint("fmg_prolong", suf, {"u": (g, u), "ec": (cg, e)}, {"out": (g, g.interior(), None)},
                      dict(order=order, **pitches(g, cg)))
            footprint("fmg_prolong", suf, {"out": "u", "ec": (cg, e)}, {"u": (g, g.interior(), u)},
                      dict(order=order, **pitches(g, cg)))
        if cg.H >= 3 and cg.W >= 3:
            footprint("fmg_restrict", suf, {"f": (g, u)}, {"fc": (cg, cg.interior(), None)}, pitches(g, cg))
        bc = draw(rng, B, 2 * H - 1, 2 * W - 1)
        for src, per in ((bc.ravel(), bc[0].size), (None, 0)):
            footprint("fmg_boundary", suf, {"bc": src}, {"dst": (g, g.boundary(), None)},
                      dict(bc_bstride=per, stride=2, B=B, H=H, W=W, ld=g.ld, bstride=g.bs))


# ----------------------------------------------------------------------------- restriction, bitwise
@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("H, W, B", [(9, 9, 1), (131, 37, 2), (259, 259, 1)])
def test_restrict_is_residual_restrict_of_a_zero_iterate(suf, H, W, B):
    from feanet_amd import mesh_setup as ms
    g = Geo(H, W, B, ESZ[suf])
    cg = coarse_geo(g)
    dt = NP[suf]
    f = g.framed(draw(np.random.default_rng([H, W]), B, H, W), 0.0, dt)
    fc0 = canary(cg.numel, dt, C1)
    got = call("fmg_restrict", suf, {"f": f, "fc": fc0}, **pitches(g, cg))["fc"]
    ktab = ms.stencil_table(None).reshape(-1, 9).astype(dt)
    want = call("mg_residual_restrict", suf,
                {"u": np.zeros(g.numel, dt), "f": f, "v_out": None, "fc": fc0, "pid": None, "ktab": ktab.ravel(),
                 "omd": ms.omega_over_d(ms.stencil_table(None), 2.0 / 3.0, dt), "rtab": fr.LIN4.astype(dt).ravel()},
                ntab=1, nrtab=1, w0=1.0, **pitches(g, cg))["fc"]
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # and it is the coarse load vector
    fn = nodes_of(g, f).astype(np.float64)
    ref, S = fr.restrict(fn), fr.restrict(np.abs(fn))
    assert np.all(np.abs(nodes_of(cg, got) - ref)[:, 1:-1, 1:-1] <= (2 * (9 + 2) * U[suf] * S)[:, 1:-1, 1:-1])


# ----------------------------------------------------------------------------- MultigridSolver.fmg
_PIDS = {}


def pids():
    if not _PIDS:
        maps = np.load(os.path.join(HERE, "golden", "c3_pattern_maps.npz"))
        _PIDS.update({int(k[4:]): maps[k] for k in maps.files if k.startswith("pid_")})
    return _PIDS


def problem_data(n, rows, B, seed=0):
    """Random right-hand sides and Dirichlet fields (zero inside, as the reference's boundary_value), different
    per sample."""
    m = n if rows is None else rows
    rng = np.random.default_rng([seed, n, m, B])
    return rng.standard_normal((B, m + 1, n + 1)), fr.ring(rng.standard_normal((B, m + 1, n + 1)), 1, np.float64)


def make_solver(n, rows, problem, B, nu, f, bc, dtype=torch.float64, **kw):
    from feanet_amd.solver import MultigridSolver
    s = MultigridSolver(n, rows=rows, problem=problem, dtype=dtype, batch=B, nu1=nu[0], nu2=nu[1], **kw)
    shape = (B, 1) + f.shape[-2:]
    s.set_rhs(f=torch.from_numpy(f).to("cuda", dtype).reshape(shape))
    s.set_boundary(torch.from_numpy(bc).to("cuda", dtype).reshape(shape))
    return s


CASES = [  # n, rows, problem, batch, cycles, interp, (nu1, nu2)
    (16, None, "poisson", 1, 1, "cubic", (1, 1)),
    (128, None, "poisson", 1, 2, "cubic", (1, 1)),
    (128, None, "poisson", 1, 1, "bilinear", (1, 1)),
    (256, None, "poisson", 1, 1, "cubic", (1, 1)),      # level 1 (129^2) streams above the 65^2 tail
    (192, 96, "poisson", 2, 1, "cubic", (1, 1)),        # 97 x 193, coarsest 4 x 7: 8 base cycles
    (64, None, "interface", 1, 2, "cubic", (1, 1)),
    (256, None, "interface", 1, 1, "cubic", (1, 1)),
    (64, None, "poisson", 2, 1, "cubic", (2, 1)),
    (64, None, "poisson", 2, 2, "bilinear", (1, 1)),
]


@pytest.mark.parametrize("n, rows, problem, B, cycles, interp, nu", CASES)
def test_fmg_against_the_reference_driver(n, rows, problem, B, cycles, interp, nu):
    f, bc = problem_data(n, rows, B)
    s = make_solver(n, rows, problem, B, nu, f, bc)
    s.fmg(cycles=cycles, interp=interp)
    got = s.solution().cpu().numpy()[:, 0]
    ref = fr.fmg(n, f, bc, levels=s.L, rows=rows, cycles=cycles, order=3 if interp == "cubic" else 1,
                 problem=problem, nu=nu, pids=pids() if problem == "interface" else None)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"fmg n={n} rows={rows} {problem} B={B} cycles={cycles} {interp} V{nu}: relative error {err:.3g}")
    assert err < 1e-10
    # the invariant the ordinary cycles rely on: coarse boundary rings zero again, nothing outside the nodes written
    for l, Lv in enumerate(s.levels):
        for name in ("a", "b", "f"):
            raw = getattr(Lv, name)
            v = Lv.view(raw)
            if l >= 1 and name != "f":
                edges = (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1])
                assert not any(bool(e.any()) for e in edges), (l, name)
            g = Geo(Lv.H, Lv.W, Lv.B, Lv.esz, Lv.ld, Lv.bs)
            assert not raw.cpu().numpy()[~g.nodes()[:raw.numel()]].any(), (l, name)
    # the finest boundary nodes carry the Dirichlet data
    assert np.array_equal(got[:, 0], bc[:, 0]) and np.array_equal(got[:, :, -1], bc[:, :, -1])


def test_fmg_fp32_within_the_conditioning_bound():
    """fp32 pass against the fp64 reference driver: max|v32 - v64| <= cond(K) u32 max|v64| (the bound
    tests/test_gpu_configs.py derives; 2.0e-4 at n = 128), on the smooth model problem."""
    n = 128
    ue, f = fr.model_problem(n)
    bc = fr.ring(ue[None], 1, np.float64)
    s = make_solver(n, None, "poisson", 1, (1, 1), f[None], bc, dtype=torch.float32)
    s.fmg()
    got = s.solution().cpu().numpy()[0, 0].astype(np.float64)
    ref = fr.fmg(n, f[None], bc)[0]
    tol = 4.0 / (2.0 * np.pi ** 2 / n ** 2) * 2.0 ** -24
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"fmg fp32 n={n}: relative error {err:.3g}, bound {tol:.3g}")
    assert err < tol


@pytest.mark.parametrize("n, problem, B", [(256, "poisson", 1), (64, "interface", 2), (256, "poisson", 64),
                                           (1024, "poisson", 1)])
def test_fmg_bitwise_without_the_groupings(n, problem, B):
    """The groupings of the sub-hierarchy plans — the coarse tail (from a level below tail_from too, with its offset
    into the pattern maps), the multi-level launches, pairs, triples, the extended tail (batch 64) — are bitwise the
    launches they replace: the same result from a solver without them."""
    f, bc = problem_data(n, None, B, seed=3)
    dtype = torch.float32 if B == 64 else torch.float64
    a = make_solver(n, None, problem, B, (1, 1), f, bc, dtype=dtype)
    b = make_solver(n, None, problem, B, (1, 1), f, bc, dtype=dtype, coarse_tail=False, mid=False, pair_levels=False)
    a.fmg(cycles=2)
    b.fmg(cycles=2)
    assert torch.equal(a.solution(), b.solution())


@pytest.mark.parametrize("n, problem, B, nu", [(256, "poisson", 1, (1, 1)), (64, "interface", 2, (2, 1)),
                                               (256, "poisson", 1, (2, 1)), (1024, "poisson", 1, (1, 1))])
def test_fmg_bitwise_without_the_groupings_and_unfused(n, problem, B, nu):
    """The same with fuse=False as well: the pass does not depend on any of the solver's performance switches.  Its
    cycles run the fused pre-sweep + restriction on the level with the stored iterate and separate launches below
    (V(2,1): a streamed level below the top pre-sweeps twice), in every solver.  Ordinary cycles are not like that:
    a fused and an unfused solver differ in the last bits after one (4.3e-16 of max |u| at 257^2), and with
    nu1 = 2 so do a fused solver with and without the coarse tail; the unfused solver still runs its own plans."""
    f, bc = problem_data(n, None, B, seed=3)
    a = make_solver(n, None, problem, B, nu, f, bc)
    b = make_solver(n, None, problem, B, nu, f, bc, coarse_tail=False, mid=False, pair_levels=False, fuse=False)
    a.fmg(cycles=2)
    b.fmg(cycles=2)
    assert torch.equal(a.solution(), b.solution())
    # the unfused solver's ordinary plans are its own, before and after
    kinds = [rec[0] for rec in b._plan("a")[0]]
    assert "mg_sweep_restrict" not in kinds and "mg_sweep" in kinds


def test_fmg_eager_captured_replayed():
    n = 128
    f, bc = problem_data(n, None, 1, seed=4)
    s = make_solver(n, None, "poisson", 1, (1, 1), f, bc)
    outs = []
    for _ in range(3):
        s.fmg()
        outs.append(s.solution())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert len([k for k in s._graphs if isinstance(k, tuple) and k[0] == "fmg"]) == 1
    # new Dirichlet data: a new program (the old graph is dropped), a different result
    s.set_boundary(torch.from_numpy(2 * bc).cuda().reshape(1, 1, n + 1, n + 1))
    s.fmg()
    assert not torch.equal(s.solution(), outs[0])
    assert len([k for k in s._graphs if isinstance(k, tuple) and k[0] == "fmg"]) == 0


def test_cycles_continue_from_fmg_as_from_load():
    n = 128
    f, bc = problem_data(n, None, 1, seed=5)
    s = make_solver(n, None, "poisson", 1, (1, 1), f, bc)
    s.fmg()
    u = s.solution()
    r = s.residual_norm()
    s.vcycle(3)
    t = make_solver(n, None, "poisson", 1, (1, 1), f, bc)
    t.load(u)
    assert torch.equal(t.solution(), u) and torch.equal(t.residual_norm(), r)
    t.vcycle(3)
    assert torch.equal(s.solution(), t.solution())
    # and a later load() starts over with the same Dirichlet data
    s.load()
    t.load()
    s.vcycle(2)
    t.vcycle(2)
    assert torch.equal(s.solution(), t.solution())


def test_solve_from_fmg():
    n = 64
    ue, f = fr.model_problem(n)
    bc = fr.ring(ue[None], 1, np.float64)
    s = make_solver(n, None, "poisson", 1, (1, 1), f[None], bc)
    u, hist = s.solve(fmg=True, eps=1e-9, max_cycles=50)
    t = make_solver(n, None, "poisson", 1, (1, 1), f[None], bc)
    t.fmg()
    want = [t.residual_norm().cpu().numpy()]
    while want[-1].max() > 1e-9:
        t.vcycle()
        want.append(t.residual_norm().cpu().numpy())
    assert torch.equal(u, t.solution())
    assert len(hist) == len(want) and all(np.array_equal(a, b) for a, b in zip(hist, want))
    # history[0] is the residual after the pass: far below the residual of the zero guess
    t.load()
    assert hist[0][0] < 0.05 * float(t.residual_norm()[0]) and hist[-1][0] <= 1e-9
    with pytest.raises(ValueError, match="u0 must be None"):
        s.solve(u0=u, fmg=True)


def test_ordinary_plans_do_not_change():
    """fmg() adds plans of its own and leaves the ordinary ones as they were: the launch records of a V-cycle and of
    the joined program are equal before and after it, and equal to those of a solver that never calls it."""
    n = 256
    f, bc = problem_data(n, None, 1, seed=6)

    def records(s):
        return [s._plan("a"), s._plan("b"), s.joined_program(3)]

    def text(s, recs):  # pointers by buffer name, as tools/plan_dump.py prints them
        names = {}
        for l, Lv in enumerate(s.levels):
            for b in ("f", "a", "b", "c", "zero", "pid"):
                if getattr(Lv, b, None) is not None:
                    names[getattr(Lv, b).data_ptr()] = f"L{l}.{b}"
        for b in ("ktab", "omd", "rtab", "ptab", "tail_pid"):
            if getattr(s, b, None) is not None:
                names[getattr(s, b).data_ptr()] = b
        return re.sub(r"\b\d{9,}\b", lambda m: names.get(int(m.group()), m.group()), repr(recs))

    s = make_solver(n, None, "poisson", 1, (1, 1), f, bc)
    before = text(s, records(s))
    s.fmg(cycles=2)
    s.load()
    assert text(s, records(s)) == before
    assert set(k for k in s._plans if not (isinstance(k, tuple) and k[0] == "fmg")) == {"a", "b"}
    t = make_solver(n, None, "poisson", 1, (1, 1), f, bc)
    assert text(t, records(t)) == before
