"""Write footprint and padding independence of every framed entry point on the GPU (tests/footprint.py: the cases,
the two runs Z and P, the assertions (a) .. (d) on bytes), and fea_dd_copy_blocks / fea_dd_copy_rects against numpy.

Every case of an entry point and dtype runs in one test, cached and nontemporal (FEANET_NT_BYTES=0); all failing
cases are reported together."""
import time

import numpy as np
import pytest
import torch

import footprint as fp

pytestmark = pytest.mark.gpu

ENTRIES = [(e, suf) for e in sorted(fp.DESC) for suf in fp.DESC[e].sufs]


@pytest.fixture(params=[False, True], ids=["cached", "nt"])
def nt(request, monkeypatch):
    """FEANET_NT_BYTES=0 selects the nontemporal-store instantiations that otherwise run only on fields > 64 MiB."""
    if request.param:
        monkeypatch.setenv("FEANET_NT_BYTES", "0")
    return request.param


@pytest.mark.parametrize("entry,suf", ENTRIES, ids=[f"{e}-{s}" for e, s in ENTRIES])
def test_footprint(entry, suf, nt):
    t0 = time.perf_counter()
    cases = fp.cases(entry, suf)
    failed = []
    for c in cases:
        try:
            fp.run_case(c, fp.gpu_launch)
        except fp.FootprintError as e:
            failed.append(f"{c}: {e}")
    print(f"{entry}_{suf}: {len(cases)} cases, {time.perf_counter() - t0:.2f} s")
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed)


def test_level_allocator_matches_the_harness():
    """_Level allocates what Geo describes (same pitch, sample stride and slack, view() = the node mask) and hands
    out zeroed buffers: the state section 3 of the header requires of the ghost ring of r, p and z."""
    from feanet_amd.solver import _Level
    dev = torch.device("cuda")
    for (H, W, B, T) in ((33, 321, 2, torch.float64), (35, 323, 3, torch.float32), (3, 3, 1, torch.float64)):
        L = _Level(H - 1, W - 1, B, T, dev, pid_np=np.ones((H, W), np.uint8))
        g = fp.Geo(H, W, B, L.f.element_size())
        assert (L.ld, L.bs, L.f.numel()) == (g.ld, g.bs, g.numel)
        for name in ("f", "a", "b", "zero", "c"):
            assert not L.buf(name).any(), f"{name} is not zero"
        idx = torch.arange(g.numel, device=dev, dtype=T)
        assert np.array_equal(np.sort(L.view(idx).cpu().numpy().ravel().astype(np.int64)), np.flatnonzero(g.nodes()))
        p = L.pid.cpu().numpy()
        assert p.size == g.pid().numel and (p[g.pid().nodes()] == 1).all() and not p[~g.pid().nodes()].any()


def test_cycle_ghost_rings_stay_zero():
    """The V-cycle kernels that produce the preconditioned residual z (and the Krylov kernels that produce r and p)
    write interior nodes only, so the ghost ring and the boundary nodes of r, p, z keep the allocator's zeros through
    a solve (include/feanet_hip.h section 3 requires them zero); every non-node element of every Krylov field and of
    every level buffer of the preconditioner is still zero after PCG iterations."""
    from feanet_amd import PCGSolver
    for kw in (dict(dtype=torch.float64), dict(dtype=torch.float64, precond_dtype=torch.float32),
               dict(dtype=torch.float32, problem="interface")):
        n, B = 64, 2
        s = PCGSolver(n, batch=B, **kw)
        rng = np.random.default_rng(3)
        s.set_boundary(torch.from_numpy(rng.random((B, 1, n + 1, n + 1))).cuda().to(s.dtype))
        s.set_rhs(f=torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda().to(s.dtype))
        s.load()
        s.iterate(3)
        g = fp.Geo(n + 1, n + 1, B, 4 if s.dtype == torch.float32 else 8)
        free = torch.from_numpy(~g.nodes()).cuda()
        bnd = torch.from_numpy(g.boundary()).cuda()
        for name, t in (("x", s.x), ("b", s.b), ("r", s.r), ("p0", s.p[0]), ("p1", s.p[1])):
            assert not t[free].any(), f"{kw}: non-node storage of {name} written"
        for name, t in (("r", s.r), ("p0", s.p[0]), ("p1", s.p[1])):
            assert not t[bnd].any(), f"{kw}: boundary nodes of {name} not zero"
        for lv, L in enumerate(s.mg.levels):
            gl = fp.Geo(L.H, L.W, B, L.f.element_size())
            fr = torch.from_numpy(~gl.nodes()).cuda()
            for name in ("f", "a", "b"):
                assert not L.buf(name)[fr].any(), f"{kw}: level {lv} buffer {name}: non-node storage written"
        L0 = s.mg.levels[0]
        b0 = torch.from_numpy(fp.Geo(L0.H, L0.W, B, L0.f.element_size()).boundary()).cuda()
        assert not L0.buf(s._zname)[b0].any(), f"{kw}: boundary nodes of the preconditioned residual z not zero"


@pytest.mark.parametrize("T,problem", [(torch.float64, "poisson"), (torch.float32, "interface")])
def test_joined_cycles_leave_the_frames_finite(T, problem):
    """fea_mg_cycle_join keeps boundary nodes as 0 * r + b and therefore needs finite values in the frames of u, f and
    ec (include/feanet_hip.h).  The allocator provides zeros, and no kernel of a joined V-cycle, the loads and the
    right-hand side set-up included, writes anything but nodes: after set_boundary / set_rhs / load and three joined
    cycles every non-node element of every level buffer is still zero."""
    from feanet_amd.solver import MultigridSolver
    n, B = 256, 2
    rng = np.random.default_rng(11)
    s = MultigridSolver(n, problem=problem, dtype=T, batch=B)
    cu = lambda a: torch.from_numpy(a).cuda().to(T)
    s.set_boundary(cu(rng.random((B, 1, n + 1, n + 1))))
    s.set_rhs(f=cu(rng.standard_normal((B, 1, n + 1, n + 1))))
    s.load(cu(rng.standard_normal((B, 1, n + 1, n + 1))))
    s.vcycle(3)
    assert torch.isfinite(s.solution()).all()
    for lv, L in enumerate(s.levels):
        free = torch.from_numpy(~fp.Geo(L.H, L.W, B, L.f.element_size()).nodes()).cuda()
        for name in ("f", "a", "b", "c", "zero"):
            t = getattr(L, name)
            if t is not None:
                assert not t[free].any(), f"level {lv} buffer {name}: non-node storage written"
