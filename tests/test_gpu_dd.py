"""GPU parity of the domain-decomposed V-cycle (feanet_amd.dd): P row slabs on one device (the
in-process LocalGroup, and two processes over gloo) against the single-GPU MultigridSolver on the
same global grid.  The decomposition uses the same kernels with the same per-node arithmetic, so
the owned rows must agree bitwise (torch.equal), cycle after cycle.

Both field precisions: a case's dtype is the decomposed solver's and the single-GPU reference's, the problem is
drawn in fp64 and cast, and the comparison of fields stays torch.equal.  The element size enters the
decomposition's own address arithmetic (dd._block, the staging and rectangle tables, the coarse-solution window)
and the kernels' strip widths, vector lengths and tiles.  The shapes marked "window" put level Ld's blocks and the
window of the coarse solution off the 4-element grid: every residue mod 4 of the block width and of the window's
origin, in rows and in columns."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _cases(argnames, f64, added):
    """Parameter sets of a test that gained a trailing dtype argument: the fp64 cases `f64` (tuples without the
    dtype) under the ids pytest gave them before (a value that is no number, string, bool or None is named by its
    argument and the case's position), then the `added` ones (tuples ending in their dtype)."""
    names = argnames.split(",")

    def auto(i, case):
        return "-".join(str(v) if isinstance(v, (int, float, str, bool, type(None))) else f"{a}{i}"
                        for a, v in zip(names, case))
    out = [pytest.param(*c, F64, id=auto(i, c)) for i, c in enumerate(f64)]
    out += [pytest.param(*c, id=auto(len(f64) + i, c[:-1]) + ("-f32" if c[-1] is F32 else "-f64"))
            for i, c in enumerate(added)]
    return out


def _global_problem(m, n, B, seed=0, dtype=F64):
    """Drawn in fp64 and cast: both precisions see the same problem."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    f = torch.randn(B, 1, m + 1, n + 1, device="cuda", dtype=torch.float64, generator=g)
    u0 = torch.randn(B, 1, m + 1, n + 1, device="cuda", dtype=torch.float64, generator=g)
    bc = torch.rand(B, 1, m + 1, n + 1, device="cuda", dtype=torch.float64, generator=g)
    inner = torch.zeros_like(bc)
    inner[..., 1:-1, 1:-1] = 1
    return f.to(dtype), u0.to(dtype), (bc * (1 - inner)).to(dtype)


def _norm_close(got, ref, m, n, what=""):
    """The decomposed fp32 residual norm against the single-GPU one (fp64 cases keep their 1e-12).  The per-node
    residuals are the same fp32 numbers on both sides and every norm kernel accumulates their squares in double
    (include/feanet_hip.h), so the two norms differ only by the order of N = (m - 1)(n - 1) double additions:
    relative 2 N 2^-53 on the square, N 2^-53 on the norm.  Prints how much of that bound the run used."""
    got, ref = (torch.as_tensor(x).detach().cpu().double().reshape(-1) for x in (got, ref))
    bound = (m - 1) * (n - 1) * 2.0 ** -53
    rel = ((got - ref).abs() / ref).max().item()
    print(f"fp32 residual norm {what}: relative difference {rel:.3e}, {rel / bound:.3g} of the bound {bound:.3e}")
    assert rel <= bound, (rel, bound)


def _coarse_window(s):
    """(row, column) of the coarse solver's solution at which rank s's paired prolongation onto level Ld - 2 reads
    its level-Ld correction in place (DDSolver._read_coarse_in_place), from the solver's own launch records.
    Fails if that launch reads level Ld's own buffer (the scatter was kept): the case would then say nothing about
    the window's alignment."""
    from feanet_amd import _lib
    from feanet_amd.dd import Kernels
    own = {s.local.levels[s.Ld].buf(name).data_ptr() for name in ("a", "b")}
    f2 = s.local.levels[s.Ld - 2].f.data_ptr()
    recs = [rec for seg in s.chunk(("cycle", "a"))[0] if isinstance(seg, Kernels) for rec in seg.launches
            if rec[0] == "mg_prolong2" and _lib.arg(rec, "f") == f2]
    assert len(recs) == 1, [rec[0] for rec in recs]
    Lc = s.coarse.levels[0]
    buf = Lc.buf(s.coarse_end)
    ec2 = _lib.arg(recs[0], "ec2")
    assert ec2 not in own, "level Ld - 2's prolongation reads level Ld's buffer, not the coarse solution"
    assert (_lib.arg(recs[0], "ldc2"), _lib.arg(recs[0], "bstridec2")) == (Lc.ld, Lc.bs)
    el, rem = divmod(ec2 - buf.data_ptr(), buf.element_size())
    assert rem == 0 and 0 <= el < Lc.bs
    return divmod(el, Lc.ld)


def _single(m, n, B, f, u0, bc, cycles, nu=(1, 1), problem="poisson", dtype=F64, **kw):
    from feanet_amd.solver import MultigridSolver
    s = MultigridSolver(n, rows=m, dtype=dtype, batch=B, nu1=nu[0], nu2=nu[1], problem=problem, **kw)
    s.set_boundary(bc)
    s.set_rhs(f=f)
    s.load(u0)
    out = []
    for _ in range(cycles):
        s.vcycle()
        out.append((s.solution(), s.residual_norm()))
    return s, out


_LOCAL_F64 = [(256, 128, 2, 1, 1, True, (1, 1), None),
              (512, 256, 4, 2, 2, True, (1, 1), None),
              (384, 256, 3, 2, 1, False, (1, 1), None),
              (1024, 1024, 4, 3, 1, True, (1, 1), None),
              (2048, 1024, 8, 3, 1, True, (1, 1), None),
              (2048, 1024, 8, 4, 1, True, (1, 1), None),
              (4096, 512, 4, 5, 1, True, (1, 1), None),
              (1024, 512, 4, 3, 1, True, (2, 2), None),
              (1024, 512, 2, 3, 1, False, (2, 1), None),
              # 2-D blocks (one-phase exchange, corners from the diagonal neighbours)
              (512, 512, 4, 2, 2, True, (1, 1), (2, 2)),
              (1024, 1024, 8, 3, 1, True, (1, 1), (4, 2)),
              (512, 1024, 2, 3, 1, True, (1, 1), (1, 2)),
              (768, 1024, 6, 2, 1, False, (1, 1), (3, 2)),
              (1024, 1024, 4, 3, 1, True, (2, 2), (2, 2))]
# fp32 at the smallest shape of each kind above
_LOCAL_F32 = [(256, 128, 2, 1, 1, True, (1, 1), None),
              (512, 256, 4, 2, 2, True, (1, 1), None),
              (384, 256, 3, 2, 1, False, (1, 1), None),
              (512, 512, 4, 2, 2, True, (1, 1), (2, 2)),
              (512, 1024, 2, 3, 1, True, (1, 1), (1, 2)),
              (768, 1024, 6, 2, 1, False, (1, 1), (3, 2)),
              (1024, 512, 4, 3, 1, True, (2, 2), None),
              (1024, 512, 2, 3, 1, False, (2, 1), None)]
# window shapes (V(1,1): G = 3 ghost lines at level Ld).  The last rank's level-Ld block and its window of the coarse
# solution, which dd._partition_for gives on the host: c_r x c_c nodes owned per rank, stored from global row gr0 and
# column gc0.  Every existing case has c = 8 .. 128 and so origin c - 3 = 1 (mod 4); these have c_c = 1, 2, 3 (mod 4)
# and gc0 = 0, 2, 3 (mod 4), in rows as in columns.  80 .. 112: the coarsest levels are 6^2, 4^2 and 8^2 nodes; the
# 640-wide grids put a local fine block (417 columns) across the fp32 strip edge at 256 columns.
#                m    n  P Ld B  graph   nu      grid    (c_r, gr0, c_c, gc0)
_WINDOWS = [(80, 80, 4, 3, 1, True, (1, 1), (2, 2), (5, 2, 5, 2)),
            (96, 96, 4, 3, 2, True, (1, 1), (2, 2), (6, 3, 6, 3)),
            (112, 112, 4, 3, 1, True, (1, 1), (2, 2), (7, 4, 7, 4)),
            (160, 80, 4, 3, 1, False, (1, 1), (2, 2), (10, 7, 5, 2)),
            (448, 320, 4, 4, 2, True, (1, 1), (2, 2), (14, 11, 10, 7)),
            (576, 576, 4, 4, 1, True, (1, 1), (2, 2), (18, 15, 18, 15)),
            (576, 576, 4, 5, 1, True, (1, 1), (2, 2), (9, 6, 9, 6)),
            (640, 640, 4, 5, 2, True, (1, 1), (2, 2), (10, 7, 10, 7)),
            (768, 640, 6, 5, 1, True, (1, 1), (3, 2), (8, 13, 10, 7)),
            (320, 320, 2, 5, 1, True, (1, 1), None, (5, 2, 10, 0))]
_WINDOW_OF = {c[:4] + (c[7],): c[8] for c in _WINDOWS}


@pytest.mark.parametrize("m,n,P,Ld,B,graph,nu,grid,dtype", _cases(
    "m,n,P,Ld,B,graph,nu,grid", _LOCAL_F64,
    [c + (F32,) for c in _LOCAL_F32] + [c[:8] + (T,) for c in _WINDOWS for T in (F32, F64)]))
def test_dd_local_group_bitwise(m, n, P, Ld, B, graph, nu, grid, dtype):
    """Communication-avoiding exchanges (one neighbour batch per cycle, exchange_depths): every owned
    node still equals the single-GPU V-cycle bit for bit — row slabs and 2-D blocks, also with deeper
    agglomeration and V(2,2); in fp32 as in fp64, and on the window shapes (_WINDOWS), where every rank's records
    must show the coarse solution read in place at the window the partition gives.

    The coarse end: the agglomerated solver's levels are the global levels Ld .., and its LDS tail starts at the
    global tail level t (the same in both precisions at these sizes) when t > Ld.  A solver's tail never starts at
    its own top level, so when t <= Ld (every window shape: t = 1 .. 4) the agglomerated solver's tail starts at its
    level 1, global level Ld + 1, below the single-GPU solver's — still bitwise, which the field comparison
    shows."""
    from feanet_amd.dd import LocalGroup
    f, u0, bc = _global_problem(m, n, B, dtype=dtype)
    s, ref = _single(m, n, B, f, u0, bc, 4, nu, dtype=dtype)
    grp = LocalGroup(n, m, P, agglomerate=Ld, batch=B, graph=graph, nu1=nu[0], nu2=nu[1], grid=grid, dtype=dtype)
    if s.tail_from is None or s.tail_from > Ld:
        assert grp.ranks[0].coarse.tail_from is None or grp.ranks[0].coarse.tail_from + Ld == s.tail_from
    else:
        assert grp.ranks[0].coarse.tail_from == 1
    window = _WINDOW_OF.get((m, n, P, Ld, grid))
    if window is not None:
        last = grp.ranks[-1]
        assert (last.part.rows_per_rank(Ld), last.parts[Ld].gr0, last.part.cols_per_rank(Ld),
                last.cparts[Ld].gr0) == window
        for r in grp.ranks:
            assert _coarse_window(r) == (r.parts[Ld].gr0, r.cparts[Ld].gr0)
    grp.set_rhs(f)
    grp.load(u0, bc)
    for k in range(4):
        grp.vcycle()
        got = grp.solution()
        assert got.dtype == dtype
        assert torch.equal(got, ref[k][0]), f"cycle {k}: max diff {(got - ref[k][0]).abs().max().item():.3e}"
        nr = grp.residual_norm()
        if dtype is F64:
            torch.testing.assert_close(nr, ref[k][1], rtol=1e-12, atol=0)
        else:
            _norm_close(nr, ref[k][1], m, n, f"{m}x{n} P={P} cycle {k}")
    # several cycles per call: the finest level's cycle boundaries joined on every slab
    s.vcycle(3)
    grp.vcycle(3)
    assert torch.equal(grp.solution(), s.solution())
    s.vcycle(2)
    grp.vcycle(2)
    assert torch.equal(grp.solution(), s.solution())


def _learned_ratio():
    here = os.path.dirname(os.path.abspath(__file__))
    w = np.load(os.path.join(here, "..", "multigrid-feanet_amd", "feanet_amd", "weights", "multigrid_interface_ratio.npz"))
    return dict(R=w["R"][0], P=w["P"][:, 0], w=w["w"])


@pytest.mark.parametrize("n,P,Ld,B,nu,grid,learned,dtype", _cases(
    "n,P,Ld,B,nu,grid,learned", [(512, 4, 2, 1, (1, 1), (2, 2), False),
                                 (512, 2, 2, 2, (1, 1), None, True),
                                 (1024, 8, 3, 1, (1, 1), (4, 2), True),
                                 (1024, 4, 3, 1, (2, 2), (2, 2), False),
                                 (768, 6, 2, 1, (1, 1), (3, 2), True)],
    [(512, 4, 2, 1, (1, 1), (2, 2), False, F32),
     (512, 2, 2, 2, (1, 1), None, True, F32),
     (768, 6, 2, 1, (1, 1), (3, 2), True, F32)]))
def test_dd_interface_local_group_bitwise(n, P, Ld, B, nu, grid, learned, dtype):
    """The two-material problem (MeshCenterInterface, FEANet/mesh.py:4-120) decomposed: every rank's levels carry
    their window of the global level's pattern map (DDSolver(problem='interface') -> MultigridSolver(pid_maps=...)),
    the agglomerated coarse solver the global maps of its levels; linear and learned (BASELINE C3) transfers.  Owned
    nodes bitwise the single-GPU two-material V-cycle, with the rhs given as the nodal source F (FNet of the global
    mesh applied before the split)."""
    from feanet_amd.dd import LocalGroup
    from feanet_amd.solver import MultigridSolver
    kw = _learned_ratio() if learned else {}
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    F = torch.rand(B, 1, n + 1, n + 1, device="cuda", dtype=torch.float64, generator=g).to(dtype)
    u0 = torch.randn(B, 1, n + 1, n + 1, device="cuda", dtype=torch.float64, generator=g).to(dtype)
    s = MultigridSolver(n, rows=n, problem="interface", dtype=dtype, batch=B, nu1=nu[0], nu2=nu[1], **kw)
    s.set_rhs(F=F)
    s.load(u0)
    grp = LocalGroup(n, n, P, agglomerate=Ld, batch=B, nu1=nu[0], nu2=nu[1], grid=grid, problem="interface",
                     dtype=dtype, **kw)
    grp.set_rhs(F=F)
    grp.load(u0)
    for k in (1, 1, 3, 2):
        s.vcycle(k)
        grp.vcycle(k)
        got = grp.solution()
        assert got.dtype == dtype
        assert torch.equal(got, s.solution()), f"{k}: max diff {(got - s.solution()).abs().max().item():.3e}"
    if dtype is F64:
        torch.testing.assert_close(grp.residual_norm(), s.residual_norm(), rtol=1e-12, atol=0)
    else:
        _norm_close(grp.residual_norm(), s.residual_norm(), n, n, f"interface {n} P={P}")


def _hnet():
    here = os.path.dirname(os.path.abspath(__file__))
    w = np.load(os.path.join(here, "..", "multigrid-feanet_amd", "feanet_amd", "weights", "hnet_iso_poisson_33x33.npz"))
    return np.stack([w[f"conv{i}"].reshape(3, 3) for i in range(3)])


@pytest.mark.parametrize("m,n,P,Ld,B,nu,grid,problem,nl,dtype", _cases(
    "m,n,P,Ld,B,nu,grid,problem,nl", [(512, 512, 4, 2, 1, (1, 1), (2, 2), "poisson", 3),
                                      (1024, 512, 2, 3, 2, (1, 1), None, "poisson", 3),
                                      (1024, 1024, 8, 3, 1, (1, 1), (4, 2), "poisson", 3),
                                      (512, 512, 4, 2, 1, (2, 1), (2, 2), "poisson", 1),
                                      (512, 512, 4, 2, 1, (1, 1), (2, 2), "interface", 3)],
    [(512, 512, 4, 2, 1, (1, 1), (2, 2), "poisson", 3, F32),
     (512, 512, 4, 2, 1, (2, 1), (2, 2), "poisson", 1, F32),
     (512, 512, 4, 2, 1, (1, 1), (2, 2), "interface", 3, F32),
     # blocks off the 4-element grid (the learned smoother's partitions keep more ghost lines, and its prolongation
     # is never paired, so level Ld is always scattered: these pin the block widths of the exchange, the send form
     # and the placement).  One HNet layer: G = 6, 10 x 10 blocks stored from 4; three layers refuse
     # (640, 640, 4, 5) (12 coarse lines per rank needed), so they run (288, 288, 4, 3): G = 8, 18 x 18 from 10
     (640, 640, 4, 5, 1, (1, 1), (2, 2), "poisson", 1, F32),
     (640, 640, 4, 5, 2, (1, 1), (2, 2), "poisson", 1, F64),
     (288, 288, 4, 3, 2, (1, 1), (2, 2), "poisson", 3, F32),
     (288, 288, 4, 3, 1, (1, 1), (2, 2), "poisson", 3, F64)]))
def test_dd_hjac_local_group_bitwise(m, n, P, Ld, B, nu, grid, problem, nl, dtype):
    """The learned smoother (MultiGrid(mode='hjac').Step of M-FEANet-mg_test.ipynb:27346-27372) decomposed: every
    relaxation one HRelax sweep, the exchange depths from the validity simulation with each sweep losing 1 + nl
    lines, the agglomerated coarse solve the zero-start hjac V-cycle (HJac two-level launches and LDS tail), and the
    first cycle after load() reading the un-reset iterate.  Owned nodes bitwise the single-GPU hjac V-cycle."""
    from feanet_amd.dd import LocalGroup
    from feanet_amd.solver import MultigridSolver
    hw = _hnet()[:nl]
    f, u0, bc = _global_problem(m, n, B, seed=9, dtype=dtype)
    s = MultigridSolver(n, rows=m, problem=problem, dtype=dtype, batch=B, nu1=nu[0], nu2=nu[1],
                        smoother="hjac", hnet=hw)
    s.set_boundary(bc)
    s.set_rhs(f=f)
    s.load(u0)
    grp = LocalGroup(n, m, P, agglomerate=Ld, batch=B, nu1=nu[0], nu2=nu[1], grid=grid, problem=problem,
                     smoother="hjac", hnet=hw, dtype=dtype)
    grp.set_rhs(f)
    grp.load(u0, bc)
    for k in (1, 1, 3, 2):
        s.vcycle(k)
        grp.vcycle(k)
        got = grp.solution()
        assert got.dtype == dtype
        assert torch.equal(got, s.solution()), f"{k}: max diff {(got - s.solution()).abs().max().item():.3e}"
    if dtype is F64:
        torch.testing.assert_close(grp.residual_norm(), s.residual_norm(), rtol=1e-12, atol=0)
    else:
        _norm_close(grp.residual_norm(), s.residual_norm(), m, n, f"hjac {m}x{n} P={P}")
    # a second load(): the first cycle again reads the un-reset iterate (the chunk is cached, its graph replayed)
    s.load(u0)
    grp.load(u0, bc)
    for k in (1, 2):
        s.vcycle(k)
        grp.vcycle(k)
    assert torch.equal(grp.solution(), s.solution())


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    p = sk.getsockname()[1]
    sk.close()
    return p


def _dd_worker(rank, world, m, n, Ld, port, outdir, grid, dtype=F64, window=False):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "multigrid-feanet_amd"))
    import torch.distributed as dist
    from feanet_amd.dd import DDSolver, TorchComm
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    f, u0, bc = _global_problem(m, n, 1, dtype=dtype)
    s = DDSolver(n, m, rank, world, comm=TorchComm(), agglomerate=Ld, grid=grid, dtype=dtype)
    if window:
        assert _coarse_window(s) == (s.parts[Ld].gr0, s.cparts[Ld].gr0)
    s.set_rhs(f)
    s.load(u0, bc)
    s.vcycle(3)
    (y0, y1), (x0, x1), u = s.owned_block()
    nr = s.residual_norm()
    torch.cuda.synchronize()
    np.save(os.path.join(outdir, f"r{rank}.npy"), u.cpu().numpy())
    np.save(os.path.join(outdir, f"i{rank}.npy"), np.array([y0, y1, x0, x1]))
    np.save(os.path.join(outdir, f"n{rank}.npy"), nr.cpu().numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("m,n,P,Ld,grid,dtype", _cases(
    "m,n,P,Ld,grid", [(512, 256, 2, 2, None), (256, 512, 2, 2, (1, 2)), (512, 512, 4, 2, (2, 2))],
    # fp32: the host staging buffers take the field dtype.  160 x 80: a window shape of _WINDOWS (5-wide blocks from
    # column 2, 10 rows from row 7), the packed strips and the gathered blocks at those widths through the host
    [(512, 512, 4, 2, (2, 2), F32), (160, 80, 4, 3, (2, 2), F32), (160, 80, 4, 3, (2, 2), F64)]))
def test_dd_processes_gloo(tmp_path, m, n, P, Ld, grid, dtype):
    """Ranks in separate processes (TorchComm over gloo: device halos staged through the host, column
    strips packed), the path the RCCL run takes with device buffers; slabs and 2-D blocks."""
    window = (m, n, P, Ld, grid) in _WINDOW_OF
    mp.spawn(_dd_worker, args=(P, m, n, Ld, _free_port(), str(tmp_path), grid, dtype, window), nprocs=P, join=True)
    got = np.full((1, 1, m + 1, n + 1), np.nan)
    for r in range(P):
        y0, y1, x0, x1 = np.load(os.path.join(tmp_path, f"i{r}.npy"))
        block = np.load(os.path.join(tmp_path, f"r{r}.npy"))
        assert block.dtype == (np.float32 if dtype is F32 else np.float64)
        got[:, :, y0:y1, x0:x1] = block
    f, u0, bc = _global_problem(m, n, 1, dtype=dtype)
    _, ref = _single(m, n, 1, f, u0, bc, 3, dtype=dtype)
    exp = ref[-1][0].cpu().numpy()
    assert np.array_equal(got, exp), np.nanmax(np.abs(got - exp))
    for r in range(P):
        if dtype is F64:
            np.testing.assert_allclose(np.load(os.path.join(tmp_path, f"n{r}.npy")), ref[-1][1].cpu().numpy(),
                                       rtol=1e-12)
        else:
            _norm_close(np.load(os.path.join(tmp_path, f"n{r}.npy")), ref[-1][1], m, n, f"gloo rank {r}")


class _FakeDist:
    """An in-process stand-in for torch.distributed with the nccl backend's behaviour as TorchComm sees it
    (device buffers sent directly; P2P messages matched per peer pair in posting order; collectives), for
    ranks running as threads of one process.  A send snapshots its buffer on the stream at posting time."""

    def __init__(self, world):
        import threading
        from collections import defaultdict
        self.world = world
        self.cv = threading.Condition()
        self.mail = {}
        self.nsend = defaultdict(int)
        self.nrecv = defaultdict(int)
        self.bar = threading.Barrier(world)
        self.slots = [None] * world
        self.tls = threading.local()
        self.isend, self.irecv = "isend", "irecv"
        self.posted = []  # (src, dst, numel) in posting order, for the test's own checks
        self.gpu_lock = threading.RLock()  # the fake's device copies never run beside another rank's capture

        class P2POp:
            def __init__(op, kind, tensor, peer, group=None):
                op.kind, op.tensor, op.peer = kind, tensor, peer
        self.P2POp = P2POp

    def _snapshot(self, t):
        """t's values as queued on this rank's stream, complete before they are published: the ranks' streams are
        not ordered with each other, while nccl orders an operation behind the work every rank queued before it."""
        with self.gpu_lock:
            c = t.clone()
            torch.cuda.current_stream().synchronize()
        return c

    def _take(self, dst, src):
        """dst <- src (another rank's snapshot), complete before the snapshot can be freed and its memory reused
        on the stream that made it."""
        with self.gpu_lock:
            dst.copy_(src)
            torch.cuda.current_stream().synchronize()

    def get_rank(self, group=None):
        return self.tls.rank

    def get_world_size(self, group=None):
        return self.world

    def get_backend(self, group=None):
        return "nccl"

    def batch_isend_irecv(self, ops):
        me = self.tls.rank
        works = []
        with self.cv:
            for op in ops:
                if op.kind == "isend":
                    k = (me, op.peer)
                    self.mail[k + (self.nsend[k],)] = self._snapshot(op.tensor)
                    self.posted.append((me, op.peer, op.tensor.numel()))
                    self.nsend[k] += 1
            self.cv.notify_all()
        fake = self

        class Work:
            def __init__(w, key, t):
                w.key, w.t = key, t

            def wait(w):
                if w.key is None:
                    return
                with fake.cv:
                    fake.cv.wait_for(lambda: w.key in fake.mail, timeout=60)
                    src = fake.mail.pop(w.key)
                assert src.shape == w.t.shape or src.numel() == w.t.numel(), (src.shape, w.t.shape)
                fake._take(w.t, src.reshape(w.t.shape))
                w.key = None
        for op in ops:
            if op.kind == "irecv":
                k = (op.peer, me)
                works.append(Work(k + (self.nrecv[k],), op.tensor))
                self.nrecv[k] += 1
        return works

    def _gather(self, t):
        me = self.tls.rank
        self.slots[me] = self._snapshot(t)
        self.bar.wait()
        parts = list(self.slots)
        self.bar.wait()
        return parts

    def all_gather_into_tensor(self, out, inp, group=None):
        parts = self._gather(inp)
        self._take(out, torch.cat([p.reshape(-1) for p in parts]))

    def all_gather(self, parts, src, group=None):
        got = self._gather(src)
        for d, s in zip(parts, got):
            self._take(d, s)

    def all_reduce(self, t, group=None, op=None):
        parts = self._gather(t)
        self._take(t, sum(parts))


_SQUARE = [(False, False), (False, True), (True, False), (True, True)]  # (overlap_l0, graph)
_FAKE_F64 = [(512, 256, 2, 2, (2, 1), "poisson"), (512, 512, 4, 2, (2, 2), "poisson"),
             (512, 1024, 8, 2, (4, 2), "poisson"),
             (512, 512, 8, 2, (4, 2), "interface"),
             (512, 512, 4, 2, (2, 2), "poisson+hjac")]
# every fp64 case over the whole (overlap_l0, graph) square, under the ids the three stacked parametrisations gave
_FAKE = [pytest.param(*c, o, g, F64, id=f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-grid{i}-{c[5]}-{o}-{g}")
         for i, c in enumerate(_FAKE_F64) for o, g in _SQUARE]
# fp32: one shape over the square, the two-material problem replayed; and a window shape of _WINDOWS (10-wide blocks
# stored from column 7, 14 rows from row 11) replayed, in both precisions
_FAKE += [pytest.param(*c, o, g, T, id=f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[5]}-{o}-{g}-{'f32' if T is F32 else 'f64'}")
          for c, T, square in (((512, 512, 4, 2, (2, 2), "poisson"), F32, _SQUARE),
                               ((512, 512, 8, 2, (4, 2), "interface"), F32, [(False, True)]),
                               ((448, 320, 4, 4, (2, 2), "poisson"), F32, [(False, True), (True, True)]),
                               ((448, 320, 4, 4, (2, 2), "poisson"), F64, [(False, True)]))
          for o, g in square]


@pytest.mark.parametrize("m,n,P,Ld,grid,problem,overlap_l0,graph,dtype", _FAKE)
def test_dd_torchcomm_direct_device_path(m, n, P, Ld, grid, problem, overlap_l0, graph, dtype, monkeypatch):
    """TorchComm's RCCL branch (device views sent directly when contiguous; otherwise the one-phase packed
    batch with its pack inside the kernel segment, one message per neighbour including the diagonal ones;
    with overlap_l0 the deferred level-0 exchange; all_gather_into_tensor into the coarse f, all_reduce of
    the norm) with the ranks as threads over an in-process fake of the nccl backend: bitwise the
    single-GPU V-cycle.  This is the path the multi-GPU bench takes; one GPU cannot host two RCCL ranks.
    graph=True: every chunk shape runs three times (eager, captured, replayed), so the halo pack ('fn' step) and
    the gather staging / placement copies are checked inside replayed HIP graph segments too."""
    import threading
    from feanet_amd.dd import DDSolver, TorchComm
    f, u0, bc = _global_problem(m, n, 1, seed=3, dtype=dtype)
    calls = (1, 1, 1, 2, 2, 2) if graph else (1, 2)
    problem, _, sm = problem.partition("+")
    skw = {"smoother": "hjac", "hnet": _hnet()} if sm == "hjac" else {}
    _, ref = _single(m, n, 1, f, u0, bc, sum(calls), problem=problem, dtype=dtype, **skw)
    torch.cuda.synchronize()
    fake = _FakeDist(P)
    out, errs = {}, []
    window = (m, n, P, Ld, grid) in _WINDOW_OF
    if graph:
        # one GPU hosts every rank here: a rank's kernel segment (eager, captured or replayed) runs while no other
        # rank captures or allocates (the fake's snapshots allocate), as with one process per GPU
        orig = DDSolver.run_kernels

        def run_kernels(self, key, i):
            with fake.gpu_lock:
                orig(self, key, i)
        monkeypatch.setattr(DDSolver, "run_kernels", run_kernels)

    def run(r):
        try:
            fake.tls.rank = r
            comm = TorchComm(dist=fake, capture=False)  # the segment-wise path (the fake's ops are host-side)
            assert comm.gpu and comm.rank == r
            # each rank on its own (non-default) stream, as each process of a real run: no rank's work goes to
            # the legacy default stream, which would synchronise with (and break) another rank's graph capture
            with torch.cuda.stream(torch.cuda.Stream()):
                s = DDSolver(n, m, r, P, comm=comm, agglomerate=Ld, grid=grid, graph=graph, overlap_l0=overlap_l0,
                             problem=problem, dtype=dtype, **skw, **({"graph_min": 1} if graph else {}))
                if window:  # the coarse solution is read in place, at this rank's window
                    with fake.gpu_lock:  # (building the chunk allocates its staging buffers)
                        assert _coarse_window(s) == (s.parts[Ld].gr0, s.cparts[Ld].gr0)
                s.set_rhs(f)
                s.load(u0, bc)
                for k in calls:  # vcycle(2): joined cycles, the deferred level-0 halo finish
                    s.vcycle(k)
                out[r] = (s.owned_block(), s.residual_norm())
                torch.cuda.current_stream().synchronize()
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
            fake.bar.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    torch.cuda.synchronize()
    got = torch.full_like(ref[-1][0], float("nan"))
    for r, (((y0, y1), (x0, x1), u), nr) in out.items():
        got[:, :, y0:y1, x0:x1] = u
        if dtype is F64:
            torch.testing.assert_close(nr, ref[-1][1], rtol=1e-12, atol=0)
        else:
            _norm_close(nr, ref[-1][1], m, n, f"fake nccl rank {r}")
    assert got.dtype == dtype and torch.equal(got, ref[-1][0])
    # every rank talked to its (up to eight) neighbours only; 2-D grids: the diagonal ones too
    assert fake.posted and all(a != b for a, b, _ in fake.posted)
    pairs = {(divmod(a, grid[1]), divmod(b, grid[1])) for a, b, _ in fake.posted}
    assert all(abs(ya - yb) <= 1 and abs(xa - xb) <= 1 for (ya, xa), (yb, xb) in pairs)
    if grid[1] > 1:
        assert any(ya != yb and xa != xb for (ya, xa), (yb, xb) in pairs)
    assert not fake.mail, "unmatched messages"


@pytest.mark.parametrize("P,grid,rank,n,dtype", _cases(
    "P,grid,rank,n", [(8, (4, 2), 3, 1024), (4, (2, 2), 0, 512), (2, (2, 1), 1, 512)], [(4, (2, 2), 0, 512, F32)]))
def test_dd_captured_cycles_match_segments(P, grid, rank, n, dtype):
    """DDSolver with a capturable communicator runs whole blocks of cycles as HIP graphs — kernels AND the halo
    exchange, the finest join split into border rectangles (beside which the exchange runs on a side stream) and
    the interior (DDSolver.join_rects) — and must issue exactly the segment-wise path's work: one rank's buffers
    are bitwise equal after the eager, captured and replayed blocks.  The communicator moves nothing (the
    projection's PackComm: pack, unpack of a zero staging buffer, no all-gather), so both runs are deterministic."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tools.dd_projection import PackComm
    from feanet_amd.dd import DDSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(P + rank)
    f = torch.randn(1, 1, n + 1, n + 1, device="cuda", dtype=torch.float64, generator=g).to(dtype)
    outs = []
    for capture, split in ((False, False), (True, False), (True, True)):
        comm = PackComm()
        comm.capturable = capture
        s = DDSolver(n, n, rank, P, comm=comm, agglomerate=2, grid=grid, split_join=split, dtype=dtype)
        if split:
            border, inner = s.join_rects()
            assert inner is not None and border
        s.set_rhs(f)
        s.load()
        for k in (1, 3, 3, 3, 2):  # eager, then captured, then replayed blocks of joined cycles
            s.vcycle(k)
        torch.cuda.synchronize()
        L0 = s.local.levels[0]
        outs.append((L0.view(L0.buf(s._state)).clone(), s.local.levels[1].view(s.local.levels[1].f).clone()))
        if capture:
            assert len(s._graphs) > 0  # captured graphs (GraphCache counts those only)
    for a, b in zip(outs[1:], outs[:1] * 2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("refuse", ["self", "peer", "einval", "peer_error"])
def test_dd_capture_refusal_is_collective(refuse):
    """The captured path's fallback (DDSolver._vcycle_captured): a capture refused on this rank ('self': the
    communicator raises a stream-capture error inside the capture) or on another rank ('peer': this rank
    captures, the agreement all-reduce reports one refusal) drops EVERY rank to the segment-wise path, with the
    cycles' results bitwise those of that path.  An error that is not a capture refusal is raised on every rank
    after the same agreement all-reduce: the failing rank its own ('einval'), a rank whose peer failed a
    RuntimeError naming it ('peer_error'), so no rank waits in a collective its peer never enters."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tools.dd_projection import PackComm
    from feanet_amd.dd import DDSolver
    P, grid, rank, n = 4, (2, 2), 1, 512
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    f = torch.randn(1, 1, n + 1, n + 1, device="cuda", dtype=torch.float64, generator=g)

    class Refusing(PackComm):
        world = 2

        def exchange_many(self, s, items, wait=True, packed=False):
            if torch.cuda.is_current_stream_capturing():
                if refuse == "self":
                    raise RuntimeError("operation not permitted when stream is capturing")
                if refuse == "einval":
                    raise RuntimeError("feanet_amd: fea_dd_copy_blocks failed (invalid arguments)")
            return super().exchange_many(s, items, wait, packed)

        def allreduce_sum(self, t):  # [refusals, other errors] of this rank plus one peer's
            peer = {"peer": [1.0, 0.0], "peer_error": [0.0, 1.0]}.get(refuse, [0.0, 0.0])
            return t + torch.tensor(peer, dtype=t.dtype, device=t.device)

    outs = []
    for comm in (PackComm(), Refusing()):
        comm.capturable = isinstance(comm, Refusing)
        s = DDSolver(n, n, rank, P, comm=comm, agglomerate=2, grid=grid)
        s.set_rhs(f)
        s.load()
        if refuse in ("einval", "peer_error") and comm.capturable:
            s.vcycle(3)  # eager once
            with pytest.raises(RuntimeError, match="invalid arguments" if refuse == "einval" else "peer rank"):
                s.vcycle(3)
            return
        for k in (1, 3, 3, 3, 2):
            s.vcycle(k)
        torch.cuda.synchronize()
        if comm.capturable:
            assert not s._capture_ok and not any(k[0] == "cap" for k in s._graphs)
        L0 = s.local.levels[0]
        outs.append(L0.view(L0.buf(s._state)).clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("grid", [(2, 2), (2, 1)])
def test_dd_segment_records(grid):
    """A chunk's segments are the named records of feanet_amd.dd (Kernels / Exchanges / Gather / Scatter) and keep
    the invariants their consumers rely on.  64^2 is the smallest grid that partitions 2 x 2 at Ld = 2 (8 coarse
    rows per rank).  Batch 2: every halo region, a row slab's too, is then a strided view that goes through the
    staging buffer, so every exchange batch has a pack launch to fold.  (With one sample a row slab's halo rows
    are contiguous and go out in place: halo_pack returns None, no "fn" launch is added, and `packed` is still set
    — it means "do not pack again", which is vacuous there; the last lines pin that as it has always been.)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tools.dd_projection import PackComm
    from feanet_amd import _lib
    from feanet_amd.dd import DDSolver, Exchanges, Gather, Kernels, Scatter
    n, Ld, P = 64, 2, grid[0] * grid[1]
    keys = [("head", "a"), ("join", "b"), ("tail", "b"), ("cycle", "a")]

    def size(rec):
        try:
            return _lib.arg(rec, "H"), _lib.arg(rec, "W")
        except (TypeError, ValueError):  # a copy, a device step, or an entry point without one H x W grid
            return None

    for rank in (0, P - 1):
        s = DDSolver(n, n, rank, P, comm=PackComm(), agglomerate=Ld, grid=grid, batch=2)
        L0 = s.local.levels[0]
        seen = set()
        for key in keys:
            segs, _ = s.chunk(key)
            assert segs and all(type(seg) in (Kernels, Exchanges, Gather, Scatter) for seg in segs)
            seen |= {type(seg) for seg in segs}
            for before, seg in zip([None] + segs, segs):
                assert not (isinstance(before, Kernels) and isinstance(seg, Kernels)), (key, "adjacent kernel segments")
                if isinstance(seg, Kernels):
                    assert seg.launches
                    assert seg.lvl0 == any(size(rec) == (L0.H, L0.W) for rec in seg.launches), key
                elif isinstance(seg, Exchanges):
                    assert seg.items
                    ends_in_pack = isinstance(before, Kernels) and before.launches[-1][0] == "fn"
                    assert seg.packed == ends_in_pack, key
                elif isinstance(seg, Gather):
                    assert seg.folded == (grid[1] > 1), key
                    assert isinstance(before, Kernels)
                    if seg.folded:
                        name, args = before.launches[-1]
                        send = s._gsend.data_ptr()
                        assert (name.endswith("_send") or (name == "copy" and args[0].data_ptr() == send)
                                or (name == "rects" and int(args[0][0][0]) == send)), (key, name)
        assert {Kernels, Exchanges, Gather} <= seen
    if grid[1] == 1:  # one sample, row slabs: the halo goes out in place — no pack launch, `packed` set regardless
        s = DDSolver(n, n, 0, P, comm=PackComm(), agglomerate=Ld, grid=grid)
        segs, _ = s.chunk(("head", "a"))
        assert isinstance(segs[-1], Exchanges) and segs[-1].packed
        assert isinstance(segs[-2], Kernels) and all(name != "fn" for name, _ in segs[-2].launches)


_SEND_KINDS = [("zr2", "poisson"), ("zr1", "poisson"), ("zr2", "interface"), ("zr1", "interface")]
_EDGE, _INNER = "edge", "inner"  # the block: (5, H, 3, 40) down to the boundary row / (1, 30, 5, 15), interior only


@pytest.mark.parametrize(
    "kind,problem,B,block,dtype",
    # the fp64, one-sample, edge-block cases under their earlier ids, then every other combination
    [pytest.param(k, p, 1, _EDGE, F64, id=f"{k}-{p}") for k, p in _SEND_KINDS] +
    [pytest.param(k, p, B, blk, T, id=f"{k}-{p}-B{B}-{blk}-{'f32' if T is F32 else 'f64'}")
     for k, p in _SEND_KINDS for T in (F64, F32) for B in (1, 2) for blk in (_EDGE, _INNER)
     if (T, B, blk) != (F64, 1, _EDGE)])
def test_restriction_send_forms_bitwise(kind, problem, B, block, dtype):
    """fea_mg_zero_restrict2_send / fea_mg_zero_restrict_send (the agglomeration's send buffer filled by the
    restriction that computes f_Ld, DDSolver._send_form): the level outputs bitwise the plain launches', and the
    send buffer holds exactly the requested block of the output level (zeros where the block leaves its interior).
    Both precisions; two samples (the send buffer is [B, r1 - r0, c1 - c0]: each sample holds its own block); and
    beside the block that reaches the boundary row an interior one 10 columns wide from column 5, as an interior
    rank of a window shape has."""
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    T = dtype
    s = MultigridSolver(512, problem=problem, dtype=T, batch=B)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    s.set_rhs(f=torch.randn(B, 1, 513, 513, device="cuda", dtype=torch.float64, generator=g).to(T))
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "zr2":
        rec = s.bind_step(("resid_restrict2", 0))
        out = s.levels[2]
    else:
        rec = s.bind_step(("resid_restrict", 0, None, None))
        out = s.levels[1]
    name, args = rec
    r0, r1, c0, c1 = (5, out.H, 3, 40) if block == _EDGE else (1, 30, 5, 15)  # edge: the last (boundary) row too
    _lib.call(name, T, *args, stream)
    ref = out.view(out.f).clone()
    ref1 = s.levels[1].view(s.levels[1].f).clone()
    for Lv in s.levels[1:3]:
        Lv.f.zero_()
    send = torch.zeros((B, r1 - r0, c1 - c0), dtype=T, device="cuda")
    if kind == "zr2":
        _lib.call("mg_zero_restrict2_send", T, *args, send.data_ptr(), r0, r1, c0, c1, stream)
    else:
        assert _lib.arg(rec, "u") is None and _lib.arg(rec, "v_out") is None  # the zero-guess form: both dropped
        carried = [_lib.arg(rec, p) for p in ("f", "fc", "pid", "ktab", "omd", "ntab", "rtab", "nrtab", "w0", "B", "H",
                                              "W", "ld", "bstride", "ldc", "bstridec")]
        _lib.call("mg_zero_restrict_send", T, *carried, send.data_ptr(), r0, r1, c0, c1, stream)
    torch.cuda.synchronize()
    assert torch.equal(out.view(out.f), ref) and torch.equal(s.levels[1].view(s.levels[1].f), ref1)
    exp = ref[:, r0:r1, c0:c1].clone()
    exp[:, out.H - 1 - r0:, :] = 0  # the output level's boundary row is not written
    assert torch.equal(send, exp)
    assert B == 1 or not torch.equal(send[0], send[1])  # (the samples' blocks differ, so a lost sample term shows)


_GATHERED_F64 = [((2, 2), 1, 256), ((4, 2), 1, 256), ((2, 4), 2, 256)]
# rank blocks gcc = 5, 10, 7 and 6 columns wide (the row length of the gathered buffer): 320 / 64, 320 / 32, 448 / 64,
# 192 / 32; one and two block rows; one and two samples — but 449^2 with two samples has more nodes than the
# MID_NODES this test sets, so its plan starts with a single-level restriction: 448 runs one sample
_GATHERED_ODD = [((1, 64), 1, 320), ((2, 64), 2, 320), ((2, 32), 2, 320), ((1, 32), 1, 320), ((1, 64), 1, 448),
                 ((2, 64), 1, 448), ((1, 32), 2, 192), ((2, 32), 1, 192)]


@pytest.mark.parametrize("grid,B,n,dtype", [
    pytest.param(*c, F64, id=f"grid{i}-{c[1]}") for i, c in enumerate(_GATHERED_F64)] + [
    pytest.param(g, B, n, T, id=f"{n}-{g[0]}x{g[1]}-B{B}-{'f32' if T is F32 else 'f64'}")
    for g, B, n, T in [c + (F32,) for c in _GATHERED_F64] + [c + (T,) for c in _GATHERED_ODD for T in (F32, F64)]])
def test_mid_down_gathered_bitwise(grid, B, n, dtype, monkeypatch):
    """fea_mg_mid_down_gathered (DDSolver._gathered_form): level a's f read from the all-gather's rank blocks
    ([Pr * Pc][B][c_r][c_c]) and placed into the framed f_a by the owning tiles — outputs bitwise fea_mg_mid_down on
    the placed field, and the placed interior equal to it.  Both precisions, and rank blocks whose width is 1, 2
    and 3 (mod 4)."""
    from feanet_amd import _lib
    from feanet_amd.solver import MultigridSolver
    T = dtype
    Pr, Pc = grid
    cr, cc = n // Pr, n // Pc
    monkeypatch.setattr(MultigridSolver, "MID_NODES", 300000)  # a coarse plan that starts with mid_down
    s = MultigridSolver(n, rows=n, dtype=T, batch=B, zero_start=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    f = torch.randn(B, 1, n + 1, n + 1, device="cuda", dtype=torch.float64, generator=g).to(T)
    f[:, :, 0] = 0
    f[:, :, -1] = 0
    f[:, :, :, 0] = 0
    f[:, :, :, -1] = 0
    s.set_rhs(f=f)
    plan, _ = s._plan("a")
    name, args = plan[0]
    assert name == "mg_mid_down", [p[0] for p in plan]
    k = _lib.arg(plan[0], "k")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call(name, T, *args, stream)
    refs = [s.levels[j].view(s.levels[j].f).clone() for j in range(k + 1)]
    # the gathered blocks: rank r = ri * Pc + ci holds nodes 1 + ri cr .., 1 + ci cc ..
    L0 = s.levels[0]
    v = L0.view(L0.f)
    blocks = torch.stack([v[:, 1 + ri * cr:1 + (ri + 1) * cr, 1 + ci * cc:1 + (ci + 1) * cc]
                          for ri in range(Pr) for ci in range(Pc)]).contiguous()
    for j in range(k + 1):
        s.levels[j].f.zero_()
    _lib.call("mg_mid_down_gathered", T, *args, blocks.data_ptr(), Pr, Pc, cr, cc, stream)
    torch.cuda.synchronize()
    got0 = s.levels[0].view(s.levels[0].f)
    assert torch.equal(got0[:, 1:-1, 1:-1], refs[0][:, 1:-1, 1:-1])
    for j in range(1, k + 1):
        assert torch.equal(s.levels[j].view(s.levels[j].f), refs[j]), j
