"""Results of a fixed list of small solver configurations as SHA-256 digests: the check that a change of the
device code leaves every computed bit as it was, across two builds of the library.

The tests compare kernels of one build with each other, so a change common to both sides passes them.  This
prints, for seeded inputs, one line  `label  result  sha256`  per result — the iterate after 3 V-cycles and the
residual history of a short solve() (PCG: iterate and history after 4 iterations) — over both dtypes, the Poisson
and the two-material problem with the shipped learned transfer weights (per-pattern R / P tables), grids that cross
the strip widths and give the two-level kernels several tasks per strip, one rectangle, batches 1 and 3, the
nontemporal instantiations (FEANET_NT_BYTES=0), the decomposed solver in one process and one decomposed rank whose
zero-guess restrictions also fill the agglomeration's send buffer.  The text holds nothing but labels and digests:

GPU box:  python tools/lab/with_lib.py OLD.so tools/field_digest.py old.txt
          python tools/lab/with_lib.py -      tools/field_digest.py new.txt      (then diff the two files)
"""
import contextlib
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "multigrid-feanet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from feanet_amd import _lib  # noqa: E402
from feanet_amd.coef import CoefPeriodicPCGSolver  # noqa: E402
from feanet_amd.dd import DDSolver, Kernels, LocalGroup  # noqa: E402
from feanet_amd.pcg import PCGSolver  # noqa: E402
from feanet_amd.periodic import PeriodicPCGSolver  # noqa: E402
from feanet_amd.solver import MultigridSolver  # noqa: E402
from tools.dd_projection import PackComm  # noqa: E402

T32, T64 = torch.float32, torch.float64
OUT = []


def learned():
    w = np.load(os.path.join(HERE, "..", "multigrid-feanet_amd", "feanet_amd", "weights",
                             "multigrid_interface_ratio.npz"))
    return dict(R=w["R"][0], P=w["P"][:, 0], w=w["w"])


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def emit(label, what, *arrays):
    OUT.append(f"{label:58s} {what:9s} {sha(*arrays)}")


def rhs(B, H, W, dtype, seed):
    """seeded on the host, so the same bits whatever the device library"""
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(B, 1, H, W, dtype=T64, generator=g).to(dtype).cuda()


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@contextlib.contextmanager
def mid_nodes(v):
    old = MultigridSolver.MID_NODES
    MultigridSolver.MID_NODES = v
    try:
        yield
    finally:
        MultigridSolver.MID_NODES = old


def mg(label, n, dtype, problem, B, rows=None, seed=1):
    kw = learned() if problem == "interface" else {}
    s = MultigridSolver(n, rows=rows, problem=problem, dtype=dtype, batch=B, **kw)
    f = rhs(B, (rows or n) + 1, n + 1, dtype, seed)
    s.set_rhs(f=f)
    s.load()
    s.vcycle(3)
    emit(label, "vcycle3", s.solution())
    u, hist = s.solve(f=f, eps=0.0, max_cycles=5)
    emit(label, "solve", u, np.stack([np.asarray(h) for h in hist]))


def pcg(label, n, precond):
    p = PCGSolver(n, dtype=T64, precond_dtype=precond)
    p.set_rhs(f=rhs(1, n + 1, n + 1, T64, 5))
    p.load()
    p.iterate(4)
    emit(label, "iterate4", p.solution())
    emit(label, "history", np.stack([np.asarray(h) for h in p.history()]))


def torus(label, family, m, n, dtype, B=3):
    """every torus kernel of one family on seeded fields (through the solver's own launches, so on its operator data),
    then x and the residual history of 4 iterations of solve()"""
    rng = np.random.default_rng([m, n])
    kw = dict(rows=m, dtype=dtype, batch=B, graph=False)
    if family == "per":
        s = PeriodicPCGSolver(n, phase=(rng.random((m, n)) < 0.4).astype(np.uint8), prop=(1, 20), **kw)
        op = s._stencil
    else:
        s = CoefPeriodicPCGSolver(n, coef=np.exp(rng.standard_normal((m, n))), **kw)
        op = s._field
    L = s.levels[0]

    def field(ref):
        buf = torch.zeros_like(ref)
        rows, cols = buf.shape[1], n if buf.shape[1] == m else n // 2
        buf[..., :cols] = torch.from_numpy(rng.standard_normal((B, rows, cols))).to(dtype).cuda()
        return buf

    u, out = field(L.f), torch.zeros_like(L.f)
    L.f.copy_(field(L.f))
    s._sweep(L, u, out)
    emit(label, "sweep", out)
    s._sweep(L, None, out)
    emit(label, "sweep0", out)
    emit(label, "apply", out, s.apply(u, out, sums=True))
    if family == "per":
        emit(label, "reduce", s._reduce(u, L.f).clone(), s._reduce(u))
    if len(s.levels) > 1:
        C = s.levels[1]
        for what, ptr in (("restrict", u.data_ptr()), ("restrict0", None)):
            s._call(family + "_residual_restrict", u=ptr, f=L.f.data_ptr(), fc=C.f.data_ptr(), **op(L), B=B,
                    **L.geom(), ldc=C.ld, bstridec=C.bs)
            emit(label, what, C.f)
        if family == "per":
            s._call("per_prolong_add", ec=field(C.f).data_ptr(), u=u.data_ptr(), B=B, **L.geom(), ldc=C.ld,
                    bstridec=C.bs)
            emit(label, "prolong", u)
    x = s.solve(field(L.f)[..., :n], rtol=0.0, max_iters=4)
    emit(label, "solve4", x, np.stack(s.history))


def main():
    name = {T32: "fp32", T64: "fp64"}
    for dtype in (T64, T32):
        for problem in ("poisson", "interface"):
            for n in (32, 256, 1024):
                for B in (1, 3):
                    mg(f"mg {problem} {n + 1}^2 {name[dtype]} B={B}", n, dtype, problem, B)
        mg(f"mg poisson 65 x 321 {name[dtype]} B=1", 320, dtype, "poisson", 1, rows=64, seed=2)
    with env("FEANET_NT_BYTES", "0"):  # every level streams: the nontemporal instantiations
        for dtype in (T64, T32):
            for problem in ("poisson", "interface"):
                mg(f"mg {problem} 257^2 {name[dtype]} B=1 NT_BYTES=0", 256, dtype, problem, 1, seed=3)
    for n in (64, 256):
        pcg(f"pcg {n + 1}^2 fp64", n, None)
        pcg(f"pcg {n + 1}^2 fp64 / fp32 preconditioner", n, T32)

    n = 256
    grp = LocalGroup(n, n, 4, agglomerate=2, grid=(2, 2))
    grp.set_rhs(f=rhs(1, n + 1, n + 1, T64, 7))
    grp.load()
    grp.vcycle(3)
    emit("dd LocalGroup 2 x 2 257^2 fp64", "vcycle3", grp.solution())

    # one rank of 2-D blocks: the restriction that computes f_Ld also fills the all-gather's send buffer
    # (fea_mg_zero_restrict_send at Ld = 2, fea_mg_zero_restrict2_send at Ld = 3; the label names the launch found);
    # the communicator moves nothing
    for n, world, grid, rank, Ld in ((512, 4, (2, 2), 0, 2), (1024, 8, (4, 2), 3, 3)):
        with mid_nodes(300000):
            d = DDSolver(n, n, rank, world, comm=PackComm(), agglomerate=Ld, grid=grid)
            d.set_rhs(rhs(1, n + 1, n + 1, T64, 9))
            d.load()
            d.vcycle(3)
            torch.cuda.synchronize()
            names = [r[0] for key in (("head", "a"), ("cycle", "a")) for seg in d.chunk(key)[0]
                     if isinstance(seg, Kernels) for r in seg.launches]
            sends = sorted({x for x in names if x.endswith("_send")})
            L0 = d.local.levels[0]
            emit(f"dd rank {rank} of {grid[0]} x {grid[1]} {n + 1}^2 Ld={Ld} {'+'.join(sends) or 'no _send'}", "vcycle3",
                 L0.view(L0.buf(d._state)), d._gsend if getattr(d, "_gsend", None) is not None else np.zeros(0))

    # the smallest m at n = 16 with more than one row task (the same for both types: one strip)
    m_tasks = next(m for m in range(2, 64) if min(_lib.lib().fea_per_parts(m, 16, e) for e in (4, 8)) > 1)
    for family in ("per", "coef"):
        for dtype in (T64, T32):
            for m, n in ((6, 258), (m_tasks, 16), (32, 130)):
                torus(f"torus {family} {m} x {n} {name[dtype]} B=3", family, m, n, dtype)

    text = "\n".join(OUT) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
