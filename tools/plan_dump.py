"""Launch plans as text, every device pointer replaced by a symbolic name: the check that a change of the host
layer leaves every launch, its order and every argument as they were.

For a set of small solver configurations (every kernel name MultigridSolver._plan_bytes accounts for, the joined
program, the PCG iteration, the decomposed solver's folded gather, in-place coarse read, first HJac chunk and the
segment builder's switches: overlap_l0, fold_gather=False, one rank, split_join) prints
each launch record as  name(arg, arg, ...)  in C-ABI order — a pointer as <level>.<buffer>, a table's name, a
PtrArray element by element, otherwise base+offset — and the integer bytes_per_vcycle().  The text holds no
address, so two checkouts that bind the same plans print the same bytes:

GPU box:  python tools/plan_dump.py OUT.txt      (then diff the files of the two checkouts)
"""
import contextlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "multigrid-feanet_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from feanet_amd import mesh_setup as ms  # noqa: E402
from feanet_amd.dd import DDSolver, Exchanges, Gather, Kernels  # noqa: E402
from feanet_amd.pcg import PCGSolver  # noqa: E402
from feanet_amd.solver import MultigridSolver  # noqa: E402
from tools.dd_projection import PackComm  # noqa: E402

T32, T64 = torch.float32, torch.float64


def hnet():
    w = np.load(os.path.join(HERE, "..", "multigrid-feanet_amd", "feanet_amd", "weights", "hnet_iso_poisson_33x33.npz"))
    return np.stack([w[f"conv{i}"].reshape(3, 3) for i in range(3)])


@contextlib.contextmanager
def mid_nodes(v):
    old = MultigridSolver.MID_NODES
    MultigridSolver.MID_NODES = v
    try:
        yield
    finally:
        MultigridSolver.MID_NODES = old


class Names:
    """Address ranges of the tensors a solver owns -> names."""

    def __init__(self):
        self.regions = []

    def add(self, name, t):
        if torch.is_tensor(t) and t.is_cuda and t.numel():
            self.regions.append((t.data_ptr(), t.numel() * t.element_size(), name))

    def add_mg(self, pre, s):
        for l, Lv in enumerate(s.levels):
            for b in ("f", "a", "b", "zero", "c", "pid"):
                self.add(f"{pre}L{l}.{b}", getattr(Lv, b, None))
        for b in ("ktab", "omd", "rtab", "ptab", "hw", "tail_pid", "ws", "norm_out", "_hist", "_cnt", "_sws", "_raw"):
            self.add(f"{pre}{b}", getattr(s, b, None))

    def add_pcg(self, p):
        for b in ("x", "b", "r", "part", "sc", "hist", "sb", "ktab"):
            self.add(f"pcg.{b}", getattr(p, b, None))
        self.add("pcg.p0", p.p[0])
        self.add("pcg.p1", p.p[1])
        for b in ("f", "a", "b", "pid"):
            self.add(f"pcg.L0.{b}", getattr(p.L0, b, None))
        self.add_mg("mg.", p.mg)

    def add_dd(self, d):
        self.add_mg("loc.", d.local)
        self.add_mg("crs.", d.coarse)
        for b in ("_gstage", "_gsend", "_raw"):
            self.add(f"dd.{b}", getattr(d, b, None))

    def ptr(self, v):
        for base, size, name in self.regions:
            if base <= v < base + size:
                return name if v == base else f"{name}+{v - base}"
        return "<unknown pointer>"

    def val(self, v):
        if v is None:
            return "NULL"
        if hasattr(v, "arr"):  # _lib.PtrArray
            return "[" + ", ".join(self.val(x) for x in v.arr) + "]"
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, (int, np.integer)):
            return self.ptr(int(v)) if int(v) >= 1 << 32 else str(int(v))
        if torch.is_tensor(v):
            return f"view({self.ptr(v.data_ptr())}, {tuple(v.shape)}, {tuple(v.stride())})"
        if isinstance(v, np.ndarray):  # fea_dd_copy_rects records
            return "[" + ", ".join("(" + ", ".join(self.val(x) for x in row) + ")" for row in v) + "]"
        return repr(v)

    def launch(self, rec):
        name, args = rec
        if name == "fn":
            return "fn(<device step>)"
        return f"{name}(" + ", ".join(self.val(a) for a in args) + ")"


OUT = []


def emit(line=""):
    OUT.append(line)


def dump_launches(names, launches, indent="  "):
    for rec in launches:
        emit(indent + names.launch(rec))


def dump_mg(label, s, joined_k=None):
    emit(f"== {label}")
    plan, end = s._plan("a")
    joined = s.joined_program(joined_k) if joined_k else None
    names = Names()
    names.add_mg("", s)
    emit(f"plan from a -> {end}")
    dump_launches(names, plan)
    plan_b, end_b = s._plan("b")
    names = Names()
    names.add_mg("", s)
    emit(f"plan from b -> {end_b}")
    dump_launches(names, plan_b)
    if joined:
        prog, jend = joined
        emit(f"joined program k={joined_k} -> {jend}")
        for key, launches in prog:
            emit(f" segment {key}")
            dump_launches(names, launches, "   ")
    emit(f"bytes_per_vcycle = {int(s.bytes_per_vcycle())}")
    emit()


def dump_first_cycle(label, s):
    """The launches of the first cycle after load() (smoother='hjac': its first finest-level sweep reads the
    un-reset iterate), recorded instead of launched."""
    emit(f"== {label}")
    s.load()
    seen = []
    s._launch = seen.extend
    s.vcycle()
    names = Names()
    names.add_mg("", s)
    dump_launches(names, seen)
    emit()


def dump_pcg(label, p):
    emit(f"== {label}")
    for q in (0, 1):
        launches = p._iteration(q)
        names = Names()
        names.add_pcg(p)
        emit(f"iteration reading p[{q}]")
        dump_launches(names, launches)
    emit()


def comm_text(seg):
    """A communication step in the wording the plan text has always had: the step's name, then its fields, a
    flag only where it is set."""
    if isinstance(seg, Exchanges):
        return repr(("exchanges", seg.items) + ((True,) if seg.packed else ()))
    if isinstance(seg, Gather):
        return repr(("gather",) + ((True,) if seg.folded else ()))
    return repr(("scatter", seg.dst))


def dump_dd(label, d, keys):
    emit(f"== {label}")
    emit(f"exchange depths {d.depths}, coarse plan -> {d.coarse_end}")
    for key in keys:
        segs, end = d.chunk(key)
        names = Names()
        names.add_dd(d)
        emit(f"chunk {key} -> {end}")
        for seg in segs:
            if isinstance(seg, Kernels):
                emit(f" kernels (level 0: {seg.lvl0})")
                dump_launches(names, seg.launches, "   ")
            else:
                emit(f" comm {comm_text(seg)}")
    emit()


def single_gpu_cases():
    """(label, constructor) of the single-GPU configurations; tests/test_gpu_mg.py pins their byte counts."""
    lin = ms.linear_transfer_kernel() / np.float32(4.0)
    tab16 = np.stack([lin * np.float32(1.0 + p / 64.0) for p in range(16)])
    M = MultigridSolver

    def two_level(s):
        """The plan of the one- and two-level launches alone: this dump, and the byte count the tests pin for it,
        stay the text they were before the three-level grouping (whose own plans and bytes
        tests/test_gpu_three_level.py pins); between them the cases still meet every kernel name of _plan_bytes."""
        s.THREE_LEVEL_DOWN = s.THREE_LEVEL_UP = False
        return s
    return [
        ("poisson n=1024 fp32", lambda: two_level(M(1024, dtype=T32)), 0),
        ("poisson n=512 fp32 MID_NODES=300000", lambda: M(512, dtype=T32), 300000),
        ("poisson n=32 fp64 unfused V(2,2), no tail", lambda: M(32, coarse_tail=False, fuse=False, nu1=2, nu2=2), 0),
        ("poisson n=32 fp64 unfused V(2,0), no tail", lambda: M(32, coarse_tail=False, fuse=False, nu1=2, nu2=0), 0),
        ("interface n=32 fp64 compat=mm_interface_q2", lambda: M(32, problem="interface", compat="mm_interface_q2"), 0),
        ("poisson n=128 fp64 zero_start", lambda: M(128, zero_start=True), 0),
        ("interface n=128 fp32 B=2, 16-row R/P", lambda: M(128, problem="interface", dtype=T32, batch=2, R=tab16,
                                                          P=tab16), 0),
        ("poisson n=256 fp32 B=64", lambda: M(256, dtype=T32, batch=64), 0),
        ("hjac n=256 fp32", lambda: M(256, dtype=T32, smoother="hjac", hnet=hnet()), 0),
        ("hjac n=512 fp32", lambda: M(512, dtype=T32, smoother="hjac", hnet=hnet()), 0),
        ("hjac n=32 fp64 unfused", lambda: M(32, smoother="hjac", hnet=hnet(), fuse=False), 0),
    ]


def attempt(label, fn):
    """Run one configuration; a refusal (e.g. no partition for this grid) is printed, not fatal."""
    try:
        fn()
    except (ValueError, RuntimeError, AssertionError) as e:
        emit(f"!! {label}: {type(e).__name__}: {e}")
        emit()


def main():
    for label, make, mid in single_gpu_cases():
        def one(label=label, make=make, mid=mid):
            with mid_nodes(mid or MultigridSolver.MID_NODES):
                dump_mg(label, make(), joined_k=3 if label == "poisson n=1024 fp32" else None)
        attempt(label, one)
    attempt("hjac first cycle", lambda: dump_first_cycle("hjac n=64 fp64, first cycle after load()",
                                                         MultigridSolver(64, smoother="hjac", hnet=hnet())))
    attempt("pcg fp64", lambda: dump_pcg("pcg n=64 fp64", PCGSolver(64, dtype=T64)))
    attempt("pcg mixed", lambda: dump_pcg("pcg n=64 fp64 / fp32 preconditioner",
                                          PCGSolver(64, dtype=T64, precond_dtype=T32)))
    attempt("pcg interface", lambda: dump_pcg("pcg interface n=64 fp32 B=2",
                                              PCGSolver(64, problem="interface", dtype=T32, batch=2)))

    joined = [("head", "a"), ("join", "b"), ("join", "a"), ("tail", "b"), ("cycle", "a")]

    def dd(label, keys=joined, mid=0, load=False, **kw):
        def one():
            with mid_nodes(mid or MultigridSolver.MID_NODES):
                d = DDSolver(comm=PackComm(), **kw)
                if load:
                    d.load()
                dump_dd(label, d, keys)
        attempt(label, one)
    # 2-D blocks: the restriction that computes f_Ld in its _send form (zero_restrict2 at Ld = 2, the single
    # restriction at Ld = 1), the coarse plan's mid_down in its _gathered form
    for Ld in (2, 1):
        dd(f"dd 512^2 4 ranks (2, 2) rank 0 Ld={Ld}, MID_NODES=300000", mid=300000, n=512, rows=512, rank=0, world=4,
           agglomerate=Ld, grid=(2, 2))
    dd("dd interface 512^2 4 ranks (2, 2) rank 3 Ld=2", n=512, rows=512, rank=3, world=4, agglomerate=2, grid=(2, 2),
       problem="interface")
    # Ld = 3: the level-pair prolongation at level 1 reads the coarse solution in place
    dd("dd 1024^2 8 ranks (4, 2) rank 3 Ld=3", n=1024, rows=1024, rank=3, world=8, agglomerate=3, grid=(4, 2))
    dd("dd 1024 x 512 2 row slabs rank 1 Ld=3", n=512, rows=1024, rank=1, world=2, agglomerate=3)
    # learned smoother: the first chunk after load() (the un-reset iterate)
    dd("dd hjac 512^2 4 ranks (2, 2) rank 0 Ld=2", keys=[("first", "a"), ("cycle", "b")], load=True, n=512, rows=512,
       rank=0, world=4, agglomerate=2, grid=(2, 2), smoother="hjac", hnet=hnet())

    # the segment builder's switches: the finest halo as a batch of its own, the agglomeration's copies unfolded,
    # one rank (no exchange, the all-gather a device copy), and split_join (which chunk() must not depend on)
    for label, kw in (("overlap_l0", dict(world=4, grid=(2, 2), overlap_l0=True)),
                      ("fold_gather=False", dict(world=4, grid=(2, 2), fold_gather=False)),
                      ("one rank", dict(world=1)),
                      ("split_join", dict(world=4, grid=(2, 2), split_join=True))):
        dd(f"dd 512^2 Ld=2 rank 0, {label}", n=512, rows=512, rank=0, agglomerate=2, **kw)

    text = "\n".join(OUT) + "\n"
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
