"""Write footprint and padding independence of the framed entry points (helper of test_footprint_host.py and
test_gpu_footprint.py, in the role of dd_oracle.py).

A framed level keeps its H x W nodes inside a ghost ring, pads every row to ld and every sample to bstride, and the
solver's allocator (_Level) adds 256 elements of slack.  The kernels load from all of that storage and rely on selects
and masked stores to keep it out of their results.  A case here describes one accepted call of an entry point: its
operands, which of them are outputs, and for each output the documented write set as a boolean mask over the WHOLE raw
allocation.  The call runs twice on the same node data:

  run Z: every non-node element of the inputs is zero, the outputs are pre-filled with the canary byte C1;
  run P: every non-node element is poison (a quiet NaN in fields, random VALID pattern ids in pattern maps, except
         where include/feanet_hip.h requires content: that content is kept), the outputs hold the canary byte C2.

check() then asserts, on bytes:
  (a) outside its write set an output still holds what it held before the call, in both runs;
  (b) every input's raw buffer is unchanged, in both runs;
  (c) the write set is bit-identical between Z and P (the result does not depend on storage that holds no node);
  (d) no element of the write set is untouched in both runs (something was stored there).
An in-place operand (x and r of fea_pcg_update) counts as an output whose "canary" is its own initial content.
A `loose` write set (a norm workspace the header only bounds) may be written anywhere inside: there an element is
either untouched in both runs or bit-identical.

Nothing here needs an oracle: tables are random with a positive diagonal, pattern maps random ids.

The same descriptors drive the task-height ladders and the sample-isolation runs of test_gpu_task_heights.py (the
section "task-height ladders" at the end): there the buffers stay on the GPU and only run Z is used."""
import ctypes

import numpy as np

from test_mg_host import ARGS, MAXP, base, multi

C1, C2 = 0xC1, 0xC2
SLACK = 256       # elements the level allocator adds behind the last sample
W0, W1 = 1.25, 0.75
FINITE = -7251.5  # poison where the header asks for finite values (fea_mg_cycle_join: boundary nodes kept as 0 * r + b)

# the Krylov entry points, in the form of test_mg_host.ARGS (argument names in header order, without the stream)
PCG_ARGS = {
    "pcg_residual": "x f r pid ktab ntab part B H W ld bs",
    "pcg_direction": "z p_in p_out pid ktab ntab scalars part B H W ld bs",
    "pcg_update": "p x r pid ktab ntab scalars part B H W ld bs",
    "pcg_dot": "r z part B H W ld bs",
}
MIXED_ARGS = {
    "fea_pcg_narrow_f64f32": "r r32 scalars sb B H W ld bs ld32 bs32",
    "fea_pcg_dot_f64f32": "r z32 part B H W ld bs ld32 bs32",
    "fea_pcg_direction_f64f32": "z32 p_in p_out pid ktab ntab scalars part B H W ld bs ld32 bs32",
    "fea_pcg_update_f64f32": "p x r r32 pid ktab ntab scalars sb part B H W ld bs ld32 bs32",
}
DD_NAMES = ("fea_dd_copy_blocks", "fea_dd_copy_rects")
NSCAL, BETA, ALPHA, RNORM, DONE = 12, 4, 3, 5, 6    # FEA_PCG_* of include/feanet_hip.h


class FootprintError(AssertionError):
    """kind: the assertion that failed, 'a' .. 'd' (module docstring); 'v': an exact expected value (the halo copies,
    fea_mg_unpack, the zeros fea_pcg_residual stores on the boundary nodes); 'h', 's', 'n': the ladder's assertions
    (height or batch dependence, a leak between samples, a NaN dropped from a norm; see "task-height ladders")."""

    def __init__(self, kind, operand, msg):
        super().__init__(f"({kind}) {operand}: {msg}")
        self.kind, self.operand = kind, operand


# ----------------------------------------------------------------------------- layout and masks
class Geo:
    """The raw allocation of a framed buffer: B samples of H x W nodes (pid: one uint8 map), slack included."""

    def __init__(self, H, W, B, esz, ld=None, bs=None, pid=False):
        if ld is None:
            from feanet_amd import _lib
            ld, bs = _lib.mg_layout(H, W, esz)
        if pid:
            B, bs = 1, (H + 2) * ld
        self.H, self.W, self.B, self.esz, self.ld, self.bs, self.is_pid = H, W, B, esz, ld, bs, pid
        self.off = 128 // esz - 1
        self.numel = B * bs + SLACK

    def coarse(self):
        return Geo((self.H + 1) // 2, (self.W + 1) // 2, self.B, self.esz)

    def pid(self):
        return Geo(self.H, self.W, 1, self.esz, self.ld, self.bs, pid=True)

    def index(self, rows, cols):
        """flat indices [B, len(rows), len(cols)] of the frame positions (r, c), r in -1 .. H, c in -1 .. W"""
        r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        return (np.arange(self.B, dtype=np.int64)[:, None, None] * self.bs + (r[None, :, None] + 1) * self.ld +
                self.off + c[None, None, :])

    def mask(self, rows, cols):
        m = np.zeros(self.numel, bool)
        m[self.index(rows, cols).ravel()] = True
        return m

    def nodes(self):
        return self.mask(np.arange(self.H), np.arange(self.W))

    def interior(self):
        return self.mask(np.arange(1, self.H - 1), np.arange(1, self.W - 1))

    def boundary(self):
        return self.nodes() & ~self.interior()

    def ring(self):
        return self.mask(np.arange(-1, self.H + 1), np.arange(-1, self.W + 1)) & ~self.nodes()

    def where(self, i):
        """a raw index in words: sample, frame row and column (node coordinates), or the slack"""
        if i >= self.B * self.bs:
            return f"slack element {i - self.B * self.bs}"
        b, rem = divmod(int(i), self.bs)
        r, c = divmod(rem, self.ld)
        return f"sample {b} row {r - 1} column {c - self.off}"

    def framed(self, nodes, fill, dtype):
        raw = np.full(self.numel, fill, dtype)
        raw[self.index(np.arange(self.H), np.arange(self.W)).ravel()] = np.asarray(nodes, dtype).ravel()
        return raw


def canary(n, dtype, byte):
    return np.full(n * np.dtype(dtype).itemsize, byte, np.uint8).view(dtype)


class Operand:
    """name; role 'in' / 'out' / 'inout'; z, p: the raw buffer before run Z / run P; mask: the write set.

    make: builds (z, p) on first use instead (the tall ladder cases never need p, and build z on the device from
    `nodes`, the compact [B, H, W] node values of a framed field, or `fill`, an output's canary byte).
    sample(B, b): where sample b lives in the raw buffer of a call with B samples (a slice or an index array); None:
    the operand is shared by all samples (tables, pattern maps, counters, loosely bounded workspaces).
    norm: 'norm' a per-sample norm (one double per sample), 'parts' a per-sample set of partial sums, 'ws' the loosely
    bounded workspace behind a norm (only the number of slots stored to is read from it)."""

    def __init__(self, name, role, z=None, p=None, mask=None, loose=False, geo=None, make=None, nodes=None,
                 fill=None, dtype=None, numel=None, sample=None, norm=None):
        self.name, self.role, self.mask, self.loose, self.geo = name, role, mask, loose, geo
        self._z, self._p, self._make, self.nodes, self.fill = z, p, make, nodes, fill
        self.dtype = np.dtype(z.dtype if z is not None else dtype)
        self.numel = z.size if z is not None else numel
        self.sample, self.norm = sample, norm
        if sample is None and geo is not None and not geo.is_pid:
            self.sample = lambda B, b, bs=geo.bs: slice(b * bs, (b + 1) * bs)
        if z is not None:
            assert z.shape == p.shape and z.dtype == p.dtype and z.ndim == 1
        assert (role == "in") == (mask is None) and (mask is None or mask.shape == (self.numel,))

    def _built(self):
        if self._z is None:
            self._z, self._p = self._make()
            assert self._z.shape == self._p.shape == (self.numel,) and self._z.dtype == self._p.dtype == self.dtype
        return self._z, self._p

    @property
    def z(self):
        return self._built()[0]

    @property
    def p(self):
        return self._built()[1]

    def where(self, i):
        return self.geo.where(i) if self.geo is not None else f"element {int(i)}"


def field_in(name, geo, dtype, nodes, keep=None, finite=False):
    """an input field; keep: mask of non-node storage whose (zero) content the header requires; finite: the header
    requires finite values in the frame (the B * bstride elements), so the poison there is finite garbage and only
    the slack behind the last sample is NaN"""
    nodes = np.asarray(nodes, dtype)

    def make():
        z, p = geo.framed(nodes, 0, dtype), geo.framed(nodes, np.nan, dtype)
        if finite:
            p[~geo.nodes() & (np.arange(geo.numel) < geo.B * geo.bs)] = FINITE
        if keep is not None:
            p[keep] = z[keep]
        return z, p
    return Operand(name, "in", make=make, geo=geo, nodes=nodes, dtype=dtype, numel=geo.numel)


def field_out(name, geo, dtype, mask):
    return Operand(name, "out", make=lambda: (canary(geo.numel, dtype, C1), canary(geo.numel, dtype, C2)), mask=mask,
                   geo=geo, fill=C1, dtype=dtype, numel=geo.numel)


def field_inout(name, geo, dtype, nodes, mask, keep=None):
    o = field_in(name, geo, dtype, nodes, keep)
    o.role, o.mask = "inout", mask
    return o


def pid_in(name, geo, ids, ntab, rng):
    """a framed pattern map: poison is random VALID ids (an id >= ntab would index past the tables)"""
    ids = np.asarray(ids, np.uint8)
    seed = int(rng.integers(1 << 30))       # (drawn now: the case's other operands do not depend on when p is built)

    def make():
        z = geo.framed(ids, 0, np.uint8)
        p = np.random.default_rng(seed).integers(0, ntab, geo.numel).astype(np.uint8)
        p[geo.nodes()] = z[geo.nodes()]
        return z, p
    return Operand(name, "in", make=make, geo=geo, nodes=ids[None], dtype=np.uint8, numel=geo.numel)


def flat_in(name, arr, sample=None):
    a = np.ascontiguousarray(arr).reshape(-1)
    return Operand(name, "in", a, a.copy(), sample=sample)


def flat_out(name, n, dtype, mask=None, loose=False, sample=None, norm=None):
    return Operand(name, "out", canary(n, dtype, C1), canary(n, dtype, C2),
                   np.ones(n, bool) if mask is None else mask, loose, sample=sample, norm=norm)


def flat_inout(name, arr, mask):
    a = np.ascontiguousarray(arr).reshape(-1)
    return Operand(name, "inout", a, a.copy(), mask)


def rows(per):
    """sample(B, b) of a flat [B, per] operand"""
    return lambda B, b: slice(b * per, (b + 1) * per)


# ----------------------------------------------------------------------------- the four assertions
def _same(a, b):
    """per element: the same bytes"""
    n = a.dtype.itemsize
    return (np.ascontiguousarray(a).view(np.uint8).reshape(-1, n) ==
            np.ascontiguousarray(b).view(np.uint8).reshape(-1, n)).all(1)


def check(ops, after_z, after_p):
    """Assertions (a) .. (d) on the buffers after run Z and run P ({operand name: raw array})."""
    for op in ops:
        az, ap = after_z[op.name], after_p[op.name]

        def fail(kind, bad, what):
            i = np.flatnonzero(bad)
            raise FootprintError(kind, op.name, f"{what}: {len(i)} elements, first at {op.where(i[0])} "
                                 f"(Z {az[i[0]]!r}, P {ap[i[0]]!r})")
        uz, up = _same(op.z, az), _same(op.p, ap)          # untouched by run Z / run P
        if op.role == "in":
            for run, u in (("Z", uz), ("P", up)):
                if not u.all():
                    fail("b", ~u, f"input modified in run {run}")
            continue
        m = op.mask
        for run, u in (("Z", uz), ("P", up)):
            if (~u & ~m).any():
                fail("a", ~u & ~m, f"written outside the write set in run {run}")
        eq = _same(az, ap)
        if op.loose:
            if (m & ~eq & ~(uz & up)).any():
                fail("c", m & ~eq & ~(uz & up), "result depends on non-node storage")
            continue
        if (m & uz & up).any():
            fail("d", m & uz & up, "write-set element never stored")
        if (m & ~eq).any():
            fail("c", m & ~eq, "result depends on non-node storage")


class Ref:
    """the device address of an operand's buffer (a call argument)"""

    def __init__(self, name):
        self.name = name


class Refs:
    """a host array of device addresses (const T* const*); None entries stay NULL"""

    def __init__(self, names):
        self.names = list(names)


class Host:
    """a host array built from the device addresses: make({name: address}) -> numpy array"""

    def __init__(self, make):
        self.make = make


class Case:
    def __init__(self, entry, suf, label):
        self.entry, self.suf, self.label = entry, suf, label
        self.ops, self.calls, self.expect = [], [], {}
        self.B = self.norm_n = self.nan_op = None     # samples; nodes a norm of the call sums; the field it is a norm of

    def __repr__(self):
        return f"{self.entry}[{self.suf} {self.label}]"

    def add(self, op):
        assert all(o.name != op.name for o in self.ops), op.name
        self.ops.append(op)
        return Ref(op.name)


def run_case(case, launch):
    """launch(case, {name: raw array}) -> {name: raw array after the case's calls}; runs Z and P, then check()."""
    after = {}
    for run in "ZP":
        bufs = {op.name: (op.z if run == "Z" else op.p).copy() for op in case.ops}
        after[run] = launch(case, bufs)
    check(case.ops, after["Z"], after["P"])
    for name, (mask, want) in case.expect.items():
        for run in "ZP":
            bad = mask & ~_same(after[run][name], want)
            if bad.any():
                raise FootprintError("v", name, f"wrong value in run {run} at element {np.flatnonzero(bad)[0]}")
    return after


def gpu_launch(case, bufs):
    """Upload, issue the case's calls on the default stream, download."""
    import torch
    dev = {n: torch.from_numpy(a.view(np.uint8)).cuda() for n, a in bufs.items()}
    keep = _issue(case, {n: t.data_ptr() for n, t in dev.items()})
    torch.cuda.synchronize()
    del keep
    return {n: dev[n].cpu().numpy().view(bufs[n].dtype) for n in bufs}


def _issue(case, addr):
    """the case's calls on the default stream, on buffers at the device addresses addr -> the host arrays the calls
    were given (alive until the caller has synchronised)"""
    from feanet_amd import _lib
    keep = []

    def conv(x):
        if isinstance(x, Ref):
            return addr[x.name]
        if isinstance(x, Refs):
            arr = (ctypes.c_void_p * len(x.names))(*[None if n is None else addr[n] for n in x.names])
            keep.append(arr)
            return ctypes.cast(arr, ctypes.c_void_p).value
        if isinstance(x, Host):
            arr = np.ascontiguousarray(x.make(addr))
            keep.append(arr)
            return arr.ctypes.data
        return x
    for sym, args in case.calls:
        rc = getattr(_lib.lib(), sym)(*[conv(a) for a in args], None)
        assert rc == 0, f"{case}: {sym} returned {rc}"
    return keep


# ----------------------------------------------------------------------------- case builder
def npdt(suf):
    return np.float32 if suf == "f32" else np.float64


class Builder:
    """One accepted call of an mg / pcg entry point on random node data (test_mg_host.base() / multi() with real
    operands).  Level j of the hierarchy under the H x W grid is geos[j]."""

    def __init__(self, entry, suf, H, W, B, two, mode, args=None):
        self.entry, self.suf, self.two, self.mode = entry, suf, two, mode
        self.dt = npdt(suf)
        self.esz = np.dtype(self.dt).itemsize
        self.rng = np.random.default_rng([H, W, B, int(two), self.esz, sum(map(ord, entry + mode))])
        self.case = Case(entry, suf, f"{H}x{W} B={B}{' two-material' if two else ''}{' ' + mode if mode else ''}")
        self.names = (args or ARGS)[entry].split()
        try:
            self.a = (multi if two else base)(entry if entry in ARGS else "mg_sweep", suf, H, W)
        except ValueError:   # base() also lays out two coarser levels, which a 3 x 3 or 5 x 5 grid does not have
            self.a = (multi if two else base)(entry if entry in ARGS else "mg_sweep", suf, 9, 9)
        self.a.update(B=B, H=H, W=W, w0=W0, w1=W1)
        self.ntab = MAXP if two else 1
        self.geos = [Geo(H, W, B, self.esz)]
        self.case.B, self.case.norm_n = B, (H - 2) * (W - 2)
        while self.geos[-1].H >= 5 and self.geos[-1].W >= 5 and self.geos[-1].H & 1 and self.geos[-1].W & 1:
            self.geos.append(self.geos[-1].coarse())

    def has(self, n):
        return n in self.names

    def set(self, **kw):
        self.a.update(kw)

    def rand(self, geo, zero_boundary=False):
        v = self.rng.standard_normal((geo.B, geo.H, geo.W)).astype(self.dt)
        if zero_boundary:
            v[:, 0] = v[:, -1] = 0
            v[:, :, 0] = v[:, :, -1] = 0
        return v

    def fin(self, arg, lev=0, name=None, krylov=False, geo=None, dt=None, finite=False):
        """a random input field; krylov: r / p / z of section 3, zero on the boundary nodes and the ghost ring;
        finite: an operand of the cycle join, whose frame must hold finite values"""
        g = geo or self.geos[lev]
        ref = self.case.add(field_in(name or arg, g, dt or self.dt, self.rand(g, krylov), g.ring() if krylov else None,
                                     finite))
        if name is None:
            self.a[arg] = ref
        return ref

    def fout(self, arg, lev=0, mask=None, name=None, geo=None, dt=None):
        g = geo or self.geos[lev]
        ref = self.case.add(field_out(name or arg, g, dt or self.dt, g.interior() if mask is None else mask))
        if name is None:
            self.a[arg] = ref
        return ref

    def pid(self, arg, lev=0, name=None):
        if not self.two:
            if name is None:
                self.a[arg] = None
            return None
        g = self.geos[lev].pid()
        ref = self.case.add(pid_in(name or arg, g, self.rng.integers(0, MAXP, (g.H, g.W)), MAXP, self.rng))
        if name is None:
            self.a[arg] = ref
        return ref

    def flat_in(self, arg, arr, sample=None):
        self.a[arg] = self.case.add(flat_in(arg, arr, sample))

    def flat_out(self, arg, n, dtype, mask=None, loose=False, sample=None, norm=None):
        self.a[arg] = self.case.add(flat_out(arg, n, dtype, mask, loose, sample, norm))

    def tables(self):
        """random coefficient tables with a positive diagonal, and omega / d"""
        rng, dt = self.rng, self.dt
        k = 0.2 * rng.standard_normal((self.ntab, 9))
        k[:, 4] = 2.0 + rng.random(self.ntab)
        for arg, arr in (("ktab", k), ("omd", 0.6 / k[:, 4]), ("rtab", 0.25 * (1 + 0.3 * rng.standard_normal((self.ntab, 9)))),
                         ("ptab", 0.25 * (1 + 0.3 * rng.standard_normal((self.ntab, 9)))),
                         ("hw", 0.1 * rng.standard_normal((self.a["nlayers"], 9)))):
            if self.has(arg):
                self.flat_in(arg, arr.astype(dt))

    def part(self):
        """the per-wave partial sums of a Krylov kernel: exactly B * fea_pcg_parts doubles"""
        from feanet_amd import _lib
        g = self.geos[0]
        per = int(_lib.lib().fea_pcg_parts(g.H, g.W, self.esz))
        n = g.B * per
        self.flat_out("part", n + 16, np.float64, np.arange(n + 16) < n, sample=rows(per), norm="parts")

    def scalars(self, done=0.0):
        s = np.zeros((self.geos[0].B, NSCAL))
        s[:, BETA], s[:, ALPHA], s[:, DONE] = 0.37, 0.61, done
        s[:, RNORM] = 3.0 * 2.0 ** (5 * np.arange(self.geos[0].B))
        self.flat_in("scalars", s, rows(NSCAL))

    def norm(self, kind):
        """norm operands of cycle_join / sweep_restrict: '' none, 'hist' appended in the call, 'defer' partials only"""
        from feanet_amd import _lib
        g = self.geos[0]
        if not kind:
            self.set(norm_ws=None, norm_hist=None, norm_cnt=None)
            self.call()
            return
        nws = _lib.norm_workspace_bytes(g.B, g.H, g.W) // 8
        per = _lib.join_norm_parts(g.B, g.H, g.W, self.esz)
        if kind == "defer":
            self.flat_out("norm_ws", nws + 16, np.float64, np.arange(nws + 16) < g.B * per, sample=rows(per),
                          norm="parts")
        else:
            self.flat_out("norm_ws", nws + 16, np.float64, np.arange(nws + 16) < nws, loose=True, norm="ws")
        row = np.arange(4 * g.B) // g.B == 1          # history row cnt[1] = 1
        hist = self.case.add(flat_out("norm_hist", 4 * g.B, np.float64, row,
                                      sample=lambda B, b: slice(B + b, B + b + 1), norm="norm"))
        self.case.nan_op = "u"
        cnt = self.case.add(flat_inout("norm_cnt", np.array([7, 1], np.uint32), np.array([False, True])))
        self.set(norm_hist=None if kind == "defer" else hist, norm_cnt=None if kind == "defer" else cnt)
        self.call()
        if kind == "defer":
            self.case.calls.append(("fea_norm_append", [self.a["norm_ws"], g.B * per, per, g.B, 1, hist, cnt]))

    def call(self):
        g = self.geos[0]
        self.a.update(ld=g.ld, bs=g.bs)
        if len(self.geos) > 1:
            self.a.update(ldc=self.geos[1].ld, bsc=self.geos[1].bs)
        if len(self.geos) > 2:
            self.a.update(ldc2=self.geos[2].ld, bsc2=self.geos[2].bs)
        sym = self.entry if self.entry.startswith("fea_") else f"fea_{self.entry}_{self.suf}"
        self.case.calls.append((sym, [self.a[n] for n in self.names]))
        return self.case


# ----------------------------------------------------------------------------- one builder per entry point
def _pack(b):
    g = b.geos[0]
    b.flat_in("src", b.rand(g), rows(g.H * g.W))
    b.flat_in("bc", b.rand(g), rows(g.H * g.W))
    b.set(geo=None, geo_bs=0, bc_bs=g.H * g.W)
    b.fout("dst", mask=g.nodes())


def _unpack(b):
    g = b.geos[0]
    nodes = b.rand(g)
    b.a["src"] = b.case.add(field_in("src", g, b.dt, nodes))
    b.flat_out("dst", g.B * g.H * g.W, b.dt, sample=rows(g.H * g.W))
    b.case.expect["dst"] = (np.ones(nodes.size, bool), nodes.ravel())


def _sweep(b):
    b.fin("u") if b.mode != "zero" else b.set(u=None)
    b.fin("f"), b.fout("out"), b.pid("pid")


def _residual_restrict(b):
    b.fin("f"), b.fout("fc", 1), b.pid("pid")
    b.set(u=None, v_out=None)
    if b.mode == "stored":
        b.fin("u")
    elif b.mode == "zero v":
        b.fout("v_out")


def _send(b, lev):
    g = b.geos[lev]
    r0, r1, c0, c1 = 0, g.H, g.W // 2, g.W       # a block that reaches three sides of the output level's boundary
    own = np.zeros((g.B, r1 - r0, c1 - c0), bool)
    own[:, 1 - r0:g.H - 1 - r0, :g.W - 1 - c0] = True
    b.set(r0=r0, r1=r1, c0=c0, c1=c1)
    b.flat_out("send", own.size + 8, b.dt, np.concatenate([own.ravel(), np.zeros(8, bool)]),
               sample=rows((r1 - r0) * (c1 - c0)))


def _zero_restrict_send(b):
    b.fin("f"), b.fout("fc", 1), b.pid("pid")
    _send(b, 1)


def _zero_restrict2(b):
    b.fin("f"), b.fout("fc", 1), b.fout("fc2", 2), b.pid("pid"), b.pid("pidc", 1)
    if b.has("send"):
        _send(b, 2)


def _sweep_restrict(b):
    b.fin("u"), b.fin("f"), b.fout("u_out"), b.fout("fc", 1), b.pid("pid")


def _prolong_sweep(b):
    b.fin("u") if b.mode != "zero" else b.set(u=None)
    b.fin("ec", 1), b.fin("f"), b.fout("out"), b.pid("pid"), b.pid("pidc", 1)


def _prolong2(b):
    b.fin("fc", 1), b.fin("ec2", 2), b.fin("f"), b.fout("out"), b.pid("pid"), b.pid("pidc", 1), b.pid("pidc2", 2)


def _prolong_add(b):
    b.fin("u"), b.fin("ec", 1), b.fout("out"), b.pid("pidc", 1)


def _residual_norm(b):
    from feanet_amd import _lib
    g = b.geos[0]
    b.fin("u"), b.fin("f"), b.pid("pid")
    nws = _lib.norm_workspace_bytes(g.B, g.H, g.W) // 8
    b.flat_out("ws", nws + 16, np.float64, np.arange(nws + 16) < nws, loose=True, norm="ws")
    b.flat_out("out", g.B + 4, np.float64, np.arange(g.B + 4) < g.B, sample=rows(1), norm="norm")
    b.case.nan_op = "u"
    if b.mode == "range":
        b.set(rlo=1, rhi=max(2, g.H // 2), clo=max(1, g.W // 3), chi=g.W - 1)
        b.case.norm_n = (b.a["rhi"] - 1) * (g.W - 1 - b.a["clo"])


def _cycle_join(b):
    b.fin("u", finite=True), b.fin("ec", 1, finite=True), b.fin("f", finite=True)
    b.fout("u_out"), b.fout("fc", 1), b.pid("pid"), b.pid("pidc", 1)


def join_rects(H, W):
    """rectangles (I0, I1, c0, c1) that leave rows and columns of the grid uncovered, and the fine / coarse node
    sets they own (include/feanet_hip.h: coarse row I with fine rows 2I-1, 2I, row H-2 with I1 = Hc-1; coarse
    column J with fine columns 2J-1, 2J)"""
    Hc = (H + 1) // 2
    cm = (W // 2) | 1
    rects = [(1, Hc - 1, 1, cm)]
    if Hc - 1 >= 3 and cm + 2 <= W - 2:
        Im = max(2, Hc // 2)
        rects = [(1, Im, 1, cm), (Im, Hc - 1, cm + 2, W - 1)]
    fine, coarse = np.zeros((H, W), bool), np.zeros((Hc, (W + 1) // 2), bool)
    for I0, I1, c0, c1 in rects:
        rows = sorted({r for I in range(I0, I1) for r in (2 * I - 1, 2 * I)} | ({H - 2} if I1 == Hc - 1 else set()))
        fine[np.ix_(rows, range(c0, c1))] = True
        coarse[I0:I1, (c0 + 1) // 2:(c1 - 1) // 2 + 1] = True
    return rects, fine, coarse


def _cycle_join_rects(b):
    g, gc = b.geos[0], b.geos[1]
    rects, fine, coarse = join_rects(g.H, g.W)
    b.fin("u", finite=True), b.fin("ec", 1, finite=True), b.fin("f", finite=True), b.pid("pid"), b.pid("pidc", 1)
    b.fout("u_out", mask=g.nodes() & g.framed(np.broadcast_to(fine, (g.B,) + fine.shape), False, bool))
    b.fout("fc", 1, mask=gc.nodes() & gc.framed(np.broadcast_to(coarse, (gc.B,) + coarse.shape), False, bool))
    arr = np.array(rects, np.int32).reshape(-1)
    b.set(nrect=len(rects), rects=Host(lambda addr: arr))


def _hsweep(b):
    b.set(nlayers=1 if b.mode == "one layer" else 3, u_raw=None)
    b.fin("u") if b.mode != "zero" else b.set(u=None)
    if b.mode == "raw":
        b.fin("u_raw")
    b.fin("f"), b.fout("out"), b.pid("pid")
    if b.has("fc"):
        b.fout("fc", 1)
    if b.has("ec"):
        b.fin("ec", 1), b.pid("pidc", 1)


def _tail(b):
    g = b.geos[0]
    nlev = int(b.mode.split()[1])
    b.set(H=g.H, W=g.W, nlev=nlev, nlayers=2)
    b.fin(b.names[0]), b.fout(b.names[1])
    if b.has("pid_levels"):
        b.set(pid_levels=None)
        if b.two:
            n = sum(((g.H - 1 >> k) + 1) * ((g.W - 1 >> k) + 1) for k in range(nlev))
            b.flat_in("pid_levels", b.rng.integers(0, MAXP, n).astype(np.uint8))


def _mid(b):
    _, k, _, TR, TC = b.mode.split()
    k, TR, TC = int(k), int(TR), int(TC)
    b.set(k=k, TR=TR, TC=TC)
    up = b.entry == "mg_mid_up"
    gathered = b.has("gsrc")
    fs = []
    for j in range(k + 1):
        if up:
            fs.append(b.fin("fs", j, name=f"f{j}").name if j < k else None)
        elif j == 0 and not gathered:
            fs.append(b.fin("fs", 0, name="f0").name)
        else:
            fs.append(b.fout("fs", j, name=f"f{j}").name)
    b.set(fs=Refs(fs), pids=Refs([b.pid("pids", j, name=f"p{j}").name for j in range(k + 1)]) if b.two else None)
    if up:
        b.fin("e", k), b.fout("out")
    if gathered:
        g = b.geos[0]
        Pr = Pc = 2
        b.set(Pr=Pr, Pc=Pc, gcr=(g.H - 1) // Pr, gcc=(g.W - 1) // Pc)
        blk = b.a["gcr"] * b.a["gcc"]             # [Pr * Pc][B][gcr][gcc]
        b.flat_in("gsrc", b.rng.standard_normal(Pr * Pc * g.B * blk).astype(b.dt),
                  lambda B, i: ((np.arange(Pr * Pc)[:, None] * B + i) * blk + np.arange(blk)[None, :]).ravel())


def _hmid(b):
    b.set(TT=int(b.mode.split()[1]), nlayers=2)
    up = b.entry == "mg_hmid_up"
    if up:
        fs = [b.fin("fs", j, name=f"f{j}").name for j in range(2)]
        us = [b.fin("us", j, name=f"u{j}").name for j in range(2)]
        b.fin("e", 2), b.fout("out")
    else:
        fs = [b.fin("fs", 0, name="f0").name] + [b.fout("fs", j, name=f"f{j}").name for j in (1, 2)]
        us = [b.fout("us", j, name=f"u{j}").name for j in range(2)]
    b.set(fs=Refs(fs), us=Refs(us),
          pids=Refs([b.pid("pids", j, name=f"p{j}").name for j in range(3)]) if b.two else None)


def _pcg_residual(b):
    g = b.geos[0]
    b.fin("x"), b.fin("f"), b.fout("r", mask=g.nodes()), b.pid("pid"), b.part()
    b.case.nan_op = "x"
    b.case.expect["r"] = (g.boundary(), np.zeros(g.numel, b.dt))      # zeros on the boundary nodes


def _pcg_direction(b):
    g32 = Geo(b.geos[0].H, b.geos[0].W, b.geos[0].B, 4)
    if b.has("z32"):
        b.fin("z32", krylov=True, geo=g32, dt=np.float32)
    else:
        b.fin("z", krylov=True)
    b.fin("p_in", krylov=True), b.fout("p_out"), b.pid("pid"), b.scalars(), b.part()
    b.case.nan_op = "z32" if b.has("z32") else "z"


def _pcg_update(b):
    g = b.geos[0]
    frozen = b.mode == "frozen"
    none = np.zeros(g.numel, bool)
    b.fin("p", krylov=True), b.pid("pid"), b.scalars(done=1.0 if frozen else 0.0), b.part()
    b.a["x"] = b.case.add(field_inout("x", g, b.dt, b.rand(g), none if frozen else g.interior()))
    b.a["r"] = b.case.add(field_inout("r", g, b.dt, b.rand(g, True), none if frozen else g.interior(), g.ring()))
    if b.has("r32"):
        g32 = Geo(g.H, g.W, g.B, 4)
        b.fout("r32", geo=g32, dt=np.float32, mask=np.zeros(g32.numel, bool) if frozen else None)
        b.flat_in("sb", np.full(g.B, 0.5), rows(1))
    b.case.nan_op = "r"           # (a frozen sample sums its r again, whatever p holds)


def _pcg_dot(b):
    g = b.geos[0]
    b.fin("r", krylov=True), b.part()
    b.case.nan_op = "r"
    if b.has("z32"):
        b.fin("z32", krylov=True, geo=Geo(g.H, g.W, g.B, 4), dt=np.float32)
    else:
        b.fin("z", krylov=True)


def _pcg_narrow(b):
    g = b.geos[0]
    b.fin("r", krylov=True), b.scalars()
    b.fout("r32", geo=Geo(g.H, g.W, g.B, 4), dt=np.float32)
    b.flat_out("sb", g.B + 4, np.float64, np.arange(g.B + 4) < g.B, sample=rows(1))


# ----------------------------------------------------------------------------- halo pack / rectangle copies
def dd_layout(kind, n):
    """n non-overlapping records in a 300-row buffer of pitch 320: record 0 is larger than 256 * 256 elements (the
    copy kernels' grid-stride loop runs), record 1 has no rows, the rest are small blocks of mixed sizes.
    -> [(row, col, rows, cols)]"""
    rec = [(5, 7, 260, 258), (2, 270, 0, 3)]
    for i in range(2, n):
        rec.append((6 * (i - 2), 272 + 9 * (i % 5), 1 + i % 4, 1 + i % 7))
    assert max(r + h for r, _, h, _ in rec) <= 300 and max(c + w for _, c, _, w in rec) <= 320
    return rec


def dd_case(entry, suf, mode):
    """fea_dd_copy_blocks (mode 'to stage' / 'from stage', 49 blocks) or fea_dd_copy_rects (33 rectangles): sources
    and destinations are regions of larger buffers; the destination is a canary everywhere else."""
    dt = npdt(suf)
    esz = np.dtype(dt).itemsize
    rng = np.random.default_rng(len(mode) + esz)
    case = Case(entry, suf, mode)
    ROWS, LD = 300, 320
    blocks = entry == "fea_dd_copy_blocks"
    rec = dd_layout(entry, 49 if blocks else 33)
    # the second buffer: blocks -> a dense staging buffer with gaps of 3 elements; rects -> a buffer of pitch 264
    if blocks:
        pos, o = [], 2
        for _, _, h, w in rec:
            pos.append(o)
            o += h * w + 3
        n2, ld2 = o, None
    else:
        ld2, pos, o = 264, [], 1
        for _, _, h, w in rec:
            pos.append(o)
            o += h * ld2 + 5
        n2 = o + ld2
    idx1 = [((r + np.arange(h))[:, None] * LD + c + np.arange(w)[None, :]).ravel() for r, c, h, w in rec]
    idx2 = [(np.arange(h)[:, None] * (w if blocks else ld2) + p + np.arange(w)[None, :]).ravel()
            for p, (_, _, h, w) in zip(pos, rec)]
    to2 = mode != "from stage"                       # copy buffer 1 -> buffer 2
    src_n, dst_n, si, di = (ROWS * LD, n2, idx1, idx2) if to2 else (n2, ROWS * LD, idx2, idx1)
    data = rng.standard_normal(src_n).astype(dt)
    mask, want = np.zeros(dst_n, bool), np.zeros(dst_n, dt)
    for s, d in zip(si, di):
        mask[d] = True
        want[d] = data[s]
    case.add(flat_in("src", data))
    case.add(flat_out("dst", dst_n, dt, mask))
    case.expect["dst"] = (mask, want)
    one, two = ("src", "dst") if to2 else ("dst", "src")

    def table(addr):
        t = []
        for (r, c, h, w), p in zip(rec, pos):
            a1, a2 = addr[one] + (r * LD + c) * esz, addr[two] + p * esz
            if blocks:
                t.append(np.array([a1, a2, LD], np.int64).tobytes() + np.array([h, w], np.int32).tobytes())
            else:
                d, s, dl, sl = (a2, a1, ld2, LD) if to2 else (a1, a2, LD, ld2)
                t.append(np.array([d, s, dl, sl, h, w], np.int64).tobytes())
        return np.frombuffer(b"".join(t), np.uint8)
    if blocks:
        case.calls.append((entry, [Host(table), len(rec), esz, int(to2)]))
    else:
        case.calls.append((entry, [Host(table), len(rec), esz]))
    return case


# ----------------------------------------------------------------------------- the descriptor table
SINGLE = [(3, 3, 1), (33, 321, 2), (35, 323, 3), (321, 9, 1)]     # one level
ONE = [(5, 5, 1), (33, 321, 2), (35, 323, 3), (321, 9, 1)]        # one transfer: the coarse level needs 3 nodes
TWO = [(9, 9, 1), (33, 321, 2), (37, 325, 2), (321, 9, 1)]        # two transfers: 9 x 9 is the smallest grid
# mid / hmid: (H, W, B) with the mode naming k and the tile; >= 2 tiles each way, the last one ragged
MID_DOWN = [((13, 13, 2), "k 1 T 4 4"), ((25, 25, 1), "k 2 T 4 4"), ((13, 25, 2), "k 1 T 4 4")]
MID_UP = [((13, 13, 2), "k 1 T 8 8"), ((25, 25, 1), "k 2 T 16 16"), ((13, 25, 2), "k 1 T 8 8")]


class Desc:
    """build: the entry point's builder; shapes: [(H, W, B)] or [((H, W, B), mode)]; modes: the call's variants;
    two: also run the 16-pattern form; sufs: the dtypes; args: the argument-name table"""

    def __init__(self, build, shapes, modes=("",), two=True, sufs=("f32", "f64"), args=ARGS, norm=False):
        self.build, self.shapes, self.modes, self.two, self.sufs, self.args, self.norm = (build, shapes, modes, two,
                                                                                        sufs, args, norm)

    def params(self):
        for s in self.shapes:
            shape, modes = (s[0], (s[1],)) if isinstance(s[0], tuple) else (s, self.modes)
            for two in ((False, True) if self.two else (False,)):
                for mode in modes:
                    yield shape, two, mode


DESC = {
    "mg_pack": Desc(_pack, SINGLE, two=False),
    "mg_unpack": Desc(_unpack, SINGLE, two=False),
    "mg_sweep": Desc(_sweep, SINGLE, ("", "zero")),
    "mg_residual_restrict": Desc(_residual_restrict, ONE, ("stored", "zero", "zero v")),
    "mg_zero_restrict_send": Desc(_zero_restrict_send, ONE),
    "mg_zero_restrict2": Desc(_zero_restrict2, TWO),
    "mg_zero_restrict2_send": Desc(_zero_restrict2, TWO),
    "mg_sweep_restrict": Desc(_sweep_restrict, ONE, ("", "hist"), norm=True),
    "mg_prolong_sweep": Desc(_prolong_sweep, ONE, ("", "zero")),
    "mg_prolong2": Desc(_prolong2, TWO),
    "mg_prolong_add": Desc(_prolong_add, ONE),
    "mg_residual_norm": Desc(_residual_norm, SINGLE, ("", "range")),
    "mg_cycle_join": Desc(_cycle_join, ONE, ("", "hist", "defer"), norm=True),
    "mg_cycle_join_rects": Desc(_cycle_join_rects, ONE),
    "mg_hsweep": Desc(_hsweep, SINGLE, ("", "zero", "raw", "one layer")),
    "mg_hsweep_restrict": Desc(_hsweep, ONE, ("", "zero", "raw")),
    "mg_prolong_hsweep": Desc(_hsweep, ONE, ("", "raw")),
    # (49 x 25, four levels down to 7 x 4, and 97 x 49 above it: three rows per wave, an even coarsest level)
    "mg_coarse_tail": Desc(_tail, [((5, 5, 2), "nlev 2"), ((17, 65, 2), "nlev 3"), ((17, 65, 2), "nlev 4"),
                                   ((49, 25, 2), "nlev 4")]),
    "mg_coarse_tail_ext": Desc(_tail, [((9, 17, 2), "nlev 2"), ((33, 129, 2), "nlev 3"), ((97, 49, 2), "nlev 4")],
                               two=False),
    "mg_hjac_tail": Desc(_tail, [((5, 5, 2), "nlev 2"), ((17, 65, 2), "nlev 3"), ((17, 65, 2), "nlev 4"),
                                 ((49, 25, 2), "nlev 4")]),
    "mg_mid_down": Desc(_mid, MID_DOWN),
    "mg_mid_down_gathered": Desc(_mid, MID_DOWN),
    "mg_mid_up": Desc(_mid, MID_UP),
    "mg_hmid_down": Desc(_hmid, [((25, 25, 2), "T 4"), ((25, 49, 1), "T 4")]),
    "mg_hmid_up": Desc(_hmid, [((25, 25, 2), "T 16"), ((25, 49, 1), "T 16")]),
    "pcg_residual": Desc(_pcg_residual, SINGLE, args=PCG_ARGS),
    "pcg_direction": Desc(_pcg_direction, SINGLE, args=PCG_ARGS),
    "pcg_update": Desc(_pcg_update, SINGLE, ("", "frozen"), args=PCG_ARGS),
    "pcg_dot": Desc(_pcg_dot, SINGLE, two=False, args=PCG_ARGS),
    "fea_pcg_narrow_f64f32": Desc(_pcg_narrow, SINGLE, two=False, sufs=("f64",), args=MIXED_ARGS),
    "fea_pcg_dot_f64f32": Desc(_pcg_dot, SINGLE, two=False, sufs=("f64",), args=MIXED_ARGS),
    "fea_pcg_direction_f64f32": Desc(_pcg_direction, SINGLE, sufs=("f64",), args=MIXED_ARGS),
    "fea_pcg_update_f64f32": Desc(_pcg_update, SINGLE, ("", "frozen"), sufs=("f64",), args=MIXED_ARGS),
    "fea_dd_copy_blocks": Desc(None, [((0, 0, 0), "to stage"), ((0, 0, 0), "from stage")], two=False),
    "fea_dd_copy_rects": Desc(None, [((0, 0, 0), "rects")], two=False),
}


def build_case(entry, suf, shape, two, mode):
    d = DESC[entry]
    if entry in DD_NAMES:
        return dd_case(entry, suf, mode)
    H, W, B = shape
    b = Builder(entry, suf, H, W, B, two, mode, d.args)
    if "ld32" in b.names:
        g32 = Geo(H, W, B, 4)
        b.set(ld32=g32.ld, bs32=g32.bs)
    d.build(b)
    b.tables()
    if d.norm:
        b.norm(mode)
    else:
        b.call()
    return b.case


def cases(entry, suf):
    return [build_case(entry, suf, shape, two, mode) for shape, two, mode in DESC[entry].params()]


# ----------------------------------------------------------------------------- task-height ladders
# A framed or Krylov launch splits a level into wave tasks of rb rows; the host picks rb from the batch size and the
# shape (pick_rb, balanced_rb, join_config of csrc/), and the results are documented to be the same bits whatever it
# picks.  A ladder runs one call at batch sizes that reach every height: the case is built once for the top rung, every
# lower rung is a prefix of its samples (and one rung holds the last sample alone), and sample b's outputs must be the
# same bytes in every rung that contains it.  Three more error kinds:
#   'h'  a sample's output differs between two rungs (the result depends on the task height or on the batch);
#   's'  an output of another sample changed when every node of sample j became NaN (a leak between samples);
#   'n'  a norm of a sample with a NaN node is finite (a diverged sample would pass as converged).
# Everything below works on numpy arrays (the host tests' stand-in kernels) and on torch tensors that stay on the GPU.
K_TARGET_WAVES, K_RB = 2048, 32       # kTargetWaves, kRB of csrc/framed_strip.h
LADDER_H, LADDER_W, LADDER_W2 = 4097, 33, 163
BATCH_RUNGS = (1, 2, 4, 8, 16)        # at H = 4097, one strip: rb = 2, 4, 8, 16, 32
CAP64 = ("mg_sweep_restrict", "mg_cycle_join")      # their cap is 64 rows: one more rung, B = 32
SMALL_RUNGS = (1, 2, 3)               # entry points whose geometry ignores B, at their DESC shapes
BATCH_FREE = ("mg_pack", "mg_unpack", "mg_coarse_tail", "mg_coarse_tail_ext", "mg_hjac_tail", "mg_mid_down",
              "mg_mid_down_gathered", "mg_mid_up", "mg_hmid_down", "mg_hmid_up")
U_DOUBLE = 2.0 ** -53                 # every norm and partial sum accumulates in double (wave_sum, k_norm_final)


def pick_rb(B, nstrips, rows, maxrb=K_RB):
    """restatement of pick_rb (csrc/framed_strip.h): the coverage guard's, not an oracle for values"""
    rb = maxrb
    while rb > 2 and B * nstrips * -(-rows // rb) < K_TARGET_WAVES:
        rb //= 2
    return rb


def nstrips(W, esz):
    return -(-(W - 2) // (64 * (16 // esz)))


def ladder_w2(entry):
    """the two-strip width: 163, or 161 where two coarser levels need (W + 1) / 2 odd as well"""
    return 161 if entry in ("mg_zero_restrict2", "mg_zero_restrict2_send", "mg_prolong2") else LADDER_W2


def rungs_of(entry):
    if entry in BATCH_FREE:
        return SMALL_RUNGS
    return BATCH_RUNGS + (32,) if entry in CAP64 else BATCH_RUNGS


def ladder_heights(entry, esz, W=LADDER_W, rungs=None):
    """the nominal (power-of-two) task height of every rung; raises when the ladder no longer reaches five distinct
    heights (six for the cap-64 kernels)"""
    cap = 2 * K_RB if entry in CAP64 else K_RB
    if entry.startswith(("pcg_", "fea_pcg_")):      # pcg_geom: the height of ONE sample, whatever the batch
        return [pick_rb(1, nstrips(W, esz), LADDER_H - 2)] * len(rungs or rungs_of(entry))
    hs = [pick_rb(B, nstrips(W, esz), LADDER_H - 2, cap) for B in (rungs or rungs_of(entry))]
    if rungs is None and len(set(hs)) != (6 if entry in CAP64 else 5):
        raise AssertionError(f"{entry}: the batch ladder reaches heights {hs}: kTargetWaves or kRB changed, re-pick "
                             "the ladder")
    return hs


def _is_np(a):
    return isinstance(a, np.ndarray)


def _bits(a):
    """the same bytes as integers: == on them is a bitwise comparison (NaNs and signed zeros included)"""
    if _is_np(a):
        return a.view(f"u{a.dtype.itemsize}")
    import torch
    return a.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()])


def _ix(a, idx):
    if isinstance(idx, slice) or _is_np(a):
        return idx
    import torch
    return torch.as_tensor(np.asarray(idx), device=a.device)


def _first(bad):
    return int(np.flatnonzero(bad)[0]) if _is_np(bad) else int(bad.nonzero()[0, 0])


def _f64(a):
    if _is_np(a):
        return a.view(np.float64)
    import torch
    return a.view(torch.float64)


def _mask(op, like):
    """the operand's write set next to `like` (uploaded once per operand)"""
    if _is_np(like):
        return op.mask
    if getattr(op, "_dmask", None) is None:
        import torch
        op._dmask = torch.from_numpy(op.mask).to(like.device)
    return op._dmask


def _start(idx):
    return idx.start if isinstance(idx, slice) else int(idx[0])


class HostBackend:
    """numpy buffers and a stand-in launch(case, bufs) -> bufs, as run_case() takes"""

    def __init__(self, launch):
        self.launch = launch

    def initial(self, case):
        return {op.name: op.z.copy() for op in case.ops}

    def clone(self, bufs):
        return {n: a.copy() for n, a in bufs.items()}


class DeviceBackend:
    """torch buffers that stay on the GPU: framed fields are laid out there from their compact node values, canaries
    are filled there, and every comparison runs there"""

    def initial(self, case):
        import torch
        TD = {"float32": torch.float32, "float64": torch.float64, "uint8": torch.uint8, "uint32": torch.int32}
        bufs = {}
        for op in case.ops:
            tdt = TD[op.dtype.name]
            if op._z is None and op.nodes is not None:
                g = op.geo
                t = torch.zeros(op.numel, dtype=tdt, device="cuda")
                torch.as_strided(t, (g.B, g.H, g.W), (g.bs, g.ld, 1), g.ld + g.off).copy_(
                    torch.from_numpy(np.ascontiguousarray(op.nodes)))
            elif op._z is None and op.fill is not None:
                t = torch.full((op.numel * op.dtype.itemsize,), op.fill, dtype=torch.uint8, device="cuda").view(tdt)
            else:
                t = torch.from_numpy(op.z.view(np.uint8)).cuda().view(tdt)
            bufs[op.name] = t
        return bufs

    def clone(self, bufs):
        return {n: t.clone() for n, t in bufs.items()}

    def launch(self, case, bufs):
        import torch
        keep = _issue(case, {n: t.data_ptr() for n, t in bufs.items()})
        torch.cuda.synchronize()
        del keep
        return bufs


def sample_nodes(geo, b):
    """flat indices of sample b's nodes"""
    return (b * geo.bs + (np.arange(geo.H, dtype=np.int64)[:, None] + 1) * geo.ld + geo.off +
            np.arange(geo.W, dtype=np.int64)[None, :]).ravel()


def per_sample_inputs(case):
    return [op for op in case.ops if op.role != "out" and op.sample is not None]


def derive(top, top_bufs, case, bufs, src):
    """The inputs of `case` (len(src) samples) become samples `src` of the top rung's: per-sample operands block by
    block (a framed sample with its ghost rows and padding), shared ones (tables, pattern maps, counters) whole."""
    assert case.B == len(src) and [o.name for o in case.ops] == [o.name for o in top.ops], (case, top)
    for op, t in zip(case.ops, top.ops):
        if op.role == "out":
            continue
        a, ta = bufs[op.name], top_bufs[op.name]
        if op.sample is None:
            assert op.numel == t.numel, (case, op.name)
            a[:] = ta
            continue
        for i, b in enumerate(src):
            a[_ix(a, op.sample(case.B, i))] = ta[_ix(ta, t.sample(top.B, b))]


def check_ab(case, before, after):
    """assertions (a), (b) and (d) of check() on one run: nothing outside the write set, inputs untouched, every
    element of an output's write set stored (it no longer holds the canary)"""
    for op in case.ops:
        moved = _bits(after[op.name]) != _bits(before[op.name])
        if op.role == "out" and not op.loose and bool((_mask(op, moved) & ~moved).any()):   # (d), on the canary
            raise FootprintError("d", op.name, f"{case}: write-set element never stored at "
                                 f"{op.where(_first(_mask(op, moved) & ~moved))}")
        if op.role != "in":
            moved = moved & ~_mask(op, moved)
        if bool(moved.any()):
            i = _first(moved)
            raise FootprintError("b" if op.role == "in" else "a", op.name,
                                 f"{case}: " + ("input modified" if op.role == "in" else "written outside the write "
                                                                                          "set") + f" at {op.where(i)}")


def partial_count(case, before, after):
    """partial sums per sample behind the call's norms: the slots of its workspace that were stored to"""
    for op in case.ops:
        if op.norm in ("ws", "parts"):
            return int((_bits(after[op.name]) != _bits(before[op.name])).sum()) // case.B
    return None


def sample_outputs(case, after, b, norms):
    """[(operand, first raw index, values, write-set mask)] of sample b: fields and flat blocks (norms False), or the
    per-sample norms and partial sets (norms True)"""
    out = []
    for op in case.ops:
        if op.role == "in" or op.sample is None or (op.norm is not None) != norms:
            continue
        idx = op.sample(case.B, b)
        a = after[op.name]
        out.append((op, _start(idx), a[_ix(a, idx)], _mask(op, a)[_ix(a, idx)]))
    return out


def compare_samples(kind, what, ca, after_a, ba, cb, after_b, bb, norms=False):
    """sample ba of case ca against sample bb of case cb: the same bytes on the write set"""
    for (op, i0, va, ma), (_, _, vb, _) in zip(sample_outputs(ca, after_a, ba, norms),
                                               sample_outputs(cb, after_b, bb, norms)):
        if norms and va.shape != vb.shape:
            if ca.entry.startswith(("pcg_", "fea_pcg_")):
                raise FootprintError(kind, op.name, f"{what}: {va.shape[0]} against {vb.shape[0]} Krylov partials")
            continue            # partial sets of different sizes: their sums are compared (compare_norms)
        bad = (_bits(va) != _bits(vb)) & ma
        if bool(bad.any()):
            i = _first(bad)
            raise FootprintError(kind, op.name, f"{what}: {int(bad.sum())} elements differ, first at "
                                 f"{op.where(i0 + i)} ({va[i].item()!r} against {vb[i].item()!r})")


def norm_values(case, after, b):
    """{operand name: sample b's norm}; a partial set counts as the sum of its partials"""
    return {op.name: float(_f64(v).sum().item()) if op.norm == "parts" else float(_f64(v)[0].item())
            for op, _, v, _ in sample_outputs(case, after, b, True)}


def compare_norms(case, seen):
    """seen: [(rung label, partial count, {operand: value})] of ONE sample.  Sums of the same non-negative squares in
    another order: equal partial counts -> the same bits; otherwise within 2 n u (relative) of each other, n the
    nodes summed and u = 2^-53, the roundoff of the double every kernel accumulates its norm in."""
    tol = 2.0 * case.norm_n * U_DOUBLE
    for i, (la, na, va) in enumerate(seen):
        for lb, nb, vb in seen[i + 1:]:
            for name in va:
                x, y = va[name], vb[name]
                if not (np.isfinite(x) and np.isfinite(y)):
                    raise FootprintError("h", name, f"{case}: non-finite norm {x!r} ({la}) / {y!r} ({lb})")
                if na == nb and x != y:
                    raise FootprintError("h", name, f"{case}: {la} and {lb} have {na} partials per sample but the "
                                         f"norm differs: {x!r} against {y!r}")
                if abs(x - y) > tol * max(abs(x), abs(y)):
                    raise FootprintError("h", name, f"{case}: norm {x!r} ({la}, {na} partials) against {y!r} ({lb}, "
                                         f"{nb} partials): relative difference above 2 n u = {tol:.3e}")


def picks(B):
    """first, middle and last sample"""
    return sorted({0, B // 2, B - 1})


def isolation(case, be, before=None, after=None):
    """Run S for j first, middle, last: every node of sample j is a quiet NaN in every per-sample input (its scalars
    row included; non-node storage as in run Z) and every other sample's outputs keep run Z's bytes.  Then, where the
    call produces norms: one NaN at an interior node of the field the norm is of makes sample j's norms non-finite."""
    if before is None:
        before = be.initial(case)
        after = be.launch(case, be.clone(before))
    for j in picks(case.B):
        bufs = be.clone(before)
        for op in per_sample_inputs(case):
            a = bufs[op.name]
            idx = sample_nodes(op.geo, j) if op.geo is not None else op.sample(case.B, j)
            a[_ix(a, idx)] = float("nan")
        got = be.launch(case, bufs)
        for b in range(case.B):
            if b != j:
                for norms in (False, True):
                    compare_samples("s", f"{case}: sample {b} with sample {j} all NaN", case, got, b, case, after, b,
                                    norms)
        if case.nan_op is None:
            continue
        bufs = be.clone(before)
        op = next(o for o in case.ops if o.name == case.nan_op)
        g = op.geo
        bufs[op.name][j * g.bs + (1 + (g.H // 2 - 1) // 2 + 1) * g.ld + g.off + g.W - 2] = float("nan")
        got = be.launch(case, bufs)
        vals = norm_values(case, got, j)
        assert vals, case
        for name, v in vals.items():
            if np.isfinite(v):
                raise FootprintError("n", name, f"{case}: sample {j} has a NaN node in {op.name} but its norm is {v!r}")


def run_ladder(build, rungs, be, isolate_at=4):
    """build(B) -> the case for B samples.  Runs the top rung, every lower rung as its prefix and the last sample
    alone; asserts (a), (b) on every run, 'h' between rungs, and the isolation checks on the rung of isolate_at
    samples.  -> [(label, partial count)] for the report."""
    top = build(rungs[-1])
    before = be.initial(top)
    after = be.launch(top, be.clone(before))
    check_ab(top, before, after)
    ntop = partial_count(top, before, after)
    seen = {b: [(f"B={top.B}", ntop, norm_values(top, after, b))] for b in range(top.B)}
    report = [(f"B={top.B}", ntop)]
    if top.B == isolate_at:
        isolation(top, be, before, after)
    for src in [tuple(range(k)) for k in rungs[:-1]] + [(top.B - 1,)]:
        label = f"B={len(src)}" + (" (last sample alone)" if src[0] else "")
        case = build(len(src))
        b0 = be.initial(case)
        derive(top, before, case, b0, src)
        a0 = be.launch(case, be.clone(b0))
        check_ab(case, b0, a0)
        n = partial_count(case, b0, a0)
        report.append((label, n))
        for i, b in enumerate(src):
            what = f"{case}: sample {b} in {label} against B={top.B}"
            compare_samples("h", what, case, a0, i, top, after, b)
            if n == ntop or case.entry.startswith(("pcg_", "fea_pcg_")):
                compare_samples("h", what, case, a0, i, top, after, b, norms=True)
            seen[b].append((label, n, norm_values(case, a0, i)))
        if len(src) == isolate_at and not src[0]:
            isolation(case, be, b0, a0)
    for b, s in seen.items():
        if s[0][2]:
            compare_norms(top, s)
    return report
