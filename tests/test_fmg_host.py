"""Full-multigrid start, CPU side: the reference interpolation and the accuracy the algorithm promises (from the CPU
oracle alone), the shifted sub-hierarchy schedule, MultigridSolver.fmg's refusals and defaults, the binding table
against include/feanet_fmg.h, and the argument checks of the three entry points (fake addresses: a rejected call
launches nothing, and there is no GPU here)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import fmg_ref as fr
from conftest import ROOT
from oracle import feanet_oracle as fo


# ----------------------------------------------------------------------------- reference interpolation
@pytest.mark.parametrize("nc", [4, 5, 9])
def test_reference_interpolation_reproduces_bicubics(nc):
    """Every bicubic x^p y^q, p, q <= 3, on nc x nc coarse nodes comes out exact to rounding on all (2 nc - 1)^2
    fine nodes, the rows and columns next to the boundary included (the one-sided formula is cubic-exact too)."""
    xc = np.linspace(-1.0, 1.0, nc)
    xf = np.linspace(-1.0, 1.0, 2 * nc - 1)
    for p in range(4):
        for q in range(4):
            e = np.outer(xc ** p, 0.5 + xc ** q)
            want = np.outer(xf ** p, 0.5 + xf ** q)
            got = fr.interp(e, 3)
            S = fr.interp(e, 3, absolute=True)
            assert np.all(np.abs(got - want) <= 2 * sum(fr.NM) * 2.0 ** -53 * S), (p, q)
    # a quartic is not reproduced: the check above can fail
    assert np.abs(fr.interp_axis(xc ** 4, 3) - xf ** 4).max() > 1e-4


@pytest.mark.parametrize("m", [2, 3, 5, 8])
def test_order_one_is_bilinear_upsample(m):
    """Equal up to the rounding of the centre nodes (bilinear_upsample averages across the rows first, the
    interpolation here along the columns first): within the field bound of two 4-term sums, exactly elsewhere."""
    e = np.random.default_rng(m).standard_normal((2, m, m))
    got, want = fr.interp(e, 1), fo.bilinear_upsample(e)
    assert np.all(np.abs(got - want) <= 2 * (4 + 2) * 2.0 ** -53 * fr.interp(e, 1, absolute=True))
    assert np.array_equal(got[:, ::2, :], want[:, ::2, :]) and np.array_equal(got[:, :, ::2], want[:, :, ::2])
    if m < 4:  # fewer than 4 coarse nodes: cubic falls back to 1/2, 1/2
        assert np.array_equal(fr.interp(e, 3), fr.interp(e, 1))


def test_reference_prolong_keeps_the_boundary():
    rng = np.random.default_rng(0)
    u, e = rng.standard_normal((9, 13)), rng.standard_normal((5, 7))
    out = fr.prolong(u, e, 3)
    ring = np.ones((9, 13), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(out[ring], u[ring])
    assert np.array_equal(out[1:-1, 1:-1], (u + fr.interp(e, 3))[1:-1, 1:-1])
    assert np.array_equal(fr.prolong(None, e, 3)[ring], np.zeros(ring.sum()))


# ----------------------------------------------------------------------------- accuracy of the algorithm
_CONVERGED = {}


def converged(n, rows=None, levels=None):
    """(u_exact, f, u_h, ||u_h - u_exact||) of the model problem: u_h by 60 oracle V-cycles (residual ~1e-13)."""
    key = (n, rows, levels)
    if key not in _CONVERGED:
        ue, f = fr.model_problem(n, rows)
        mg = fo.OracleMultigrid(n, "poisson", np.float64, levels=levels, rows=rows)
        geo, _ = fo.square_geometry(ue.shape, np.float64)
        bc = ue * (1 - geo)
        mg.set_boundary(geo, bc)
        v = bc[None].copy()
        for _ in range(60):
            v = mg.step(v, f[None])
        assert mg.residual_norm(v, f[None]).max() < 1e-12
        _CONVERGED[key] = (ue, f, v[0], float(np.linalg.norm(v[0] - ue)))
    return _CONVERGED[key]


@pytest.mark.parametrize("n", [64, 128])
def test_one_pass_reaches_discretisation_accuracy(n):
    """DESIGN §14's table from the reference alone.  Measured here, n = 64 / 128: cubic 0.644 / 0.591, bilinear
    2.145 / 2.153 times the discretisation error against the exact solution; two cycles per level leave an
    algebraic error of 0.0740 / 0.0745 of it."""
    ue, f, uh, disc = converged(n)
    cubic = fr.fmg(n, f[None], ue[None], cycles=1, order=3)[0]
    bilin = fr.fmg(n, f[None], ue[None], cycles=1, order=1)[0]
    two = fr.fmg(n, f[None], ue[None], cycles=2, order=3)[0]
    r_cubic, r_bilin = np.linalg.norm(cubic - ue) / disc, np.linalg.norm(bilin - ue) / disc
    r_two = np.linalg.norm(two - uh) / disc
    print(f"n={n}: cubic {r_cubic:.4f}  bilinear {r_bilin:.4f}  two cycles (algebraic) {r_two:.4f}")
    assert r_cubic < 1.0
    assert r_bilin > 2.0
    assert r_two < 0.1


def test_coarsest_level_has_to_be_solved():
    """97 x 193 nodes, 6 levels, coarsest 4 x 7 nodes: 8 base cycles leave the algebraic error at 1.12 times the
    discretisation error (measured here), one base cycle (2 sweeps) at 38.6 times."""
    n, rows, L = 192, 96, 6
    ue, f, uh, disc = converged(n, rows, L)
    r8 = np.linalg.norm(fr.fmg(n, f[None], ue[None], levels=L, rows=rows, base_cycles=8)[0] - uh) / disc
    r1 = np.linalg.norm(fr.fmg(n, f[None], ue[None], levels=L, rows=rows, base_cycles=1)[0] - uh) / disc
    print(f"97 x 193: base_cycles=8 {r8:.3f}  base_cycles=1 {r1:.1f}")
    assert r8 < 1.2
    assert r1 > 10.0
    assert fr.default_base_cycles(4, 7) == 8 and fr.default_base_cycles(3, 3) == 1


# ----------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("L, nu1, nu2, fuse", [(6, 1, 1, True), (5, 2, 1, True), (4, 1, 2, False), (3, 0, 1, True)])
def test_shifted_schedule_is_the_sub_hierarchys(L, nu1, nu2, fuse):
    from feanet_amd.schedule import shift_schedule, vcycle_schedule
    for s in range(L):
        for start in ("a", "b"):
            for t in [None] + list(range(1, L - s)):
                steps, end = vcycle_schedule(L - s, nu1, nu2, None, start, t, fuse)
                shifted = shift_schedule(steps, s)
                assert len(shifted) == len(steps)
                for a, b in zip(steps, shifted):  # level for level: same step, same buffers, level + s
                    assert b[0] == a[0] and b[1] == a[1] + s and b[2:] == a[2:]
                assert all(s <= st[1] < L for st in shifted)
    assert shift_schedule(vcycle_schedule(4)[0], 0) == vcycle_schedule(4)[0]


# ----------------------------------------------------------------------------- MultigridSolver.fmg: refusals, defaults
def stub_solver(coarsest=(3, 3), **kw):
    """A MultigridSolver with the attributes fmg's checks read (no device behind it)."""
    from feanet_amd.solver import MultigridSolver
    s = object.__new__(MultigridSolver)
    s.smoother, s.compat, s.zero_start = "jac", None, False
    s.levels = [types.SimpleNamespace(H=2 * coarsest[0] - 1, W=2 * coarsest[1] - 1),
                types.SimpleNamespace(H=coarsest[0], W=coarsest[1])]
    s.__dict__.update(kw)
    return s


@pytest.mark.parametrize("kw, what", [(dict(smoother="hjac"), "hjac"), (dict(compat="mm_interface_q2"), "compat"),
                                      (dict(zero_start=True), "zero_start")])
def test_fmg_refuses_what_it_does_not_support(kw, what):
    with pytest.raises(ValueError, match=what):
        stub_solver(**kw).fmg()


def test_fmg_refuses_bad_arguments_and_shallow_hierarchies():
    with pytest.raises(ValueError, match="interp"):
        stub_solver().fmg(interp="quintic")
    with pytest.raises(ValueError, match="cycles"):
        stub_solver().fmg(cycles=0)
    with pytest.raises(ValueError, match="cycles"):
        stub_solver().fmg(base_cycles=0)
    with pytest.raises(ValueError, match="more levels"):
        stub_solver(coarsest=(9, 9)).fmg()
    with pytest.raises(ValueError, match="more levels"):
        stub_solver(coarsest=(4, 8)).fmg()  # 12 interior nodes
    stub_solver(coarsest=(4, 7))._fmg_check(1, "cubic", None)  # 10 interior nodes: accepted
    with pytest.raises(ValueError, match="u0 must be None"):
        stub_solver().solve(u0=np.zeros(1), fmg=True)


@pytest.mark.parametrize("coarsest, want", [((3, 3), 1), ((4, 4), 8), ((3, 4), 8), ((4, 6), 8), ((4, 7), 8)])
def test_base_cycles_default(coarsest, want):
    assert stub_solver(coarsest=coarsest).fmg_base_cycles() == want


# ----------------------------------------------------------------------------- header, table, symbols
def fmg_declarations():
    """test_abi.header_declarations for include/feanet_fmg.h."""
    src = open(os.path.join(ROOT, "include", "feanet_fmg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = []
    for ret, name, params in re.findall(r"\b(int|size_t|long long)\s+(fea_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        fields, raw = [], {}
        for p in " ".join(params.split()).split(","):
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", p.strip())
            ctype, pname = m.group(1).strip(), m.group(2)
            cls = "P" if "*" in ctype else {"int": "I", "long long": "LL", "float": "S", "double": "S"}[
                ctype.replace("const", "").strip()]
            fields.append((cls, pname))
            raw[pname] = ctype
        decls.append((name, ret, fields, raw))
    return decls


def test_fmg_table_matches_header():
    from feanet_amd import _lib
    decls = fmg_declarations()
    names = [d[0] for d in decls]
    # names and order: each table entry is the _f32 / _f64 pair, in the header's order
    assert names == [f"fea_{b}_{s}" for b in _lib._FMG for s in ("f32", "f64")] and len(names) == 6
    assert names == _lib.fmg_exported_symbols()
    for name, ret, fields, raw in decls:
        sig = _lib._FMG[name[4:-4]]
        assert ret == "int"
        assert [tuple(p.split()) for p in sig] == fields, name
        assert fields[-1] == ("P", "stream")
        want = "float" if name.endswith("f32") else "double"
        assert all(want in t for t in raw.values() if "float" in t or "double" in t), name
    # none of these names sits in the tables of feanet_hip.h, whose own tests pin their key sets
    assert not set(_lib._FMG) & set(_lib._SIGS) and not any(n in _lib._EXTRA for n in names)
    assert not any(n in _lib.exported_symbols() for n in names)


def test_fmg_launch_records_resolve():
    from feanet_amd import _lib
    rec = _lib.launch("fmg_boundary", bc=None, bc_bstride=0, stride=2, dst=5, B=1, H=9, W=9, ld=32, bstride=352)
    assert rec == ("fmg_boundary", (None, 0, 2, 5, 1, 9, 9, 32, 352))
    assert _lib.arg(rec, "stride") == 2 and _lib.arg(_lib.replace(rec, dst=7), "dst") == 7
    with pytest.raises(TypeError, match=r"fea_fmg_prolong\b.*'order'"):
        _lib.launch("fmg_prolong", u=None, ec=1, out=2, B=1, H=9, W=9, ld=32, bstride=352, ldc=32, bstridec=224)


def test_library_exports_the_fmg_symbols():
    from feanet_amd import _lib
    lib = _lib.lib()
    assert [n for n in _lib.fmg_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_fmg_prolong_f64.argtypes[-2] is ctypes.c_int and lib.fea_fmg_prolong_f64.restype is ctypes.c_int


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
FAKE = {"u": 0x10000, "ec": 0x20000, "out": 0x30000, "f": 0x40000, "fc": 0x50000, "bc": 0x60000, "dst": 0x70000}


def good_args(name, esz, H=9, W=13):
    from feanet_amd import _lib
    ld, bs = _lib.mg_layout(H, W, esz)
    ldc, bsc = _lib.mg_layout((H + 1) // 2, (W + 1) // 2, esz)
    a = dict(B=2, H=H, W=W, ld=ld, bstride=bs)
    if name == "fmg_prolong":
        a.update(u=FAKE["u"], ec=FAKE["ec"], out=FAKE["out"], ldc=ldc, bstridec=bsc, order=3)
    elif name == "fmg_restrict":
        a.update(f=FAKE["f"], fc=FAKE["fc"], ldc=ldc, bstridec=bsc)
    else:
        a.update(bc=FAKE["bc"], bc_bstride=(2 * H - 1) * (2 * W - 1), stride=2, dst=FAKE["dst"])
    return a


def invoke(name, suf, a):
    from feanet_amd import _lib
    fn = getattr(_lib.lib(), f"fea_{name}_{suf}")
    return fn(*[a[p.split()[1]] for p in _lib._FMG[name][:-1]], None)


@pytest.mark.parametrize("suf, esz", [("f32", 4), ("f64", 8)])
@pytest.mark.parametrize("name", ["fmg_prolong", "fmg_restrict", "fmg_boundary"])
def test_entry_points_reject_bad_arguments(name, suf, esz):
    """Everything below is refused before any launch (a launch would fail differently: no device here)."""
    from feanet_amd import _lib
    good = good_args(name, esz)
    A = 128 // esz
    cases = {"B = 0": dict(B=0), "B < 0": dict(B=-1), "H < 3": dict(H=1), "W < 3": dict(W=1),
             "ld below the layout's": dict(ld=good["ld"] - A), "ld unaligned": dict(ld=good["ld"] + 1),
             "bstride short": dict(bstride=good["bstride"] - 1), "ld 0": dict(ld=0)}
    if name != "fmg_boundary":
        cases.update({"even H": dict(H=good["H"] + 1, bstride=4 * good["bstride"]), "even W": dict(W=good["W"] + 1,
                      ld=2 * good["ld"], bstride=4 * good["bstride"]), "H = 2": dict(H=2), "W = 2": dict(W=2),
                      "ldc below the layout's": dict(ldc=good["ldc"] - A), "ldc unaligned": dict(ldc=good["ldc"] + 1),
                      "bstridec short": dict(bstridec=good["bstridec"] - 1), "ldc 0": dict(ldc=0)})
    if name == "fmg_prolong":
        cases.update({"ec NULL": dict(ec=None), "out NULL": dict(out=None), "order 0": dict(order=0),
                      "order 2": dict(order=2), "order 4": dict(order=4), "order -3": dict(order=-3),
                      "out == ec": dict(out=FAKE["ec"]), "u == ec": dict(u=FAKE["ec"])})
    elif name == "fmg_restrict":
        cases.update({"f NULL": dict(f=None), "fc NULL": dict(fc=None), "fc == f": dict(fc=FAKE["f"]),
                      "no coarse interior (H = 3)": dict(H=3), "no coarse interior (W = 3)": dict(W=3)})
    else:
        cases.update({"dst NULL": dict(dst=None), "stride 0": dict(stride=0), "stride < 0": dict(stride=-2),
                      "bc_bstride < 0": dict(bc_bstride=-1), "dst == bc": dict(dst=FAKE["bc"]),
                      "B too large": dict(B=70000, bstride=good["bstride"])})
    for what, change in cases.items():
        assert invoke(name, suf, {**good, **change}) == FEA_EINVAL, f"fea_{name}_{suf}: {what} was not rejected"
    # the smallest grids are not rejected for their size: with a NULL operand they still fail as arguments only
    small = good_args(name, esz, H=5, W=5)
    first = _lib._FMG[name][1 if name == "fmg_prolong" else (3 if name == "fmg_boundary" else 0)].split()[1]
    assert invoke(name, suf, {**small, first: None}) == FEA_EINVAL
