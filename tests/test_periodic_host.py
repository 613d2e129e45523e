"""The periodic cell, CPU side: the binding table against include/feanet_periodic.h, the argument checks
of the entry points (fake addresses: a rejected call launches nothing, and there is no GPU here), the task rule behind
fea_per_parts, and what the definitions promise, from the numpy oracle of periodic_ref.py and dense solves alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import energy_ref as er
import flux_ref as fx
import periodic_ref as pf
import phase_ref as pr
from conftest import ROOT

PROPS = [(1, 20), (20, 1), (1, 1000)]
SHAPES = [(2, 2), (4, 6), (6, 10), (12, 16), (20, 66), (32, 130), (64, 64), (4096, 4096), (5, 7)]


# ----------------------------------------------------------------------------- header, table, symbols
def declarations():
    """(name, return type, [(class, parameter)]) of include/feanet_periodic.h, classes as in feanet_amd._lib (the
    comparison test_energy_host.py makes for its header)."""
    src = open(os.path.join(ROOT, "include", "feanet_periodic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = []
    for ret, name, params in re.findall(r"\b(int|size_t|long long)\s+(fea_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        fields = []
        for p in " ".join(params.split()).split(","):
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", p.strip())
            ctype, pname = m.group(1).strip(), m.group(2)
            fields.append(("P" if "*" in ctype else {"int": "I", "long long": "LL", "double": "D"}[ctype], pname))
        decls.append((name, ret, fields))
    return decls


def test_periodic_table_matches_header():
    from feanet_amd import _lib
    decls = {d[0]: d for d in declarations()}
    typed = ["per_sweep", "per_residual_restrict", "per_prolong_add", "per_apply", "per_reduce"]
    assert list(_lib._PERIODIC) == typed + ["fea_per_parts", "fea_per_final"]
    assert sorted(decls) == sorted(_lib.periodic_exported_symbols())
    table = lambda n: [tuple(p.split()) for p in _lib._PERIODIC[n]]
    for base in typed:
        a, b = decls[f"fea_{base}_f32"], decls[f"fea_{base}_f64"]
        assert a[2] == b[2] == table(base), base
        assert a[1] == b[1] == "int" and table(base)[-1] == ("P", "stream")
    assert decls["fea_per_parts"][1] == "long long" and _lib._PERIODIC_RES["fea_per_parts"] is ctypes.c_longlong
    assert decls["fea_per_parts"][2] == table("fea_per_parts")
    assert decls["fea_per_final"][1] == "int" and decls["fea_per_final"][2] == table("fea_per_final")
    # a table of its own: the other headers' tables, whose tests pin their key sets, do not hold the names
    others = set(_lib._SIGS) | set(_lib._EXTRA) | set(_lib._FMG) | set(_lib._PHASE) | set(_lib._FLUX) | \
        set(_lib._ENERGY)
    assert not others & (set(_lib._PERIODIC) | {"fea_" + n for n in typed})
    held = set(_lib.exported_symbols()) | set(_lib.fmg_exported_symbols()) | set(_lib.phase_exported_symbols()) | \
        set(_lib.flux_exported_symbols()) | set(_lib.energy_exported_symbols())
    assert not held & set(_lib.periodic_exported_symbols())
    assert _lib.ABI_VERSION == 3  # feanet_hip.h and fea_abi_version are untouched


def test_library_exports_the_periodic_symbols():
    from feanet_amd import _lib, build
    lib = _lib.lib()
    assert [n for n in _lib.periodic_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_per_sweep_f64.argtypes[4] is ctypes.c_longlong and len(lib.fea_per_sweep_f32.argtypes) == 13
    assert lib.fea_per_parts.restype is ctypes.c_longlong and lib.fea_per_final.restype is ctypes.c_int
    assert "periodic_ops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "periodic_ops.hip"))
    rec = _lib.launch("per_reduce", a=1, b=None, part=2, B=1, m=4, n=6, ld=8, bstride=32)
    assert _lib.arg(rec, "ld") == 8 and _lib.arg(_lib.launch("per_final", part=1, per=2, sums=3, count=4), "count") == 4
    with pytest.raises(TypeError, match="launches on a stream"):
        _lib.launch("per_parts", m=3, n=3, elem_size=8)


@pytest.mark.parametrize("esz", [4, 8])
def test_per_parts_is_the_single_sample_task_rule(esz):
    from feanet_amd import _lib
    lib = _lib.lib()
    for m, n in SHAPES:
        assert int(lib.fea_per_parts(m, n, esz)) == pf.parts(m, n, esz), (m, n)
    assert lib.fea_per_parts(2, 2, esz) == 1 and lib.fea_per_parts(20, 66, 8) == 10
    assert lib.fea_per_parts(20, 66, 4) == 10
    assert lib.fea_per_parts(32, 130, 8) == 2 * lib.fea_per_parts(32, 128, 8)
    for bad in ((0, 9, 8), (9, 0, 8), (9, 9, 2), (9, 9, 16), (-4, 4, 4), ((1 << 20) + 1, 4, 8)):
        assert lib.fea_per_parts(*bad) == -1


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
A0, A1, A2, PID, TAB, OMD, PART = 0x100000, 0x400000, 0x800000, 0x1000000, 0x2000000, 0x2100000, 0x3000000


def invoke(name, a):
    from feanet_amd import _lib
    base = name[4:-4] if name[-4:] in ("_f32", "_f64") else name
    sig = _lib._PERIODIC[base]
    return getattr(_lib.lib(), name)(*[a[p.split()[1]] for p in sig[:-1]], None)


@pytest.mark.parametrize("suf, esz", [("f32", 4), ("f64", 8)])
def test_entry_points_reject_bad_arguments(suf, esz):
    """every FEA_EINVAL case; each good call differs from a launch only by its NULL field, so nothing is launched"""
    vec = 16 // esz
    m, n = 12, 18
    ld = -(-n // vec) * vec
    geom = dict(B=2, m=m, n=n, ld=ld, bstride=m * ld)
    sten = dict(pid=PID, ldp=32, ktab=TAB)
    layout = {"B 0": dict(B=0), "m 0": dict(m=0), "n 0": dict(n=0), "n beyond the pitch": dict(n=ld + 1),
              "ld not a vector multiple": dict(ld=ld + 1), "bstride below the sample": dict(bstride=m * ld - vec),
              "bstride not a vector multiple": dict(bstride=m * ld + 1)}
    pid = {"pid NULL": dict(pid=None), "ldp below the row": dict(ldp=16), "ldp odd": dict(ldp=33),
           "pid unaligned": dict(pid=PID + 1), "ktab NULL": dict(ktab=None)}
    sweep = dict(u=A0, f=A1, out=A2, omd=OMD, **sten, **geom)
    cases = {**layout, **pid, "f NULL": dict(f=None), "out NULL": dict(out=None), "omd NULL": dict(omd=None),
             "out is u": dict(out=A0), "out inside f": dict(out=A1 + 16 * ld), "u unaligned": dict(u=A0 + esz)}
    for what, change in cases.items():
        assert invoke(f"fea_per_sweep_{suf}", {**sweep, **change}) == FEA_EINVAL, f"sweep: {what} was not rejected"
    apply = dict(p=A0, y=A1, part=None, **sten, **geom)
    for what, change in {**layout, **pid, "p NULL": dict(p=None), "y NULL": dict(y=None), "y is p": dict(y=A0)}.items():
        assert invoke(f"fea_per_apply_{suf}", {**apply, **change}) == FEA_EINVAL, f"apply: {what} was not rejected"
    red = dict(a=A0, b=A1, part=PART, **geom)
    cases = {**layout, "a NULL": dict(a=None), "part NULL": dict(part=None), "b unaligned": dict(b=A1 + esz)}
    for what, change in cases.items():
        assert invoke(f"fea_per_reduce_{suf}", {**red, **change}) == FEA_EINVAL, f"reduce: {what} was not rejected"
    ldc = -(-(n // 2) // vec) * vec
    co = dict(ldc=ldc, bstridec=(m // 2) * ldc)
    rr = dict(u=A0, f=A1, fc=A2, **sten, **geom, **co)
    cases = {**layout, **pid, "m odd": dict(m=11), "n odd": dict(n=17), "f NULL": dict(f=None),
             "fc NULL": dict(fc=None),
             "ldc below the coarse row": dict(ldc=ldc - vec), "bstridec below the coarse sample": dict(bstridec=ldc)}
    for what, change in cases.items():
        assert invoke(f"fea_per_residual_restrict_{suf}", {**rr, **change}) == FEA_EINVAL, f"restrict: {what}"
    pa = dict(ec=A0, u=A1, **geom, **co)
    cases = {**layout, "m odd": dict(m=11), "n odd": dict(n=17), "ec NULL": dict(ec=None), "u NULL": dict(u=None),
             "ldc odd": dict(ldc=ldc + 1)}
    for what, change in cases.items():
        assert invoke(f"fea_per_prolong_add_{suf}", {**pa, **change}) == FEA_EINVAL, f"prolong_add: {what}"
    good = dict(part=PART, per=8, sums=A0, count=4)
    for what, change in {"part NULL": dict(part=None), "sums NULL": dict(sums=None), "per 0": dict(per=0),
                         "count 0": dict(count=0)}.items():
        assert invoke("fea_per_final", {**good, **change}) == FEA_EINVAL, f"final: {what} was not rejected"


def test_host_layer_refuses_before_it_touches_the_device():
    from feanet_amd import homogenize
    img = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="method"):
        homogenize.effective_conductivity(img, bc="periodic", method="mg")
    with pytest.raises(ValueError, match="precond_dtype"):
        homogenize.effective_conductivity(img, bc="periodic", precond_dtype=np.float32)
    with pytest.raises(ValueError, match="route"):
        homogenize.effective_conductivity(img, bc="periodic", route="hill")
    with pytest.raises(ValueError, match=r"\[rows, n\]"):
        homogenize.effective_conductivity(np.zeros((2, 8, 8), np.uint8), bc="periodic")
    with pytest.raises(ValueError, match="unknown bc"):
        homogenize.effective_conductivity(img, bc="neumann")


# ----------------------------------------------------------------------------- map and operator
@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_wrapped_map_and_mirror_property(name):
    """The rolled map is the wrap-padded phase_pattern_map; on every level of the hierarchy the own-row (mirrored) form
    of K u equals the neighbour-row definition with difference exactly 0, for the three contrasts."""
    from feanet_amd import mesh_setup as ms
    from feanet_amd.periodic import coarse_shapes, load_table
    for m, n in ((12, 16), (32, 48), (20, 66), (5, 7), (4, 4)):
        img = pr.image(name, m, n)
        for prop in PROPS:
            levels = pf.hierarchy(img, prop, "stiff")
            assert [p.shape for p in levels] == coarse_shapes(m, n)
            ktab = ms.stencil_table(prop).reshape(16, 9).astype(np.float64)
            for ph in levels:
                pid = pf.wrapped_map(ph)
                assert np.array_equal(pid, pf.rolled_map(ph)) and pid.shape == ph.shape
                u = np.random.default_rng(7).standard_normal((2,) + ph.shape)
                assert np.abs(pf.apply_own(u, pid, ktab) - pf.apply_neighbour(u, pid, ktab)).max() == 0.0
        tab = ms.stencil_table((1, 20))
        assert np.array_equal(load_table(tab, 0.125), pf.load_table(tab, 0.125))
    assert coarse_shapes(64, 64)[-1] == (2, 2) and coarse_shapes(20, 66) == [(20, 66), (10, 33)]
    assert coarse_shapes(8, 24)[-1] == (2, 6) and coarse_shapes(5, 8) == [(5, 8)]


def test_device_map_rule_on_the_host():
    """feanet_amd.periodic.wrapped_pattern_map (torch.roll) on CPU tensors equals the oracle's map"""
    import torch
    from feanet_amd.periodic import wrapped_pattern_map
    for name in pr.IMAGES:
        img = pr.image(name, 12, 18)
        assert np.array_equal(wrapped_pattern_map(torch.from_numpy(img)).numpy(), pf.wrapped_map(img))


@pytest.mark.parametrize("prop", PROPS)
def test_dense_k_is_symmetric_with_a_row_sum_defect(prop):
    """K from the float32 table is symmetric bit for bit; its rows sum to zero only to float32 rounding: max|K 1| is
    printed and below 1e-6 kmax (and not 0: the reason for the projection); K applied equals the dense product; the
    load table is -K X_j wherever no tap wraps."""
    worst = 0.0
    for name in pr.IMAGES:
        img = pr.image(name, 12, 16)
        K = pf.dense_table(img, prop)
        assert np.array_equal(K, K.T)
        worst = max(worst, np.abs(K.sum(1)).max())
        o = pf.Oracle(img, prop)
        u = np.random.default_rng(3).standard_normal((1, 12, 16))
        assert np.abs(o.K(u).ravel() - K @ u.ravel()).max() <= 1e-13 * max(prop)
        X = fx.load_cases(12, 16, 2.0)[:, :12, :16]
        b = o.rhs()
        for j in range(2):
            kx = -(K @ X[j].ravel()).reshape(12, 16) + (K.sum(1).reshape(12, 16) * X[j])   # without the row-sum term
            assert np.abs(kx - b[j])[1:-1, 1:-1].max() <= 1e-12 * max(prop)
    print(f"prop {prop}: max|K 1| = {worst:.3e} ({worst / max(prop):.3e} kmax)")
    assert 0 < worst <= 1e-6 * max(prop)


def test_exact_and_table_right_hand_sides_agree():
    img = pr.six_discs(12, 16)
    K, b = pf.dense_exact(img, (1, 20))
    assert np.abs(K - K.T).max() <= 1e-14 and np.abs(K.sum(1)).max() <= 1e-13
    assert np.abs(b.reshape(2, 12, 16) - pf.Oracle(img, (1, 20)).rhs()).max() <= 1e-6 * 20
    assert np.abs(K - pf.dense_table(img, (1, 20))).max() <= 1e-6 * 20
    # the LU solve of the regularised system is the pseudo-inverse solution
    Kt = pf.dense_table(img, (1, 20))
    bt = pf.Oracle(img, (1, 20)).rhs().reshape(2, -1)
    assert np.abs(pf.pinv_solve(Kt, bt) - pf.pinv_svd(Kt, bt)).max() <= 1e-12 * np.abs(pf.pinv_svd(Kt, bt)).max()


# ----------------------------------------------------------------------------- projection, preconditioner
def test_projection_is_what_lets_the_recurrence_converge():
    """six_discs 16 x 16, (1, 20), rtol 1e-10, 40 iterations: on K itself the recurrence does not get there (the
    residual's mean drifts with K 1 != 0 until p^T K p loses its sign or the norm stalls); on P K P it does."""
    o = pf.Oracle(pr.six_discs(16, 16), (1, 20))
    _, its, flags, hist = o.pcg(rtol=1e-10, max_iters=40, project=False)
    reached = min(h.max() for h in hist) / hist[0].max()
    print(f"unprojected: flags {flags}, iterations {its}, best max_b ||r|| / ||r0|| = {reached:.2e}")
    assert (flags != 1).all() and (np.array([h / hist[0] for h in hist]).min(0) > 1e-10).all()
    x, its, flags, hist = o.pcg(rtol=1e-10, max_iters=40)
    print(f"projected: flags {flags}, iterations {its}")
    assert (flags == 1).all() and (hist[-1] <= 1e-10 * hist[0]).all() and its.max() < 40
    assert np.abs(x.reshape(2, -1).mean(1)).max() <= 1e-15


@pytest.mark.parametrize("m, n, levels", [(8, 8, 3), (6, 10, 2), (5, 7, 1), (4, 4, 2)])
def test_cycle_is_symmetric_and_positive_on_the_mean_free_subspace(m, n, levels):
    img = pr.image("random_elements", m, n)
    o = pf.Oracle(img, (1, 20))
    assert len(o.pids) == levels
    M = pf.cycle_matrix(o)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    N = m * n
    Q = np.linalg.qr(np.eye(N) - 1.0 / N)[0][:, :N - 1]   # an orthonormal basis of the mean-free subspace
    w = np.linalg.eigvalsh(Q.T @ (0.5 * (M + M.T)) @ Q)
    print(f"{m} x {n}: {levels} levels, eigenvalues of M on the mean-free subspace {w[0]:.4f} .. {w[-1]:.4f}")
    assert w[0] > 0


# ----------------------------------------------------------------------------- what the definitions promise
def test_laminates_give_the_arithmetic_and_harmonic_means():
    """stripes along an axis: the arithmetic mean along them, the harmonic mean across, 1e-12 relative (dense solve).
    With the float32 table at (1, 20) and (20, 1), where the laminate's solution is reproduced to rounding; at
    (1, 1000) the table's own float32 rounding of the weights shows (1.2e-9 relative on the harmonic mean), so that
    contrast is held to 1e-12 with the exact element matrices and to 1e-8 with the table."""
    for prop, exact in [(p, False) for p in PROPS[:2]] + [(PROPS[2], True)]:
        k0, k1 = float(prop[0]), float(prop[1])
        arith, harm = 0.5 * (k0 + k1), 2.0 / (1.0 / k0 + 1.0 / k1)
        for img, want in ((pr.stripes(12, 16), [arith, harm]), (fx.parallel_stripes(12, 16, 0), [arith, harm]),
                          (fx.parallel_stripes(12, 16, 1), [harm, arith]),
                          (fx.parallel_stripes(6, 10, 0, 5), [arith, harm])):
            r = pf.homogenize(img, prop, exact=exact)
            assert np.abs(r["K_E"] - np.diag(want)).max() <= 1e-12 * arith, (prop, r["K_E"])
            if exact:
                assert np.abs(pf.homogenize(img, prop)["K_E"] - np.diag(want)).max() <= 1e-8 * arith
    r = pf.homogenize(pr.stripes(12, 16), (1, 20))
    assert np.allclose(np.diag(r["K_E"]), [10.5, 2 / 1.05], rtol=1e-12, atol=0)
    assert np.diag(er.homogenize_image("stripes", 12, 16, (1, 20))["K_E"])[1] > 7   # the Dirichlet bound, far above


@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_roll_invariance(name):
    img = pr.image(name, 12, 16)
    a, b = pf.homogenize(img, (1, 20)), pf.homogenize(np.roll(img, (3, 5), (0, 1)), (1, 20))
    assert np.abs(a["K_E"] - b["K_E"]).max() <= 1e-12 * np.abs(a["K_E"]).max()
    assert np.abs(a["K_flux"] - b["K_flux"]).max() <= 1e-12 * np.abs(a["K_E"]).max()


@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_dirichlet_bounds_periodic_from_above(name):
    """K_dirichlet - K_periodic (energy route, exact element matrices: the hierarchy of bounds is a theorem only for the
    exact K) is positive semi-definite: smallest eigenvalue >= -1e-10 max|K|."""
    d = er.homogenize_image(name, 12, 16, (1, 20), exact=True)["K_E"]
    p = pf.homogenize_image(name, 12, 16, (1, 20), exact=True)["K_E"]
    w = np.linalg.eigvalsh(d - p)
    print(f"{name}: eigenvalues of K_dirichlet - K_periodic {w}")
    assert w[0] >= -1e-10 * np.abs(d).max() and p[0, 1] == p[1, 0]


def test_prototype_figures():
    """the CPU table of DESIGN §18 and its iteration counts"""
    r = pf.homogenize_image("half_plane", 12, 16, (1, 20))
    assert np.allclose(np.diag(r["K_E"]), [8.125, 1.5534], rtol=1e-4)
    assert np.allclose(np.diag(er.homogenize_image("half_plane", 12, 16, (1, 20))["K_E"]), [8.125, 4.9297], rtol=1e-4)
    for prop, want in (((1, 20), 22), ((1, 1000), 30)):
        _, its, flags, _ = pf.Oracle(pr.six_discs(12, 16), prop).pcg()
        assert (flags == 1).all() and its.max() == want
    x, its, flags, hist = pf.Oracle(pr.stripes(12, 16), (1, 20)).pcg()
    assert its[0] == 0 and flags[0] == 1 and hist[0][0] <= pf.Oracle(pr.stripes(12, 16), (1, 20)).floor()
