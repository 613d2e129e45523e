"""Element coefficient fields on the periodic cell, CPU side: the binding table against
include/feanet_coef.h, the argument checks of the entry points (fake addresses: a rejected call launches nothing, and
there is no GPU here), and what the definitions promise, from the numpy oracle of coef_ref.py and dense solves alone."""
import os
import re

import numpy as np
import pytest

import coef_ref as cf
import periodic_ref as pf
import phase_ref as pr
from conftest import ROOT

TYPED = ["coef_sweep", "coef_apply", "coef_residual_restrict", "coef_coarsen"]


# ----------------------------------------------------------------------------- header, table, symbols
def declarations():
    """(name, return type, [(class, parameter)]) of include/feanet_coef.h, classes as in feanet_amd._lib (the
    comparison test_periodic_host.py makes for its header)."""
    src = open(os.path.join(ROOT, "include", "feanet_coef.h")).read()
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


def test_coef_table_matches_header():
    from feanet_amd import _lib
    decls = {d[0]: d for d in declarations()}
    assert list(_lib._COEF) == TYPED and _lib._COEF_RES == {}
    assert sorted(decls) == sorted(_lib.coef_exported_symbols()) and len(decls) == 8
    table = lambda n: [tuple(p.split()) for p in _lib._COEF[n]]
    for base in TYPED:
        a, b = decls[f"fea_{base}_f32"], decls[f"fea_{base}_f64"]
        assert a[2] == b[2] == table(base), base
        assert a[1] == b[1] == "int" and table(base)[-1] == ("P", "stream")
    # a table of its own: the other headers' tables, whose tests pin their key sets, do not hold the names
    others = set(_lib._SIGS) | set(_lib._EXTRA) | set(_lib._FMG) | set(_lib._PHASE) | set(_lib._FLUX) | \
        set(_lib._ENERGY) | set(_lib._PERIODIC)
    assert not others & (set(_lib._COEF) | {"fea_" + n for n in TYPED})
    held = set(_lib.exported_symbols()) | set(_lib.fmg_exported_symbols()) | set(_lib.phase_exported_symbols()) | \
        set(_lib.flux_exported_symbols()) | set(_lib.energy_exported_symbols()) | \
        set(_lib.periodic_exported_symbols())
    assert not held & set(_lib.coef_exported_symbols())
    assert _lib.ABI_VERSION == 3  # feanet_hip.h and fea_abi_version are untouched


def test_library_exports_the_coef_symbols():
    import ctypes
    from feanet_amd import _lib, build
    lib = _lib.lib()
    assert [n for n in _lib.coef_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_coef_sweep_f64.argtypes[4] is ctypes.c_longlong and lib.fea_coef_sweep_f32.argtypes[5] is \
        ctypes.c_double and len(lib.fea_coef_sweep_f32.argtypes) == 12
    assert "coef_ops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "coef_ops.hip"))
    rec = _lib.launch("coef_apply", p=1, y=2, part=None, k=3, ldk=8, B=1, m=4, n=6, ld=8, bstride=32)
    assert _lib.arg(rec, "ldk") == 8 and _lib.arg(rec, "part") is None


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
A0, A1, A2, KF, KC, PART = 0x100000, 0x400000, 0x800000, 0x1000000, 0x2000000, 0x3000000


def invoke(name, a):
    from feanet_amd import _lib
    sig = _lib._COEF[name[4:-4]]
    return getattr(_lib.lib(), name)(*[a[p.split()[1]] for p in sig[:-1]], None)


@pytest.mark.parametrize("suf, esz", [("f32", 4), ("f64", 8)])
def test_entry_points_reject_bad_arguments(suf, esz):
    """every FEA_EINVAL case; each call differs from a good one by the one thing named, and a rejected call launches
    nothing"""
    vec = 16 // esz
    m, n = 12, 18
    ld = -(-n // vec) * vec
    geom = dict(B=2, m=m, n=n, ld=ld, bstride=m * ld)
    field = dict(k=KF, ldk=ld)
    layout = {"B 0": dict(B=0), "m 1": dict(m=1), "n 1": dict(n=1), "m 0": dict(m=0),
              "n beyond the pitch": dict(n=ld + 1), "ld not a vector multiple": dict(ld=ld + 1), "bstride below the sample": dict(bstride=m * ld - vec),
              "bstride not a vector multiple": dict(bstride=m * ld + 1)}
    kbad = {"k NULL": dict(k=None), "k unaligned": dict(k=KF + esz), "ldk below the row": dict(ldk=ld - vec),
            "ldk not a vector multiple": dict(ldk=ld + 1)}
    sweep = dict(u=A0, f=A1, out=A2, omega=2.0 / 3.0, **field, **geom)
    cases = {**layout, **kbad, "f NULL": dict(f=None), "out NULL": dict(out=None), "out is u": dict(out=A0),
             "out inside f": dict(out=A1 + 16 * ld), "u unaligned": dict(u=A0 + esz)}
    for what, change in cases.items():
        assert invoke(f"fea_coef_sweep_{suf}", {**sweep, **change}) == FEA_EINVAL, f"sweep: {what} was not rejected"
    apply = dict(p=A0, y=A1, part=None, **field, **geom)
    for what, change in {**layout, **kbad, "p NULL": dict(p=None), "y NULL": dict(y=None), "y is p": dict(y=A0),
                         "y inside p": dict(y=A0 + 16 * ld)}.items():
        assert invoke(f"fea_coef_apply_{suf}", {**apply, **change}) == FEA_EINVAL, f"apply: {what} was not rejected"
    ldc = -(-(n // 2) // vec) * vec
    co = dict(ldc=ldc, bstridec=(m // 2) * ldc)
    rr = dict(u=A0, f=A1, fc=A2, **field, **geom, **co)
    cases = {**layout, **kbad, "m odd": dict(m=11), "n odd": dict(n=17), "f NULL": dict(f=None),
             "fc NULL": dict(fc=None), "fc inside u": dict(fc=A0 + 16), "fc is f": dict(fc=A1),
             "ldc below the coarse row": dict(ldc=ldc - vec), "bstridec below the coarse sample": dict(bstridec=ldc)}
    for what, change in cases.items():
        assert invoke(f"fea_coef_residual_restrict_{suf}", {**rr, **change}) == FEA_EINVAL, f"restrict: {what}"
    cz = dict(k=KF, ldk=ld, kc=KC, ldkc=ldc, m=m, n=n, rule=2)
    cases = {"k NULL": dict(k=None), "kc NULL": dict(kc=None), "kc unaligned": dict(kc=KC + esz), "m odd": dict(m=11),
             "n odd": dict(n=17), "m 0": dict(m=0), "ldk below the row": dict(ldk=ld - vec),
             "ldkc below the coarse row": dict(ldkc=ldc - vec), "ldkc not a vector multiple": dict(ldkc=ldc + 1),
             "rule 3": dict(rule=3), "rule -1": dict(rule=-1), "kc inside k": dict(kc=KF + 16)}
    for what, change in cases.items():
        assert invoke(f"fea_coef_coarsen_{suf}", {**cz, **change}) == FEA_EINVAL, f"coarsen: {what} was not rejected"


def test_check_field_rejects_bad_fields():
    import torch
    from feanet_amd.coef import check_field, effective_conductivity_field
    good = cf.lognormal(6, 8)
    out = check_field(good)
    assert out.dtype == torch.float64 and tuple(out.shape) == (6, 8) and np.array_equal(out.numpy(), good)
    assert check_field(torch.from_numpy(good.astype(np.float32))).dtype == torch.float64
    assert check_field(np.ones((4, 4), np.uint8)).dtype == torch.float64
    for what, bad in {"three axes": np.ones((2, 6, 8)), "one axis": np.ones(8), "a zero": np.where(good > 1, good, 0.0),
                      "a negative value": -good, "a NaN": np.where(good > 1, good, np.nan),
                      "an infinity": np.where(good > 1, good, np.inf), "one row": np.ones((1, 8)),
                      "complex": np.ones((4, 4), np.complex128)}.items():
        with pytest.raises(ValueError):
            check_field(bad)
        with pytest.raises(ValueError):
            check_field(torch.from_numpy(bad))
    with pytest.raises(ValueError, match="route"):
        effective_conductivity_field(good, route="hill")
    with pytest.raises(ValueError, match="positive"):
        effective_conductivity_field(-good)


# ----------------------------------------------------------------------------- operator and right-hand sides
@pytest.mark.parametrize("m, n", [(12, 16), (2, 2), (5, 7), (2, 6), (6, 2)])
def test_difference_form_is_the_assembled_matrix(m, n):
    """difference form == dense K to 1e-13 max|K u|, on a lognormal field of contrast sigma 2; both right-hand sides
    against assembly; K is symmetric and its rows sum to zero to rounding"""
    k = cf.lognormal(m, n, 2.0)
    K, b = cf.dense(k)
    u = np.random.default_rng([5, m, n]).standard_normal((3, m, n))
    want = (K @ u.reshape(3, -1).T).T.reshape(3, m, n)
    err = np.abs(cf.apply_diff(u, k) - want).max()
    print(f"{m} x {n}: |difference form - K u| = {err:.2e}, max|K u| = {np.abs(want).max():.2e}")
    assert err <= 1e-13 * np.abs(want).max()
    assert np.abs(K - K.T).max() <= 1e-14 * np.abs(K).max() and np.abs(K.sum(1)).max() <= 1e-13 * np.abs(K).max()
    assert np.abs(np.diag(K) - cf.diagonal(k).ravel()).max() <= 1e-14 * np.abs(K).max()
    assert np.abs(cf.rhs(k, 2.0 / n) - b.reshape(2, m, n)).max() <= 4e-16 * k.max() * (2.0 / n) * 4


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_constants_are_in_the_kernel_exactly(dt):
    """K 1 == 0 exactly in both precisions (the float32 table of §18 has 3e-6 here), for any constant"""
    for seed in range(4):
        k = cf.lognormal(12, 16, 2.5, seed)
        for c in (1.0, -3.7, 1e6):
            assert np.abs(cf.apply_diff(np.full((2, 12, 16), c, dt), k, dt)).max() == 0.0


def test_image_as_a_field_is_the_exact_two_material_problem():
    """a 0/1 image with prop (1, 20) written as a field: periodic_ref.homogenize(exact=True) to 1e-12, both routes"""
    for name in ("six_discs", "random_elements"):
        img = pr.image(name, 12, 16)
        ref = pf.homogenize(img, (1, 20), exact=True)
        got = cf.homogenize(cf.from_image(img, (1, 20)))
        scale = np.abs(ref["K_E"]).max()
        assert np.abs(got["K_E"] - ref["K_E"]).max() <= 1e-12 * scale
        assert np.abs(got["K_flux"] - ref["K_flux"]).max() <= 1e-12 * scale


def test_four_valued_laminate():
    """columns of width 4 with the values 1, 3, 20, 7.5 at 12 x 16: the arithmetic mean 7.875 along the columns, the
    harmonic mean 2.637362637... across, to 1e-12"""
    k = cf.laminate()
    v = np.array([1.0, 3.0, 20.0, 7.5])
    arith, harm = v.mean(), 1.0 / (1.0 / v).mean()
    assert arith == 7.875 and abs(harm - 2.637362637362637) <= 1e-14
    r = cf.homogenize(k)
    assert np.abs(r["K_E"] - np.diag([arith, harm])).max() <= 1e-12 * arith, r["K_E"]
    assert np.abs(r["K_flux"] - np.diag([arith, harm])).max() <= 1e-12 * arith, r["K_flux"]
    r = cf.homogenize(k.T.copy())
    assert np.abs(r["K_E"] - np.diag([harm, arith])).max() <= 1e-12 * arith


def test_sensitivity_is_the_derivative_in_single_elements():
    """sens[q][R, C] against central differences of the dense K_eff in that element's coefficient.  K_eff is smooth in
    k_e; with a relative step of 1e-4 the truncation is of order 1e-8 of the derivative's scale and the rounding of
    the quotient 1e-12 / 1e-4: allowed 1e-6 max|sens|."""
    k = cf.lognormal(8, 12, 1.0, 3)
    ref = cf.homogenize(k)
    worst = 0.0
    for R, C in ((0, 0), (3, 7), (7, 11), (4, 0)):
        step = 1e-4 * k[R, C]
        hi, lo = k.copy(), k.copy()
        hi[R, C] += step
        lo[R, C] -= step
        q = (cf.dense_k_eff(hi) - cf.dense_k_eff(lo)) / (hi[R, C] - lo[R, C])
        got = ref["sens"][:, R, C]
        worst = max(worst, np.abs(got - [q[0, 0], q[0, 1], q[1, 1]]).max())
    print(f"sensitivity against central differences: worst {worst:.2e}, max|sens| {np.abs(ref['sens']).max():.2e}")
    assert worst <= 1e-6 * np.abs(ref["sens"]).max()
    # the field sums back: K_E is linear in k at fixed fields
    a = (ref["sens"] * k).reshape(3, -1).sum(1)
    assert np.abs(a - [ref["K_E"][0, 0], ref["K_E"][0, 1], ref["K_E"][1, 1]]).max() <= 1e-14 * np.abs(a).max()


# ----------------------------------------------------------------------------- hierarchy and preconditioner
def test_coarsening_rules():
    k = cf.lognormal(8, 12, 1.5)
    for rule in cf.RULES:
        levels = cf.hierarchy(k, rule)
        from feanet_amd.periodic import coarse_shapes
        assert [x.shape for x in levels] == coarse_shapes(8, 12)
        assert all((x > 0).all() for x in levels)
    a, h, g = (cf.coarsen(k, r) for r in cf.RULES)
    assert (h <= g * (1 + 1e-15)).all() and (g <= a * (1 + 1e-15)).all()   # the means' inequality, block by block
    blocks = k.reshape(4, 2, 6, 2).transpose(0, 2, 1, 3).reshape(4, 6, 4)
    assert np.abs(a - blocks.mean(-1)).max() <= 1e-15 * a.max()
    assert np.abs(h - 1.0 / (1.0 / blocks).mean(-1)).max() <= 1e-15 * a.max()
    assert np.abs(g - np.exp(np.log(blocks).mean(-1))).max() <= 1e-15 * a.max()
    const = np.full((4, 4), 3.0)
    for r in cf.RULES:
        assert np.abs(cf.coarsen(const, r) - 3.0).max() <= 1e-15 * 3
    assert cf.coarsen(k.astype(np.float32), "geometric", np.float32).dtype == np.float32


@pytest.mark.parametrize("rule", cf.RULES)
@pytest.mark.parametrize("m, n, levels", [(8, 8, 3), (6, 10, 2), (5, 7, 1), (4, 4, 2)])
def test_cycle_is_symmetric_and_positive_on_the_mean_free_subspace(m, n, levels, rule):
    o = cf.Oracle(cf.lognormal(m, n, 1.5), coarsen=rule)
    assert len(o.ks) == levels
    M = pf.cycle_matrix(o)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    N = m * n
    Q = np.linalg.qr(np.eye(N) - 1.0 / N)[0][:, :N - 1]   # an orthonormal basis of the mean-free subspace
    w = np.linalg.eigvalsh(Q.T @ (0.5 * (M + M.T)) @ Q)
    print(f"{m} x {n} {rule}: {levels} levels, eigenvalues of M on the mean-free subspace {w[0]:.4f} .. {w[-1]:.4f}")
    assert w[0] > 0


# the table of DESIGN §19: 16 x 16, three levels, omega 2/3, rtol 1e-10, the fields of coef_ref.TABLE_FIELDS
TABLE = {
    "lognormal, sigma 1.0": {"arithmetic": (15, 15), "harmonic": (17, 17), "geometric": (14, 14)},
    "lognormal, sigma 2.5": {"arithmetic": (34, 34), "harmonic": (63, 63), "geometric": (29, 29)},
    "random binary, 1 : 1000": {"arithmetic": (36, 37), "harmonic": (101, 106), "geometric": (49, 49)},
}


def test_coarsening_table():
    """The iteration counts of DESIGN §19, and what they say: every rule converges on every field; at low contrast the
    rules are within three iterations of each other; on the high-contrast lognormal field the geometric mean needs the
    fewest; on the random binary field the arithmetic mean does and the harmonic mean needs by far the most.  No rule
    wins everywhere."""
    t = cf.coarsening_table()
    for name, row in t.items():
        print(name, row)
    assert t == TABLE
    best = lambda name: min(cf.RULES, key=lambda r: max(t[name][r]))
    assert all(min(c) > 0 for row in t.values() for c in row.values())
    low = [max(c) for c in t["lognormal, sigma 1.0"].values()]
    assert max(low) - min(low) <= 3
    assert best("lognormal, sigma 2.5") == "geometric" and best("random binary, 1 : 1000") == "arithmetic"
    assert max(t["random binary, 1 : 1000"]["harmonic"]) >= 2 * max(t["random binary, 1 : 1000"]["arithmetic"])


def test_the_solve_references_converge_well_inside_max_iters():
    """the oracle of the device tests' lognormal solve (32 x 48, sigma 1, seed 0) and of its fp32 form"""
    k = cf.lognormal(32, 48, 1.0, 0)
    x, its, flags, hist = cf.Oracle(k).pcg(rtol=1e-10)
    print(f"lognormal 32 x 48: iterations {its}, flags {flags}")
    assert (flags == 1).all() and its.max() <= 60
    ref = cf.homogenize_lognormal(32, 48)
    got = cf.routes_of(x, k)
    assert np.abs(got["K_E"] - ref["K_E"]).max() <= 100 * 1e-10 * np.abs(ref["K_E"]).max()
    assert np.abs(got["K_flux"] - ref["K_flux"]).max() <= 100 * 1e-10 * np.abs(ref["K_E"]).max()
