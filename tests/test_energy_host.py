"""Energy forms of load-case pairs, CPU side: the binding table against include/feanet_energy.h, the argument checks of
the entry points (fake addresses: a rejected call launches nothing, and there is no GPU here), the task rule behind
fea_energy_parts, the numpy reference (energy_ref.py) against flux_ref.py, and what the definitions promise, from
dense numpy solves alone: the energy route equals the flux route, its derivative with respect to a coefficient is
A_p / |V|, and its error is second order in the error of the field."""
import ctypes
import os
import re

import numpy as np
import pytest

import energy_ref as er
import flux_ref as fx
import phase_ref as pr
from conftest import ROOT

# the node shapes of test_gpu_energy.py
SHAPES = [(3, 3), (4, 5), (13, 17), (34, 130), (34, 258), (70, 300), (33, 33), (49, 33), (65, 65)]


# ----------------------------------------------------------------------------- header, table, symbols
def energy_declarations():
    """(name, return type, [(class, parameter)]) of include/feanet_energy.h, classes as in feanet_amd._lib (the
    comparison test_flux_host.py makes for its header)."""
    src = open(os.path.join(ROOT, "include", "feanet_energy.h")).read()
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


def test_energy_table_matches_header():
    from feanet_amd import _lib
    decls = {d[0]: d for d in energy_declarations()}
    assert list(decls) == ["fea_energy_parts", "fea_energy_f32", "fea_energy_f64", "fea_energy_final"]
    assert sorted(decls) == sorted(_lib.energy_exported_symbols())
    assert list(_lib._ENERGY) == ["energy", "fea_energy_parts", "fea_energy_final"]
    table = lambda n: [tuple(p.split()) for p in _lib._ENERGY[n]]
    assert decls["fea_energy_f32"][2] == decls["fea_energy_f64"][2] == table("energy")
    assert decls["fea_energy_f32"][1] == decls["fea_energy_f64"][1] == decls["fea_energy_final"][1] == "int"
    assert decls["fea_energy_parts"][1] == "long long" and _lib._ENERGY_RES["fea_energy_parts"] is ctypes.c_longlong
    assert decls["fea_energy_parts"][2] == table("fea_energy_parts")
    assert decls["fea_energy_final"][2] == table("fea_energy_final")
    assert table("energy")[-1] == table("fea_energy_final")[-1] == ("P", "stream")
    # a table of its own: the other headers' tables, whose tests pin their key sets, do not hold the names
    others = set(_lib._SIGS) | set(_lib._EXTRA) | set(_lib._FMG) | set(_lib._PHASE) | set(_lib._FLUX)
    assert not others & (set(_lib._ENERGY) | {"fea_energy", "energy_final", "energy_parts"})
    held = set(_lib.exported_symbols()) | set(_lib.fmg_exported_symbols()) | set(_lib.phase_exported_symbols()) | \
        set(_lib.flux_exported_symbols())
    assert not held & set(_lib.energy_exported_symbols())
    assert _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "feanet_energy.h")).read()
    assert re.search(r"#define\s+FEA_ENERGY_NSUMS\s+6\b", src) and er.NSUMS == 6


def test_launch_records_resolve_the_names():
    from feanet_amd import _lib
    kw = dict(u=1, v=2, phase=None, ldp=5, dens=None, ldd=0, cstride=0, dbstride=0, part=3, B=1, H=4, W=6, ld=32,
              ubstride=192, vbstride=192)
    rec = _lib.launch("energy", **kw)
    assert rec[0] == "energy" and len(rec[1]) == len(_lib._ENERGY["energy"]) - 1
    assert _lib.arg(rec, "vbstride") == 192 and _lib.arg(_lib.replace(rec, dens=7), "dens") == 7
    assert _lib.arg(_lib.launch("energy_final", part=2, per=3, sums=4, B=1), "per") == 3
    with pytest.raises(TypeError, match="lacks parameter"):
        _lib.launch("energy", **{k: v for k, v in kw.items() if k != "v"})
    with pytest.raises(TypeError, match="launches on a stream"):
        _lib.launch("energy_parts", H=3, W=3, elem_size=8)


def test_library_exports_the_energy_symbols():
    from feanet_amd import _lib, build
    lib = _lib.lib()
    assert [n for n in _lib.energy_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_energy_f64.argtypes[3] is ctypes.c_longlong and len(lib.fea_energy_f32.argtypes) == 16
    assert lib.fea_energy_parts.restype is ctypes.c_longlong and lib.fea_energy_final.restype is ctypes.c_int
    assert "energy_ops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "energy_ops.hip"))


# ----------------------------------------------------------------------------- task rule
@pytest.mark.parametrize("esz", [4, 8])
def test_energy_parts_is_the_flux_task_rule(esz):
    """Strips over node columns 1 .. W-1, row tasks of the height ONE sample gets: fea_flux_parts' rule, restated in
    energy_ref.energy_parts."""
    from feanet_amd import _lib
    lib = _lib.lib()
    for H, W in SHAPES + [(4097, 33)]:
        got = int(lib.fea_energy_parts(H, W, esz))
        assert got == er.energy_parts(H, W, esz) == int(lib.fea_flux_parts(H, W, esz)), (H, W)
    # W - 2 a whole strip: the last strip holds the boundary column alone
    assert er.energy_parts(34, 130, 8) == 2 * er.energy_parts(34, 129, 8)
    assert er.energy_parts(34, 258, 4) == 2 * er.energy_parts(34, 257, 4)
    assert lib.fea_energy_parts(70, 300, 8) == 3 * 34 and lib.fea_energy_parts(3, 3, esz) == 1
    for bad in ((2, 9, 8), (9, 2, 8), (9, 9, 2), (9, 9, 16), (0, 0, 4)):
        assert lib.fea_energy_parts(*bad) == -1


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
U, V, PH, DENS, PART, SUMS = 0x100000, 0x400000, 0x800000, 0x1000000, 0x2000000, 0x3000000


def invoke(name, a):
    from feanet_amd import _lib
    sig = _lib._ENERGY["energy" if name in ("fea_energy_f32", "fea_energy_f64") else name]
    return getattr(_lib.lib(), name)(*[a[p.split()[1]] for p in sig[:-1]], None)


def check_energy_refusals(suf, esz):
    """every FEA_EINVAL case of fea_energy_* (also run by test_gpu_energy.py, where a launch would be real)"""
    from feanet_amd import _lib
    H, W = 9, 131
    He, We = H - 1, W - 1
    ld, bs = _lib.mg_layout(H, W, esz)
    vec = 16 // esz
    ldd = -(-We // vec) * vec
    good = dict(u=U, v=V, phase=PH, ldp=We, dens=DENS, ldd=ldd, cstride=He * ldd, dbstride=3 * He * ldd, part=PART,
                B=2, H=H, W=W, ld=ld, ubstride=bs, vbstride=bs)
    cases = {"u NULL": dict(u=None), "v NULL": dict(v=None), "part NULL": dict(part=None), "B 0": dict(B=0),
             "B < 0": dict(B=-2), "H 2": dict(H=2), "W 2": dict(W=2), "ld below the row": dict(ld=ld - 128 // esz),
             "ld not a multiple of the line": dict(ld=ld + 1), "ubstride below the sample": dict(ubstride=bs - 1),
             "vbstride below the sample": dict(vbstride=bs - 1), "vbstride 0": dict(vbstride=0),
             "ldp below the row": dict(ldp=We - 1), "ldp 0": dict(ldp=0), "ldp < 0": dict(ldp=-We),
             "ldd below the row": dict(ldd=ldd - vec), "ldd odd": dict(ldd=ldd + 1),
             "cstride below the component": dict(cstride=He * ldd - vec), "cstride odd": dict(cstride=He * ldd + 1),
             "dbstride below three components": dict(dbstride=3 * He * ldd - vec),
             "dbstride odd": dict(dbstride=3 * He * ldd + 1), "dens unaligned": dict(dens=DENS + esz),
             "dens is u": dict(dens=U), "dens is v": dict(dens=V), "dens inside v": dict(dens=V + 16 * ld),
             "u inside dens": dict(u=DENS + 16 * ldd), "v inside dens": dict(v=DENS + 16 * ldd)}
    for what, change in cases.items():
        assert invoke(f"fea_energy_{suf}", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"
    # the pitch of an image that is not given, and the strides of a field that is not asked for, are not looked at;
    # u == v and overlapping u, v are allowed: these fail as arguments only through the NULL part
    for ok in (dict(phase=None, ldp=0), dict(dens=None, ldd=0, cstride=0, dbstride=0), dict(v=U),
               dict(v=U + bs * esz, B=1)):
        assert invoke(f"fea_energy_{suf}", {**good, **ok, "part": None}) == FEA_EINVAL
    good = dict(part=PART, per=8, sums=SUMS, B=2)
    cases = {"part NULL": dict(part=None), "sums NULL": dict(sums=None), "per 0": dict(per=0), "per < 0": dict(per=-8),
             "B 0": dict(B=0), "B < 0": dict(B=-1)}
    for what, change in cases.items():
        assert invoke("fea_energy_final", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"


@pytest.mark.parametrize("suf, esz", [("f32", 4), ("f64", 8)])
def test_energy_rejects_bad_arguments(suf, esz):
    check_energy_refusals(suf, esz)


def test_host_layer_refuses_cpu_tensors_and_bad_routes():
    import torch
    from feanet_amd import flux, homogenize
    with pytest.raises(RuntimeError, match="MI355X"):
        flux.energy_forms(torch.zeros(1, 1, 5, 7, dtype=torch.float64))
    with pytest.raises(TypeError):
        flux.energy_forms(np.zeros((1, 1, 5, 7)))
    with pytest.raises(ValueError, match="route"):
        homogenize.effective_conductivity(np.zeros((8, 8), np.uint8), route="hill")
    with pytest.raises(ValueError, match=r"shape \[2\]"):
        homogenize.effective_conductivity_torch(np.zeros((8, 8), np.uint8), torch.ones(3))
    assert "float32-rounded" in homogenize.effective_conductivity_torch.__doc__
    assert homogenize.EnergyHomogenizationResult._fields == ("K_eff", "dK_dprop", "sensitivity", "K_eff_flux",
                                                             "route_gap", "iterations", "flags", "converged")
    assert flux.EnergyForms._fields == ("A", "density")


# ----------------------------------------------------------------------------- the numpy reference
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_reference_agrees_with_flux_ref(dt):
    """k0 A_0[uu] + k1 A_1[uu] is flux_ref's energy sum (the same expression, k inside or outside the element value:
    within the field bound of the sum); d is symmetric in its arguments bit for bit, and d(u, u) is the uu value."""
    rng = np.random.default_rng(2)
    u, v = rng.standard_normal((2, 3, 13, 17)).astype(dt)
    img = (rng.random((12, 16)) < 0.4).astype(np.uint8)
    k0, k1 = 1.0, 20.0
    for wide in (False, True):
        a, b = er.element_values(u, v, dt, wide), er.element_values(v, u, dt, wide)
        assert np.array_equal(a["uv"], b["uv"]) and np.array_equal(a["uu"], b["vv"]) and np.array_equal(a["vv"], b["uu"])
        same = er.element_values(u, u, dt, wide)
        assert np.array_equal(same["uu"], same["uv"]) and np.array_equal(same["uv"], same["vv"])
        assert np.array_equal(same["uu"], a["uu"]) and a["uu"].dtype == (np.float64 if wide else dt)
    s = er.sums_of(er.element_values(u, v, dt, wide=True), img)
    e = fx.sums_of(fx.element_values(u, img, k0, k1, 0.5, dt, wide=True))[:, 4]
    S = fx.companions(u, img, k0, k1, 0.5, dt)["e"].reshape(3, -1).sum(1)
    assert (np.abs(k0 * s[:, 0] + k1 * s[:, 1] - e) <= 8 * 2.0 ** -53 * S).all()
    none = er.sums_of(er.element_values(u, v, dt, wide=True), None)
    assert (none[:, 1::2] == 0).all() and np.allclose(none[:, 0::2], s[:, 0::2] + s[:, 1::2], rtol=1e-13)
    # the companions bound the values
    C = er.companions(u, v, dt)
    vals = er.element_values(u, v, dt, wide=True)
    assert all((np.abs(vals[n]) <= C[n]).all() for n in er.NAMES)


# ----------------------------------------------------------------------------- the definitions, by dense solves
M, N = 12, 16
PROPS = [(1, 20), (1, 1000), (20, 1)]
REL = 1e-4


def fd_tolerance(r, prop):
    """Central differences with the step s = REL k1 carry the truncation error s^2 |f'''| / 6.  K_eff(k1) at fixed k0
    is a Stieltjes function of t = k1, a positive sum of terms a t / (b + t); for one term t^2 |f'''| / 6 =
    a b t^2 / (b + t)^4 <= (4 / 27) f / t, so the error of the difference quotient is within (4 / 27) REL^2 f / k1.
    The roundoff of the quotient, about 2^-53 f / (REL k1) times the conditioning of the dense solve, stays below the
    rest of REL^2 max|K_eff| / k1 = 1e-8 max|K_eff| / k1."""
    return REL ** 2 * np.abs(r["K_E"]).max() / prop[1]


@pytest.mark.parametrize("prop", PROPS)
@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_identities_with_the_exact_stiffness(name, prop):
    """K_E = K_eff of the flux route to 1e-10; K_E exactly symmetric; dK_E / dk1 = A_1 / |V| by central differences;
    K_E = k0 dK[0] + k1 dK[1] (Euler: K_E is homogeneous of degree one)."""
    img = pr.image(name, M, N)
    r = er.homogenize_image(name, M, N, prop, exact=True)
    scale = np.abs(r["K_E"]).max()
    assert np.abs(r["K_E"] - r["K_flux"]).max() <= 1e-10 * scale
    assert r["K_E"][0, 1] == r["K_E"][1, 0] and r["gap"] <= 1e-10
    cd, cd_flux = er.central_difference(img, prop, REL, exact=True)
    tol = fd_tolerance(r, prop)
    err = np.abs(cd - r["dK"][1]).max()
    print(f"{name} {prop}: |central difference - A_1 / |V|| = {err:.2e} (allowed {tol:.2e})")
    assert err <= tol and np.abs(cd_flux - r["dK"][1]).max() <= tol + 1e-10 * scale / (REL * prop[1])


# Measured here with the float32 table on the six 12 x 16 images (worst image per contrast; the central difference
# divides by the step the float32-rounded coefficients take, and is given in units of max|K_eff| / k1):
#   prop (1, 20):    |K_E - K_flux| 3.19e-07 (offcentre_disc)    central difference 1.43e-07 (random_elements)
#   prop (1, 1000):  |K_E - K_flux| 1.71e-05 (offcentre_disc)    central difference 2.17e-07 (six_discs)
#   prop (20, 1):    |K_E - K_flux| 8.13e-08 (random_elements)   central difference 2.76e-08 (random_elements)
# The difference of the two routes on the diagonal IS the Hill defect of test_flux_host.py (same numbers): the table's
# K differs from the exact element sum by float32 rounding, and the stationarity that makes the routes agree holds
# for the table's K only.  The bounds are four times the worst measured value, as there.
TABLE_MEASURED = {(1, 20): (3.19e-07, 1.43e-07), (1, 1000): (1.71e-05, 2.17e-07), (20, 1): (8.13e-08, 2.76e-08)}


@pytest.mark.parametrize("prop", PROPS)
def test_identities_with_the_float32_table(prop):
    worst = [0.0, 0.0]
    for name in pr.IMAGES:
        img = pr.image(name, M, N)
        r = er.homogenize_image(name, M, N, prop)
        scale = np.abs(r["K_E"]).max()
        cd, _ = er.central_difference(img, prop, REL, exact=False)
        worst = [max(worst[0], np.abs(r["K_E"] - r["K_flux"]).max() / scale),
                 max(worst[1], np.abs(cd - r["dK"][1]).max() / (scale / prop[1]))]
        assert r["K_E"][0, 1] == r["K_E"][1, 0]
    print(f"prop {prop}: routes differ by {worst[0]:.3e}, central difference off by {worst[1]:.3e} max|K_eff| / k1")
    assert worst[0] <= 4 * TABLE_MEASURED[prop][0] and worst[1] <= 4 * TABLE_MEASURED[prop][1]
    assert worst[0] > 1e-12          # not the exact K: the float32 table shows


@pytest.mark.parametrize("prop", PROPS)
@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_energy_route_is_second_order(name, prop):
    """An interior perturbation dv of the exact discrete solution moves K_E by a(dv_i, dv_j) / |V| alone: scaling dv
    by 1/10 reduces the K_E error by between 50 and 200 times, the flux route's by between 5 and 20 times; on the
    diagonal the perturbed value lies above."""
    img = pr.image(name, M, N)
    r = er.homogenize_image(name, M, N, prop, exact=True)
    k0, k1 = er.coefficients(prop, True)
    dv = er.interior_perturbation(M, N, 3) * np.abs(r["u"]).max()
    eE, eF = [], []
    for eps in (1e-3, 1e-4):
        p = er.routes(r["u"] + eps * dv, img, k0, k1)
        eE.append(np.abs(p["K_E"] - r["K_E"]).max())
        eF.append(np.abs(p["K_flux"] - r["K_flux"]).max())
        assert (np.diag(p["K_E"] - r["K_E"]) > 0).all()
        quad = eps * eps * er.routes(dv, img, k0, k1)["K_E"]
        assert np.abs(p["K_E"] - r["K_E"] - quad).max() <= 1e-9 * np.abs(quad).max() + 1e-13 * np.abs(r["K_E"]).max()
    print(f"{name} {prop}: K_E error falls {eE[0] / eE[1]:.1f} times, flux route {eF[0] / eF[1]:.1f} times")
    assert 50 <= eE[0] / eE[1] <= 200 and 5 <= eF[0] / eF[1] <= 20


def test_homogeneous_image_and_euler_identity():
    """k I from either phase, dK_dprop = I on the phase present and 0 on the other; K_E = sum_p k_p dK_dprop[p]."""
    for value in (0, 1):
        r = er.homogenize(np.full((M, N), value, np.uint8), (1, 20))
        k = (1.0, 20.0)[value]
        assert np.abs(r["K_E"] - k * np.eye(2)).max() <= 1e-12 * k
        assert np.abs(r["dK"][value] - np.eye(2)).max() <= 1e-12 and (r["dK"][1 - value] == 0).all()
    r = er.homogenize_image("six_discs", M, N, (1, 20))
    assert np.array_equal(r["K_E"], 1.0 * r["dK"][0] + 20.0 * r["dK"][1])
