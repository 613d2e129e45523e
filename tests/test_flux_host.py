"""Element flux fields and effective conductivity, CPU side: the binding table against include/feanet_flux.h, the
argument checks of the entry points (fake addresses: a rejected call launches nothing, and there is no GPU here), the
task rule behind fea_flux_parts, and what the definitions promise, from dense numpy solves alone (flux_ref.py): the
energy and Hill identities, the symmetry of K_eff, homogeneous images and parallel stripes."""
import ctypes
import os
import re

import numpy as np
import pytest

import flux_ref as fx
import phase_ref as pr
from conftest import ROOT

# the node shapes of test_gpu_flux.py (kernel cases, the ladder, the solver level)
SHAPES = [(3, 3), (4, 6), (5, 130), (9, 131), (34, 258), (7, 259), (66, 515), (4097, 33), (65, 65), (49, 97)]


# ----------------------------------------------------------------------------- header, table, symbols
def flux_declarations():
    """(name, return type, [(class, parameter)]) of include/feanet_flux.h, classes as in feanet_amd._lib."""
    src = open(os.path.join(ROOT, "include", "feanet_flux.h")).read()
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


def test_flux_table_matches_header():
    from feanet_amd import _lib
    decls = {d[0]: d for d in flux_declarations()}
    assert list(decls) == ["fea_flux_parts", "fea_flux_f32", "fea_flux_f64", "fea_flux_final"]
    assert sorted(decls) == sorted(_lib.flux_exported_symbols())
    assert list(_lib._FLUX) == ["flux", "fea_flux_parts", "fea_flux_final"]
    table = lambda n: [tuple(p.split()) for p in _lib._FLUX[n]]
    # the typed pair shares one signature: pointers are P whatever they point to, no scalar of type T
    assert decls["fea_flux_f32"][2] == decls["fea_flux_f64"][2] == table("flux")
    assert decls["fea_flux_f32"][1] == decls["fea_flux_f64"][1] == decls["fea_flux_final"][1] == "int"
    assert decls["fea_flux_parts"][1] == "long long" and _lib._FLUX_RES["fea_flux_parts"] is ctypes.c_longlong
    assert decls["fea_flux_parts"][2] == table("fea_flux_parts")
    assert decls["fea_flux_final"][2] == table("fea_flux_final")
    assert table("flux")[-1] == table("fea_flux_final")[-1] == ("P", "stream")
    # a table of its own: the other headers' tables, whose tests pin their key sets, do not hold the names
    others = set(_lib._SIGS) | set(_lib._EXTRA) | set(_lib._FMG) | set(_lib._PHASE)
    assert not others & (set(_lib._FLUX) | {"fea_flux", "flux_final", "flux_parts"})
    held = set(_lib.exported_symbols()) | set(_lib.fmg_exported_symbols()) | set(_lib.phase_exported_symbols())
    assert not held & set(_lib.flux_exported_symbols())
    assert _lib.ABI_VERSION == 3


def test_launch_records_resolve_the_names():
    from feanet_amd import _lib
    kw = dict(u=1, phase=None, ldp=5, k0=1.0, k1=20.0, h=0.5, q=None, ldq=0, cstride=0, qbstride=0, part=2, B=1, H=4,
              W=6, ld=32, bstride=192)
    rec = _lib.launch("flux", **kw)
    assert rec[0] == "flux" and len(rec[1]) == len(_lib._FLUX["flux"]) - 1
    assert _lib.arg(rec, "k1") == 20.0 and _lib.arg(_lib.replace(rec, q=7), "q") == 7
    fin = _lib.launch("flux_final", part=2, per=3, sums=4, B=1)
    assert _lib.arg(fin, "per") == 3
    with pytest.raises(TypeError, match="lacks parameter"):
        _lib.launch("flux", **{k: v for k, v in kw.items() if k != "h"})
    with pytest.raises(TypeError, match="launches on a stream"):
        _lib.launch("flux_parts", H=3, W=3, elem_size=8)


def test_library_exports_the_flux_symbols():
    from feanet_amd import _lib, build
    lib = _lib.lib()
    assert [n for n in _lib.flux_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_flux_f64.argtypes[3] is ctypes.c_double and lib.fea_flux_f32.argtypes[5] is ctypes.c_double
    assert lib.fea_flux_parts.restype is ctypes.c_longlong and lib.fea_flux_final.restype is ctypes.c_int
    assert "flux_ops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "flux_ops.hip"))


# ----------------------------------------------------------------------------- task rule
@pytest.mark.parametrize("esz", [4, 8])
def test_flux_parts_is_the_krylov_task_rule(esz):
    """Row tasks exactly as fea_pcg_parts counts them (the height ONE sample gets); strips over one more column."""
    from feanet_amd import _lib
    lib = _lib.lib()
    for H, W in SHAPES:
        got = int(lib.fea_flux_parts(H, W, esz))
        assert got == fx.flux_parts(H, W, esz), (H, W)
        ns_k, ns_f = -(-(W - 2) // fx.SW[esz]), -(-(W - 1) // fx.SW[esz])
        rows_k = int(lib.fea_pcg_parts(H, W, esz)) // ns_k
        if fx.pick_rb(1, ns_k, H - 2) == fx.pick_rb(1, ns_f, H - 2):
            assert got == ns_f * rows_k, (H, W)
    # the last strip holds the boundary column alone
    assert lib.fea_flux_parts(5, 130, 8) == 2 * lib.fea_pcg_parts(5, 130, 8)
    assert lib.fea_flux_parts(34, 258, 4) == 2 * lib.fea_pcg_parts(34, 258, 4)
    assert lib.fea_flux_parts(4097, 33, esz) == 2048
    for bad in ((2, 9, 8), (9, 2, 8), (9, 9, 2), (9, 9, 16), (0, 0, 4)):
        assert lib.fea_flux_parts(*bad) == -1


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
U, PH, Q, PART, SUMS = 0x100000, 0x800000, 0x1000000, 0x2000000, 0x3000000


def invoke(name, a):
    from feanet_amd import _lib
    sig = _lib._FLUX["flux" if name in ("fea_flux_f32", "fea_flux_f64") else name]
    return getattr(_lib.lib(), name)(*[a[p.split()[1]] for p in sig[:-1]], None)


@pytest.mark.parametrize("suf, esz", [("f32", 4), ("f64", 8)])
def test_flux_rejects_bad_arguments(suf, esz):
    from feanet_amd import _lib
    H, W = 9, 131
    He, We = H - 1, W - 1
    ld, bs = _lib.mg_layout(H, W, esz)
    vec = 16 // esz
    ldq = -(-We // vec) * vec
    good = dict(u=U, phase=PH, ldp=We, k0=1.0, k1=20.0, h=0.25, q=Q, ldq=ldq, cstride=He * ldq,
                qbstride=2 * He * ldq, part=PART, B=2, H=H, W=W, ld=ld, bstride=bs)
    cases = {"u NULL": dict(u=None), "part NULL": dict(part=None), "B 0": dict(B=0), "B < 0": dict(B=-2),
             "H 2": dict(H=2), "W 2": dict(W=2), "ld below the row": dict(ld=ld - 128 // esz),
             "ld not a multiple of the line": dict(ld=ld + 1), "bstride below the sample": dict(bstride=bs - 1),
             "ldp below the row": dict(ldp=We - 1), "ldp 0": dict(ldp=0), "ldp < 0": dict(ldp=-We),
             "ldq below the row": dict(ldq=ldq - vec), "ldq odd": dict(ldq=ldq + 1),
             "cstride below the component": dict(cstride=He * ldq - vec), "cstride odd": dict(cstride=He * ldq + 1),
             "qbstride below the sample": dict(qbstride=2 * He * ldq - vec),
             "qbstride odd": dict(qbstride=2 * He * ldq + 1), "q unaligned": dict(q=Q + esz),
             "q is u": dict(q=U), "q inside u": dict(q=U + 16 * ld), "u inside q": dict(u=Q + 16 * ldq),
             "h 0": dict(h=0.0), "h < 0": dict(h=-0.25), "h inf": dict(h=float("inf")), "h nan": dict(h=float("nan"))}
    for what, change in cases.items():
        assert invoke(f"fea_flux_{suf}", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"
    # the pitch of an image that is not given, and the strides of a field that is not asked for, are not looked at:
    # these fail as arguments only through the NULL part
    assert invoke(f"fea_flux_{suf}", {**good, "phase": None, "ldp": 0, "part": None}) == FEA_EINVAL
    assert invoke(f"fea_flux_{suf}", {**good, "q": None, "ldq": 0, "cstride": 0, "qbstride": 0, "part": None}) == FEA_EINVAL


def test_flux_final_rejects_bad_arguments():
    good = dict(part=PART, per=8, sums=SUMS, B=2)
    cases = {"part NULL": dict(part=None), "sums NULL": dict(sums=None), "per 0": dict(per=0), "per < 0": dict(per=-8),
             "B 0": dict(B=0), "B < 0": dict(B=-1)}
    for what, change in cases.items():
        assert invoke("fea_flux_final", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"


def test_host_layer_refuses_cpu_tensors_and_bad_images():
    import torch
    from feanet_amd import flux, homogenize
    with pytest.raises(RuntimeError, match="MI355X"):
        flux.element_flux(torch.zeros(1, 1, 5, 7, dtype=torch.float64))
    with pytest.raises(TypeError):
        flux.element_flux(np.zeros((1, 1, 5, 7)))
    with pytest.raises(ValueError, match="method"):
        homogenize.effective_conductivity(np.zeros((8, 8), np.uint8), method="jacobi")
    with pytest.raises(ValueError, match=r"\[rows, n\]"):
        homogenize.effective_conductivity(np.zeros((2, 8, 8), np.uint8))
    assert flux.coefficients((1, 0.1)) == (1.0, float(np.float32(0.1)))


# ----------------------------------------------------------------------------- the definitions, by dense solves
M, N = 12, 16
PROPS = [(1, 20), (1, 1000), (20, 1)]


def test_element_matrix_is_the_energy_expression():
    """e = k u_e^T Ke u_e with the reference's element matrix, and K assembled from it equals the float32 table's K
    up to the table's float32 rounding on the rows of the interior nodes (a boundary node's table row also counts
    the elements outside the grid, as phase 0; no solve reads those rows)."""
    Ke = fx.element_matrix()
    assert np.allclose(Ke, Ke.T) and np.abs(Ke.sum(1)).max() < 1e-15
    rng = np.random.default_rng(1)
    u = rng.standard_normal((50, 2, 2))
    e = fx.element_values(u, None, 3.0, 3.0, 0.7, np.float64)["e"][:, 0, 0]
    ue = u.reshape(50, 4)
    assert np.abs(e - 3.0 * np.einsum("bi,ij,bj->b", ue, Ke, ue)).max() < 1e-13
    img = pr.six_discs(M, N)
    Kx, Kt = fx.assemble_exact(img, (1, 20)), fx.assemble_table(img, (1, 20))
    inner = np.zeros((M + 1, N + 1), bool)
    inner[1:-1, 1:-1] = True
    assert np.abs(Kx - Kt)[inner.ravel()].max() < 20 * 4 * 2.0 ** -23 and np.array_equal(Kx, Kx.T)
    assert np.abs(Kx - Kt)[~inner.ravel()].max() > 0.1


@pytest.mark.parametrize("prop", PROPS)
@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_identities_with_the_exact_stiffness(name, prop):
    """Sum e = u^T K u, Hill's identity Sum e = -|V| G . <q>, K_eff symmetric, <g> = G: to 1e-10."""
    r = fx.homogenize(pr.image(name, M, N), prop, exact=True)
    assert np.abs(r["uKu"] - r["energy"]).max() <= 1e-10 * r["energy"].max()
    assert r["hill"].max() <= 1e-10
    assert r["sym"] <= 1e-10
    assert np.abs(r["mean_grad"] - np.eye(2)).max() <= 1e-10


# Measured here with the float32 table and mirrored own-row taps on the six 12 x 16 images (worst image per contrast):
#   prop (1, 20):    Hill 3.19e-07 (offcentre_disc)   symmetry 2.25e-07 (offcentre_disc)
#   prop (1, 1000):  Hill 1.71e-05 (offcentre_disc)   symmetry 1.57e-05 (six_discs)
#   prop (20, 1):    Hill 7.87e-08 (half_plane)       symmetry 4.51e-08 (stripes)
# The table's rows are float32 sums of float32 products a Ke, so K_ij carries a relative error of a few 2^-24 that
# grows with the contrast; the identities hold for the exact K only.  The bounds are four times the worst measured
# value (test_gpu_flux.py holds the device sums to the same Hill bound).
HILL_MEASURED, SYM_MEASURED = 1.71e-05, 1.57e-05
HILL_BOUND, SYM_BOUND = 4 * HILL_MEASURED, 4 * SYM_MEASURED


def test_identities_with_the_float32_table():
    worst = [0.0, 0.0]
    for prop in PROPS:
        at = [0.0, 0.0]
        for name in pr.IMAGES:
            r = fx.homogenize(pr.image(name, M, N), prop)
            at = [max(at[0], r["hill"].max()), max(at[1], r["sym"])]
            assert np.abs(r["mean_grad"] - np.eye(2)).max() <= 1e-10  # the gradient sums telescope: K plays no part
        print(f"prop {prop}: Hill defect {at[0]:.3e}, symmetry defect {at[1]:.3e}")
        worst = [max(worst[0], at[0]), max(worst[1], at[1])]
    assert worst[0] <= HILL_BOUND and worst[1] <= SYM_BOUND
    assert worst[0] > 1e-12          # not the exact K: the float32 table shows


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("value", [0, 1])
def test_homogeneous_image_gives_k_times_identity(value, exact):
    """The linear load cases are the solutions, every element value is the same sum of a few small integers times h:
    exactly k I, exactly zero off the diagonal."""
    r = fx.homogenize(np.full((M, N), value, np.uint8), (1, 20), exact=exact)
    k = (1.0, 20.0)[value]
    assert np.array_equal(r["K_eff"], k * np.eye(2))
    assert np.array_equal(r["mean_grad"], np.eye(2))
    assert np.abs(r["energy"] - k * M * N * (2.0 / N) ** 2).max() <= 1e-12 * k


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("axis", [0, 1])
def test_parallel_stripes_give_the_arithmetic_mean(axis, exact):
    """Stripes along the gradient: the linear field stays the solution of that load case, K_eff[axis, axis] is the
    arithmetic mean of half 1 and half 20; across the stripes it lies between the harmonic and the arithmetic mean."""
    img = fx.parallel_stripes(M, N, axis)
    assert img.mean() == 0.5
    r = fx.homogenize(img, (1, 20), exact=exact)
    assert abs(r["K_eff"][axis, axis] - 10.5) <= 1e-9
    assert 2.0 / (1 / 1.0 + 1 / 20.0) - 1e-9 <= r["K_eff"][1 - axis, 1 - axis] < 10.5
