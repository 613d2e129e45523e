"""Two-material set-up from an element phase image, CPU side: the padded pattern rule against the reference's maps,
the symmetry (mirror) property on every level of the six study images, the coarsening thresholds, the binding table
against include/feanet_phase.h, the argument checks of the two entry points (fake addresses: a rejected call launches
nothing, and there is no GPU here) and the constructors' refusals that come before the device is touched."""
import os
import re

import numpy as np
import pytest

import phase_ref as pr
from conftest import ROOT

PROPS = [(1, 20), (20, 1), (1, 1000)]
RULES = ["majority", "stiff"]


# ----------------------------------------------------------------------------- the padded rule
@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("N", [5, 9, 17, 33, 65, 129])
def test_padded_map_contains_the_reference(N, shape):
    from feanet_amd import mesh_setup as ms
    got = ms.phase_pattern_map(ms.element_phase(N, shape))
    assert got.dtype == np.uint8 and got.shape == (N, N)
    assert np.array_equal(got, ms.interface_pattern_map(N, shape))


def test_pattern_rule_by_hand():
    """Every node's pattern spelled out from PATTERN_BITS, boundary nodes with phase 0 outside; bool, int and uint8
    images agree."""
    from feanet_amd import mesh_setup as ms
    rng = np.random.default_rng(3)
    ph = (rng.random((5, 7)) < 0.5).astype(np.int64)
    got = ms.phase_pattern_map(ph)

    def el(r, c):
        return int(ph[r, c]) if 0 <= r < 5 and 0 <= c < 7 else 0
    for r in range(6):
        for c in range(8):
            bits = [el(r - 1, c), el(r - 1, c - 1), el(r, c - 1), el(r, c)]
            assert list(ms.PATTERN_BITS[got[r, c]]) == bits, (r, c)
    assert np.array_equal(ms.phase_pattern_map(ph.astype(bool)), got)
    assert np.array_equal(ms.phase_pattern_map(ph.astype(np.uint8)), got)
    assert np.array_equal(ms.phase_pattern_map(np.ones((1, 1), np.int8)), [[2, 3], [4, 5]])


@pytest.mark.parametrize("m, n", [(64, 64), (48, 96)])
@pytest.mark.parametrize("name", list(pr.IMAGES))
def test_mirror_mismatches_are_zero_on_every_level(name, m, n):
    from feanet_amd import mesh_setup as ms
    img = pr.image(name, m, n)
    assert img.shape == (m, n) and 0 < img.sum() < img.size
    L = pr.default_levels(m, n)
    assert (m >> (L - 1), n >> (L - 1)) in ((2, 2), (3, 6))
    for prop in PROPS:
        ktab = ms.stencil_table(prop)
        for rule in RULES:
            imgs, maps = pr.hierarchy(img, L, prop, rule)
            assert len(imgs) == L and len(maps) == L
            for p in imgs:
                pid = maps[(p.shape[0] + 1, p.shape[1] + 1)]
                assert ms.stencil_mirror_mismatches(ktab, pid) == 0, (prop, rule, p.shape)


def test_boundary_pattern_zero_has_mismatches():
    """The reference's rule (pattern 0 on the boundary nodes) on the half plane: the assertion can fire."""
    from feanet_amd import mesh_setup as ms
    pid = ms.phase_pattern_map(pr.half_plane(64, 64))
    assert pid[0].any() and pid[-1].any() and pid[:, 0].any()
    forced = pid.copy()
    forced[0] = forced[-1] = 0
    forced[:, 0] = forced[:, -1] = 0
    for prop in PROPS:
        assert ms.stencil_mirror_mismatches(ms.stencil_table(prop), forced) > 0
    assert ms.stencil_mirror_mismatches(ms.stencil_table((1, 1)), forced) == 0  # equal coefficients: one stencil


# ----------------------------------------------------------------------------- coarsening
def test_min_count_table():
    from feanet_amd import mesh_setup as ms
    table = {("stiff", (1, 20)): 1, ("stiff", (20, 1)): 4, ("majority", (1, 20)): 2, ("majority", (20, 1)): 3,
             ("stiff", (1, 1000)): 1, ("majority", (1, 1000)): 2,
             ("stiff", (1, 1)): 4, ("majority", (1, 1)): 3, ("stiff", (5.0, 5.0)): 4, ("majority", (5.0, 5.0)): 3}
    for (rule, prop), want in table.items():
        assert ms.phase_min_count(prop, rule) == want, (rule, prop)
    for rule in ("sample", "soft", "", None):
        with pytest.raises(ValueError, match="rule"):
            ms.phase_min_count((1, 20), rule)


def test_coarsen_counts_children():
    from feanet_amd import mesh_setup as ms
    # one coarse element per number of phase-1 children 0..4, all placements of them
    cells = [np.array(b, np.uint8).reshape(2, 2) for b in np.ndindex(2, 2, 2, 2)]
    fine = np.block([cells])
    assert fine.shape == (2, 32)
    for k in (1, 2, 3, 4):
        got = ms.coarsen_phase(fine, k)
        assert got.dtype == np.uint8 and got.shape == (1, 16)
        assert np.array_equal(got[0], [int(c.sum() >= k) for c in cells])
    for k in (0, 5):
        with pytest.raises(ValueError, match="min_count"):
            ms.coarsen_phase(fine, k)
    with pytest.raises(ValueError, match="coarsening"):
        ms.coarsen_phase(np.zeros((3, 4), np.uint8), 2)


def test_hierarchy_shapes_and_refusals():
    from feanet_amd import mesh_setup as ms
    img = pr.six_discs(48, 96)
    imgs = ms.phase_hierarchy(img, 5, (1, 20), "stiff")
    assert [p.shape for p in imgs] == [(48, 96), (24, 48), (12, 24), (6, 12), (3, 6)]
    assert np.array_equal(imgs[0], img) and all(p.dtype == np.uint8 for p in imgs)
    # "stiff" at prop[1] > prop[0]: a coarse element is 1 iff any descendant is
    assert np.array_equal(imgs[2], img.reshape(12, 4, 24, 4).max(axis=(1, 3)))
    with pytest.raises(ValueError, match="levels"):
        ms.phase_hierarchy(img, 6)
    with pytest.raises(ValueError, match="0 or 1"):
        ms.phase_hierarchy(img + 1, 2)
    with pytest.raises(ValueError, match="dtype"):
        ms.phase_pattern_map(img.astype(np.float32))
    with pytest.raises(ValueError, match=r"\[m, n\]"):
        ms.phase_pattern_map(img[None])


# ----------------------------------------------------------------------------- header, table, symbols
def phase_declarations():
    """(name, return type, [(class, parameter)]) of include/feanet_phase.h, classes as in feanet_amd._lib."""
    src = open(os.path.join(ROOT, "include", "feanet_phase.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = []
    for ret, name, params in re.findall(r"\b(int|size_t|long long)\s+(fea_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        fields = []
        for p in " ".join(params.split()).split(","):
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", p.strip())
            ctype, pname = m.group(1).strip(), m.group(2)
            fields.append(("P" if "*" in ctype else {"int": "I", "long long": "LL"}[ctype], pname))
        decls.append((name, ret, fields))
    return decls


def test_phase_table_matches_header():
    from feanet_amd import _lib
    decls = phase_declarations()
    assert [d[0] for d in decls] == list(_lib._PHASE) == _lib.phase_exported_symbols()
    assert [d[0] for d in decls] == ["fea_phase_pattern_map", "fea_phase_coarsen"]
    for name, ret, fields in decls:
        assert ret == "int"
        assert [tuple(p.split()) for p in _lib._PHASE[name]] == fields, name
        assert fields[-1] == ("P", "stream")
    # a table of its own: the tables of feanet_hip.h and feanet_fmg.h, whose tests pin their key sets, do not hold them
    assert not any(n in _lib._EXTRA or n in _lib.exported_symbols() or n in _lib.fmg_exported_symbols()
                   for n in _lib._PHASE)
    assert _lib.ABI_VERSION == 3


def test_library_exports_the_phase_symbols():
    import ctypes
    from feanet_amd import _lib
    lib = _lib.lib()
    assert [n for n in _lib.phase_exported_symbols() if not hasattr(lib, n)] == []
    assert lib.fea_phase_coarsen.argtypes[-2] is ctypes.c_int and lib.fea_phase_coarsen.restype is ctypes.c_int
    assert lib.fea_phase_pattern_map.argtypes[1] is ctypes.c_longlong


def test_phase_source_is_in_the_build_list():
    from feanet_amd import build
    assert "phase_ops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "phase_ops.hip"))


# ----------------------------------------------------------------------------- argument checks
FEA_EINVAL = -1
SRC, DST = 0x10000, 0x80000


def invoke(name, a):
    from feanet_amd import _lib
    return getattr(_lib.lib(), name)(*[a[p.split()[1]] for p in _lib._PHASE[name][:-1]], None)


def test_pattern_map_rejects_bad_arguments():
    good = dict(phase=SRC, ldp=6, He=4, We=6, pid=DST, ldpid=7)
    cases = {"phase NULL": dict(phase=None), "pid NULL": dict(pid=None), "He 0": dict(He=0), "We 0": dict(We=0),
             "He < 0": dict(He=-4), "We < 0": dict(We=-6), "ldp below the row": dict(ldp=5), "ldp 0": dict(ldp=0),
             "ldp < 0": dict(ldp=-6), "ldpid below the node row": dict(ldpid=6), "ldpid 0": dict(ldpid=0)}
    for what, change in cases.items():
        assert invoke("fea_phase_pattern_map", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"
    # the smallest image is not refused for its size: 1 x 1 with a NULL operand fails as an argument only
    assert invoke("fea_phase_pattern_map", dict(phase=SRC, ldp=1, He=1, We=1, pid=None, ldpid=2)) == FEA_EINVAL


def test_coarsen_rejects_bad_arguments():
    good = dict(fine=SRC, ldf=6, He=4, We=6, coarse=DST, ldc=3, min_count=2)
    cases = {"fine NULL": dict(fine=None), "coarse NULL": dict(coarse=None), "He 1": dict(He=1), "We 1": dict(We=1),
             "He 0": dict(He=0), "We 0": dict(We=0), "He < 0": dict(He=-4), "odd He": dict(He=5),
             "odd We": dict(We=5), "ldf below the row": dict(ldf=5), "ldf 0": dict(ldf=0),
             "ldc below the coarse row": dict(ldc=2), "ldc 0": dict(ldc=0), "min_count 0": dict(min_count=0),
             "min_count 5": dict(min_count=5), "min_count < 0": dict(min_count=-1), "in place": dict(coarse=SRC)}
    for what, change in cases.items():
        assert invoke("fea_phase_coarsen", {**good, **change}) == FEA_EINVAL, f"{what} was not rejected"
    assert invoke("fea_phase_coarsen", dict(fine=SRC, ldf=2, He=2, We=2, coarse=None, ldc=1, min_count=4)) == FEA_EINVAL


# ----------------------------------------------------------------------------- constructors
def test_constructors_refuse_before_the_device_is_touched():
    """Nothing here reaches the device: each argument set is refused with a ValueError that names what is wrong."""
    import torch
    from feanet_amd import MultigridSolver, PCGSolver
    from feanet_amd.dd import DDSolver
    img = pr.half_plane(64, 64)
    for cls in (MultigridSolver, PCGSolver):
        with pytest.raises(ValueError, match="interface"):
            cls(64, phase=img)  # problem="poisson"
        with pytest.raises(ValueError, match="interface"):
            cls(64, phase_levels=[img])
        with pytest.raises(ValueError, match="shape"):
            cls(64, problem="interface", phase=img, shape=1)
        with pytest.raises(ValueError, match="the phase image is"):
            cls(64, problem="interface", phase=img[:32])
        with pytest.raises(ValueError, match="the phase image is"):
            cls(64, rows=32, problem="interface", phase=img)
        with pytest.raises(ValueError, match="the phase image is"):
            cls(96, rows=48, problem="interface", phase=pr.half_plane(96, 48))  # [rows, n], not [n, rows]
        with pytest.raises(ValueError, match="one value per element"):
            cls(64, problem="interface", phase=img.reshape(-1))
        with pytest.raises(ValueError, match="0 or 1"):
            cls(64, problem="interface", phase=img * 2)
        with pytest.raises(ValueError, match="0 or 1"):
            cls(64, problem="interface", phase=torch.from_numpy(img.astype(np.int64)) - 1)
        with pytest.raises(ValueError, match="dtype"):
            cls(64, problem="interface", phase=img.astype(np.float64))
        with pytest.raises(ValueError, match="coarsen"):
            cls(64, problem="interface", phase=img, coarsen="soft")
        with pytest.raises(ValueError, match="coarsen"):
            cls(64, problem="interface", coarsen="sample")
    with pytest.raises(ValueError, match="pid_maps"):
        MultigridSolver(64, problem="interface", phase=img, pid_maps=[np.zeros((65, 65), np.uint8)])
    with pytest.raises(ValueError, match="phase"):
        DDSolver(64, 64, 0, 1, problem="interface", phase=img)
