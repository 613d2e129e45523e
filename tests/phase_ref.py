"""numpy side of the element-phase-image tests (test_phase_host.py, test_gpu_phase.py); a helper, not a test, in the
role of fmg_ref.py.

The six study images of DESIGN's phase-image section as functions of (m, n) elements and a seed; the numpy hierarchy
-> {(H, W): pattern map} -> OracleMultigrid(pids=...); the oracle with HRelax sweeps; the full-multigrid driver of
fmg_ref.py on the same maps; and a numpy conjugate gradient (Level.K with boundary rows and columns zeroed as the
operator, OracleMultigrid.step(0, r) as the preconditioner, dot products in float64, the device's per-sample
freeze), in full precision or with an fp32 cycle inside fp64 recurrences."""
import numpy as np

import fmg_ref as fr
from oracle import feanet_oracle as orc


# ----------------------------------------------------------------------------- the six images
def _centres(m, n):
    y, x = np.mgrid[0:m, 0:n] + 0.5
    return y, x


def offcentre_disc(m, n, seed=0):
    y, x = _centres(m, n)
    return ((x - 0.3 * n) ** 2 + (y - 0.6 * m) ** 2 < (0.22 * min(m, n)) ** 2).astype(np.uint8)


def six_discs(m, n, seed=0):
    y, x = _centres(m, n)
    rng = np.random.default_rng([seed, m, n])
    img = np.zeros((m, n), bool)
    for _ in range(6):
        cx, cy = rng.uniform(0.15, 0.85) * n, rng.uniform(0.15, 0.85) * m
        r = rng.uniform(0.05, 0.14) * min(m, n)
        img |= (x - cx) ** 2 + (y - cy) ** 2 < r * r
    return img.astype(np.uint8)


def stripes(m, n, seed=0):
    """vertical stripes 8 elements wide (they reach the top and bottom boundaries)"""
    y, x = _centres(m, n)
    return ((x // 8) % 2).astype(np.uint8)


def checkerboard(m, n, seed=0):
    """squares of 4 x 4 elements"""
    y, x = _centres(m, n)
    return (((x // 4) + (y // 4)) % 2).astype(np.uint8)


def half_plane(m, n, seed=0):
    """x < 0.4 n: phase 1 touches three sides of the boundary"""
    y, x = _centres(m, n)
    return (x < 0.4 * n).astype(np.uint8)


def random_elements(m, n, seed=0):
    """30 % of the elements phase 1, independently"""
    return (np.random.default_rng([seed, m, n, 30]).random((m, n)) < 0.3).astype(np.uint8)


IMAGES = {"offcentre_disc": offcentre_disc, "six_discs": six_discs, "stripes": stripes,
          "checkerboard": checkerboard, "half_plane": half_plane, "random_elements": random_elements}


def image(name, m, n, seed=0):
    return IMAGES[name](m, n, seed)


# ----------------------------------------------------------------------------- hierarchy, oracle
def default_levels(m, n):
    """MultigridSolver's level count with `rows` given: the most levels with >= 2 intervals each way."""
    L = 1
    while n % (1 << L) == 0 and m % (1 << L) == 0 and (n >> L) >= 2 and (m >> L) >= 2:
        L += 1
    return L


def maps_of(images):
    """{(H, W): pattern map} of a list of per-level phase images, for oracle Level(pids=...)."""
    from feanet_amd import mesh_setup as ms
    return {(p.shape[0] + 1, p.shape[1] + 1): ms.phase_pattern_map(p) for p in images}


def hierarchy(phase, L, prop=(1, 20), rule="majority"):
    """(per-level images, {(H, W): map}) by the numpy functions of feanet_amd.mesh_setup."""
    from feanet_amd import mesh_setup as ms
    imgs = ms.phase_hierarchy(phase, L, prop, rule)
    return imgs, maps_of(imgs)


def oracle(phase, L, dt, prop=(1, 20), rule="majority", images=None, **kw):
    """OracleMultigrid on the image's hierarchy (or on the explicit per-level `images`)."""
    m, n = np.shape(phase)
    pids = maps_of(images) if images is not None else hierarchy(phase, L, prop, rule)[1]
    return orc.OracleMultigrid(n, "interface", dt, levels=L, prop=prop, rows=m, pids=pids, **kw)


def with_hrelax(mg, hw):
    """The oracle with every sweep an HRelax (M-FEANet-mg_test.ipynb:147-155), as tests/test_gpu_hnet.py builds it."""
    for l in mg.levels:
        l.sweep = (lambda ll, o: (lambda v, ff: (lambda j: j + orc.hnet(j - v, ll.geo, hw))(o(v, ff))))(l, l.sweep)
    return mg


def fmg(phase, L, f, bc, prop=(1, 20), rule="majority", **kw):
    """fmg_ref.fmg on the image's maps: its sub-hierarchies pick their levels' maps by (H, W)."""
    m, n = np.shape(phase)
    return fr.fmg(n, f, bc, levels=L, rows=m, problem="interface", pids=hierarchy(phase, L, prop, rule)[1],
                  prop=prop, **kw)


def stationary_cycles(mg, f, rtol, max_cycles):
    """Cycles of the oracle's stationary iteration from zero until ||r|| <= rtol ||r0|| (max_cycles if never)."""
    v = np.zeros_like(f)
    r0 = mg.residual_norm(v, f)
    for k in range(1, max_cycles + 1):
        v = mg.step(v, f)
        if (mg.residual_norm(v, f) <= rtol * r0).all():
            return k
    return max_cycles


# ----------------------------------------------------------------------------- numpy PCG
def dot64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).reshape(a.shape[0], -1).sum(1)


def scale_of(rn):
    """s_b of mixed precision: 2^-floor(log2 ||r0||); 1 for a zero or non-finite norm."""
    rn = np.asarray(rn, np.float64)
    ok = np.isfinite(rn) & (rn > 0)
    return np.where(ok, 2.0 ** -np.floor(np.log2(np.where(ok, rn, 1.0))), 1.0)


def numpy_pcg(mg_o, x0, f, iters, dt, eps=0.0, rtol=None, mg32=None):
    """CG in `dt` on mg_o's finest K, preconditioned by mg_o.step(0, r) — or, with mg32 (an fp32 oracle of the same
    hierarchy; dt float64), by mg32.step(0, float32(r s_b)).  Returns the iterates after each iteration, the history
    and the per-sample iteration counts."""
    lv = mg_o.levels[0]
    geo = np.zeros((lv.H, lv.W), dt)
    geo[1:-1, 1:-1] = 1
    x = np.asarray(x0, dt).copy()
    B = x.shape[0]
    r = ((np.asarray(f, dt) - lv.K(x)) * geo).astype(dt)
    p = np.zeros_like(x)
    hist = [np.sqrt(dot64(r, r))]
    sb = scale_of(hist[0])
    thresh = rtol * hist[0] if rtol is not None else np.full(B, eps)
    done = hist[0] <= thresh
    iters_b = np.zeros(B, np.int64)
    rz_prev = np.ones(B)
    xs = []
    for it in range(iters):
        if mg32 is None:
            z = np.asarray(mg_o.step(np.zeros_like(r), r), dt)
        else:
            r32 = (r * sb[:, None, None]).astype(np.float32)
            z = np.asarray(mg32.step(np.zeros_like(r32), r32), dt)
        rz = dot64(r, z)
        beta = np.where(done | (it == 0), 0.0, rz / rz_prev)
        p = (z + beta.astype(dt)[:, None, None] * p).astype(dt)
        Kp = (lv.K(p) * geo).astype(dt)
        pAp = dot64(p, Kp)
        alpha = np.where(done, 0.0, rz / np.where(done, 1.0, pAp)).astype(dt)[:, None, None]
        x = (x + alpha * p).astype(dt)
        r = (r - alpha * Kp).astype(dt)
        rz_prev = np.where(done, rz_prev, rz)
        hist.append(np.sqrt(dot64(r, r)))
        iters_b += ~done
        done = done | (hist[-1] <= thresh)
        xs.append(x.copy())
        if done.all():
            break
    return xs, hist, iters_b
