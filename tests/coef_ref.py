"""numpy side of the coefficient-field tests (test_coef_host.py, test_gpu_coef.py); a helper, not a test, in the role
of periodic_ref.py, on which it builds.  Definitions: DESIGN §19.

The difference form of the operator in a chosen dtype with its absolute companion, the diagonal and the sweep, the two
right-hand sides, the three coarsening rules and the hierarchy, the dense K and b assembled element by element with a
pseudo-inverse solve, both K_eff routes and the sensitivity field on the unwrapped field, an oracle solver shaped like
periodic_ref.Oracle, the study fields and the coarsening table.

Fields are [B, m, n] arrays, k is [m, n]; index 0 is the row direction, index 1 the column direction.  Node (r, c)
touches the elements NW (r-1, c-1), NE (r-1, c), SW (r, c-1), SE (r, c), wrapped."""
import functools

import numpy as np

import energy_ref as er
import flux_ref as fx
import periodic_ref as pf

OMEGA = 2.0 / 3.0
RULES = ("arithmetic", "harmonic", "geometric")
# depth of the fixed expressions in rounded operations (derived in test_gpu_coef.py)
OPS_APPLY, OPS_SWEEP, OPS_RESTRICT = 8, 18, 18


# ----------------------------------------------------------------------------- study fields
def lognormal(m, n, sigma=1.0, seed=0):
    """exp(sigma g), g standard normal: [m, n] float64"""
    return np.exp(sigma * np.random.default_rng([seed, m, n]).standard_normal((m, n)))


def binary(m, n, lo=1.0, hi=1000.0, seed=0):
    """each element lo or hi with probability 1/2"""
    return np.where(np.random.default_rng([seed, m, n, 1]).random((m, n)) < 0.5, lo, hi)


def laminate(m=12, n=16, values=(1.0, 3.0, 20.0, 7.5), width=4):
    """columns of `width` elements with the values in turn: the arithmetic mean along the rows' direction (index 0),
    the harmonic mean across"""
    v = np.asarray(values, np.float64)
    return np.tile(v[(np.arange(n) // width) % len(v)], (m, 1))


def from_image(img, prop):
    """the two-material image as a field"""
    return np.where(np.asarray(img) != 0, float(prop[1]), float(prop[0]))


# ----------------------------------------------------------------------------- operator
def corner_fields(k):
    """(k_NW, k_NE, k_SW, k_SE) of every node"""
    return np.roll(k, (1, 1), (0, 1)), np.roll(k, 1, 0), np.roll(k, 1, 1), k


def apply_diff(u, k, dt=np.float64, absolute=False):
    """(K u) = ((k_NW t_NW + k_NE t_NE) + (k_SW t_SW + k_SE t_SE)) * (1/6), t_NW = (d_N + d_W) + 2 d_NW, ..., every
    operation rounded to dt (no fused multiply-add).  absolute: the companion S, every value by its absolute value and
    every subtraction an addition, in fp64."""
    if absolute:
        dt = np.float64
        u, k = np.abs(np.asarray(u, dt)), np.abs(np.asarray(k, dt))
        d = lambda dr, dc: u + pf.shifted(u, dr, dc)
    else:
        u, k = np.asarray(u, dt), np.asarray(k, dt)
        d = lambda dr, dc: u - pf.shifted(u, dr, dc)
    knw, kne, ksw, kse = corner_fields(k)
    dn, ds, dw, de = d(-1, 0), d(1, 0), d(0, -1), d(0, 1)
    two = dt(2)
    tnw = (dn + dw) + two * d(-1, -1)
    tne = (dn + de) + two * d(-1, 1)
    tsw = (ds + dw) + two * d(1, -1)
    tse = (ds + de) + two * d(1, 1)
    return ((knw * tnw + kne * tne) + (ksw * tsw + kse * tse)) * (dt(1) / dt(6))


def diagonal(k, dt=np.float64):
    knw, kne, ksw, kse = corner_fields(np.asarray(k, dt))
    return (dt(2) / dt(3)) * ((knw + kne) + (ksw + kse))


def omd(k, omega=OMEGA, dt=np.float64):
    return dt(omega) / diagonal(k, dt)


def sweep(u, f, k, omega=OMEGA, dt=np.float64):
    w = omd(k, omega, dt)
    f = np.asarray(f, dt)
    if u is None:
        return w * f
    u = np.asarray(u, dt)
    return w * (f - apply_diff(u, k, dt)) + u


def sweep_companion(u, f, k, omega=OMEGA):
    """S of the sweep: |w| (|f| + S_K) + |u|"""
    w = np.abs(omd(k, omega))
    if u is None:
        return w * np.abs(f)
    return w * (np.abs(f) + apply_diff(u, k, absolute=True)) + np.abs(u)


def rhs(k, h):
    """[2, m, n] float64: b_0 = (h/2) ((k_SW + k_SE) - (k_NW + k_NE)), b_1 = (h/2) ((k_NE + k_SE) - (k_NW + k_SW))"""
    knw, kne, ksw, kse = corner_fields(np.asarray(k, np.float64))
    return np.stack([0.5 * h * ((ksw + kse) - (knw + kne)), 0.5 * h * ((kne + kse) - (knw + ksw))])


# ----------------------------------------------------------------------------- hierarchy
def coarsen(k, rule, dt=np.float64):
    """the mean of each 2 x 2 block: arithmetic in dt; harmonic and geometric in double, rounded to dt once"""
    k = np.asarray(k, dt)
    a, b, c, d = k[0::2, 0::2], k[0::2, 1::2], k[1::2, 0::2], k[1::2, 1::2]
    if rule == "arithmetic":
        return ((a + b) + (c + d)) * dt(0.25)
    a, b, c, d = (x.astype(np.float64) for x in (a, b, c, d))
    if rule == "harmonic":
        return (4.0 / ((1.0 / a + 1.0 / b) + (1.0 / c + 1.0 / d))).astype(dt)
    if rule == "geometric":
        return np.exp(((np.log(a) + np.log(b)) + (np.log(c) + np.log(d))) * 0.25).astype(dt)
    raise ValueError(rule)


def hierarchy(k, rule="geometric", dt=np.float64, levels=None):
    """the level fields on periodic.coarse_shapes (levels: at most that many)"""
    out = [np.asarray(k, dt)]
    while out[-1].shape[0] % 2 == 0 and out[-1].shape[1] % 2 == 0 and min(out[-1].shape) > 2 and \
            (levels is None or len(out) < levels):
        out.append(coarsen(out[-1], rule, dt))
    return out


# ----------------------------------------------------------------------------- oracle solver
class Oracle(pf.Oracle):
    """The solver of feanet_amd.coef in numpy, every field operation in `dt`; cycle() and pcg() are
    periodic_ref.Oracle's."""

    def __init__(self, k, size=2.0, dt=np.float64, nu=1, coarse_sweeps=2, coarsen="geometric", omega=OMEGA,
                 levels=None):
        base = np.float32 if dt == np.float32 else np.float64
        self.ks = [x.astype(dt) for x in hierarchy(np.asarray(k, base), coarsen, base, levels)]
        self.pids = self.ks  # periodic_ref.Oracle.cycle counts its levels on this
        self.m, self.n = self.ks[0].shape
        self.h = size / self.n
        self.dt, self.nu, self.coarse_sweeps, self.omega = dt, nu, coarse_sweeps, omega
        self.base = base

    def K(self, u, l=0):
        return apply_diff(u, self.ks[l], self.dt)

    def sweep(self, u, f, l):
        return sweep(u, f, self.ks[l], self.omega, self.dt)

    def rhs(self):
        return rhs(self.ks[0].astype(np.float64), self.h)

    def floor(self):
        u_t = 2.0 ** -24 if self.dt == np.float32 else 2.0 ** -53
        return 22 * u_t * (32.0 * float(self.ks[0].max()) / 6.0) * self.h * np.sqrt(self.m * self.n)


# ----------------------------------------------------------------------------- dense
def dense(k, size=2.0):
    """(K [m n, m n], b [2, m n]) assembled element by element from flux_ref.element_matrix(), as
    periodic_ref.dense_exact does for an image"""
    k = np.asarray(k, np.float64)
    m, n = k.shape
    h = size / n
    Ke = fx.element_matrix()
    K = np.zeros((m * n, m * n))
    b = np.zeros((2, m * n))
    X = np.array([[0.0, 0.0, h, h], [0.0, h, 0.0, h]])
    for R in range(m):
        for C in range(n):
            nd = pf.element_nodes(m, n, R, C)
            np.add.at(K, (nd[:, None], nd[None, :]), k[R, C] * Ke)
            for j in range(2):
                np.add.at(b[j], nd, -k[R, C] * (Ke @ X[j]))
    return K, b


def routes_of(chi, k, size=2.0):
    """Both routes on the fluctuations chi [2, m, n]: dict K_E, K_flux, gap, sens [3, m, n] (the derivative of
    K_E[0, 0], K_E[0, 1], K_E[1, 1] with respect to each element's own coefficient: the element densities / |V|)"""
    k = np.asarray(k, np.float64)
    m, n = k.shape
    h = size / n
    vol = m * n * h * h
    U = pf.unwrap(np.asarray(chi, np.float64), size)
    d = er.element_values(U[0:1], U[1:2], np.float64)
    sens = np.stack([d[q][0] for q in er.NAMES]) / vol
    a = (sens * k).reshape(3, -1).sum(1)
    K_E = np.array([[a[0], a[1]], [a[1], a[2]]])
    q = fx.element_values(U, None, 1.0, 1.0, h, np.float64)
    K_flux = -np.array([[(k * q[c][j]).sum() / (m * n) for j in range(2)] for c in ("q_r", "q_c")])
    gap = np.abs(K_E - 0.5 * (K_flux + K_flux.T)).max() / np.abs(K_E).max()
    return dict(K_E=K_E, K_flux=K_flux, gap=gap, sens=sens)


def homogenize(k, size=2.0):
    """The dense pipeline: chi = pinv(P K P) P b, both routes -> dict chi, K_E, K_flux, gap, sens"""
    k = np.asarray(k, np.float64)
    K, b = dense(k, size)
    chi = pf.mean_free(pf.pinv_solve(K, b).reshape(2, *k.shape))
    return dict(chi=chi, **routes_of(chi, k, size))


@functools.lru_cache(maxsize=None)
def homogenize_lognormal(m, n, sigma=1.0, seed=0):
    """homogenize() on a lognormal study field (cached: the references are shared and never changed)"""
    return homogenize(lognormal(m, n, sigma, seed))


def dense_k_eff(k, size=2.0):
    return homogenize(k, size)["K_E"]


# ----------------------------------------------------------------------------- the coarsening table
TABLE_FIELDS = (("lognormal, sigma 1.0", lambda m, n: lognormal(m, n, 1.0)),
                ("lognormal, sigma 2.5", lambda m, n: lognormal(m, n, 2.5)),
                ("random binary, 1 : 1000", lambda m, n: binary(m, n)))


def coarsening_table(m=16, n=16, levels=3, rtol=1e-10, max_iters=200):
    """{field: {rule: (iterations of load case 0, of load case 1)}} of the fp64 oracle with omega = 2/3; a count is
    -1 where the sample did not converge"""
    out = {}
    for name, make in TABLE_FIELDS:
        k = make(m, n)
        out[name] = {}
        for rule in RULES:
            _, its, flags, _ = Oracle(k, coarsen=rule, levels=levels).pcg(rtol=rtol, max_iters=max_iters)
            out[name][rule] = tuple(int(i) if f == 1 else -1 for i, f in zip(its, flags))
    return out
