"""numpy side of the periodic-cell tests (test_periodic_host.py, test_gpu_periodic.py); a helper, not a test, in the
role of energy_ref.py, on which it builds.  Definitions: DESIGN §18.

The wrapped pattern map, the operator in its own-row and its neighbour-row form with the absolute companion of
generic_ref.py, the load table, the full-weighting restriction and its transpose, the V(nu, nu) cycle from a zero guess,
the projected (and, to pin the reason, the unprojected) preconditioned conjugate gradient, the dense K from the table
or from exact element matrices with a pseudo-inverse solve, and both K_eff routes on the unwrapped field through
flux_ref / energy_ref's element expressions.

Fields are [B, m, n] arrays; grid axes: index 0 is the row direction, index 1 the column direction."""
import functools

import numpy as np

import energy_ref as er
import flux_ref as fx
from feanet_amd import mesh_setup as ms

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
RK = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 4.0
OMEGA = 2.0 / 3.0
SW = {4: 256, 8: 128}


def parts(m, n, esz):
    """fea_per_parts: strips over node columns 0 .. n-1, row tasks of the height ONE sample gets"""
    ns = -(-n // SW[esz])
    return ns * -(-m // fx.pick_rb(1, ns, m))


# ----------------------------------------------------------------------------- maps and hierarchy
def wrapped_map(phase):
    m, n = np.shape(phase)
    return ms.phase_pattern_map(np.pad(np.asarray(phase, np.uint8), 1, mode="wrap"))[1:m + 1, 1:n + 1]


def rolled_map(phase):
    """the same map from the definition: e1 = (r-1, c), e2 = (r-1, c-1), e3 = (r, c-1), e4 = (r, c), wrapped"""
    ph = np.asarray(phase, np.int64)
    code = np.roll(ph, 1, 0) + 2 * np.roll(ph, (1, 1), (0, 1)) + 4 * np.roll(ph, 1, 1) + 8 * ph
    return ms._BITS_TO_ID[code]


def hierarchy(phase, prop=(1, 20), coarsen="stiff"):
    """the level images: halved while both extents are even and the smaller one exceeds 2"""
    out = [np.asarray(phase, np.uint8)]
    k = ms.phase_min_count(prop, coarsen)
    while out[-1].shape[0] % 2 == 0 and out[-1].shape[1] % 2 == 0 and min(out[-1].shape) > 2:
        out.append(ms.coarsen_phase(out[-1], k))
    return out


# ----------------------------------------------------------------------------- operator and transfers
def shifted(u, dr, dc):
    """u(r + dr, c + dc), wrapped"""
    return np.roll(u, (-dr, -dc), (-2, -1))


def apply_own(u, pid, ktab, absolute=False):
    """(K u)(i) = sum_t ktab[pid(i)][8 - t] u(i + d_t): the kernels' form.  absolute: the companion S."""
    k = ktab.reshape(-1, 9)
    if absolute:
        k, u = np.abs(k), np.abs(u)
    acc = np.zeros_like(u)
    for t, (dr, dc) in enumerate(TAPS):
        acc = acc + k[pid, 8 - t] * shifted(u, dr, dc)
    return acc


def apply_neighbour(u, pid, ktab):
    """(K u)(i) = sum_t ktab[pid(i + d_t)][t] u(i + d_t): the definition"""
    k = ktab.reshape(-1, 9)
    acc = np.zeros_like(u)
    for t, (dr, dc) in enumerate(TAPS):
        acc = acc + shifted(k[pid, t] * u, dr, dc)
    return acc


def load_table(ktab, h):
    k = np.asarray(ktab, np.float64).reshape(-1, 9)
    bt = np.zeros((k.shape[0], 2))
    for t, (dr, dc) in enumerate(TAPS):
        bt[:, 0] += k[:, 8 - t] * dr
        bt[:, 1] += k[:, 8 - t] * dc
    return -h * bt


def restrict(r, absolute=False):
    """fc(I, J) = sum k[dr, dc] r(2 I + dr, 2 J + dc)"""
    r = np.abs(r) if absolute else r
    acc = np.zeros(r.shape[:-2] + (r.shape[-2] // 2, r.shape[-1] // 2), r.dtype)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            acc = acc + r.dtype.type(RK[dr + 1, dc + 1]) * shifted(r, dr, dc)[..., ::2, ::2]
    return acc


def prolong(ec, absolute=False):
    """the transpose of restrict: [.., mc, nc] -> [.., 2 mc, 2 nc]"""
    ec = np.abs(ec) if absolute else ec
    out = np.zeros(ec.shape[:-2] + (2 * ec.shape[-2], 2 * ec.shape[-1]), ec.dtype)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            t = np.zeros_like(out)
            t[..., ::2, ::2] = ec.dtype.type(RK[dr + 1, dc + 1]) * ec
            out = out + np.roll(t, (dr, dc), (-2, -1))
    return out


def mean_free(v):
    return v - v.reshape(v.shape[0], -1).astype(np.float64).mean(1).astype(v.dtype)[:, None, None]


def dot64(a, b):
    return (a.astype(np.float64) * b.astype(np.float64)).reshape(a.shape[0], -1).sum(1)


# ----------------------------------------------------------------------------- cycle and conjugate gradients
class Oracle:
    """The solver of feanet_amd.periodic in numpy, every field operation in `dt` (float32, float64 or longdouble)."""

    def __init__(self, phase, prop=(1, 20), size=2.0, dt=np.float64, nu=1, coarse_sweeps=2, coarsen="stiff",
                 omega=OMEGA):
        self.images = hierarchy(phase, prop, coarsen)
        self.pids = [wrapped_map(p) for p in self.images]
        self.m, self.n = self.images[0].shape
        self.h = size / self.n
        self.prop, self.dt, self.nu, self.coarse_sweeps = prop, dt, nu, coarse_sweeps
        self.ktab32 = ms.stencil_table(prop).reshape(16, 9)
        self.ktab = self.ktab32.astype(dt)
        base = np.float32 if dt == np.float32 else np.float64
        self.omd = ms.omega_over_d(self.ktab32.reshape(16, 3, 3), omega, base).astype(dt)
        self.bt = load_table(self.ktab32, self.h)

    def K(self, u, l=0):
        return apply_own(u, self.pids[l], self.ktab)

    def sweep(self, u, f, l):
        if u is None:
            return self.omd[self.pids[l]] * f
        return self.omd[self.pids[l]] * (f - self.K(u, l)) + u

    def cycle(self, f, l=0):
        """M f: V(nu, nu) from a zero guess"""
        f = np.asarray(f, self.dt)
        if l == len(self.pids) - 1:
            u = None
            for _ in range(self.coarse_sweeps):
                u = self.sweep(u, f, l)
            return u
        u = None
        for _ in range(self.nu):
            u = self.sweep(u, f, l)
        u = u + prolong(self.cycle(restrict(f - self.K(u, l)), l + 1))
        for _ in range(self.nu):
            u = self.sweep(u, f, l)
        return u

    def rhs(self):
        """[2, m, n] float64: the two load cases"""
        return np.moveaxis(self.bt[self.pids[0]], -1, 0).copy()

    def floor(self):
        u_t = 2.0 ** -24 if self.dt == np.float32 else 2.0 ** -53
        kmax = float(max(np.float32(self.prop[0]), np.float32(self.prop[1])))
        return 22 * u_t * (32.0 * kmax / 6.0) * self.h * np.sqrt(self.m * self.n)

    def pcg(self, b=None, rtol=1e-10, max_iters=200, project=True):
        """-> x [B, m, n] (mean-free), iterations [B], flags [B], history (list of [B] norms).  project=False: the
        recurrence on K itself (b is still made mean-free), to show what the projection is for."""
        dt = self.dt
        P = mean_free if project else (lambda v: v)
        r = mean_free(np.asarray(self.rhs() if b is None else b, dt))
        B = r.shape[0]
        x, p = np.zeros_like(r), np.zeros_like(r)
        rr0 = np.sqrt(dot64(r, r))
        flags = (rr0 <= self.floor()).astype(np.int64)
        iters = np.zeros(B, np.int64)
        rn, rz_old, hist = rr0.copy(), np.full(B, np.inf), [rr0.copy()]
        col = lambda s: s.astype(dt)[:, None, None]
        for _ in range(max_iters):
            if (flags != 0).all():
                break
            z = P(self.cycle(r))
            rz = dot64(r, z)
            act = flags == 0
            with np.errstate(all="ignore"):
                p = np.where(act[:, None, None], z + col(rz / rz_old) * p, p)
                y = self.K(p)
                pAp = dot64(p, y)
                y = P(y)
                bad = ~(np.isfinite(pAp) & (pAp > 0))
                flags = np.where(act & bad, 2, flags)
                act = act & ~bad
                alpha = col(rz / pAp)
                x = np.where(act[:, None, None], x + alpha * p, x)
                r = np.where(act[:, None, None], r - alpha * y, r)
            new = np.sqrt(dot64(r, r))
            rn = np.where(act, new, rn)
            rz_old = np.where(act, rz, rz_old)
            iters += act
            hist.append(rn.copy())
            flags = np.where(act & (new <= rtol * rr0), 1, flags)
        return mean_free(x), iters, flags, hist


def cycle_matrix(o):
    """M [m n, m n] of Oracle o, column by column"""
    N = o.m * o.n
    return o.cycle(np.eye(N).reshape(N, o.m, o.n)).reshape(N, N).T


# ----------------------------------------------------------------------------- dense
def dense_table(phase, prop):
    """K [m n, m n] float64 of the torus from the float32 table, own-row form (entries ADD where taps meet, as on a
    2 x k level)"""
    pid = wrapped_map(phase)
    k = ms.stencil_table(prop).reshape(16, 9).astype(np.float64)
    m, n = pid.shape
    idx = np.arange(m * n).reshape(m, n)
    K = np.zeros((m * n, m * n))
    for t, (dr, dc) in enumerate(TAPS):
        np.add.at(K, (idx.ravel(), shifted(idx, dr, dc).ravel()), k[pid, 8 - t].ravel())
    return K


def element_nodes(m, n, R, C):
    """a, b, c, d of element (R, C) on the torus"""
    R1, C1 = (R + 1) % m, (C + 1) % n
    return np.array([R * n + C, R * n + C1, R1 * n + C, R1 * n + C1])


def dense_exact(phase, prop, size=2.0):
    """(K, b [2, m n]) assembled element by element from flux_ref.element_matrix(): b_j = -sum_e k_e Ke X_j|_e with the
    element's own (unwrapped) node coordinates"""
    phase = np.asarray(phase)
    m, n = phase.shape
    h = size / n
    Ke = fx.element_matrix()
    K = np.zeros((m * n, m * n))
    b = np.zeros((2, m * n))
    X = np.array([[0.0, 0.0, h, h], [0.0, h, 0.0, h]])
    for R in range(m):
        for C in range(n):
            nd = element_nodes(m, n, R, C)
            k = float(prop[int(phase[R, C] != 0)])
            np.add.at(K, (nd[:, None], nd[None, :]), k * Ke)
            for j in range(2):
                np.add.at(b[j], nd, -k * (Ke @ X[j]))
    return K, b


def projected(K):
    """P K P, P = I - 1 1^T / N, by rank-one updates"""
    return K - K.mean(0)[None, :] - K.mean(1)[:, None] + K.mean()


def pinv_solve(K, b):
    """pinv(P K P) P b for b [B, N].  The null space of P K P is known exactly (the constants), so the pseudo-inverse
    solution is the solution of the regular system (P K P + s 1 1^T / N) x = P b, s = the mean diagonal of K: an LU
    solve instead of an SVD (test_periodic_host.py compares the two at 12 x 16)."""
    N = K.shape[0]
    A = projected(K)
    A += np.trace(K) / N / N
    return np.linalg.solve(A, (b - b.mean(1)[:, None]).T).T


def pinv_svd(K, b):
    """the same by numpy's pinv.  The cut-off: the constant mode of P K P sits at the rounding level of max|K| (1e-15
    relative, which numpy's default would keep and invert), the smallest other singular value above 1e-4 of the
    largest on every image here"""
    return (np.linalg.pinv(projected(K), rcond=1e-10) @ (b - b.mean(1)[:, None]).T).T


def unwrap(chi, size=2.0):
    """U [2, m+1, n+1] = the periodic extension of chi [2, m, n] + the linear fields"""
    m, n = chi.shape[-2:]
    U = np.pad(chi, ((0, 0), (0, 1), (0, 1)), mode="wrap")
    return U + fx.load_cases(m, n, size)


def routes_of(chi, phase, prop, size=2.0, exact=False):
    return er.routes(unwrap(np.asarray(chi, np.float64), size), phase, *er.coefficients(prop, exact), size)


def homogenize(phase, prop, size=2.0, exact=False):
    """The dense pipeline: chi = pinv(P K P) P b (pinv_solve), both routes on the unwrapped field
    -> dict chi, u, K_E, dK, K_flux, gap"""
    phase = np.asarray(phase, np.uint8)
    m, n = phase.shape
    if exact:
        K, b = dense_exact(phase, prop, size)
    else:
        K = dense_table(phase, prop)
        b = np.moveaxis(load_table(ms.stencil_table(prop), size / n)[wrapped_map(phase)], -1, 0).reshape(2, -1)
    chi = pinv_solve(K, b).reshape(2, m, n)
    chi = mean_free(chi)
    return dict(chi=chi, u=unwrap(chi, size), **routes_of(chi, phase, prop, size, exact))


@functools.lru_cache(maxsize=None)
def homogenize_image(name, m, n, prop, size=2.0, exact=False):
    """homogenize() on a study image of phase_ref.py by name (cached: the references are shared and never changed)"""
    import phase_ref as pr
    return homogenize(pr.image(name, m, n), prop, size, exact)
