"""numpy side of the flux tests (test_flux_host.py, test_gpu_flux.py); a helper, not a test, in the role of
phase_ref.py.

The element expressions of include/feanet_flux.h evaluated in a chosen dtype, their fp64 values with the absolute
companions of generic_ref.py, dense assemblies of K (from the project's float32 stencil table with mirrored own-row
taps, the form the framed kernels apply; and exactly, from the Q1 element matrix), a dense Dirichlet solve, and the
two-load-case homogenisation on top of them.

Grid axes: index 0 is the row direction (coordinate r h), index 1 the column direction (c h)."""
import functools

import numpy as np

NSUMS = 5
SW = {4: 256, 8: 128}          # strip width in node columns (64 lanes x 16 bytes)
K_TARGET_WAVES, K_RB = 2048, 32


# ----------------------------------------------------------------------------- task grid (restated, not an oracle)
def pick_rb(B, nstrips, rows, maxrb=K_RB):
    rb = maxrb
    while rb > 2 and B * nstrips * -(-rows // rb) < K_TARGET_WAVES:
        rb //= 2
    return rb


def flux_parts(H, W, esz):
    """The Krylov task rule (pcg_geom: row tasks of the height ONE sample gets, over node rows 1 .. H-2) with strips
    over node columns 1 .. W-1."""
    ns = -(-(W - 1) // SW[esz])
    rb = pick_rb(1, ns, H - 2)
    return ns * -(-(H - 2) // rb)


# ----------------------------------------------------------------------------- the element expressions
def corners(u):
    """a, b, c, d of every element of u [..., H, W]"""
    return u[..., :-1, :-1], u[..., :-1, 1:], u[..., 1:, :-1], u[..., 1:, 1:]


def coefficient(phase, k0, k1, shape, dt):
    if phase is None:
        return np.full(shape, k0, dt)
    return np.where(np.asarray(phase) != 0, k1, k0).astype(dt)


def element_values(u, phase, k0, k1, h, dt, wide=False):
    """The fixed expressions with every operation rounded to dt (no fused multiply-add).  wide: the same inputs and
    constants (u, k, i2h and 1/6 as dt values) widened, every operation in fp64 — the exact reference of the dt
    kernel.  u [B, H, W].  -> dict of [B, He, We] arrays q_r, q_c, g_r, g_c, e"""
    ct = np.float64 if wide else dt
    u = np.asarray(u, dt).astype(ct)
    a, b, c, d = corners(u)
    k = coefficient(phase, dt(k0), dt(k1), a.shape[-2:], ct)
    i2h, quarter, sixth = ct(dt(1.0 / (2.0 * h))), ct(0.25), ct(dt(1.0 / 6.0))
    sc = (b - a) + (d - c)
    sr = (c - a) + (d - b)
    w = (a - b) - (c - d)
    g_c, g_r = sc * i2h, sr * i2h
    e = k * ((sc * sc + sr * sr) * quarter + w * w * sixth)
    return dict(q_r=-k * g_r, q_c=-k * g_c, g_r=g_r, g_c=g_c, e=e)


ORDER = ("q_r", "q_c", "g_r", "g_c", "e")


def sums_of(vals):
    """[B, 5] float64 sums over the elements, in the kernel's order"""
    return np.stack([np.asarray(vals[n], np.float64).reshape(vals[n].shape[0], -1).sum(1) for n in ORDER], 1)


def companions(u, phase, k0, k1, h, dt):
    """The absolute companions S (generic_ref.py: every factor by its absolute value, every subtraction an addition)
    of the five element values, in fp64, at the inputs the dt kernel reads (i2h rounded to dt)."""
    au = np.abs(np.asarray(u, np.float64))
    a, b, c, d = corners(au)
    k = np.abs(coefficient(phase, k0, k1, a.shape[-2:], np.float64))
    i2h = float(dt(1.0 / (2.0 * h)))
    s4 = a + b + c + d
    g = s4 * i2h
    return dict(q_r=k * g, q_c=k * g, g_r=g, g_c=g, e=k * (2 * s4 * s4 * 0.25 + s4 * s4 * float(dt(1.0 / 6.0))))


# ----------------------------------------------------------------------------- dense K
def assemble_table(phase, prop):
    """K [H W, H W] float64 from the float32 stencil table and the padded pattern map, every row from its OWN node's
    pattern with mirrored taps: K[i, i + d] = ktab[pid[i]][-d] (kapply's two-material form)."""
    from feanet_amd import mesh_setup as ms
    pid = ms.phase_pattern_map(phase)
    ktab = ms.stencil_table(prop).astype(np.float64)
    H, W = pid.shape
    K = np.zeros((H * W, H * W))
    idx = np.arange(H * W).reshape(H, W)
    for t in range(9):
        dy, dx = t // 3 - 1, t % 3 - 1
        r0, r1, c0, c1 = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
        i = idx[r0:r1, c0:c1]
        K[i.ravel(), (i + dy * W + dx).ravel()] = ktab[pid[r0:r1, c0:c1], 2 - t // 3, 2 - t % 3].ravel()
    return K


def element_matrix():
    """Ke of the Q1 Laplace element in fp64 for the node order (a, b, c, d): FEANet's float32 matrix
    (q1_element_stiffness, nodes in cyclic order a, b, d, c) with its entries restored to exact sixths."""
    from feanet_amd import mesh_setup as ms
    cyc = np.round(ms.q1_element_stiffness().astype(np.float64) * 6.0) / 6.0
    p = [0, 1, 3, 2]                       # (a, b, c, d) -> cyclic position
    return cyc[np.ix_(p, p)]


def assemble_exact(phase, prop):
    """K [H W, H W] float64 assembled element by element from element_matrix() and k = prop[phase]."""
    phase = np.asarray(phase)
    He, We = phase.shape
    H, W = He + 1, We + 1
    Ke = element_matrix()
    K = np.zeros((H * W, H * W))
    for R in range(He):
        for C in range(We):
            n = np.array([R * W + C, R * W + C + 1, (R + 1) * W + C, (R + 1) * W + C + 1])
            K[np.ix_(n, n)] += float(prop[int(phase[R, C] != 0)]) * Ke
    return K


def dirichlet_solve(K, ubc):
    """ubc [B, H, W] with the Dirichlet data on its boundary nodes -> u [B, H, W], K u = 0 on the interior nodes."""
    B, H, W = ubc.shape
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    I, Bd = np.flatnonzero(inner), np.flatnonzero(~inner)
    u = np.array(ubc, np.float64).reshape(B, -1)
    u[:, I] = np.linalg.solve(K[np.ix_(I, I)], -(K[np.ix_(I, Bd)] @ u[:, Bd].T)).T
    return u.reshape(B, H, W)


def load_cases(m, n, size):
    """[2, m+1, n+1] fp64: u = r h and u = c h, h = size / n"""
    h = size / n
    r, c = np.arange(m + 1) * h, np.arange(n + 1) * h
    return np.stack([np.broadcast_to(r[:, None], (m + 1, n + 1)), np.broadcast_to(c[None, :], (m + 1, n + 1))]).copy()


def homogenize(phase, prop, size=2.0, exact=False):
    """The dense pipeline: K (float32 table, or exact), the two load cases solved, the flux sums in fp64.
    -> dict K_eff [2, 2], mean_flux, mean_grad [2, 2], energy [2], uKu [2], hill [2], sym"""
    phase = np.asarray(phase, np.uint8)
    m, n = phase.shape
    h = size / n
    K = assemble_exact(phase, prop) if exact else assemble_table(phase, prop)
    k0, k1 = (float(prop[0]), float(prop[1])) if exact else (float(np.float32(prop[0])), float(np.float32(prop[1])))
    u = dirichlet_solve(K, load_cases(m, n, size))
    s = sums_of(element_values(u, phase, k0, k1, h, np.float64))
    mean_flux, mean_grad, energy = s[:, 0:2] / (m * n), s[:, 2:4] / (m * n), s[:, 4]
    uf = u.reshape(2, -1)
    K_eff = -mean_flux.T
    return dict(u=u, K_eff=K_eff, mean_flux=mean_flux, mean_grad=mean_grad, energy=energy,
                uKu=np.einsum("bi,ij,bj->b", uf, K, uf),
                hill=np.abs(energy + m * n * h * h * np.diag(mean_flux)) / energy,
                sym=abs(K_eff[0, 1] - K_eff[1, 0]) / np.abs(K_eff).max())


@functools.lru_cache(maxsize=None)
def homogenize_image(name, m, n, prop, size=2.0):
    """homogenize() on a study image of phase_ref.py by name (cached: the references are shared and never changed)"""
    import phase_ref as pr
    return homogenize(pr.image(name, m, n), prop, size)


def parallel_stripes(m, n, axis, width=None):
    """half-and-half stripes running ALONG `axis` (0: along the rows' direction r, so the image varies with c)"""
    width = width or (n if axis == 0 else m) // 4
    y, x = np.mgrid[0:m, 0:n]
    return (((x if axis == 0 else y) // width) % 2).astype(np.uint8)
