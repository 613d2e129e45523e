"""numpy references of the full-multigrid start (include/feanet_fmg.h, MultigridSolver.fmg); helper of
test_fmg_host.py and test_gpu_fmg.py, in the role of generic_ref.py.

interp: the interpolation of a coarse solution, columns inside each coarse row first, then across the rows.  One
direction, n coarse nodes, fine node 2j+1 between coarse j and j+1:
    cubic, 0 < j < n-2:  (-1, 9, 9, -1)/16 of coarse j-1 .. j+2
    cubic, j == 0:       (5, 15, -5, 1)/16 of coarse 0 .. 3         (one-sided)
    cubic, j == n-2:     (1, -5, 15, 5)/16 of coarse n-4 .. n-1
    order 1, or n < 4:   (1/2, 1/2) of coarse j, j+1
fine node 2j copies coarse j.  `absolute` gives the companion S of tests/generic_ref.py (every weight and value by
its absolute value): a fine value is u plus at most 4 x 4 weighted coarse values, 17 terms of 2 factors (a weight,
exact in either format, and a value), so the bound is 2 (17 + 2) u S.

fmg: the driver composed from the CPU oracle (oracle.feanet_oracle): right-hand sides f_(l+1) = P^T f_l (restrict
with lin/4), Dirichlet data injected at every level's boundary nodes, OracleMultigrid(n >> s, levels=L - s) for the
V-cycles of the sub-hierarchy s .. L-1.
"""
import numpy as np

from oracle import feanet_oracle as fo

NM = (17, 2)
LIN4 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32) / np.float32(4)
MID = np.array([-1, 9, 9, -1], np.float64) / 16
LO = np.array([5, 15, -5, 1], np.float64) / 16
HI = np.array([1, -5, 15, 5], np.float64) / 16


def interp_axis(e, order, absolute=False):
    """e [..., n] -> [..., 2n - 1] along the last axis."""
    e = np.asarray(e)
    dt = e.dtype.type
    n = e.shape[-1]
    out = np.zeros(e.shape[:-1] + (2 * n - 1,), e.dtype)
    out[..., ::2] = e
    fix = (lambda w: np.abs(w)) if absolute else (lambda w: w)
    if order == 3 and n >= 4:
        mid, lo, hi = (fix(w).astype(e.dtype) for w in (MID, LO, HI))
        out[..., 3:2 * n - 4:2] = (mid[0] * e[..., :-3] + mid[1] * e[..., 1:-2] + mid[2] * e[..., 2:-1]
                                   + mid[3] * e[..., 3:])
        out[..., 1] = lo[0] * e[..., 0] + lo[1] * e[..., 1] + lo[2] * e[..., 2] + lo[3] * e[..., 3]
        out[..., -2] = hi[0] * e[..., -4] + hi[1] * e[..., -3] + hi[2] * e[..., -2] + hi[3] * e[..., -1]
    else:
        assert order in (1, 3)
        out[..., 1::2] = dt(0.5) * e[..., :-1] + dt(0.5) * e[..., 1:]
    return out


def interp(e, order, absolute=False):
    """e [..., Hc, Wc] -> [..., 2 Hc - 1, 2 Wc - 1]: along the columns of each coarse row, then across the rows."""
    e = np.abs(e) if absolute else np.asarray(e)
    rows = interp_axis(e, order, absolute)
    return np.swapaxes(interp_axis(np.swapaxes(rows, -1, -2), order, absolute), -1, -2)


def prolong(u, ec, order, absolute=False):
    """fea_fmg_prolong: u + I(ec) on the interior nodes (u None: zero); the boundary nodes keep u's values."""
    up = interp(ec, order, absolute)
    out = np.zeros_like(up) if u is None else (np.abs(u) if absolute else np.array(u, copy=True))
    base = 0 if u is None else out[..., 1:-1, 1:-1]
    out[..., 1:-1, 1:-1] = base + up[..., 1:-1, 1:-1]
    return out


def restrict(f):
    """fea_fmg_restrict: the coarse load vector P^T f (interior; zero boundary nodes)."""
    return fo.restrict(f, np.zeros(np.shape(f)[-2:], np.uint8), LIN4[None])


def ring(bc, stride, dtype):
    """The Dirichlet field of a level: the fine field `bc` ([..., H, W]; None: zero) sampled at `stride` on the
    boundary nodes, zero inside."""
    if bc is None:
        return None
    s = np.asarray(bc, dtype)[..., ::stride, ::stride]
    out = np.zeros_like(s)
    out[..., 0, :], out[..., -1, :] = s[..., 0, :], s[..., -1, :]
    out[..., :, 0], out[..., :, -1] = s[..., :, 0], s[..., :, -1]
    return out


def default_base_cycles(Hc, Wc):
    return 1 if (Hc - 2) * (Wc - 2) == 1 else 8


def vcycle(mg, v, f, nu1, nu2):
    """OracleMultigrid.step with nu1 pre- and nu2 post-sweeps per level (coarse levels from zero, the coarsest
    nu1 + nu2 sweeps): the schedule of feanet_amd.schedule.vcycle_schedule, from the oracle's own operators."""
    lv, L = mg.levels, mg.L
    B = fo._as3(v).shape[0]
    vs, fs = [None] * L, [None] * L
    vs[0], fs[0] = fo._as3(v).astype(mg.dtype), fo._as3(f).astype(mg.dtype)
    for j in range(L):
        if j:
            vs[j] = np.zeros((B, lv[j].H, lv[j].W), mg.dtype)
        for _ in range(nu1 + (nu2 if j == L - 1 else 0)):
            vs[j] = lv[j].sweep(vs[j], fs[j])
        if j < L - 1:
            fs[j + 1] = fo.restrict(fs[j] - lv[j].K(vs[j]), lv[j].pid, mg.rtab, mg.w[0])
    for j in range(L - 2, -1, -1):
        vs[j] = vs[j] + fo.prolong(vs[j + 1], lv[j + 1].pid, mg.ptab, mg.w[1])
        for _ in range(nu2):
            vs[j] = lv[j].sweep(vs[j], fs[j])
    return vs[0]


def fmg(n, f, bc=None, levels=None, rows=None, cycles=1, order=3, base_cycles=None, problem="poisson",
        dtype=np.float64, nu=(1, 1), pids=None, **kw):
    """The full-multigrid pass on an (rows + 1) x (n + 1) grid: f [B, H, W] assembled right-hand side, bc [B, H, W]
    Dirichlet field (its boundary nodes are used).  Returns the fine iterate [B, H, W]."""
    m = n if rows is None else rows
    L = int(np.log2(min(n, m))) if levels is None else levels
    f = fo._as3(np.asarray(f, dtype))
    B = f.shape[0]
    fs = [f]
    for _ in range(L - 1):
        fs.append(restrict(fs[-1]))
    if bc is not None:
        bc = fo._as3(np.asarray(bc, dtype))
    v = None
    for s in range(L - 1, -1, -1):
        mg = fo.OracleMultigrid(n >> s, problem, dtype, levels=L - s, rows=m >> s, pids=pids, **kw)
        H, W = (m >> s) + 1, (n >> s) + 1
        geo, zero = fo.square_geometry((H, W), dtype)
        bcl = ring(bc, 1 << s, dtype)
        bcl = np.broadcast_to(zero, (B, H, W)).copy() if bcl is None else bcl
        mg.set_boundary(geo, bcl)
        if v is None:
            v = np.zeros((B, H, W), dtype)
            ncyc = default_base_cycles(H, W) if base_cycles is None else base_cycles
        else:
            v = prolong(None, v, order)
            ncyc = cycles
        v = v * geo + bcl
        for _ in range(ncyc):
            v = mg.step(v, fs[s]) if tuple(nu) == (1, 1) else vcycle(mg, v, fs[s], nu[0], nu[1])
    return v


def model_problem(n, rows=None, size=2.0, dtype=np.float64):
    """The smooth test problem of DESIGN §14 on the mesh's own domain [-size/2, size/2] x [-l_y/2, l_y/2],
    l_y = size rows / n:  u = sin(pi x) sin(2 pi y / l_y) + x y + 1 + (x^2 - y^2)/2, -laplace u = F.
    Returns (u_exact, f assembled)."""
    m = n if rows is None else rows
    h = size / n
    ly = h * m
    y, x = np.meshgrid(np.arange(m + 1) * h - ly / 2, np.arange(n + 1) * h - size / 2, indexing="ij")
    s = np.sin(np.pi * x) * np.sin(2 * np.pi * y / ly)
    u = s + x * y + 1 + (x * x - y * y) / 2
    F = (np.pi ** 2 + (2 * np.pi / ly) ** 2) * s
    f = fo.conv3x3(F.astype(dtype), fo.fnet_stencil(h))
    return u.astype(dtype), np.asarray(f, dtype)
