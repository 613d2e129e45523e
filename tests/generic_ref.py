"""Plain fp64 references and derived error bounds of the generic NCHW operators (include/feanet_hip.h section (1),
generic_ops.hip) and their adjoints; helper of test_generic_ref_host.py and test_gpu_generic_adjoint.py, in the role
of footprint.py.

References: torch on the CPU in fp64, in the reference's own formulation (conv2d over the split field, cropped
stride-2 conv2d plus zero pad, conv_transpose2d); gradients are torch autograd of these.  Every size is given as H
and W separately.  Inputs are drawn as fp32 values and widened, so the f32 and the f64 kernels read exactly the same
numbers and the references hold for both.  Tables are random.

Absolute companion S of a quantity: the same operation with every factor replaced by its absolute value and every
subtraction by an addition (K^T g -> |K|^T |g|).  Every operator here is a polynomial in its inputs, so S of a value is
the operator's `absolute` form at the absolute inputs, and S of a gradient is autograd of that form with the absolute
upstream gradient.

Field bound.  An output element is a sum of n terms, the longest a product of m factors.  Evaluated in a floating
point format of unit roundoff u, in any order and with or without fused multiply-adds, no term passes through more
than n + m - 1 roundings, so |computed - exact| <= ((1 + u)^(n+m-1) - 1) S < (n + m) u S (1 + small).  The bound is
      |out - ref| <= 2 (n + m) u S          u = 2^-24 (f32), 2^-53 (f64)
The factor 2 covers the second-order terms and, in f64, the error of the fp64 reference itself (which obeys the same
(n + m) u S).  Where S == 0 no term exists and the output must be exactly 0.  (n, m) of each operator: FIELD.

Weight-gradient bound.  The kernels form every product and every sum in double and round once to T:
      |gw - ref| <= u_T |ref| + 2 N 2^-53 S        (S includes |scale|)
with N the number of summed products: N 2^-53 S for the kernel's double sum, the same again for the reference's.  In
f32 this is one rounding of the result, about an ulp.

The stencil gradient of the Jacobi sweep is a composition: fea_jacobi_sweep_adj writes gf = omd (geo g) in T, the
wrapper forms u0 = u geo + bc in T, and fea_stencil_weight_grad sums -gf u0.  The kernel is held to the bound above at
the inputs it was given (the test rebuilds them: gf is the op's own d/df, u0 the same two T operations on the CPU).
Against the fp64 reference of the whole sweep the four T roundings of gf and u0 (two each) enter every product:
`roundings=4` adds 2 * 4 u_T S, by the argument of the field bound.

Residual norm.  Its residual v obeys the field bound b of `residual`; the squares and their sum are formed in double.
| ||v|| - ||v_ref|| | <= ||v - v_ref|| <= ||b||, plus 2 (N + 2) 2^-53 ||v_ref|| for the double sum of N squares, the
square root, and the reference's own.  With f == NULL v is u itself and b = 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
DT = {"f32": torch.float32, "f64": torch.float64}
SUFS = ("f32", "f64")
W0, W1 = 0.75, -1.25            # exact in fp32; W1 negative: the companion takes |w|

# same-grid shapes (H, W, B, ntab): the smallest that cross the 64-column and 4-row block edges, all but the first
# and third with H != W
SAME = [(1, 1, 1, 1), (1, 65, 2, 3), (3, 3, 1, 1), (4, 64, 3, 7), (5, 63, 2, 16), (7, 129, 2, 16), (131, 5, 1, 4),
        (66, 130, 1, 5)]
# transfer shapes, fine (H, W, B, C, ntab): C > 1 split mode (ntab == C); C == 1, ntab > 1 pid mode
TRANSFER = [(3, 3, 1, 1, 1), (5, 131, 2, 16, 16), (131, 5, 1, 3, 3), (9, 127, 2, 16, 16), (7, 129, 3, 1, 6),
            (17, 9, 2, 2, 2)]

# (n, m) of the field bound: n accumulated terms, m factors in the longest
FIELD = {
    "knet": (9, 2),            # sum_d K[d] u[i+d]
    "residual": (10, 2),       # f - sum_d K[d] u[i+d]
    # out = geo (geo u + bc) + geo omd f - geo omd sum_d K[d] (geo u + bc)[i+d] + bc: 2 + 1 + 18 + 1 terms, the
    # longest geo omd K geo u
    "jacobi": (22, 5),
    "knet_adj": (9, 2),        # sum_d K[d] g[j-d]               (also -d/du of the residual)
    "jacobi_adj": (11, 4),     # gu = geo (geo g - sum_d K[d] omd geo g[j-d])
    "jacobi_adj_f": (1, 3),    # gf = omd geo g
    "restrict_adj": (4, 3),    # a fine node lies in the windows of at most 2 x 2 coarse nodes: w0 R[k] g
    "prolong_adj": (9, 3),     # w1 sum_k P[k] g[2a-1+k]
}


def field_nm(op, C=1):
    if op == "restrict":
        return 9 * C, 3        # w0 sum_ch sum_k R_ch[k] x_ch
    if op == "prolong":
        return 4 * C + 1, 3    # add + w1 sum_ch (at most 2 x 2 coarse nodes) P_ch[k] e_ch
    return FIELD[op]


# ----------------------------------------------------------------------------- inputs
def rng_for(*key):
    return np.random.default_rng([int(k) for k in key])


def draw(rng, *shape):
    """standard normal fp32 values, widened to fp64"""
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32).astype(np.float64))


def draw_pid(rng, H, W, ntab):
    """a random pattern map [H, W] (int64) in which every id below ntab occurs"""
    assert H * W >= ntab
    p = rng.integers(0, ntab, H * W)
    p[rng.permutation(H * W)[:ntab]] = np.arange(ntab)
    return torch.from_numpy(p.reshape(H, W))


def draw_tables(rng, ntab):
    """stencils [ntab, 3, 3] with a centre weight in [1, 2), and omega / d rounded to fp32"""
    k = rng.standard_normal((ntab, 3, 3))
    k[:, 1, 1] = 1.0 + rng.random(ntab)
    k = k.astype(np.float32).astype(np.float64)
    omd = (2.0 / 3.0 / k[:, 1, 1]).astype(np.float32).astype(np.float64)
    return torch.from_numpy(k), torch.from_numpy(omd)


def draw_geo(rng, kind, B, H, W):
    """(geo, bc) of the Jacobi sweep: 'none' (None, None: the square domain), 'bcast' [1, 1, H, W], 'sample'
    [B, 1, H, W] with another random mask and other boundary values in every sample"""
    if kind == "none":
        return None, None
    nb = B if kind == "sample" else 1
    geo = torch.from_numpy((rng.random((nb, 1, H, W)) > 0.3).astype(np.float64))
    return geo, draw(rng, nb, 1, H, W)


# ----------------------------------------------------------------------------- the operators (any float dtype)
def onehot(pid, n, dtype):
    return torch.stack([pid == p for p in range(n)]).to(dtype)[None]          # [1, n, H, W]


def knet(u, ktab, pid=None, absolute=False):
    """KNet.forward: split by the node's pattern, one conv2d.  u [B, 1, H, W], ktab [n, 3, 3]"""
    x = u if pid is None else u * onehot(pid, ktab.shape[0], u.dtype)
    return F.conv2d(x, ktab[None] if pid is not None else ktab[None, :1], padding=1)


def residual(u, f, ktab, pid=None, absolute=False):
    k = knet(u, ktab, pid)
    return f + k if absolute else f - k


def interior_mask(H, W, dtype):
    m = torch.zeros((1, 1, H, W), dtype=dtype)
    m[..., 1:-1, 1:-1] = 1
    return m


def jacobi(u, f, ktab, omd, pid=None, geo=None, bc=None, absolute=False):
    """JacobiBlock.jacobi_convolution: reset(reset(u) + omd (f - K reset(u))), reset(v) = v geo + bc"""
    H, W = u.shape[-2:]
    g = interior_mask(H, W, u.dtype) if geo is None else geo
    om = omd[0] if pid is None else omd[pid]
    u0 = u * g if bc is None else u * g + bc
    k = knet(u0, ktab, pid)
    out = (u0 + om * (f + k if absolute else f - k)) * g
    return out if bc is None else out + bc


def restrict(x, rtab, w0=1.0, pid=None, absolute=False):
    """cropped stride-2 conv2d plus zero pad; x [B, C, H, W]; C == 1 and several kernels: split by pid first"""
    B, C, H, W = x.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if C == 1 and rtab.shape[0] > 1:
        x = x * onehot(pid, rtab.shape[0], x.dtype)
    if Hc < 3 or Wc < 3:       # no interior coarse node: identically zero
        return torch.zeros((B, 1, Hc, Wc), dtype=x.dtype) + 0 * (x.sum() + rtab.sum())
    w = abs(w0) if absolute else w0
    return F.pad(w * F.conv2d(x[:, :, 1:-1, 1:-1], rtab[None], stride=2), (1, 1, 1, 1))


def prolong(e, ptab, w1=1.0, pidc=None, add=None, absolute=False):
    """add + w1 conv_transpose2d(e, P, stride 2, padding 1); e [B, C, Hc, Wc]"""
    if e.shape[1] == 1 and ptab.shape[0] > 1:
        e = e * onehot(pidc, ptab.shape[0], e.dtype)
    w = abs(w1) if absolute else w1
    out = w * F.conv_transpose2d(e, ptab[:, None], stride=2, padding=1)
    return out if add is None else out + add


def split_x(x, pid, C):
    return x * onehot(pid, C, x.dtype)


# ----------------------------------------------------------------------------- values, gradients, companions
def evaluate(fn, tensors, wrt, g, dtype=torch.float64, absolute=False, **consts):
    """out = fn(**tensors, **consts) in `dtype` and the gradients of sum(g . out) w.r.t. the tensors named in wrt
    (zeros where out does not depend on one).  -> (out, {name: grad})"""
    t = {k: None if v is None else v.to(dtype).clone().requires_grad_(k in wrt) for k, v in tensors.items()}
    out = fn(absolute=absolute, **t, **consts)
    grads = {}
    if wrt:
        gs = torch.autograd.grad(out, [t[k] for k in wrt], g.to(dtype), allow_unused=True)
        grads = {k: torch.zeros_like(t[k]) if gr is None else gr for k, gr in zip(wrt, gs)}
    return out.detach(), grads


class Ref:
    """fp64 value, gradients and their absolute companions of one operator call"""

    def __init__(self, fn, tensors, wrt, g, **consts):
        self.fn, self.tensors, self.wrt, self.g, self.consts = fn, tensors, tuple(wrt), g, consts
        self.out, self.grad = evaluate(fn, tensors, self.wrt, g, **consts)
        absd = {k: None if v is None else v.abs() for k, v in tensors.items()}
        self.S, self.Sgrad = evaluate(fn, absd, self.wrt, g.abs(), absolute=True, **consts)

    def in_dtype(self, dtype):
        """the same call evaluated by torch on the CPU in `dtype` (another summation order than the kernels')"""
        return evaluate(self.fn, self.tensors, self.wrt, self.g, dtype=dtype, **self.consts)


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def ratio(err, bound):
    """max err / bound; inf where the bound is 0 and the error is not"""
    err, bound = err.reshape(-1), bound.reshape(-1)
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max())


def field_ratio(got, ref, S, nm, suf):
    n, m = nm
    return ratio((_f64(got) - ref).abs(), 2 * (n + m) * U[suf] * S)


def wgrad_bound(ref, S, N, suf, roundings=0):
    return U[suf] * ref.abs() + 2 * N * 2.0 ** -53 * S + 2 * roundings * U[suf] * S


def wgrad_ratio(got, ref, S, N, suf, roundings=0):
    return ratio((_f64(got).reshape(ref.shape) - ref).abs(), wgrad_bound(ref, S, N, suf, roundings))


def norm_bound(field_b, ref, N):
    """field_b: the field bound of the residual on the interior nodes [B, ...] (zeros for the f == NULL form)"""
    return field_b.reshape(ref.shape[0], -1).norm(dim=1) + 2 * (N + 2) * 2.0 ** -53 * ref.abs()


WORST = {}


def report(op, suf, r, where=""):
    """print one ratio line and keep the worst per (op, dtype); -> r"""
    WORST[(op, suf)] = max(WORST.get((op, suf), 0.0), r)
    print(f"ratio {op:28s} {suf} {where:24s} err/bound = {r:.3g}   (worst so far {WORST[(op, suf)]:.3g})")
    return r


def check(op, suf, r, where=""):
    assert report(op, suf, r, where) <= 1.0, f"{op} {suf} {where}: error is {r:.3g} times its bound"


# ----------------------------------------------------------------------------- weight-gradient kernels, explicitly
def stencil_wgrad(g, u, pid, ntab, scale=1.0):
    """gw[p][d] = scale sum_i g[i] u[i+d] [pid(i+d) == p] and its companion; fields [B, 1, H, W] fp64"""
    def one(g, u, s):
        k = torch.zeros((ntab, 3, 3), dtype=torch.float64, requires_grad=True)
        (gk,) = torch.autograd.grad(knet(u, k, pid if ntab > 1 else None), k, g)
        return s * gk
    return one(g, u, scale), one(g.abs(), u.abs(), abs(scale))


def transfer_wgrad(cf, c_split, ff, f_split, C, interior, scale=1.0):
    """gw[ch][k] = scale sum_(b, a, c) cf[ch_c][a][c] ff[ch_f][2a-1+ky][2c-1+kx] and its companion (header, (1))"""
    def one(cf, ff, s):
        B, _, Hc, Wc = cf.shape
        a0 = 1 if interior else 0
        fp = F.pad(ff, (1, 1, 1, 1))
        gw = torch.zeros((C, 3, 3), dtype=torch.float64)
        for ch in range(C):
            c = cf[:, ch if c_split else 0, a0:Hc - a0, a0:Wc - a0]
            for ky in range(3):
                for kx in range(3):
                    f = fp[:, ch if f_split else 0, ky:ky + 2 * Hc:2, kx:kx + 2 * Wc:2][:, a0:Hc - a0, a0:Wc - a0]
                    gw[ch, ky, kx] = s * (c * f).sum()
        return gw
    return one(cf, ff, scale), one(cf.abs(), ff.abs(), abs(scale))


# ----------------------------------------------------------------------------- cases shared by host and GPU tests
def same_case(H, W, B, ntab, geo_kind="none"):
    """operands of the same-grid operators at one shape: a dict of fp64 CPU tensors (pid int64 or None)"""
    rng = rng_for(H, W, B, ntab, len(geo_kind))
    ktab, omd = draw_tables(rng, ntab)
    geo, bc = draw_geo(rng, geo_kind, B, H, W)
    return dict(H=H, W=W, B=B, ntab=ntab, u=draw(rng, B, 1, H, W), f=draw(rng, B, 1, H, W), g=draw(rng, B, 1, H, W),
                ktab=ktab, omd=omd, pid=draw_pid(rng, H, W, ntab) if ntab > 1 else None, geo=geo, bc=bc)


def transfer_case(H, W, B, C, ntab):
    rng = rng_for(H, W, B, C, ntab, 7)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    pidmode = C == 1 and ntab > 1
    return dict(H=H, W=W, B=B, C=C, ntab=ntab, Hc=Hc, Wc=Wc, x=draw(rng, B, C, H, W), e=draw(rng, B, C, Hc, Wc),
                add=draw(rng, B, 1, H, W), gc=draw(rng, B, 1, Hc, Wc), gf=draw(rng, B, 1, H, W),
                rtab=draw(rng, ntab, 3, 3), ptab=draw(rng, ntab, 3, 3),
                pid=draw_pid(rng, H, W, ntab) if pidmode else None,
                pidc=draw_pid(rng, Hc, Wc, ntab) if pidmode else None)


def knet_ref(c, wrt=("u", "ktab")):
    return Ref(knet, dict(u=c["u"], ktab=c["ktab"]), wrt, c["g"], pid=c["pid"])


def residual_ref(c, wrt=("u", "f", "ktab")):
    return Ref(residual, dict(u=c["u"], f=c["f"], ktab=c["ktab"]), wrt, c["g"], pid=c["pid"])


def jacobi_ref(c, wrt=("u", "f", "ktab")):
    return Ref(jacobi, dict(u=c["u"], f=c["f"], ktab=c["ktab"], omd=c["omd"], geo=c["geo"], bc=c["bc"]), wrt, c["g"],
               pid=c["pid"])


def restrict_ref(c, wrt=("x", "rtab")):
    return Ref(restrict, dict(x=c["x"], rtab=c["rtab"]), wrt, c["gc"], w0=W0, pid=c["pid"])


def prolong_ref(c, wrt=("e", "ptab", "add")):
    return Ref(prolong, dict(e=c["e"], ptab=c["ptab"], add=c["add"]), wrt, c["gf"], w1=W1, pidc=c["pidc"])
