"""The references and bounds of tests/generic_ref.py are themselves sound (CPU only):

* the torch formulation equals oracle.feanet_oracle (knet_apply, jacobi_sweep, restrict, prolong) at rectangular
  shapes in fp64, inside the f64 field bound;
* a correct evaluation in another summation order passes: the same operators evaluated by torch on the CPU in fp32
  stay inside the f32 bounds at every shape the GPU test uses, and a weight gradient summed in double by numpy loops and
  rounded once to fp32 stays inside the weight-gradient bound;
* a wrong evaluation fails: one tap dropped, taps not mirrored in the adjoint, the pattern map read transposed on an
  H != W grid, sample 0's geometry used for sample 1, the restriction adjoint including the coarse boundary ring, a
  weight gradient summed in fp32.

Every check prints its err / bound ratio (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import generic_ref as gr
from oracle import feanet_oracle as orc

GEO_KINDS = ("none", "bcast", "sample")


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ----------------------------------------------------------------------------- the oracle agrees
@pytest.mark.parametrize("H,W,B,ntab", [(5, 9, 2, 3), (12, 7, 1, 1), (7, 67, 2, 16)])
def test_same_grid_refs_equal_oracle(H, W, B, ntab):
    c = gr.same_case(H, W, B, ntab, "bcast")
    pid = np.zeros((H, W), np.int64) if c["pid"] is None else c["pid"].numpy()
    ktab = c["ktab"].numpy()
    u, f = c["u"].numpy()[:, 0], c["f"].numpy()[:, 0]
    r = gr.knet_ref(c, ())
    gr.check("knet vs oracle", "f64", gr.field_ratio(torch.from_numpy(orc.knet_apply(u, pid, ktab))[:, None], r.out,
                                                     r.S, gr.FIELD["knet"], "f64"))
    # the oracle's omega / d in fp64 (omega_over_d), handed to both
    c["omd"] = torch.from_numpy(orc.omega_over_d(ktab, 2.0 / 3.0, np.float64))
    r = gr.jacobi_ref(c, ())
    got = orc.jacobi_sweep(u, f, pid, ktab, c["geo"].numpy()[0, 0], c["bc"].numpy()[0, 0])
    gr.check("jacobi vs oracle", "f64", gr.field_ratio(torch.from_numpy(got)[:, None], r.out, r.S, gr.FIELD["jacobi"],
                                                       "f64"))


@pytest.mark.parametrize("H,W,B,ntab", [(5, 9, 2, 3), (9, 5, 1, 1), (7, 67, 2, 16)])
def test_transfer_refs_equal_oracle(H, W, B, ntab):
    """the oracle splits implicitly by the node's pattern: both the pid mode (C == 1) and the explicit split agree"""
    c = gr.transfer_case(H, W, B, 1, ntab)
    pid = np.zeros((H, W), np.int64) if c["pid"] is None else c["pid"].numpy()
    pidc = np.zeros((c["Hc"], c["Wc"]), np.int64) if c["pidc"] is None else c["pidc"].numpy()
    want_r = torch.from_numpy(orc.restrict(c["x"].numpy()[:, 0], pid, c["rtab"].numpy(), gr.W0))[:, None]
    want_p = torch.from_numpy(orc.prolong(c["e"].numpy()[:, 0], pidc, c["ptab"].numpy(), gr.W1))[:, None]
    c["add"] = None
    for mode in ("pid", "split"):
        if mode == "split" and ntab > 1:
            c = dict(c, x=gr.split_x(c["x"], c["pid"], ntab), e=gr.split_x(c["e"], c["pidc"], ntab), pid=None, pidc=None)
        C = c["x"].shape[1]
        r = gr.restrict_ref(c, ())
        gr.check(f"restrict vs oracle ({mode})", "f64", gr.field_ratio(want_r, r.out, r.S, gr.field_nm("restrict", C),
                                                                       "f64"))
        r = gr.prolong_ref(c, ())
        gr.check(f"prolong vs oracle ({mode})", "f64", gr.field_ratio(want_p, r.out, r.S, gr.field_nm("prolong", C),
                                                                      "f64"))


# ----------------------------------------------------------------------------- a correct fp32 evaluation passes
def stencil_wgrad_loops(g, u, pid, ntab, scale):
    """the double-sum-then-round weight gradient in another order: numpy, tap by tap, rows first"""
    g, u = g.numpy()[:, 0], u.numpy()[:, 0]
    B, H, W = u.shape
    up = np.zeros((B, H + 2, W + 2))
    up[:, 1:-1, 1:-1] = u
    pp = np.full((H + 2, W + 2), -1)
    pp[1:-1, 1:-1] = 0 if pid is None else pid.numpy()
    gw = np.zeros((ntab, 3, 3))
    for p in range(ntab):
        for dr in range(3):
            for dc in range(3):
                prod = g * up[:, dr:dr + H, dc:dc + W] * (pp[dr:dr + H, dc:dc + W] == p)
                gw[p, dr, dc] = scale * prod.sum(axis=2).sum(axis=1).sum()
    return torch.from_numpy(gw)


@pytest.mark.parametrize("H,W,B,ntab", gr.SAME, ids=ids(gr.SAME))
def test_fp32_evaluation_inside_bounds_same_grid(H, W, B, ntab):
    N = B * H * W
    for kind in GEO_KINDS:
        c = gr.same_case(H, W, B, ntab, kind)
        where = f"{H}x{W} {kind}"
        for op, ref, nm_out, nm_u, nm_f in (("knet", gr.knet_ref(c), "knet", "knet_adj", None),
                                            ("residual", gr.residual_ref(c), "residual", "knet_adj", None),
                                            ("jacobi", gr.jacobi_ref(c), "jacobi", "jacobi_adj", "jacobi_adj_f")):
            if kind != "none" and op != "jacobi":
                continue
            out, grad = ref.in_dtype(torch.float32)
            gr.check(op, "f32", gr.field_ratio(out, ref.out, ref.S, gr.FIELD[nm_out], "f32"), where)
            gr.check(op + " d/du", "f32", gr.field_ratio(grad["u"], ref.grad["u"], ref.Sgrad["u"], gr.FIELD[nm_u],
                                                         "f32"), where)
            if nm_f:
                gr.check(op + " d/df", "f32", gr.field_ratio(grad["f"], ref.grad["f"], ref.Sgrad["f"],
                                                             gr.FIELD[nm_f], "f32"), where)
            elif op == "residual":
                assert torch.equal(grad["f"].double(), c["g"])
        if kind == "none":
            ref = gr.knet_ref(c)
            gw = stencil_wgrad_loops(c["g"], c["u"], c["pid"], ntab, 1.0).float()
            gr.check("stencil wgrad", "f32", gr.wgrad_ratio(gw, ref.grad["ktab"], ref.Sgrad["ktab"], N, "f32"), where)
            want, S = gr.stencil_wgrad(c["g"], c["u"], c["pid"], ntab)       # the explicit form is the autograd one
            assert gr.wgrad_ratio(want, ref.grad["ktab"], S, N, "f64") <= 1 and torch.equal(S, ref.Sgrad["ktab"])


@pytest.mark.parametrize("H,W,B,C,ntab", gr.TRANSFER, ids=ids(gr.TRANSFER))
def test_fp32_evaluation_inside_bounds_transfer(H, W, B, C, ntab):
    c = gr.transfer_case(H, W, B, C, ntab)
    where = f"{H}x{W} C={C} ntab={ntab}"
    pidmode = C == 1 and ntab > 1
    for op, ref, x, adj in (("restrict", gr.restrict_ref(c, ("x",) if pidmode else ("x", "rtab")), "x", "restrict_adj"),
                            ("prolong", gr.prolong_ref(c, ("e", "add") if pidmode else ("e", "ptab", "add")), "e",
                             "prolong_adj")):
        out, grad = ref.in_dtype(torch.float32)
        gr.check(op, "f32", gr.field_ratio(out, ref.out, ref.S, gr.field_nm(op, C), "f32"), where)
        gr.check(f"{op} d/d{x}", "f32", gr.field_ratio(grad[x], ref.grad[x], ref.Sgrad[x], gr.FIELD[adj], "f32"), where)
    if H == 3:     # no interior coarse node: the restriction and its gradients are exactly zero
        ref = gr.restrict_ref(c)
        assert not ref.S.any() and not ref.Sgrad["x"].any() and not ref.Sgrad["rtab"].any()
    if not pidmode:    # the explicit transfer gradient is the autograd one, and its fp32 rounding passes
        Hc, Wc = c["Hc"], c["Wc"]
        for ref, name, args, N in ((gr.restrict_ref(c), "rtab", (c["gc"], False, c["x"], True, C, True, gr.W0),
                                    B * max(0, Hc - 2) * max(0, Wc - 2)),
                                   (gr.prolong_ref(c), "ptab", (c["e"], True, c["gf"], False, C, False, gr.W1),
                                    B * Hc * Wc)):
            want, S = gr.transfer_wgrad(*args)
            assert gr.wgrad_ratio(want, ref.grad[name], S, N, "f64") <= 1
            assert gr.ratio((S - ref.Sgrad[name]).abs(), 2 * N * 2.0 ** -53 * S) <= 1
            gr.check(f"transfer wgrad {name}", "f32", gr.wgrad_ratio(want.float(), ref.grad[name], S, N, "f32"), where)


# ----------------------------------------------------------------------------- a wrong evaluation fails
def must_fail(what, r):
    print(f"wrong variant: {what}: err/bound = {r:.3g}")
    assert r > 1.0, f"the bound accepts a wrong result: {what}"


@pytest.mark.parametrize("suf", gr.SUFS)
def test_wrong_variants_fail(suf):
    dt = gr.DT[suf]
    H, W, B, ntab = 5, 63, 2, 16
    c = gr.same_case(H, W, B, ntab, "sample")
    ref = gr.knet_ref(c)
    # one tap dropped
    k = c["ktab"].clone()
    k[:, 2, 0] = 0
    must_fail("knet, one tap dropped", gr.field_ratio(gr.knet(c["u"].to(dt), k.to(dt), c["pid"]), ref.out, ref.S,
                                                      gr.FIELD["knet"], suf))
    # adjoint with the taps not mirrored: sum_d K_p(j)[d] g[j+d]
    g, kt = c["g"].to(dt), c["ktab"].to(dt)
    unmirrored = (F.conv2d(g, kt[:, None], padding=1) * gr.onehot(c["pid"], ntab, dt)).sum(1, keepdim=True)
    mirrored = (F.conv2d(g, kt.flip(1, 2)[:, None], padding=1) * gr.onehot(c["pid"], ntab, dt)).sum(1, keepdim=True)
    gr.check("knet_adj, explicit form", suf, gr.field_ratio(mirrored, ref.grad["u"], ref.Sgrad["u"],
                                                            gr.FIELD["knet_adj"], suf))
    must_fail("knet_adj, taps not mirrored", gr.field_ratio(unmirrored, ref.grad["u"], ref.Sgrad["u"],
                                                            gr.FIELD["knet_adj"], suf))
    # the pattern map read with H and W swapped: pid[c * H + r]
    pid_t = c["pid"].reshape(W, H).T
    must_fail("knet, pid read transposed", gr.field_ratio(gr.knet(c["u"].to(dt), kt, pid_t), ref.out, ref.S,
                                                          gr.FIELD["knet"], suf))
    must_fail("knet_adj, pid read transposed",
              gr.field_ratio(gr.evaluate(gr.knet, dict(u=c["u"], ktab=c["ktab"]), ("u",), c["g"], dt, pid=pid_t)[1]["u"],
                             ref.grad["u"], ref.Sgrad["u"], gr.FIELD["knet_adj"], suf))
    # sample 0's geometry (and boundary values) used for sample 1
    ref = gr.jacobi_ref(c)
    t = dict(u=c["u"], f=c["f"], ktab=c["ktab"], omd=c["omd"], geo=c["geo"][:1], bc=c["bc"])
    out, grad = gr.evaluate(gr.jacobi, t, ("u", "f"), c["g"], dt, pid=c["pid"])
    must_fail("jacobi, geo of sample 0", gr.field_ratio(out, ref.out, ref.S, gr.FIELD["jacobi"], suf))
    must_fail("jacobi d/du, geo of sample 0", gr.field_ratio(grad["u"], ref.grad["u"], ref.Sgrad["u"],
                                                             gr.FIELD["jacobi_adj"], suf))
    must_fail("jacobi d/df, geo of sample 0", gr.field_ratio(grad["f"], ref.grad["f"], ref.Sgrad["f"],
                                                             gr.FIELD["jacobi_adj_f"], suf))
    out, _ = gr.evaluate(gr.jacobi, dict(t, geo=c["geo"], bc=c["bc"][:1]), (), c["g"], dt, pid=c["pid"])
    must_fail("jacobi, bc of sample 0", gr.field_ratio(out, ref.out, ref.S, gr.FIELD["jacobi"], suf))
    # restriction adjoint that also scatters the coarse boundary ring
    tc = gr.transfer_case(9, 127, 2, 16, 16)
    ref = gr.restrict_ref(tc)
    ringed = gr.W0 * F.conv_transpose2d(tc["gc"].to(dt), tc["rtab"].to(dt)[None], stride=2, padding=1)
    masked = tc["gc"].clone()
    masked[..., 0, :] = masked[..., -1, :] = masked[..., :, 0] = masked[..., :, -1] = 0
    good = gr.W0 * F.conv_transpose2d(masked.to(dt), tc["rtab"].to(dt)[None], stride=2, padding=1)
    gr.check("restrict_adj, explicit form", suf, gr.field_ratio(good, ref.grad["x"], ref.Sgrad["x"],
                                                                gr.FIELD["restrict_adj"], suf))
    must_fail("restrict_adj with the coarse ring", gr.field_ratio(ringed, ref.grad["x"], ref.Sgrad["x"],
                                                                  gr.FIELD["restrict_adj"], suf))


def test_weight_gradient_summed_in_fp32_fails():
    worst = 0.0
    for H, W, B, ntab in gr.SAME[4:]:
        c = gr.same_case(H, W, B, ntab)
        ref = gr.knet_ref(c)
        _, grad = ref.in_dtype(torch.float32)            # torch's conv backward: products and sums in fp32
        r = gr.wgrad_ratio(grad["ktab"], ref.grad["ktab"], ref.Sgrad["ktab"], B * H * W, "f32")
        print(f"wrong variant: stencil wgrad summed in fp32 at {H}x{W}: err/bound = {r:.3g}")
        worst = max(worst, r)
    tc = gr.transfer_case(9, 127, 2, 16, 16)
    ref = gr.restrict_ref(tc)
    _, grad = ref.in_dtype(torch.float32)
    must_fail("transfer wgrad summed in fp32", gr.wgrad_ratio(grad["rtab"], ref.grad["rtab"], ref.Sgrad["rtab"],
                                                              2 * 3 * 62, "f32"))
    must_fail("stencil wgrad summed in fp32", worst)
