"""The generic NCHW operators and their adjoints (generic_ops.hip) off the square fp64 path: rectangular grids, both
dtypes, per-sample geometry, the weight-gradient workspaces and the write sets of the adjoint entry points.

Values and gradients go through feanet_amd.ops (the torch.ops.feanet.* product path) and are held to the fp64
references and the derived bounds of tests/generic_ref.py (field bound 2 (n + m) u S, weight-gradient bound
u_T |ref| + 2 N 2^-53 S); nothing is scaled by max|ref| and no tolerance is fitted.  Direct _lib.call is used only
where the output or the workspace must be a caller-owned buffer inside a canary-filled allocation.

Every check prints its err / bound ratio (pytest -s)."""
import functools

import pytest
import torch

import generic_ref as gr

pytestmark = pytest.mark.gpu

CANARY = 0xC1
PAD = 256                       # guard bytes on either side of a caller-owned buffer


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def dev(t, suf):
    return None if t is None else t.to(gr.DT[suf]).cuda()


def leaf(t, suf):
    return dev(t, suf).requires_grad_(True)


def dpid(p):
    return None if p is None else p.to(torch.uint8).cuda()


# references: computed once per shape, shared by both dtypes and never modified
@functools.lru_cache(maxsize=None)
def same_refs(H, W, B, ntab, kind="none"):
    c = gr.same_case(H, W, B, ntab, kind)
    r = dict(c=c, jacobi=gr.jacobi_ref(c))
    if kind == "none":
        c1 = dict(c, ktab=c["ktab"][:1], pid=None)
        r.update(knet=gr.knet_ref(c), residual=gr.residual_ref(c), conv=gr.knet_ref(c1))
    return r


@functools.lru_cache(maxsize=None)
def transfer_refs(H, W, B, C, ntab):
    c = gr.transfer_case(H, W, B, C, ntab)
    pidmode = C == 1 and ntab > 1
    return dict(c=c, pidmode=pidmode, restrict=gr.restrict_ref(c, ("x",) if pidmode else ("x", "rtab")),
                prolong=gr.prolong_ref(c, ("e", "add") if pidmode else ("e", "ptab", "add")))


def field(op, suf, got, ref, S, nm, where):
    assert got.dtype == gr.DT[suf] and tuple(got.shape) == tuple(ref.shape), (op, got.dtype, got.shape, ref.shape)
    gr.check(op, suf, gr.field_ratio(got, ref, S, gr.FIELD[nm] if isinstance(nm, str) else nm, suf), where)


def wgrad(op, suf, got, ref, S, N, where, roundings=0):
    assert got.dtype == gr.DT[suf] and tuple(got.shape) == tuple(ref.shape), (op, got.dtype, got.shape, ref.shape)
    gr.check(op, suf, gr.wgrad_ratio(got, ref, S, N, suf, roundings), where)


# ----------------------------------------------------------------------------- same-grid operators
@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,ntab", gr.SAME, ids=ids(gr.SAME))
def test_knet_residual_split(H, W, B, ntab, suf):
    from feanet_amd import ops
    R = same_refs(H, W, B, ntab)
    c, where, N = R["c"], f"{H}x{W} B={B} ntab={ntab}", B * H * W
    pid, g = dpid(c["pid"]), dev(c["g"], suf)
    # y = K u
    ref = R["knet"]
    u, k = leaf(c["u"], suf), leaf(c["ktab"], suf)
    y = ops.knet_apply(u, k, pid)
    field("knet", suf, y, ref.out, ref.S, "knet", where)
    y.backward(g)
    field("knet d/du", suf, u.grad, ref.grad["u"], ref.Sgrad["u"], "knet_adj", where)
    wgrad("knet d/dK", suf, k.grad, ref.grad["ktab"], ref.Sgrad["ktab"], N, where)
    # conv3x3 with the weight as HNet holds it ([1, 1, 3, 3], layer weight[0])
    ref = R["conv"]
    x, w = leaf(c["u"], suf), leaf(c["ktab"][:1, None], suf)
    y = ops.conv3x3(x, w[0])
    field("conv3x3", suf, y, ref.out, ref.S, "knet", where)
    y.backward(g)
    field("conv3x3 d/dx", suf, x.grad, ref.grad["u"], ref.Sgrad["u"], "knet_adj", where)
    wgrad("conv3x3 d/dw", suf, w.grad[0], ref.grad["ktab"], ref.Sgrad["ktab"], N, where)
    # r = f - K u
    ref = R["residual"]
    u, f, k = leaf(c["u"], suf), leaf(c["f"], suf), leaf(c["ktab"], suf)
    r = ops.residual(u, f, k, pid)
    field("residual", suf, r, ref.out, ref.S, "residual", where)
    r.backward(g)
    field("residual d/du", suf, u.grad, ref.grad["u"], ref.Sgrad["u"], "knet_adj", where)
    assert torch.equal(f.grad, g), "residual d/df is the upstream gradient itself"
    wgrad("residual d/dK", suf, k.grad, ref.grad["ktab"], ref.Sgrad["ktab"], N, where)
    # split_x: exact, forward and backward
    x = leaf(c["u"], suf)
    xs = ops.split_x(x, pid, ntab)
    want = c["u"] if c["pid"] is None else gr.split_x(c["u"], c["pid"], ntab)
    assert xs.dtype == gr.DT[suf] and torch.equal(xs.cpu().double(), want)
    gs = gr.draw(gr.rng_for(H, W, 11), B, ntab, H, W)
    xs.backward(dev(gs, suf))
    want = gs if c["pid"] is None else torch.gather(gs, 1, c["pid"].expand(B, 1, H, W))
    assert torch.equal(x.grad.cpu().double(), want)
    # per-sample interior norms of the residual, and of a field itself (f = None)
    if H >= 3 and W >= 3:
        ref = R["residual"]
        inner = lambda t: t[..., 1:-1, 1:-1].reshape(B, -1)
        n, m = gr.FIELD["residual"]
        Ni = (H - 2) * (W - 2)
        for form, got, v, b in (("residual_norm", ops.residual_norm(dev(c["u"], suf), dev(c["f"], suf),
                                                                     dev(c["ktab"], suf), pid),
                                 inner(ref.out), 2 * (n + m) * gr.U[suf] * inner(ref.S)),
                                ("residual_norm f=None", ops.residual_norm(dev(c["u"], suf)), inner(c["u"]),
                                 torch.zeros(B, Ni, dtype=torch.float64))):
            want = v.norm(dim=1)
            assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
            gr.check(form, suf, gr.ratio((got.cpu() - want).abs(), gr.norm_bound(b, want, Ni)), where)


JACOBI = [(H, W, B, ntab, kind) for H, W, B, ntab in gr.SAME for kind in ("none", "bcast", "sample")
          if kind != "sample" or B >= 2]


@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,ntab,kind", JACOBI, ids=ids(JACOBI))
def test_jacobi(H, W, B, ntab, kind, suf):
    """Forward, d/du, d/df and d/dK with geo / bc absent, broadcast and per sample (geo_bstride = bc_bstride = H W)."""
    from feanet_amd import ops
    R = same_refs(H, W, B, ntab, kind)
    c, ref, where, N, dt = R["c"], R["jacobi"], f"{H}x{W} B={B} ntab={ntab} {kind}", B * H * W, gr.DT[suf]
    if kind == "sample":
        assert c["geo"].shape[0] == B and not torch.equal(c["geo"][0], c["geo"][1])
    u, f, k = leaf(c["u"], suf), leaf(c["f"], suf), leaf(c["ktab"], suf)
    out = ops.jacobi_sweep(u, f, k, dev(c["omd"], suf), dpid(c["pid"]), dev(c["geo"], suf), dev(c["bc"], suf))
    field("jacobi", suf, out, ref.out, ref.S, "jacobi", where)
    out.backward(dev(c["g"], suf))
    field("jacobi d/du", suf, u.grad, ref.grad["u"], ref.Sgrad["u"], "jacobi_adj", where)
    field("jacobi d/df", suf, f.grad, ref.grad["f"], ref.Sgrad["f"], "jacobi_adj_f", where)
    # the weight-gradient kernel at the inputs it was given: gf is the op's own d/df, u0 = u geo + bc in T
    u0 = c["u"].to(dt) * (gr.interior_mask(H, W, dt) if c["geo"] is None else c["geo"].to(dt))
    if c["bc"] is not None:
        u0 = u0 + c["bc"].to(dt)
    want, S = gr.stencil_wgrad(f.grad.cpu().double(), u0.double().expand(B, 1, H, W), c["pid"], ntab, -1.0)
    wgrad("jacobi d/dK (kernel)", suf, k.grad, want, S, N, where)
    # and the whole composition against the fp64 sweep: four T roundings enter every product
    wgrad("jacobi d/dK (composition)", suf, k.grad, ref.grad["ktab"], ref.Sgrad["ktab"], N, where, roundings=4)


# ----------------------------------------------------------------------------- transfer operators
@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,C,ntab", gr.TRANSFER, ids=ids(gr.TRANSFER))
def test_restrict_prolong(H, W, B, C, ntab, suf):
    from feanet_amd import ops
    R = transfer_refs(H, W, B, C, ntab)
    c, pidmode, where = R["c"], R["pidmode"], f"{H}x{W} B={B} C={C} ntab={ntab}"
    Hc, Wc = c["Hc"], c["Wc"]
    ref = R["restrict"]
    x, rt = leaf(c["x"], suf), dev(c["rtab"], suf).requires_grad_(not pidmode)
    fc = ops.restrict(x, rt, gr.W0, dpid(c["pid"]))
    field("restrict", suf, fc, ref.out, ref.S, gr.field_nm("restrict", C), where)
    fc.backward(dev(c["gc"], suf))
    field("restrict d/dx", suf, x.grad, ref.grad["x"], ref.Sgrad["x"], "restrict_adj", where)
    if not pidmode:
        wgrad("restrict d/dR", suf, rt.grad, ref.grad["rtab"], ref.Sgrad["rtab"], B * (Hc - 2) * (Wc - 2), where)
    ref = R["prolong"]
    e, pt, add = leaf(c["e"], suf), dev(c["ptab"], suf).requires_grad_(not pidmode), leaf(c["add"], suf)
    out = ops.prolong(e, pt, gr.W1, dpid(c["pidc"]), add)
    field("prolong", suf, out, ref.out, ref.S, gr.field_nm("prolong", C), where)
    out.backward(dev(c["gf"], suf))
    field("prolong d/de", suf, e.grad, ref.grad["e"], ref.Sgrad["e"], "prolong_adj", where)
    assert torch.equal(add.grad.cpu().double(), c["gf"]), "prolong d/dadd is the upstream gradient itself"
    if not pidmode:
        wgrad("prolong d/dP", suf, pt.grad, ref.grad["ptab"], ref.Sgrad["ptab"], B * Hc * Wc, where)
    if H == 3:     # no interior coarse node: the restriction and all its gradients are exactly zero
        assert not fc.any() and not x.grad.any() and not rt.grad.any()


# ----------------------------------------------------------------------------- <A x, y> = <x, A^T y> in f32
def _dot(a, b):
    return float((a.detach().cpu().double() * b.detach().cpu().double()).sum())


def _identity(op, Ax, y, x, ATy, S_Ax, nm, where):
    """tolerance: 2 (n + m) u times the sum of the absolute products, sum |y| S(A x) = sum |x| S(A^T y)"""
    n, m = gr.FIELD[nm]
    P = float((y.abs() * S_Ax).sum())
    d = abs(_dot(Ax, y) - _dot(x, ATy))
    tol = 2 * (n + m) * gr.U["f32"] * P
    gr.check(f"identity {op}", "f32", d / tol if tol else (float("inf") if d else 0.0), where)


@pytest.mark.parametrize("H,W,B,ntab", gr.SAME[3:], ids=ids(gr.SAME[3:]))
def test_adjoint_identity_same_grid(H, W, B, ntab):
    from feanet_amd import ops
    kind = "sample" if B >= 2 else "bcast"
    c = same_refs(H, W, B, ntab, kind)["c"]
    where, pid = f"{H}x{W} B={B} ntab={ntab}", dpid(c["pid"])
    x, y = c["u"], c["g"]
    xd = leaf(x, "f32")
    Ax = ops.knet_apply(xd, dev(c["ktab"], "f32"), pid)
    Ax.backward(dev(y, "f32"))
    _identity("knet", Ax, y, x, xd.grad, gr.knet(x.abs(), c["ktab"].abs(), c["pid"]), "knet_adj", where)
    # the sweep is linear in u for f = 0 and no boundary values
    xd = leaf(x, "f32")
    zero = torch.zeros_like(x)
    Ax = ops.jacobi_sweep(xd, dev(zero, "f32"), dev(c["ktab"], "f32"), dev(c["omd"], "f32"), pid, dev(c["geo"], "f32"))
    Ax.backward(dev(y, "f32"))
    S = gr.jacobi(x.abs(), zero, c["ktab"].abs(), c["omd"], c["pid"], c["geo"], None, absolute=True)
    _identity("jacobi", Ax, y, x, xd.grad, S, "jacobi_adj", where)


@pytest.mark.parametrize("H,W,B,C,ntab", gr.TRANSFER[1:], ids=ids(gr.TRANSFER[1:]))
def test_adjoint_identity_transfer(H, W, B, C, ntab):
    from feanet_amd import ops
    c = transfer_refs(H, W, B, C, ntab)["c"]
    where = f"{H}x{W} B={B} C={C} ntab={ntab}"
    xd = leaf(c["x"], "f32")
    Ax = ops.restrict(xd, dev(c["rtab"], "f32"), gr.W0, dpid(c["pid"]))
    Ax.backward(dev(c["gc"], "f32"))
    S = gr.restrict(c["x"].abs(), c["rtab"].abs(), gr.W0, c["pid"], absolute=True)
    _identity("restrict", Ax, c["gc"], c["x"], xd.grad, S, "restrict_adj", where)
    ed = leaf(c["e"], "f32")
    Ae = ops.prolong(ed, dev(c["ptab"], "f32"), gr.W1, dpid(c["pidc"]))
    Ae.backward(dev(c["gf"], "f32"))
    S = gr.prolong(c["e"].abs(), c["ptab"].abs(), gr.W1, c["pidc"], absolute=True)
    _identity("prolong", Ae, c["gf"], c["e"], ed.grad, S, "prolong_adj", where)


# ----------------------------------------------------------------------------- upstream gradients of any layout
@pytest.mark.parametrize("suf", gr.SUFS)
def test_upstream_gradient_layouts(suf):
    """A stride-0 expanded gradient (y.sum().backward()) and a channels-sliced view give bitwise the gradients of the
    same values held in a plain contiguous tensor."""
    from feanet_amd import ops
    c = same_refs(5, 63, 2, 16, "sample")["c"]
    t = transfer_refs(9, 127, 2, 16, 16)["c"]
    pid = dpid(c["pid"])
    omd, geo, bc = dev(c["omd"], suf), dev(c["geo"], suf), dev(c["bc"], suf)
    calls = {
        "knet": (lambda u, k: ops.knet_apply(u, k, pid), (c["u"], c["ktab"])),
        "residual": (lambda u, f, k: ops.residual(u, f, k, pid), (c["u"], c["f"], c["ktab"])),
        "jacobi": (lambda u, f, k: ops.jacobi_sweep(u, f, k, omd, pid, geo, bc), (c["u"], c["f"], c["ktab"])),
        "split_x": (lambda x: ops.split_x(x, pid, 16), (c["u"],)),
        "restrict": (lambda x, r: ops.restrict(x, r, gr.W0), (t["x"], t["rtab"])),
        "prolong": (lambda e, p, a: ops.prolong(e, p, gr.W1, None, a), (t["e"], t["ptab"], t["add"])),
    }

    def grads(fn, inputs, make_g):
        xs = [leaf(x, suf) for x in inputs]
        out = fn(*xs)
        g = make_g(out)
        if g is None:
            out.sum().backward()
        else:
            out.backward(g)
        return [x.grad for x in xs]

    for name, (fn, inputs) in calls.items():
        ones = grads(fn, inputs, torch.ones_like)
        summed = grads(fn, inputs, lambda out: None)
        for a, b in zip(ones, summed):
            assert torch.equal(a, b), f"{name}: sum().backward() differs from a contiguous gradient of ones"
        big = {}

        def sliced(out):
            Cn = out.shape[1]
            big["g"] = dev(gr.draw(gr.rng_for(5, len(name)), out.shape[0], 3 * Cn, *out.shape[2:]), suf)
            v = big["g"][:, Cn:2 * Cn]
            assert not v.is_contiguous()
            return v
        got = grads(fn, inputs, sliced)
        want = grads(fn, inputs, lambda out: big["g"][:, out.shape[1]:2 * out.shape[1]].contiguous())
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"{name}: a channels-sliced gradient differs from its contiguous copy"


# ----------------------------------------------------------------------------- caller-owned outputs and workspaces
class Guarded:
    """nbytes of device memory inside a canary-filled allocation"""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + PAD

    def body(self, dtype=torch.uint8):
        return self.buf[PAD:PAD + self.n].view(dtype)

    def check(self, what, esz=None):
        assert bool((self.buf[:PAD] == CANARY).all()), f"{what}: bytes before the buffer were written"
        assert bool((self.buf[PAD + self.n:] == CANARY).all()), f"{what}: bytes behind the buffer were written"
        if esz:
            untouched = (self.body().reshape(-1, esz) == CANARY).all(1)
            assert not bool(untouched.any()), f"{what}: {int(untouched.sum())} elements never stored"


def esz(suf):
    return 4 if suf == "f32" else 8


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,ntab", [gr.SAME[1], gr.SAME[5], gr.SAME[7]], ids=ids([gr.SAME[1], gr.SAME[5], gr.SAME[7]]))
def test_field_adjoint_write_sets_same_grid(H, W, B, ntab, suf):
    from feanet_amd import _lib
    kind = "sample" if B >= 2 else "bcast"
    R = same_refs(H, W, B, ntab, kind)
    c, dt, where = R["c"], gr.DT[suf], f"{H}x{W} B={B} ntab={ntab}"
    g, k, omd, geo, pid = dev(c["g"], suf), dev(c["ktab"], suf), dev(c["omd"], suf), dev(c["geo"], suf), dpid(c["pid"])
    nb = B * H * W * esz(suf)
    out = Guarded(nb)
    _lib.call("knet_apply_adj", dt, g.data_ptr(), out.ptr, ops_ptr(pid), k.data_ptr(), ntab, B, H, W, stream())
    torch.cuda.synchronize()
    out.check("knet_apply_adj out", esz(suf))
    ref = gr.knet_ref(c, ("u",))
    field("knet_apply_adj", suf, out.body(dt).reshape(B, 1, H, W), ref.grad["u"], ref.Sgrad["u"], "knet_adj", where)
    gu, gf = Guarded(nb), Guarded(nb)
    gs = 0 if geo.shape[0] == 1 else H * W
    _lib.call("jacobi_sweep_adj", dt, g.data_ptr(), gu.ptr, gf.ptr, ops_ptr(pid), k.data_ptr(), omd.data_ptr(), ntab,
              geo.data_ptr(), gs, B, H, W, stream())
    torch.cuda.synchronize()
    gu.check("jacobi_sweep_adj gu", esz(suf)), gf.check("jacobi_sweep_adj gf", esz(suf))
    ref = R["jacobi"]
    field("jacobi_sweep_adj gu", suf, gu.body(dt).reshape(B, 1, H, W), ref.grad["u"], ref.Sgrad["u"], "jacobi_adj", where)
    field("jacobi_sweep_adj gf", suf, gf.body(dt).reshape(B, 1, H, W), ref.grad["f"], ref.Sgrad["f"], "jacobi_adj_f",
          where)
    # gf is optional: gu alone is the same
    gu2 = Guarded(nb)
    _lib.call("jacobi_sweep_adj", dt, g.data_ptr(), gu2.ptr, None, ops_ptr(pid), k.data_ptr(), omd.data_ptr(), ntab,
              geo.data_ptr(), gs, B, H, W, stream())
    torch.cuda.synchronize()
    gu2.check("jacobi_sweep_adj gu (no gf)", esz(suf))
    assert torch.equal(gu2.body(), gu.body())


def ops_ptr(t):
    return None if t is None else t.data_ptr()


TR_WS = [gr.TRANSFER[0], gr.TRANSFER[3], gr.TRANSFER[4], gr.TRANSFER[5]]


@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,C,ntab", TR_WS, ids=ids(TR_WS))
def test_field_adjoint_write_sets_transfer(H, W, B, C, ntab, suf):
    from feanet_amd import _lib
    R = transfer_refs(H, W, B, C, ntab)
    c, dt, where = R["c"], gr.DT[suf], f"{H}x{W} B={B} C={C} ntab={ntab}"
    Hc, Wc = c["Hc"], c["Wc"]
    gc, gf, rt, pt = dev(c["gc"], suf), dev(c["gf"], suf), dev(c["rtab"], suf), dev(c["ptab"], suf)
    pid, pidc = dpid(c["pid"]), dpid(c["pidc"])
    gx = Guarded(B * C * H * W * esz(suf))
    _lib.call("restrict_adj", dt, gc.data_ptr(), C, gx.ptr, ops_ptr(pid), rt.data_ptr(), ntab, gr.W0, B, H, W, stream())
    torch.cuda.synchronize()
    gx.check("restrict_adj gx", esz(suf))
    ref = R["restrict"]
    field("restrict_adj", suf, gx.body(dt).reshape(B, C, H, W), ref.grad["x"], ref.Sgrad["x"], "restrict_adj", where)
    ge = Guarded(B * C * Hc * Wc * esz(suf))
    _lib.call("prolong_adj", dt, gf.data_ptr(), C, ge.ptr, ops_ptr(pidc), pt.data_ptr(), ntab, gr.W1, B, Hc, Wc,
              stream())
    torch.cuda.synchronize()
    ge.check("prolong_adj ge", esz(suf))
    ref = R["prolong"]
    field("prolong_adj", suf, ge.body(dt).reshape(B, C, Hc, Wc), ref.grad["e"], ref.Sgrad["e"], "prolong_adj", where)


def _weight_grad_runs(name, suf, launch, nout, ws_bytes):
    """launch(gw_ptr, ws_ptr): the result with a NaN-filled workspace of exactly ws_bytes, again on the used
    workspace, and with a zeroed one: finite, bitwise equal, nothing written outside gw and ws.  -> gw [nout]"""
    dt = gr.DT[suf]
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    runs = []
    for fill in (float("nan"), None, 0.0):
        if fill is not None:
            ws = Guarded(ws_bytes)
            ws.body(torch.float64).fill_(fill)
        gw = Guarded(nout * esz(suf))
        launch(gw.ptr, ws.ptr)
        torch.cuda.synchronize()
        gw.check(f"{name} gw", esz(suf)), ws.check(f"{name} ws")
        runs.append(gw.body(dt).clone())
    assert bool(torch.isfinite(runs[0]).all()), f"{name}: the result depends on what the workspace held"
    assert torch.equal(runs[0].view(torch.uint8), runs[1].view(torch.uint8)), f"{name}: two launches differ"
    assert torch.equal(runs[0].view(torch.uint8), runs[2].view(torch.uint8)), f"{name}: NaN and zeroed workspace differ"
    return runs[0]


@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,ntab", [gr.SAME[1], gr.SAME[3], gr.SAME[5], gr.SAME[7]],
                         ids=ids([gr.SAME[1], gr.SAME[3], gr.SAME[5], gr.SAME[7]]))
def test_stencil_weight_grad_workspace(H, W, B, ntab, suf):
    from feanet_amd import _lib
    c, dt, where = same_refs(H, W, B, ntab)["c"], gr.DT[suf], f"{H}x{W} B={B} ntab={ntab}"
    g, u, pid = dev(c["g"], suf), dev(c["u"], suf), dpid(c["pid"])
    size = getattr(_lib.lib(), f"fea_stencil_weight_grad_ws_bytes_{suf}")
    scale = -1.5

    def run(b0, nb):
        off = b0 * H * W * esz(suf)
        return _weight_grad_runs("stencil_weight_grad", suf, lambda gw, ws: _lib.call(
            "stencil_weight_grad", dt, g.data_ptr() + off, u.data_ptr() + off, ops_ptr(pid), ntab, scale, gw, ws, nb,
            H, W, stream()), ntab * 9, int(size(ntab, nb, H, W)))
    gw = run(0, B)
    want, S = gr.stencil_wgrad(c["g"], c["u"], c["pid"], ntab, scale)
    wgrad("stencil_weight_grad", suf, gw.reshape(ntab, 3, 3), want, S, B * H * W, where)
    # a sample's contribution does not depend on the batch it is in: every per-sample run is within its own bound,
    # so the batch equals their sum within the bound of the batch plus the bounds of the samples
    tol = gr.wgrad_bound(want, S, B * H * W, suf)
    total = torch.zeros_like(want)
    for b in range(B):
        wb, Sb = gr.stencil_wgrad(c["g"][b:b + 1], c["u"][b:b + 1], c["pid"], ntab, scale)
        total += run(b, 1).cpu().double().reshape(ntab, 3, 3)
        tol = tol + gr.wgrad_bound(wb, Sb, H * W, suf)
    gr.check("stencil_weight_grad per sample", suf, gr.ratio((gw.cpu().double().reshape(ntab, 3, 3) - total).abs(), tol),
             where)


@pytest.mark.parametrize("suf", gr.SUFS)
@pytest.mark.parametrize("H,W,B,C,ntab", [gr.TRANSFER[0], gr.TRANSFER[1], gr.TRANSFER[3], gr.TRANSFER[5]],
                         ids=ids([gr.TRANSFER[0], gr.TRANSFER[1], gr.TRANSFER[3], gr.TRANSFER[5]]))
def test_transfer_weight_grad_workspace(H, W, B, C, ntab, suf):
    from feanet_amd import _lib
    c, dt, where = transfer_refs(H, W, B, C, ntab)["c"], gr.DT[suf], f"{H}x{W} B={B} C={C}"
    Hc, Wc = c["Hc"], c["Wc"]
    size = getattr(_lib.lib(), f"fea_transfer_weight_grad_ws_bytes_{suf}")
    # restriction weights: cf = g [B, 1, Hc, Wc], ff = x (split); prolongation weights: cf = e (split), ff = g
    for mode, cf, c_split, ff, f_split, interior, scale, N in (
            ("R", c["gc"], False, c["x"], True, True, gr.W0, (Hc - 2) * (Wc - 2)),
            ("P", c["e"], True, c["gf"], False, False, gr.W1, Hc * Wc)):
        cd, fd = dev(cf, suf), dev(ff, suf)

        def run(b0, nb):
            co = b0 * cf.shape[1] * Hc * Wc * esz(suf)
            fo = b0 * ff.shape[1] * H * W * esz(suf)
            return _weight_grad_runs(f"transfer_weight_grad {mode}", suf, lambda gw, ws: _lib.call(
                "transfer_weight_grad", dt, cd.data_ptr() + co, int(c_split), fd.data_ptr() + fo, int(f_split), C,
                int(interior), scale, gw, ws, nb, Hc, Wc, stream()), C * 9, int(size(C, nb, Hc, Wc)))
        gw = run(0, B).cpu().double().reshape(C, 3, 3)
        want, S = gr.transfer_wgrad(cf, c_split, ff, f_split, C, interior, scale)
        gr.check(f"transfer_weight_grad {mode}", suf, gr.wgrad_ratio(gw, want, S, B * N, suf), where)
        tol = gr.wgrad_bound(want, S, B * N, suf)
        total = torch.zeros_like(want)
        for b in range(B):
            wb, Sb = gr.transfer_wgrad(cf[b:b + 1], c_split, ff[b:b + 1], f_split, C, interior, scale)
            total += run(b, 1).cpu().double().reshape(C, 3, 3)
            tol = tol + gr.wgrad_bound(wb, Sb, N, suf)
        gr.check(f"transfer_weight_grad {mode} per sample", suf, gr.ratio((gw - total).abs(), tol), where)
