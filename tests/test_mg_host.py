"""Argument checks of the framed multigrid entry points (every fea_mg_*_{f32,f64} of _lib._SIGS, and
fea_norm_append): each returns FEA_EINVAL for NULL operands, a bad layout, bad grid sizes, bad table counts,
aliased outputs and out-of-range windows.  Every call here must be rejected, so nothing is launched and no GPU is
needed: the pointers are fake addresses that a rejected call never touches (the pointer arrays and the rectangle
list that the library reads on the host are real).

A case is the accepted call of its entry point (base(), or its two-material form) with one thing broken.

Not here, because the library accepts them: fea_mg_prolong_sweep with a prolongation table of neither 1 nor ntab
patterns (both counts > 1); a pitch that is no multiple of a 128-byte line in the learned-smoother and tail entry
points (they need ld >= W + a line only); any ld / bstride in fea_mg_coarse_tail (unchecked); out == u in
fea_mg_residual_norm (its `out` holds the norms)."""
import ctypes

import pytest

FEA_EINVAL = -1
MAXP = 16                      # FEA_MAX_PATTERNS
SHAPES = [(33, 33), (33, 17)]
SUFS = ["f32", "f64"]

_keep = []                     # host arrays handed to the library


def fake(name):
    """A distinct fake device address per operand name."""
    return 0x10000 * (1 + sorted(PTRS).index(name))


def parr(*ptrs):
    a = (ctypes.c_void_p * len(ptrs))(*ptrs)
    _keep.append(a)
    return ctypes.cast(a, ctypes.c_void_p).value


def iarr(*v):
    a = (ctypes.c_int * len(v))(*v)
    _keep.append(a)
    return ctypes.cast(a, ctypes.c_void_p).value


PTRS = {"src", "dst", "geo", "bc", "u", "f", "out", "pid", "pidc", "pidc2", "ktab", "omd", "rtab", "ptab", "v_out", "fc",
        "fc2", "send", "u_out", "ec", "ec2", "norm_ws", "norm_hist", "norm_cnt", "ws", "u_raw", "hw", "f_t", "v_t",
        "u_t", "f_x", "v_x", "pid_levels", "gsrc", "e", "f0", "f1", "f2", "u0", "u1", "u2", "p0", "p1", "p2", "rects"}

# entry -> argument names in the order of include/feanet_hip.h (without the trailing stream)
ARGS = {
    "mg_pack": "src dst geo geo_bs bc bc_bs B H W ld bs",
    "mg_unpack": "src dst B H W ld bs",
    "mg_sweep": "u f out pid ktab omd ntab B H W ld bs",
    "mg_residual_restrict": "u f v_out fc pid ktab omd ntab rtab nrtab w0 B H W ld bs ldc bsc",
    "mg_zero_restrict_send": "f fc pid ktab omd ntab rtab nrtab w0 B H W ld bs ldc bsc send r0 r1 c0 c1",
    "mg_zero_restrict2": "f fc fc2 pid pidc ktab omd ntab rtab nrtab w0 B H W ld bs ldc bsc ldc2 bsc2",
    "mg_zero_restrict2_send": "f fc fc2 pid pidc ktab omd ntab rtab nrtab w0 B H W ld bs ldc bsc ldc2 bsc2 "
                              "send r0 r1 c0 c1",
    "mg_sweep_restrict": "u f u_out fc pid ktab omd ntab rtab nrtab w0 B H W ld bs ldc bsc norm_ws norm_hist norm_cnt",
    "mg_prolong_sweep": "u ec f out pid pidc ktab omd ntab ptab nptab w1 B H W ld bs ldc bsc",
    "mg_prolong2": "fc ec2 f out pid pidc pidc2 ktab omd ntab ptab nptab w1 B H W ld bs ldc bsc ldc2 bsc2",
    "mg_prolong_add": "u ec out pidc ptab nptab w1 B H W ld bs ldc bsc",
    "mg_residual_norm": "u f pid ktab ntab out ws B H W ld bs rlo rhi clo chi",
    "mg_cycle_join": "u ec f u_out fc pid pidc ktab omd ntab ptab nptab rtab nrtab w1 w0 B H W ld bs ldc bsc "
                     "norm_ws norm_hist norm_cnt",
    "mg_cycle_join_rects": "u ec f u_out fc pid pidc ktab omd ntab ptab nptab rtab nrtab w1 w0 B H W ld bs ldc bsc "
                           "nrect rects",
    "mg_hsweep": "u u_raw f out pid ktab omd ntab hw nlayers B H W ld bs",
    "mg_hsweep_restrict": "u u_raw f out fc pid ktab omd ntab hw nlayers rtab nrtab w0 B H W ld bs ldc bsc",
    "mg_prolong_hsweep": "u u_raw ec f out pid pidc ktab omd ntab hw nlayers ptab nptab w1 B H W ld bs ldc bsc",
    "mg_coarse_tail": "f_t v_t H W nlev ld bs pid_levels ktab omd ntab rtab ptab w0 w1 nu1 nu2 q2 B",
    "mg_coarse_tail_ext": "f_x v_x H W ld bs nlev ktab omd ntab rtab ptab w0 w1 B",
    "mg_hjac_tail": "f_t u_t H W nlev ld bs pid_levels ktab omd ntab rtab ptab hw nlayers w0 w1 nu1 nu2 B",
    "mg_mid_down": "fs pids k B H W ktab omd ntab rtab nrtab w0 TR TC",
    "mg_mid_down_gathered": "fs pids k B H W ktab omd ntab rtab nrtab w0 TR TC gsrc Pr Pc gcr gcc",
    "mg_mid_up": "fs e out pids k B H W ktab omd ntab ptab nptab w1 TR TC",
    "mg_hmid_down": "fs us pids B H W ktab omd ntab hw nlayers rtab nrtab w0 TT",
    "mg_hmid_up": "fs us e out pids B H W ktab omd ntab hw nlayers ptab nptab w1 TT",
}
HS = ("mg_hsweep", "mg_hsweep_restrict", "mg_prolong_hsweep")
TAILS = ("mg_coarse_tail", "mg_coarse_tail_ext", "mg_hjac_tail")
# the elements of the pointer arrays f, u and pid that each of these reads (k = 1: two levels; hmid: three)
NELEM = {"mg_mid_down": (2, 0, 1), "mg_mid_down_gathered": (2, 0, 1), "mg_mid_up": (1, 0, 2), "mg_hmid_down": (3, 2, 2),
         "mg_hmid_up": (2, 2, 3)}
MIDS = ("mg_mid_down", "mg_mid_down_gathered", "mg_mid_up", "mg_hmid_down", "mg_hmid_up")


def esz(suf):
    return 4 if suf == "f32" else 8


def base(name, suf, H, W):
    """Arguments of a call that the library accepts: one pattern, no optional operand but those it needs."""
    from feanet_amd import _lib
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    a = {n: fake(n) for n in PTRS}
    a.update(pid=None, pidc=None, pidc2=None, pid_levels=None, pids=None, norm_ws=None, norm_hist=None, norm_cnt=None,
             u_raw=None, geo_bs=0, bc_bs=0, B=1, H=H, W=W, ntab=1, nrtab=1, nptab=1, w0=4.0, w1=1.0, nlayers=1,
             nlev=2, nu1=1, nu2=1, q2=0, k=1, TR=4, TC=4, TT=4, rlo=0, rhi=0, clo=0, chi=0,
             r0=1, r1=3, c0=1, c1=3, nrect=1, rects=iarr(1, Hc - 1, 1, W - 1),
             Pr=2, Pc=2, gcr=(H - 1) // 2, gcc=(W - 1) // 2,
             fs=parr(fake("f0"), fake("f1"), fake("f2")), us=parr(fake("u0"), fake("u1"), fake("u2")))
    a["ld"], a["bs"] = _lib.mg_layout(H, W, esz(suf))
    a["ldc"], a["bsc"] = _lib.mg_layout(Hc, Wc, esz(suf))
    a["ldc2"], a["bsc2"] = _lib.mg_layout((Hc + 1) // 2, (Wc + 1) // 2, esz(suf))
    return a


def multi(name, suf, H, W):
    """The accepted two-material call: 16 patterns in every table the entry point has, every pattern map."""
    a = base(name, suf, H, W)
    a.update(ntab=MAXP, nrtab=MAXP, nptab=MAXP, pid=fake("pid"), pidc=fake("pidc"), pidc2=fake("pidc2"),
             pid_levels=fake("pid_levels"), pids=parr(fake("p0"), fake("p1"), fake("p2")))
    return a


def call(name, suf, a):
    from feanet_amd import _lib
    fn = getattr(_lib.lib(), f"fea_{name}_{suf}")
    return fn(*[a[n] for n in ARGS[name].split()], None)


def cases(name, suf, H, W):
    """(label, arguments) of every call of `name` that must be rejected."""
    A = 128 // esz(suf)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    names = ARGS[name].split()
    has = lambda *n: all(x in names for x in n)
    out = []

    def bad(label, _from=None, **over):
        a = dict(_from or base(name, suf, H, W))
        a.update(over)
        out.append((label, a))

    def even(h, w):  # the same call on a grid with an even side, in that grid's own layout
        from feanet_amd import _lib
        ld, bs = _lib.mg_layout(h, w, esz(suf))
        return dict(H=h, W=w, ld=ld, bs=bs)

    m = multi(name, suf, H, W)
    # --- required pointers, batch
    optional = {"mg_pack": {"src", "geo", "bc"}, "mg_sweep": {"u"}, "mg_residual_restrict": {"u", "v_out", "omd"},
                "mg_prolong_sweep": {"u"}, "mg_hsweep": {"u"}, "mg_hsweep_restrict": {"u"}}.get(name, set())
    for n in names:
        if n in PTRS and n not in optional and n not in ("pid", "pidc", "pidc2", "pid_levels", "u_raw", "norm_ws",
                                                         "norm_hist", "norm_cnt"):
            bad(f"NULL {n}", **{n: None})
    for n in ("fs", "us"):
        if has(n):
            bad(f"NULL {n}", **{n: None})
    bad("B = 0", B=0)
    if name in ("mg_pack", "mg_unpack", "mg_hjac_tail") or name in HS or name in MIDS:
        bad("B = 65536", B=65536)
    if name == "mg_residual_restrict":
        bad("zero guess without omd", u=None, omd=None)
    # --- layout and sizes
    b = base(name, suf, H, W)
    if name in TAILS or name in HS:  # these need ld >= W + a line and bs >= (H + 2) ld; the tail checks neither
        if name != "mg_coarse_tail":
            bad("ld one element too small", ld=W + A - 1)
            bad("bs one element too small", bs=(H + 2) * b["ld"] - 1)
    elif name not in MIDS:
        bad("ld one line too small", ld=b["ld"] - A)
        bad("ld not a multiple of a line", ld=b["ld"] + 1)
        bad("bs one element too small", bs=b["bs"] - 1)
    if name == "mg_coarse_tail_ext":
        bad("H = 3", H=3), bad("W = 3", W=3)
    bad("H = 2", H=2), bad("W = 2", W=2)
    if has("ldc") or name in MIDS or name == "mg_coarse_tail_ext" or (name in TAILS and b["nlev"] > 1):
        bad("even H", **even(H + 1, W)), bad("even W", **even(H, W + 1))
    if has("ldc") and name in HS:
        bad("ldc one element too small", ldc=Wc + A - 1)
        bad("bsc one element too small", bsc=(Hc + 2) * b["ldc"] - 1)
    elif has("ldc"):
        bad("ldc one line too small", ldc=b["ldc"] - A)
        bad("ldc not a multiple of a line", ldc=b["ldc"] + 1)
        bad("bsc one element too small", bsc=b["bsc"] - 1)
    if has("ldc2"):
        bad("ldc2 one line too small", ldc2=b["ldc2"] - A)
        bad("bsc2 one element too small", bsc2=b["bsc2"] - 1)
    # --- tables
    if has("ntab"):
        bad("ntab = 0", ntab=0)
        bad("ntab = 17", m, ntab=MAXP + 1, nrtab=MAXP + 1, nptab=MAXP + 1)
        if name == "mg_coarse_tail_ext":
            bad("ntab = 2 (one material only)", m, ntab=2)
        for p in ("pid", "pidc", "pidc2", "pid_levels", "pids"):
            if has(p):
                bad(f"16 patterns without {p}", m, **{p: None})
    if name == "mg_prolong_add":
        bad("nptab = 0", nptab=0)
        bad("nptab = 17", m, nptab=MAXP + 1)
        bad("16 patterns without pidc", m, pidc=None)
    for n in ("nrtab", "nptab"):
        if has(n, "ntab"):
            if name != "mg_prolong_sweep":
                bad(f"{n} = 8 of 16", m, **{n: 8})
            bad(f"16 patterns, one {n[1]}tab", m, **{n: 1})
            if name in MIDS:
                bad(f"one pattern, {n} = 2", **{n: 2})
    if name == "mg_prolong_sweep":
        bad("nptab = 0", nptab=0)
        bad("nptab = 17", m, nptab=MAXP + 1)
        bad("one stencil, 16 ptab", m, ntab=1)
    # --- aliasing
    for o, i in (("out", "u"), ("u_out", "u")):
        if has(o, i) and name not in MIDS and name != "mg_residual_norm":  # (its `out` is the norms, not a field)
            bad(f"{o} == {i}", **{o: fake(i)})
    if name == "mg_prolong_sweep":
        bad("zero guess, out == f", u=None, out=fake("f"))
    # --- windows and rectangles
    if has("send"):
        hc, wc = ((Hc + 1) // 2, (Wc + 1) // 2) if has("ldc2") else (Hc, Wc)
        bad("r0 < 0", r0=-1), bad("c0 < 0", c0=-1)
        bad("empty rows", r1=1), bad("reversed rows", r0=3, r1=2)
        bad("empty columns", c1=1), bad("reversed columns", c0=3, c1=2)
        bad("rows past the coarse grid", r1=hc + 1), bad("columns past the coarse grid", c1=wc + 1)
    if name == "mg_cycle_join_rects":
        bad("nrect = 0", nrect=0), bad("nrect = 5", nrect=5, rects=iarr(*([1, Hc - 1, 1, W - 1] * 5)))
        for label, r in (("I0 = 0", (0, Hc - 1, 1, W - 1)), ("I1 past the grid", (1, Hc, 1, W - 1)),
                         ("empty rows", (3, 3, 1, W - 1)), ("reversed rows", (4, 3, 1, W - 1)),
                         ("c0 = 0", (1, Hc - 1, 0, W - 1)), ("even c0", (1, Hc - 1, 2, W - 1)),
                         ("c1 past the grid", (1, Hc - 1, 1, W)), ("even c1", (1, Hc - 1, 1, W - 3)),
                         ("empty columns", (1, Hc - 1, 5, 5)), ("reversed columns", (1, Hc - 1, 7, 5))):
            bad(label, rects=iarr(*r))
        bad("second rectangle bad", nrect=2, rects=iarr(1, 3, 1, W - 1, 3, Hc - 1, 2, W - 1))
    if name == "mg_residual_norm":
        bad("rlo = 0", rlo=0, rhi=H - 1), bad("rhi past the interior", rlo=1, rhi=H), bad("rhi < rlo", rlo=5, rhi=4)
        bad("clo = 0", clo=0, chi=W - 1), bad("chi past the interior", clo=1, chi=W), bad("chi < clo", clo=5, chi=4)
    if has("norm_hist"):
        bad("history without workspace", norm_hist=fake("norm_hist"), norm_cnt=fake("norm_cnt"))
        bad("history without counter", norm_hist=fake("norm_hist"), norm_ws=fake("norm_ws"))
    # --- learned smoother, tails, several levels per launch
    if has("nlayers"):
        bad("nlayers = -1", nlayers=-1), bad("nlayers = 4", nlayers=4), bad("layers without weights", hw=None)
    if has("u_raw") and "u" in optional:
        bad("u_raw without u", u=None, u_raw=fake("u_raw"))
    if has("nlev"):
        bad("nlev = 0", nlev=0), bad("nlev = 9", nlev=9), bad("a level below 3 nodes", nlev=6)
    if has("nu1"):
        bad("nu1 = -1", nu1=-1), bad("nu2 = -1", nu2=-1)
    if name in TAILS:
        bad("H past the tail's limit", H=257), bad("W past the tail's limit", W=257)
    if has("k"):
        bad("k = 0", k=0), bad("k = 5", k=5), bad("TR = 0", TR=0), bad("TC = 0", TC=0)
        bad("tile past the LDS", TR=4096, TC=4096)
    if has("TT"):
        bad("TT = 0", TT=0), bad("tile past the LDS", TT=4096)
    if has("Pr"):
        bad("Pr = 0", Pr=0, gcr=H - 1), bad("Pc = 0", Pc=0, gcc=W - 1), bad("gcr = 0", gcr=0), bad("gcc = 0", gcc=0)
        bad("blocks do not tile the rows", gcr=b["gcr"] - 1), bad("blocks do not tile the columns", gcc=b["gcc"] + 1)
    if name in MIDS:
        f = [fake("f0"), fake("f1"), fake("f2")]
        u = [fake("u0"), fake("u1"), fake("u2")]
        p = [fake("p0"), fake("p1"), fake("p2")]
        without = lambda v, j: parr(*[None if i == j else x for i, x in enumerate(v)])
        nf, nu, npid = NELEM[name]
        for j in range(nf):
            bad(f"NULL f[{j}]", fs=without(f, j))
        for j in range(nu):
            bad(f"NULL u[{j}]", us=without(u, j))
        for j in range(npid):
            bad(f"16 patterns, NULL pid[{j}]", m, pids=without(p, j))
        if name == "mg_hmid_down":
            bad("u[0] == f[0]", us=parr(f[0], u[1], u[2])), bad("u[1] == f[1]", us=parr(u[0], f[1], u[2]))
        if name == "mg_hmid_up":
            bad("out == f[0]", out=f[0]), bad("out == u[0]", out=u[0])
        if name == "mg_mid_up":
            bad("out == f[0]", out=f[0])
        if has("e"):
            bad("out == e", out=fake("e"))
    return out


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("name", sorted(ARGS))
def test_rejected(name, suf):
    for H, W in SHAPES:
        cs = cases(name, suf, H, W)
        assert len(cs) >= 8
        for label, a in cs:
            assert call(name, suf, a) == FEA_EINVAL, f"fea_{name}_{suf} at {H} x {W}: {label} accepted"


def test_covers_every_framed_entry_point():
    from feanet_amd import _lib
    assert sorted(ARGS) == sorted(n for n in _lib._SIGS if n.startswith("mg_"))
    for name, names in ARGS.items():
        assert len(names.split()) + 1 == len(_lib._SIGS[name]), name


def test_norm_append():
    from feanet_amd import _lib
    L = _lib.lib()
    ok = [fake("ws"), 64, 8, 2, 1, fake("norm_hist"), fake("norm_cnt"), None]   # ws stride per B nrows hist cnt stream
    for i in (0, 5, 6):
        a = list(ok)
        a[i] = None
        assert L.fea_norm_append(*a) == FEA_EINVAL
    for i, v in ((2, 0), (3, 0), (4, 0)):
        a = list(ok)
        a[i] = v
        assert L.fea_norm_append(*a) == FEA_EINVAL
    a = list(ok)
    a[1], a[4] = 15, 2                      # two rows of B * per = 16 partials overlap at a stride of 15
    assert L.fea_norm_append(*a) == FEA_EINVAL
