"""Argument checks of the generic NCHW entry points (include/feanet_hip.h section (1): every fea_*_{f32,f64} of
_lib._SIGS that is neither framed (mg_) nor Krylov (pcg_)): each returns FEA_EINVAL for NULL operands, bad sizes, bad
table counts and aliased stencil operands.  Modelled on test_mg_host.py: every call here must be rejected, so nothing
is launched and no GPU is needed; the pointers are fake addresses that a rejected call never touches.

A case is the accepted call of its entry point (base()) with one thing broken.

Not here, because the library accepts them: a NULL pattern map with several table rows (every node then has pattern 0);
r == f in fea_residual, out == f in fea_jacobi_sweep and out == add in fea_prolong (those operands are read at the
node itself only); gu == gf in fea_jacobi_sweep_adj is not checked either; any geo / bc stride (the caller's layout);
C of any size in fea_split_x; an ntab that does not match the pattern map's ids (the ids are data)."""
import pytest

FEA_EINVAL = -1
MAXP = 16
SUFS = ["f32", "f64"]
SHAPES = [(33, 17), (5, 131)]          # fine H x W, odd; the coarse grid is (H + 1) / 2 x (W + 1) / 2

OPTIONAL = {"pid", "pidc", "geo", "bc", "add", "gf"}
OPTIONAL_IN = {"residual_norm": {"f", "ktab"}}     # (f == NULL: the norm of u itself; ktab only with f)
TRANSFER = ("restrict", "restrict_adj", "prolong", "prolong_adj")
COARSE = ("prolong", "prolong_adj", "transfer_weight_grad")


def generic_entries():
    from feanet_amd import _lib
    return sorted(n for n in _lib._SIGS if not n.startswith(("mg_", "pcg_")))


ENTRIES = ["jacobi_sweep", "jacobi_sweep_adj", "jacobi_sweep_pbc", "knet_apply", "knet_apply_adj", "pbc_pad", "prolong",
           "prolong_adj", "residual", "residual_norm", "restrict", "restrict_adj", "split_x", "stencil_weight_grad",
           "transfer_weight_grad"]


def sig(name):
    """[(type, parameter)] of the entry point, without the stream"""
    from feanet_amd import _lib
    return [tuple(p.split()) for p in _lib._SIGS[name]][:-1]


def base(name, H, W):
    """Arguments of a call that the library accepts: one pattern, one channel, no optional operand."""
    a = {}
    ptrs = sorted(n for t, n in sig(name) if t == "P")
    for t, n in sig(name):
        if t == "P":
            opt = n in OPTIONAL or n in OPTIONAL_IN.get(name, ())
            a[n] = None if (opt and n not in ("f", "ktab")) else 0x10000 * (1 + ptrs.index(n))
        elif t == "S":
            a[n] = 1.0
        else:
            a[n] = 0
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    a.update({k: v for k, v in dict(B=2, H=H, W=W, Hc=Hc, Wc=Wc, N=H, ntab=1, C=1, lo=1, hi=2, c_split=0, f_split=1,
                                    interior=1).items() if k in a})
    return a


def call(name, suf, a):
    from feanet_amd import _lib
    return getattr(_lib.lib(), f"fea_{name}_{suf}")(*[a[n] for _, n in sig(name)], None)


def cases(name, H, W):
    """(label, arguments) of every call of `name` that must be rejected."""
    params = [n for _, n in sig(name)]
    has = lambda *n: all(x in params for x in n)
    out = []

    def bad(label, **over):
        a = base(name, H, W)
        a.update(over)
        out.append((label, a))

    # --- required pointers
    for t, n in sig(name):
        if t == "P" and n not in OPTIONAL and n not in OPTIONAL_IN.get(name, ()):
            bad(f"NULL {n}", **{n: None})
    if name == "residual_norm":
        bad("f without ktab", ktab=None)
    # --- sizes
    bad("B = 0", B=0), bad("B = -1", B=-1), bad("B = 65536", B=65536)
    for n in ("H", "W", "Hc", "Wc", "N"):
        if has(n):
            bad(f"{n} = 0", **{n: 0}), bad(f"{n} = -3", **{n: -3})
    if name in ("restrict", "restrict_adj"):
        bad("even H", H=H + 1), bad("even W", W=W + 1), bad("H = 1", H=1), bad("W = 1", W=1), bad("H = 2", H=2)
    if name in COARSE:
        bad("Hc = 1", Hc=1), bad("Wc = 1", Wc=1)
    if name == "residual_norm":
        bad("H = 2", H=2), bad("W = 2", W=2)
    if name in ("pbc_pad", "jacobi_sweep_pbc"):
        bad("N = 1 (no period)", N=1)
    if name == "pbc_pad":
        bad("lo + hi = 65", lo=33, hi=32), bad("lo = -1", lo=-1), bad("hi = -1", hi=-1)
    # --- tables and channels
    if has("ntab"):
        bad("ntab = 0", ntab=0), bad("ntab = 17", ntab=MAXP + 1), bad("ntab = -1", ntab=-1)
    if name == "split_x":
        bad("C = 0", C=0)
    if name == "transfer_weight_grad":
        bad("C = 0", C=0), bad("C = 17", C=MAXP + 1)
    if name in TRANSFER:
        bad("C = 0", C=0), bad("C = 4, ntab = 3", C=4, ntab=3), bad("C = 4, ntab = 1", C=4, ntab=1)
        bad("C = 3, ntab = 4", C=3, ntab=4), bad("C = ntab = 17", C=MAXP + 1, ntab=MAXP + 1)
    # --- aliasing: a stencil read of the aliased operand would race with the stores
    for o, i in (("out", "u"), ("y", "u"), ("r", "u"), ("out", "g"), ("gu", "g"), ("gf", "g")):
        if has(o, i) and name != "residual_norm":          # (its `out` holds the norms, not a field)
            bad(f"{o} == {i}", **{o: base(name, H, W)[i]})
    return out


@pytest.mark.parametrize("suf", SUFS)
@pytest.mark.parametrize("name", ENTRIES)
def test_rejected(name, suf):
    for H, W in SHAPES:
        cs = cases(name, H, W)
        assert len(cs) >= 8
        for label, a in cs:
            assert call(name, suf, a) == FEA_EINVAL, f"fea_{name}_{suf} at {H} x {W}: {label} accepted"


def test_covers_every_generic_entry_point():
    assert ENTRIES == generic_entries()


def test_aliasing_rules_are_the_documented_ones():
    """The stencil operands that may not alias an output, entry by entry (the header states them)."""
    want = {"knet_apply": ["y == u"], "residual": ["r == u"], "jacobi_sweep": ["out == u"],
            "jacobi_sweep_pbc": ["out == u"], "knet_apply_adj": ["out == g"], "jacobi_sweep_adj": ["gu == g", "gf == g"]}
    for name in ENTRIES:
        got = [label for label, _ in cases(name, *SHAPES[0]) if " == " in label]
        assert got == want.get(name, []), name
