"""Argument checks of the Krylov entry points (fea_pcg_*): every one returns FEA_EINVAL for NULL operands, a
bad ld / bstride, ntab outside 1..16 and ntab > 1 without a pattern map.  Nothing is launched, so no GPU is
needed: the pointers are fake addresses that a rejected call never touches."""
import pytest

FEA_EINVAL = -1
H = W = 33
PTR = {"x": 0x1000, "f": 0x2000, "r": 0x3000, "p": 0x4000, "q": 0x5000, "z": 0x6000, "pid": 0x7000,
       "ktab": 0x8000, "sc": 0x9000, "part": 0xa000, "hist": 0xb000}


def layout(suf):
    from feanet_amd import _lib
    return _lib.mg_layout(H, W, 4 if suf == "f32" else 8)


# entry -> (operand names in order, has a stencil table?)
ENTRIES = {
    "pcg_residual": (["x", "f", "r", "pid", "ktab", "ntab", "part"], True),
    "pcg_direction": (["z", "p", "q", "pid", "ktab", "ntab", "sc", "part"], True),
    "pcg_update": (["p", "x", "r", "pid", "ktab", "ntab", "sc", "part"], True),
    "pcg_dot": (["r", "z", "part"], False),
}


def call(name, suf, over=None, ntab=1, B=1, ld=None, bs=None, h=H, w=W):
    from feanet_amd import _lib
    over = over or {}
    names, _ = ENTRIES[name]
    l0, b0 = layout(suf)
    args = []
    for a in names:
        if a == "ntab":
            args.append(ntab)
        elif a in over:
            args.append(over[a])
        elif a == "pid":
            args.append(PTR["pid"] if ntab > 1 else None)
        else:
            args.append(PTR[a])
    fn = getattr(_lib.lib(), f"fea_{name}_{suf}")
    return fn(*args, B, h, w, l0 if ld is None else ld, b0 if bs is None else bs, None)


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_operands(name, suf):
    names, _ = ENTRIES[name]
    for a in names:
        if a in ("ntab", "pid"):
            continue
        assert call(name, suf, over={a: None}) == FEA_EINVAL, f"{name}: NULL {a} accepted"
    assert call(name, suf, B=0) == FEA_EINVAL


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_layout(name, suf):
    l0, b0 = layout(suf)
    A = 128 // (4 if suf == "f32" else 8)
    assert call(name, suf, ld=l0 - A) == FEA_EINVAL          # pitch too small for the strips' loads
    assert call(name, suf, ld=l0 + 1) == FEA_EINVAL          # not a multiple of a 128-byte line
    assert call(name, suf, bs=b0 - 1) == FEA_EINVAL          # samples overlap
    assert call(name, suf, h=2) == FEA_EINVAL                # fewer than 3 rows
    assert call(name, suf, w=2) == FEA_EINVAL


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(n for n, (_, tab) in ENTRIES.items() if tab))
def test_bad_tables(name, suf):
    assert call(name, suf, ntab=0) == FEA_EINVAL
    assert call(name, suf, ntab=17, over={"pid": PTR["pid"]}) == FEA_EINVAL
    assert call(name, suf, ntab=16, over={"pid": None}) == FEA_EINVAL   # ntab > 1 needs the pattern map


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_aliasing_rules(suf):
    """The direction must ping-pong (p_out is neither p_in nor z); the update's three fields are distinct; the
    residual may overwrite f but not x."""
    assert call("pcg_direction", suf, over={"q": PTR["p"]}) == FEA_EINVAL
    assert call("pcg_direction", suf, over={"q": PTR["z"]}) == FEA_EINVAL
    assert call("pcg_update", suf, over={"x": PTR["p"]}) == FEA_EINVAL
    assert call("pcg_update", suf, over={"r": PTR["x"]}) == FEA_EINVAL
    assert call("pcg_residual", suf, over={"r": PTR["x"]}) == FEA_EINVAL


def test_scalar_step_and_parts():
    from feanet_amd import _lib
    L = _lib.lib()
    ok = (PTR["part"], 4, PTR["sc"], PTR["hist"], 8, 1, 0, None)
    for i in (0, 2, 3):
        bad = list(ok)
        bad[i] = None
        assert L.fea_pcg_scalar_step(*bad) == FEA_EINVAL
    for i, v in ((1, 0), (4, 0), (5, 0), (6, -1), (6, 4)):
        bad = list(ok)
        bad[i] = v
        assert L.fea_pcg_scalar_step(*bad) == FEA_EINVAL
    assert L.fea_pcg_parts(2, 33, 8) == -1 and L.fea_pcg_parts(33, 33, 2) == -1
    # one partial per (128-column fp64 / 256-column fp32 strip, row task): independent of the batch by construction
    assert L.fea_pcg_parts(33, 33, 8) >= 1
    assert L.fea_pcg_parts(4097, 4097, 8) % 32 == 0 and L.fea_pcg_parts(4097, 4097, 4) % 16 == 0


def test_constructor_rejections_need_no_device():
    """Arguments that would make the preconditioner non-symmetric are refused before anything touches the GPU."""
    import numpy as np
    from feanet_amd import PCGSolver
    with pytest.raises(ValueError, match="smoother"):
        PCGSolver(16, smoother="hjac")
    with pytest.raises(ValueError, match="compat"):
        PCGSolver(16, compat="mm_interface_q2")
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="R and P"):
        PCGSolver(16, problem="interface", R=rng.standard_normal((16, 3, 3)), P=rng.standard_normal((16, 3, 3)))
    with pytest.raises(ValueError, match="positive"):
        PCGSolver(16, w=(1.0, -1.0))
