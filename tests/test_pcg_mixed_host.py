"""Mixed-precision Krylov entry points (fea_pcg_*_f64f32) without a GPU: the header and the binding list them, every
one returns FEA_EINVAL for a NULL operand, a bad fp64 or fp32 layout, aliased fields and ntab > 1 without a pattern
map, and PCGSolver refuses bad dtype pairs before anything touches a device.  Nothing is launched: the pointers are
fake addresses that a rejected call never touches."""
import os
import re

import pytest

from conftest import ROOT

FEA_EINVAL = -1
H = W = 33
PTR = {"x": 0x10000, "r": 0x20000, "p": 0x30000, "q": 0x40000, "z32": 0x50000, "r32": 0x60000, "pid": 0x70000,
       "ktab": 0x80000, "sc": 0x90000, "part": 0xa0000, "sb": 0xb0000}

# entry -> operand names in order (then B, H, W, ld, bstride, ld32, bstride32, stream)
ENTRIES = {
    "pcg_narrow_f64f32": ["r", "r32", "sc", "sb"],
    "pcg_dot_f64f32": ["r", "z32", "part"],
    "pcg_direction_f64f32": ["z32", "p", "q", "pid", "ktab", "ntab", "sc", "part"],
    "pcg_update_f64f32": ["p", "x", "r", "r32", "pid", "ktab", "ntab", "sc", "sb", "part"],
}
TABLED = sorted(n for n, ops in ENTRIES.items() if "ktab" in ops)


def layouts():
    from feanet_amd import _lib
    return _lib.mg_layout(H, W, 8) + _lib.mg_layout(H, W, 4)


def call(name, over=None, ntab=1, B=1, h=H, w=W, ld=None, bs=None, ld32=None, bs32=None):
    from feanet_amd import _lib
    over = over or {}
    args = []
    for a in ENTRIES[name]:
        if a == "ntab":
            args.append(ntab)
        elif a in over:
            args.append(over[a])
        elif a == "pid":
            args.append(PTR["pid"] if ntab > 1 else None)
        else:
            args.append(PTR[a])
    l64, b64, l32, b32 = layouts()
    fn = getattr(_lib.lib(), f"fea_{name}")
    return fn(*args, B, h, w, l64 if ld is None else ld, b64 if bs is None else bs, l32 if ld32 is None else ld32,
              b32 if bs32 is None else bs32, None)


def test_header_and_binding_list_the_entry_points():
    from feanet_amd import _lib
    src = open(os.path.join(ROOT, "include", "feanet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fea_[a-z0-9_]+)\s*\(", src))
    for name in ENTRIES:
        assert f"fea_{name}" in declared, f"fea_{name} is not declared in feanet_hip.h"
        assert f"fea_{name}" in _lib.exported_symbols()
        assert hasattr(_lib.lib(), f"fea_{name}"), f"fea_{name} is not exported"


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_operands(name):
    for a in ENTRIES[name]:
        if a in ("ntab", "pid"):
            continue
        assert call(name, over={a: None}) == FEA_EINVAL, f"{name}: NULL {a} accepted"
    assert call(name, B=0) == FEA_EINVAL


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_layouts(name):
    """ld is a multiple of 16 doubles, ld32 of 32 floats (128-byte lines), each wide enough for its own frame."""
    l64, b64, l32, b32 = layouts()
    assert l64 % 16 == 0 and l32 % 32 == 0
    assert call(name, ld32=l32 + 16) == FEA_EINVAL       # a multiple of 16, not of 32
    assert call(name, ld32=l32 + 1) == FEA_EINVAL
    assert call(name, ld32=l32 - 32) == FEA_EINVAL       # too narrow for the fp32 frame
    assert call(name, bs32=b32 - 1) == FEA_EINVAL        # fp32 samples overlap
    assert call(name, ld=l64 + 8) == FEA_EINVAL          # not a multiple of 16
    assert call(name, ld=l64 + 1) == FEA_EINVAL
    assert call(name, ld=l64 - 16) == FEA_EINVAL
    assert call(name, bs=b64 - 1) == FEA_EINVAL
    assert call(name, ld=l32, bs=b32, ld32=l64, bs32=b64) == FEA_EINVAL  # the two frames swapped
    assert call(name, h=2) == FEA_EINVAL
    assert call(name, w=2) == FEA_EINVAL


@pytest.mark.parametrize("name", TABLED)
def test_bad_tables(name):
    assert call(name, ntab=0) == FEA_EINVAL
    assert call(name, ntab=17, over={"pid": PTR["pid"]}) == FEA_EINVAL
    assert call(name, ntab=16, over={"pid": None}) == FEA_EINVAL   # ntab > 1 needs the pattern map
    assert call(name, over={"ktab": None}) == FEA_EINVAL


def test_aliasing_rules():
    """The direction ping-pongs (p_out is neither p_in nor the fp32 z); the update's four fields are distinct; no
    fp64 field shares its address with an fp32 one."""
    assert call("pcg_direction_f64f32", over={"q": PTR["p"]}) == FEA_EINVAL
    assert call("pcg_direction_f64f32", over={"q": PTR["z32"]}) == FEA_EINVAL
    assert call("pcg_update_f64f32", over={"x": PTR["p"]}) == FEA_EINVAL
    assert call("pcg_update_f64f32", over={"r": PTR["p"]}) == FEA_EINVAL
    assert call("pcg_update_f64f32", over={"r": PTR["x"]}) == FEA_EINVAL
    for a in ("p", "x", "r"):
        assert call("pcg_update_f64f32", over={"r32": PTR[a]}) == FEA_EINVAL
    assert call("pcg_narrow_f64f32", over={"r32": PTR["r"]}) == FEA_EINVAL
    assert call("pcg_narrow_f64f32", over={"sb": PTR["sc"]}) == FEA_EINVAL


def test_partials_are_the_fp64_geometrys():
    """The mixed kernels run on the fp64 task grid: PCGSolver sizes its partial buffer with elem_size 8."""
    from feanet_amd import _lib
    L = _lib.lib()
    p64, p32 = L.fea_pcg_parts(513, 513, 8), L.fea_pcg_parts(513, 513, 4)
    assert p64 > 0 and p64 % 4 == 0    # 4 fp64 strips of 128 columns
    assert p64 == 2 * p32              # against 2 fp32 strips of 256, the same row tasks


def test_constructor_dtype_checks_need_no_device():
    import torch
    from feanet_amd import PCGSolver
    with pytest.raises(TypeError, match="precond_dtype"):
        PCGSolver(16, dtype=torch.float64, precond_dtype=torch.float16)
    with pytest.raises(TypeError, match="precond_dtype"):
        PCGSolver(16, dtype=torch.float64, precond_dtype=torch.int32)
    with pytest.raises(TypeError, match="dtype"):
        PCGSolver(16, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="dtype"):
        PCGSolver(16, dtype=torch.int64, precond_dtype=torch.float32)
    with pytest.raises(ValueError, match="wider"):
        PCGSolver(16, dtype=torch.float32, precond_dtype=torch.float64)
