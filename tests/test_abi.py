"""The C-ABI library builds, loads on a CPU-only host and exports every entry point declared in
include/feanet_hip.h, and the binding's signature table names and types every parameter as the header declares it
(no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def header_functions():
    src = open(os.path.join(ROOT, "include", "feanet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fea_[a-z0-9_]+)\s*\(", src)))


def header_declarations():
    """{fea_* name: (return type, [(type class, parameter name)], {parameter name: C type})} of every declaration in
    the header, comments stripped.  Type classes: any pointer "P", int (and unsigned) "I", long long "LL", float /
    double "S"."""
    src = open(os.path.join(ROOT, "include", "feanet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = {}
    for ret, name, params in re.findall(r"\b(int|size_t|long long)\s+(fea_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        assert name not in decls, name
        fields, raw = [], {}
        params = " ".join(params.split())
        for p in ([] if params == "void" else params.split(",")):
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", p.strip())
            ctype, pname = m.group(1).strip(), m.group(2)
            assert ctype, f"{name}: parameter without a name in {p!r}"
            cls = "P" if "*" in ctype else {"int": "I", "unsigned": "I", "long long": "LL", "float": "S",
                                            "double": "S"}[ctype.replace("const", "").strip()]
            fields.append((cls, pname))
            raw[pname] = ctype
        decls[name] = (ret, fields, raw)
    return decls


_CLASS = {"P": "P", "PI": "P", "PLL": "P", "I": "I", "LL": "LL", "S": "S", "D": "S"}


def table_mismatches(sigs, extra, decls):
    """What the signature table (_lib._SIGS, _lib._EXTRA) says differently from the header's declarations."""
    import ctypes
    restype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong}
    bad = []

    def fields(sig):
        return [(_CLASS[t], n) for t, n in (p.split() for p in sig)]

    table = {name: (fields(sig), res) for name, (sig, res) in extra.items()}
    for base, sig in sigs.items():
        for suf in ("f32", "f64"):  # one entry for the pair: both suffixes must declare the same names
            table[f"fea_{base}_{suf}"] = (fields(sig), ctypes.c_int)
    for name in sorted(set(table) | set(decls)):
        if name not in table or name not in decls:
            bad.append(f"{name}: only in the {'header' if name in decls else 'table'}")
            continue
        ret, want = decls[name][:2]
        got, res = table[name]
        if got != want:
            bad.append(f"{name}: table {got} != header {want}")
        if res is not restype[ret]:
            bad.append(f"{name}: returns {ret}, table {res}")
        if len({n for _, n in want}) != len(want):
            bad.append(f"{name}: a parameter name repeats")
    return bad


def test_signature_table_matches_header():
    """Every one of the header's declarations: parameter names, their order and type classes equal the table's; the
    _f32 and _f64 declarations of a pair share one table entry, so they carry the same names."""
    from feanet_amd import _lib
    decls = header_declarations()
    assert len(decls) == 110 and sorted(decls) == header_functions()
    assert table_mismatches(_lib._SIGS, _lib._EXTRA, decls) == []
    # the scalar parameters of a typed pair are float in _f32 and double in _f64
    for base, sig in _lib._SIGS.items():
        scalars = [p.split()[1] for p in sig if p.startswith("S ")]
        for suf, ctype in (("f32", "float"), ("f64", "double")):
            raw = decls[f"fea_{base}_{suf}"][2]
            assert [n for n, t in raw.items() if t in ("float", "double")] == scalars, (base, suf)
            assert all(raw[n] == ctype for n in scalars), (base, suf)


@pytest.mark.parametrize("corrupt", ["rename", "swap", "type", "drop", "restype"])
def test_signature_check_catches_a_corrupted_entry(corrupt):
    """The comparison itself: one table entry changed in one way must be reported (and only that entry)."""
    import ctypes
    from feanet_amd import _lib
    sigs, extra = dict(_lib._SIGS), dict(_lib._EXTRA)
    sig = list(sigs["mg_cycle_join"])
    i = sig.index("S w1")
    assert sig[1] == "P ec" and sig[i + 1] == "S w0" and "LL bstridec" in sig and "P norm_cnt" in sig
    if corrupt == "rename":
        sig[1] = "P e"
    elif corrupt == "swap":
        sig[i], sig[i + 1] = sig[i + 1], sig[i]
    elif corrupt == "type":
        sig[sig.index("LL bstridec")] = "I bstridec"
    elif corrupt == "drop":
        sig.remove("P norm_cnt")
    else:
        extra["fea_mg_join_norm_parts"] = (extra["fea_mg_join_norm_parts"][0], ctypes.c_int)
    sigs["mg_cycle_join"] = sig
    assert sigs != _lib._SIGS or extra != _lib._EXTRA
    bad = table_mismatches(sigs, extra, header_declarations())
    victim = "fea_mg_join_norm_parts" if corrupt == "restype" else "fea_mg_cycle_join_f"
    assert bad and all(b.startswith(victim) for b in bad), bad
    assert len(bad) == (1 if corrupt == "restype" else 2), bad


def _header_order(name):
    return [n for _, n in header_declarations()[f"fea_{name}_f64"][1]][:-1]


def test_launch_records_by_name():
    """_lib.launch / arg / replace: the record is (name, plain tuple in header order without the stream); a missing
    or an unknown parameter is a TypeError naming the entry point and the parameter."""
    from feanet_amd import _lib
    for name, nparams in (("mg_cycle_join", 26), ("mg_mid_up", 16)):
        order = _header_order(name)
        assert len(order) == nparams and "stream" not in order
        kw = {p: 100 + i for i, p in enumerate(order)}
        rec = _lib.launch(name, **dict(reversed(list(kw.items()))))  # keyword order does not matter
        assert rec == (name, tuple(range(100, 100 + nparams))) and type(rec) is tuple and type(rec[1]) is tuple
        assert [_lib.arg(rec, p) for p in order] == list(rec[1])
        for p in order:
            less = dict(kw)
            del less[p]
            with pytest.raises(TypeError, match=rf"fea_{name}\b.*'{p}'"):
                _lib.launch(name, **less)
        with pytest.raises(TypeError, match=rf"fea_{name}\b.*'nosuch'"):
            _lib.launch(name, nosuch=1, **kw)
        with pytest.raises(TypeError, match=rf"fea_{name}\b.*'stream'"):
            _lib.launch(name, stream=0, **kw)
        with pytest.raises(TypeError, match=rf"fea_{name}\b.*'nosuch'"):
            _lib.arg(rec, "nosuch")
        with pytest.raises(TypeError, match=rf"fea_{name}\b.*'nosuch'"):
            _lib.replace(rec, nosuch=1)
        new = _lib.replace(rec, u=7) if "u" in order else _lib.replace(rec, out=7)
        slot = order.index("u" if "u" in order else "out")
        assert _lib.arg(new, order[slot]) == 7 and type(new[1]) is tuple
        assert [v for i, v in enumerate(new[1]) if i != slot] == [v for i, v in enumerate(rec[1]) if i != slot]
        assert rec[1][slot] == 100 + slot  # the original record is untouched
    # a NULL pointer is written out, never defaulted; dtype-free entry points are launch names without the fea_ prefix
    rec = _lib.launch("norm_append", ws=None, stride=2, per=3, B=1, nrows=2, hist=5, cnt=6)
    assert rec == ("norm_append", (None, 2, 3, 1, 2, 5, 6))
    with pytest.raises(TypeError, match="fea_copy"):
        _lib.arg(("copy", (1, 2)), "u")


def test_header_lists_both_families():
    names = header_functions()
    assert "fea_knet_apply_f64" in names and "fea_mg_prolong_sweep_f32" in names
    assert len(names) >= 30


def test_library_exports_every_declared_symbol():
    from feanet_amd import _lib
    lib = _lib.lib()
    missing = [n for n in header_functions() if not hasattr(lib, n)]
    assert not missing, f"not exported: {missing}"
    assert sorted(_lib.exported_symbols()) == header_functions()


def test_host_only_queries():
    from feanet_amd import _lib
    assert _lib.lib().fea_abi_version() == _lib.ABI_VERSION
    for H, W, esz in [(3, 3, 8), (5, 5, 8), (4097, 4097, 8), (1025, 1025, 4), (8193, 8193, 8), (517, 4097, 8),
                      (9, 100, 4)]:
        ld, bs = _lib.mg_layout(H, W, esz)
        A = 128 // esz
        assert ld % A == 0 and ld >= W + A and bs == (H + 2) * ld
    with pytest.raises(ValueError):
        _lib.mg_layout(2, 100, 8)       # fewer than 3 rows
    assert _lib.norm_workspace_bytes(2, 4097, 4097) >= 2 * 65 * 129 * 8


def test_ops_refuse_cpu_tensors():
    import torch
    from feanet_amd import ops
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.knet_apply(torch.zeros(1, 1, 5, 5), torch.zeros(1, 9))


def test_no_oracle_in_product():
    """Nothing under multigrid-feanet_amd/ may import the oracle (test infrastructure only)."""
    pkg = os.path.join(ROOT, "multigrid-feanet_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, fn)).read()
                assert "feanet_oracle" not in txt and "from oracle" not in txt, fn
