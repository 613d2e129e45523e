"""tools/compare_code_objects.py on synthetic disassembly: the four function classes, the metadata and
symbol-set checks and the exit status with and without --allow (CPU only, no compiler involved)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools import compare_code_objects as cco  # noqa: E402

BASE = """\
v_add_f32_e32 v1, v2, v3
s_load_dwordx2 s[4:5], s[0:1], 0x10
v_mul_f64 v[4:5], v[6:7], v[8:9]
v_accvgpr_write_b32 a0, v1
s_endpgm"""
RENAMED = BASE.replace("v1,", "v11,").replace("s[4:5]", "s[6:7]").replace("a0", "a2").replace("v1\n", "v11\n")
RESCHEDULED = "\n".join(BASE.split("\n")[i] for i in (1, 0, 2, 3, 4))
CHANGED = BASE.replace("v_mul_f64", "v_fma_f64").replace("v[8:9]", "v[8:9], v[4:5]")
LONGER = BASE.replace("s_endpgm", "s_nop 0\ns_endpgm")
NOTE = [("vgpr_count", "12"), ("sgpr_count", "8"), ("kernarg_segment_size", "64")]


def lib(**funcs):
    """a load() triple of one code object whose functions are all kernels with the note NOTE"""
    return ({n: [t] for n, t in funcs.items()}, {n: [list(NOTE)] for n in funcs}, 1)


def test_classify():
    assert cco.classify(BASE, BASE) == "identical"
    assert cco.classify(BASE, RENAMED) == "renamed"
    assert cco.classify(BASE, RESCHEDULED) == "rescheduled"
    assert cco.classify(BASE, RESCHEDULED.replace("v3", "v13")) == "rescheduled"
    assert cco.classify(BASE, CHANGED) == "changed"
    assert cco.classify(BASE, LONGER) == "changed"
    # only register operands are folded: another mnemonic, immediate or special register is a change
    assert cco.classify(BASE, BASE.replace("0x10", "0x18")) == "changed"
    assert cco.classify(BASE, BASE.replace("v_add_f32_e32", "v_sub_f32_e32")) == "changed"
    assert cco.classify("v_cndmask_b32_e32 v1, v2, v3, vcc", "v_cndmask_b32_e64 v1, v2, v3, s[2:3]") == "changed"


def test_parse_functions():
    text = ("\nlib.co:\tfile format elf64-amdgpu\n\nDisassembly of section .text:\n\n<k_a>:\n"
            "\tv_add_f32_e32 v1, v2, v3 // 000000001000: 02020702\n\ts_endpgm\n\t...\n\n<k_b>:\n\ts_endpgm\n")
    assert cco.parse_functions(text) == [("k_a", "v_add_f32_e32 v1, v2, v3\ns_endpgm"), ("k_b", "s_endpgm")]


def test_compare_classes_and_allow():
    old = lib(k_same=BASE, k_ren=BASE, k_sch=BASE)
    new = lib(k_same=BASE, k_ren=RENAMED, k_sch=RESCHEDULED)
    assert cco.compare(old, old)[1] == 0
    out, status = cco.compare(old, new)
    assert status == 1
    assert "disassembly differs (renamed): k_ren" in out and "disassembly differs (rescheduled): k_sch" in out
    assert cco.compare(old, new, ("renamed",))[1] == 1
    out, status = cco.compare(old, new, ("renamed", "rescheduled"))
    assert status == 0
    assert out[:4] == ["renamed: 1", "  k_ren", "rescheduled: 1", "  k_sch"]
    assert "1 identical, 1 renamed, 1 rescheduled, 0 changed" in out[-1]
    # a changed function fails whatever is allowed
    out, status = cco.compare(old, lib(k_same=BASE, k_ren=RENAMED, k_sch=CHANGED), ("renamed", "rescheduled"))
    assert status == 1 and "disassembly differs (changed): k_sch" in out


def test_compare_headline():
    old = lib(k_a=BASE, k_b=BASE)
    assert cco.compare(old, old)[0][-1].startswith("IDENTICAL: ")
    new = lib(k_a=BASE, k_b=RENAMED)
    assert cco.compare(old, new)[0][-1].startswith("DIFFERENT: ")
    assert cco.compare(old, new, ("renamed",))[0][-1].startswith("ALLOWED: ")
    assert cco.compare(old, lib(k_a=BASE, k_b=CHANGED), ("renamed", "rescheduled"))[0][-1].startswith("DIFFERENT: ")


def test_compare_metadata_and_symbols():
    old = lib(k_a=BASE, k_b=BASE)
    # identical disassembly, one metadata field off: fails with nothing allowed and with everything allowed
    new = lib(k_a=BASE, k_b=BASE)
    new[1]["k_a"] = [[("vgpr_count", "13")] + NOTE[1:]]
    for allow in ((), ("renamed", "rescheduled")):
        out, status = cco.compare(old, new, allow)
        assert status == 1 and "metadata differs: k_a: vgpr_count" in out and out[-1].startswith("DIFFERENT: ")
    # ... and an allowed class does not excuse it
    new = lib(k_a=RENAMED, k_b=BASE)
    new[1]["k_a"] = [[("vgpr_count", "13")] + NOTE[1:]]
    out, status = cco.compare(old, new, ("renamed", "rescheduled"))
    assert status == 1 and "metadata differs: k_a: vgpr_count" in out
    out, status = cco.compare(old, lib(k_a=BASE), ("renamed", "rescheduled"))
    assert status == 1 and "function k_b: 1 definition(s) in OLD, 0 in NEW" in out
    out, status = cco.compare(old, lib(k_a=BASE, k_b=BASE, k_c=BASE))
    assert status == 1 and "kernel note k_c: 0 definition(s) in OLD, 1 in NEW" in out


def test_main_arguments(monkeypatch, capsys):
    libs = {"old.so": lib(k_a=BASE, k_b=BASE), "ren.so": lib(k_a=BASE, k_b=RENAMED), "chg.so": lib(k_a=BASE, k_b=CHANGED)}
    monkeypatch.setattr(cco, "load", lambda so: libs[so])
    assert cco.main(["cco", "old.so", "old.so"]) == 0
    assert cco.main(["cco", "old.so", "ren.so"]) == 1
    # --allow in either form, before or after the libraries
    assert cco.main(["cco", "--allow", "renamed,rescheduled", "old.so", "ren.so"]) == 0
    assert cco.main(["cco", "old.so", "ren.so", "--allow=renamed"]) == 0
    assert cco.main(["cco", "old.so", "ren.so", "--allow", "rescheduled"]) == 1
    assert cco.main(["cco", "old.so", "chg.so", "--allow", "renamed,rescheduled"]) == 1
    assert "ALLOWED: " in capsys.readouterr().out
    # `changed` cannot be allowed, nor can nothing; a missing library is a usage error
    for argv in (["--allow", "changed", "old.so", "ren.so"], ["--allow", "renamed,changed", "old.so", "ren.so"],
                 ["--allow", "", "old.so", "ren.so"], ["old.so"]):
        with pytest.raises(SystemExit) as e:
            cco.main(["cco"] + argv)
        assert e.value.code == 2
