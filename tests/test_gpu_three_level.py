"""The three-level register kernels (k_mg_zero_restrict3, k_mg_prolong3: the register-strip form of fea_mg_mid_down /
fea_mg_mid_up, TR = -u, TC = -1, k = 3) against the launches they replace, at every task height, and the solver
plans that use them."""
import numpy as np
import pytest
import torch

from test_gpu_mg import Frame, npdt, rand_state, tables

pytestmark = pytest.mark.gpu

# (columns n, rows m, batch): 16 is the smallest grid with three coarser levels (17 -> 9 -> 5 -> 3); rows != columns
# both ways; 512 columns are five fp64 strips (104 owned columns each) and three fp32 ones (224); 488 x 120 ends its
# last strip a few columns past an owned boundary and its lowest level has an even number of nodes (62 x 16);
# 384 x 96 both ways: 385 / 193 / 97 columns over 97 / 49 / 25 rows, the levels MultigridSolver(768, rows=768) groups
SHAPES = [(16, 16, 1), (16, 16, 3), (32, 32, 3), (64, 64, 1), (256, 32, 1), (32, 256, 3), (512, 32, 1), (488, 120, 1),
          (384, 96, 1), (96, 384, 3)]


def heights(rows_u):
    """every task height of up to 16 units, a ladder above (past the level's own: one task per strip)"""
    hs = set(range(1, min(rows_u, 16) + 1)) | {rows_u - 1, rows_u, rows_u + 5}
    return sorted(h for h in hs if h >= 1)


def chain4(n, m, B, T):
    return [Frame(n >> j, B, T, "poisson", m=m >> j) for j in range(4)]


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_zero_restrict3_bitwise(T, n, m, B):
    """The strip form of fea_mg_mid_down (k = 3) is bitwise fea_mg_zero_restrict2 followed by the single-level zero-guess restriction of
    the third level, on all three outputs, at every task height; boundary nodes keep their sentinels and the frames
    around the outputs (padding, ghost rows) are the same bytes as after the reference launches."""
    from feanet_amd import _lib
    rng = np.random.default_rng(13 * n + m + B)
    lv = chain4(n, m, B, T)
    _, _, _, _, kt, om, rt, _ = tables("poisson", T)
    _, f = rand_state(rng, B, (lv[0].H, lv[0].W), T)
    lv[0].put("f", f)
    sent = [None] + [np.full((B, x.H, x.W), 3.0 + j) for j, x in enumerate(lv[1:])]
    ptr = [x.L.f.data_ptr() for x in lv]

    def prefill():
        for x, s in zip(lv[1:], sent[1:]):
            x.put("f", s)

    prefill()
    _lib.call("mg_zero_restrict2", T, ptr[0], ptr[1], ptr[2], None, None, kt.data_ptr(), om.data_ptr(), 1,
              rt.data_ptr(), 1, 1.25, *lv[0].args(), lv[1].L.ld, lv[1].L.bs, lv[2].L.ld, lv[2].L.bs, None)
    _lib.call("mg_residual_restrict", T, None, ptr[2], None, ptr[3], None, kt.data_ptr(), om.data_ptr(), 1,
              rt.data_ptr(), 1, 1.25, *lv[2].args(), lv[3].L.ld, lv[3].L.bs, None)
    ref = [x.get("f") for x in lv[1:]]
    raw = [x.L.f.clone() for x in lv[1:]]
    for j, r in enumerate(ref):  # the reference itself wrote interiors only
        assert (r[:, 0, :] == 3 + j).all() and (r[:, -1, :] == 3 + j).all()
        assert (r[:, :, 0] == 3 + j).all() and (r[:, :, -1] == 3 + j).all()
        assert (r[:, 1:-1, 1:-1] != 3 + j).any()
    for units in heights(lv[3].H - 2):
        prefill()
        _lib.call("mg_mid_down", T, _lib.PtrArray(ptr), None, 3, B, lv[0].H, lv[0].W, kt.data_ptr(), om.data_ptr(), 1,
                  rt.data_ptr(), 1, 1.25, -units, -1, None)
        for j, x in enumerate(lv[1:]):
            got = x.get("f")
            assert np.array_equal(got, ref[j]), f"units {units}, f_l+{j + 1}: {np.argwhere(got != ref[j])[:5]}"
            assert torch.equal(x.L.f, raw[j]), f"units {units}: the frame of f_l+{j + 1} differs"


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_prolong3_bitwise(T, n, m, B):
    """The strip form of fea_mg_mid_up (k = 3) is bitwise fea_mg_prolong_sweep(u = NULL) on the third level followed by fea_mg_prolong2, at
    every task height; the output's boundary nodes keep their sentinel and its frame the reference's bytes."""
    from feanet_amd import _lib
    rng = np.random.default_rng(17 * n + m + B)
    lv = chain4(n, m, B, T)
    _, _, _, _, kt, om, _, pt = tables("poisson", T)
    for x in lv[:3]:
        x.put("f", rand_state(rng, B, (x.H, x.W), T)[1])
    e3 = rng.standard_normal((B, lv[3].H, lv[3].W)).astype(npdt(T))
    e3[:, 0, :] = e3[:, -1, :] = e3[:, :, 0] = e3[:, :, -1] = 0
    lv[3].put("a", e3)
    lv[2].put("a", np.zeros((B, lv[2].H, lv[2].W)))
    sent = np.full((B, lv[0].H, lv[0].W), 7.0)
    lv[0].put("b", sent)
    fp = [x.L.f.data_ptr() for x in lv]
    tabs = (kt.data_ptr(), om.data_ptr(), 1, pt.data_ptr(), 1, 0.75)
    _lib.call("mg_prolong_sweep", T, None, lv[3].L.a.data_ptr(), fp[2], lv[2].L.a.data_ptr(), None, None, *tabs,
              *lv[2].args(), lv[3].L.ld, lv[3].L.bs, None)
    _lib.call("mg_prolong2", T, fp[1], lv[2].L.a.data_ptr(), fp[0], lv[0].L.b.data_ptr(), None, None, None, *tabs,
              *lv[0].args(), lv[1].L.ld, lv[1].L.bs, lv[2].L.ld, lv[2].L.bs, None)
    ref = lv[0].get("b")
    raw = lv[0].L.b.clone()
    assert (ref[:, 0, :] == 7).all() and (ref[:, -1, :] == 7).all() and (ref[:, :, 0] == 7).all()
    assert (ref[:, :, -1] == 7).all() and (ref[:, 1:-1, 1:-1] != 7).any()
    for units in heights(-(-(lv[0].H - 2) // 4)):
        lv[0].put("b", sent)
        _lib.call("mg_mid_up", T, _lib.PtrArray(fp[:3]), lv[3].L.a.data_ptr(), lv[0].L.b.data_ptr(), None, 3, B,
                  lv[0].H, lv[0].W, *tabs, -units, -1, None)
        got = lv[0].get("b")
        assert np.array_equal(got, ref), f"units {units}: {np.argwhere(got != ref)[:5]}"
        assert torch.equal(lv[0].L.b, raw), f"units {units}: the frame of the output differs"


def test_strip_form_refusals():
    """The strip form carries one stencil pattern and exactly three levels: ntab > 1, k != 3, TC other than -1 and
    the gathered entry point are FEA_EINVAL (the solver keeps such plans on the one- and two-level launches)."""
    from feanet_amd import _lib
    T = torch.float64

    def down(lv, kt, om, rt, nt, k=3, TR=-1, TC=-1, pid=None, name="mg_mid_down", extra=()):
        _lib.call(name, T, _lib.PtrArray([x.L.f.data_ptr() for x in lv]), pid, k, 1, lv[0].H, lv[0].W, kt.data_ptr(),
                  om.data_ptr(), nt, rt.data_ptr(), nt, 1.0, TR, TC, *extra, None)

    def up(lv, kt, om, pt, nt, k=3, TR=-1, TC=-1, pid=None):
        _lib.call("mg_mid_up", T, _lib.PtrArray([x.L.f.data_ptr() for x in lv[:3]]), lv[3].L.a.data_ptr(),
                  lv[0].L.b.data_ptr(), pid, k, 1, lv[0].H, lv[0].W, kt.data_ptr(), om.data_ptr(), nt, pt.data_ptr(),
                  nt, 1.0, TR, TC, None)
    lv = [Frame(32 >> j, 1, T, "poisson") for j in range(4)]
    _, _, _, _, kt, om, rt, pt = tables("poisson", T)
    down(lv, kt, om, rt, 1), up(lv, kt, om, pt, 1)  # the accepted calls
    for kw in (dict(k=2), dict(k=4), dict(TC=-2), dict(TC=4), dict(TR=4)):
        with pytest.raises(RuntimeError, match="invalid arguments"):
            down(lv, kt, om, rt, 1, **kw)
        with pytest.raises(RuntimeError, match="invalid arguments"):
            up(lv, kt, om, pt, 1, **kw)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        down(lv, kt, om, rt, 1, name="mg_mid_down_gathered", extra=(lv[0].L.f.data_ptr(), 2, 2, 16, 16))
    lm = [Frame(32 >> j, 1, T, "interface") for j in range(4)]
    _, _, _, _, kt, om, rt, pt = tables("interface", T)
    pids = _lib.PtrArray([x.pid() for x in lm])
    with pytest.raises(RuntimeError, match="invalid arguments"):
        down(lm, kt, om, rt, kt.shape[0], pid=pids)
    with pytest.raises(RuntimeError, match="invalid arguments"):
        up(lm, kt, om, pt, kt.shape[0], pid=pids)


NEW = ("mg_mid_down", "mg_mid_up")


def plan_names(s):
    return [nm for nm, _ in s._plan("a")[0]]


def test_default_switches():
    """Going up the three-level launch is on, going down it is off (it measured slower than the two launches it
    replaces, profiles/r07_ab/three_level.txt); the kernel stays, tested above and in the plans below."""
    from feanet_amd.solver import MultigridSolver
    assert MultigridSolver.THREE_LEVEL_UP is True and MultigridSolver.THREE_LEVEL_DOWN is False
    assert plan_names(MultigridSolver(1024, dtype=torch.float64)) == [
        "mg_sweep_restrict", "mg_zero_restrict2", "mg_residual_restrict", "mg_coarse_tail", "mg_mid_up",
        "mg_prolong_sweep"]


@pytest.mark.parametrize("T,n,eligible", [(torch.float64, 1024, True), (torch.float32, 1024, True),
                                          (torch.float64, 512, False), (torch.float64, 64, False)])
def test_solver_three_level_bitwise(T, n, eligible):
    """1025^2 has three launch-bound levels (513^2, 257^2, 129^2) between the finest and the 65^2 tail: the plan runs
    them as one launch each way where the direction's switch is on.  513^2 has two (they pair) and 65^2 none: no new
    step.  vcycle(3) with the grouping on is bitwise vcycle(3) with it off, and each switch acts alone."""
    from feanet_amd.solver import MultigridSolver
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    f = torch.randn(1, 1, n + 1, n + 1, dtype=T, device="cuda", generator=g)
    outs = []
    for down, up in ((True, True), (False, False), (True, False), (False, True)):
        s = MultigridSolver(n, dtype=T)
        s.THREE_LEVEL_DOWN, s.THREE_LEVEL_UP = down, up
        names = plan_names(s)
        assert ("mg_mid_down" in names) == (eligible and down), names
        assert ("mg_mid_up" in names) == (eligible and up), names
        if eligible and down and up:
            assert names == ["mg_sweep_restrict", "mg_mid_down", "mg_coarse_tail", "mg_mid_up",
                             "mg_prolong_sweep"], names
        if eligible and not down and not up:
            assert names == ["mg_sweep_restrict", "mg_zero_restrict2", "mg_residual_restrict", "mg_coarse_tail",
                             "mg_prolong_sweep", "mg_prolong2", "mg_prolong_sweep"], names
        s.set_rhs(f=f)
        s.load()
        s.vcycle(3)
        outs.append(s.solution())
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def _arg_level(rec):
    from feanet_amd import _lib
    return _lib.arg(rec, "Ht" if rec[0] == "mg_coarse_tail" else "H")


def test_metric_plan():
    """The 4097^2 cycle with both directions on has six launches: the join, zero_restrict2 (levels 1-2),
    the strip mid_down (3-5), the tail, the strip mid_up (5-3), prolong2 (2-1).  As shipped (down off) levels 3-5 go down as
    zero_restrict2 + the single-level restriction: seven.  The plans only: nothing runs."""
    from feanet_amd.solver import MultigridSolver
    s = MultigridSolver(4096, dtype=torch.float64)
    assert s._joinable()  # the first and the last step of the plan run as one cycle join
    assert plan_names(s)[1:-1] == ["mg_zero_restrict2", "mg_zero_restrict2", "mg_residual_restrict", "mg_coarse_tail",
                                   "mg_mid_up", "mg_prolong2"]
    s._plans.clear()
    s.THREE_LEVEL_DOWN = True
    assert plan_names(s) == ["mg_sweep_restrict", "mg_zero_restrict2", "mg_mid_down", "mg_coarse_tail",
                             "mg_mid_up", "mg_prolong2", "mg_prolong_sweep"]
    from feanet_amd import _lib
    for rec in s._plan("a")[0]:
        if rec[0] in NEW:
            assert (_lib.arg(rec, "k"), _lib.arg(rec, "TR"), _lib.arg(rec, "TC")) == (3, -1, -1)
    lv = {rec[0]: _arg_level(rec) for rec in s._plan("a")[0][1:-1]}
    assert lv == {"mg_zero_restrict2": 2049, "mg_mid_down": 513, "mg_coarse_tail": 65, "mg_mid_up": 513,
                  "mg_prolong2": 2049}


def test_other_plans_keep_their_launches():
    """No grouping for a batch that fills the chip (256 x 1025^2: its 513^2 level is not launch-bound), for an even
    number of levels above the tail (2049^2: four, they pair), for the two-material problem, the learned smoother,
    a zero-start solver and V(2,2) — with both switches on."""
    from feanet_amd.solver import MultigridSolver
    import os
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multigrid-feanet_amd", "feanet_amd",
                             "weights", "hnet_iso_poisson_33x33.npz"))
    hnet = np.stack([w[f"conv{i}"].reshape(3, 3) for i in range(3)])
    for kw in (dict(n=1024, dtype=torch.float32, batch=256), dict(n=2048), dict(n=1024, problem="interface"),
               dict(n=1024, smoother="hjac", hnet=hnet), dict(n=1024, zero_start=True), dict(n=1024, nu1=2, nu2=2)):
        s = MultigridSolver(**kw)
        s.THREE_LEVEL_DOWN = s.THREE_LEVEL_UP = True
        assert not set(NEW) & set(plan_names(s)), kw
        del s
        torch.cuda.empty_cache()


def test_three_level_bytes():
    """bytes_per_vcycle of the 1025^2 fp32 plans, by hand: the join moves 3 fields of level 0 and 2 of level 1 (fine
    nodes 1023^2, then 511^2, 255^2, 127^2, 63^2); the three-level launch going down reads f_1 and writes f_2, f_3, f_4
    (the two launches it replaces read f_3 again); going up it reads f_1, f_2, f_3, e_4 and writes u_1."""
    from feanet_amd.solver import MultigridSolver
    n0, n1, n2, n3, n4 = (k * k for k in (1023, 511, 255, 127, 63))
    join, down3, up3 = 4 * (3 * n0 + 2 * n1), 4 * (n1 + n2 + n3 + n4), 4 * (2 * n1 + n2 + n3 + n4)
    assert (join + down3 + 4 * n3 + up3, join + down3 + up3) == (18526268, 18461752)
    s = MultigridSolver(1024, dtype=torch.float32)
    assert s.bytes_per_vcycle() == 18526268
    s._plans.clear()
    s.THREE_LEVEL_DOWN = True
    assert s.bytes_per_vcycle() == 18461752
