"""Which template bodies of the coarse tail a shape list reaches, on the CPU.

The fused V(1,1) path of fea_mg_coarse_tail (TailFast, csrc/coarse_tail.hip) splits a level's rows over 16 waves and
dispatches on the rows per wave and on the parity of the wave's first window row; fea_mg_coarse_tail_ext splits the
level above the tail the same way.  A body that no tested shape reaches has never run.  The partition is restated
here in plain Python, formula by formula with the lines it restates, and the shape lists of
tests/test_gpu_odd_grids.py are checked against it: every reachable body is reached.  What the shapes of
test_gpu_mg.test_coarse_tail_kernel / test_coarse_tail_ext_bitwise reach on their own is recorded too.

The second half shows that the oracle comparison of test_gpu_odd_grids.py notices the faults these bodies could
have: a sub-cycle whose prolongation drops one coarse row of a three-row wave, or whose coarsest level skips its last
column, is rejected by the same close() call at the same tolerance (as test_footprint_host.py does for the
footprint harness).  Nothing is launched."""
import numpy as np
import pytest
import torch

from oracle import feanet_oracle as orc
from test_gpu_mg import close, npdt
from test_gpu_odd_grids import EXT_SHAPES, TAIL_SHAPES, W0, W1
from test_schedule import tail_oracle

WAVES = 1024 // 64                           # kTailThreads / 64                          coarse_tail.hip:22-24
DOWN_ROWS = (31 + WAVES - 1) // WAVES        # kTailDownRows = 2                          :97
UP_ROWS = (63 + WAVES - 1) // WAVES          # kTailUpRows = 4                            :99
EXT_DOWN_ROWS = (63 + WAVES - 1) // WAVES    # ext_down's PER = 4                         :736
EXT_UP_ROWS = 2 * ((127 + 2 * WAVES - 1) // (2 * WAVES))  # ext_up's PER = 8              :802
MAX_N = 65                                   # kTailMaxN                                  :27


def tail_n(n0, k):
    return ((n0 - 1) >> k) + 1               # tail_n                                     :73


def dim_ok(n, nlev):
    """tail_dim_ok                                                                        :917-925"""
    if n < 3 or n > MAX_N:
        return False
    for _ in range(1, nlev):
        if (n - 1) & 1:
            return False
        n = (n + 1) // 2
        if n < 3:
            return False
    return True


def down_waves(H):
    """TailFast::down on a level of H rows: (wave, I0, I1, PER of the body)                :257-269"""
    Hc = (H + 1) // 2                        #                                            :259
    per = (Hc - 2 + WAVES - 1) // WAVES      #                                            :260
    out = []
    for wv in range(WAVES):
        I0 = 1 + wv * per                    #                                            :261
        I1 = min(Hc - 1, I0 + per)
        if I0 >= I1:                         #                                            :266
            continue
        out.append((wv, I0, I1, per, 1 if per == 1 else DOWN_ROWS))  #                    :267-268
    return out


def up_waves(H):
    """TailFast::up: (wave, y0, y1, per, (PAR, PER) of the body)                           :383-391, 375-382"""
    per = (H - 2 + WAVES - 1) // WAVES       #                                            :386
    out = []
    for wv in range(WAVES):
        y0 = 1 + wv * per                    #                                            :387
        y1 = min(H - 1, y0 + per)
        if y0 >= y1:                         #                                            :388
            continue
        par = (y0 - 1) & 1                   #                                            :389
        out.append((wv, y0, y1, per, (par, per if per in (1, 2, 3) else UP_ROWS)))  # switch (per)  :376-381
    return out


def coarsest_waves(H):
    """TailFast::coarsest: (wave, y0, y1, per, PER of the body)                            :392-404"""
    per = (H - 2 + WAVES - 1) // WAVES       #                                            :395
    out = []
    for wv in range(WAVES):
        y0 = 1 + wv * per                    #                                            :396
        y1 = min(H - 1, y0 + per)
        if y0 >= y1:                         #                                            :397
            continue
        out.append((wv, y0, y1, per, per if per in (1, 2, 3) else UP_ROWS))  #            :398-403
    return out


def ext_down_waves(Ht):
    """ext_down: coarse rows [I0, I1) of the tail's top level per wave, one compiled body  :736-740, 774-776"""
    per = (Ht - 2 + WAVES - 1) // WAVES      #                                            :738
    out = []
    for wv in range(WAVES):
        I0 = 1 + wv * per                    #                                            :739
        I1 = min(Ht - 1, I0 + per)
        if I0 >= I1:                         #                                            :740
            continue
        out.append((wv, I0, I1, per, EXT_DOWN_ROWS))
    return out


def ext_up_waves(H):
    """ext_up: fine rows [y0, y1) of level X per wave, one compiled body of 8 rows         :802-807, 861"""
    per = 2 * ((H - 2 + 2 * WAVES - 1) // (2 * WAVES))  #                                 :805
    out = []
    for wv in range(WAVES):
        y0 = 1 + wv * per                    #                                            :806
        y1 = min(H - 1, y0 + per)
        if y0 >= y1:                         #                                            :807
            continue
        out.append((wv, y0, y1, per, EXT_UP_ROWS))
    return out


def fast_bodies(Ht, Wt, nlev):
    """What the fused path (nu = (1, 1), tail_fast :441-456) runs on an Ht x Wt tail of nlev levels: the bodies of
    each phase over all levels, and whether some last wave has fewer rows than the others' per."""
    assert dim_ok(Ht, nlev) and dim_ok(Wt, nlev), (Ht, Wt, nlev)
    r = dict(down=set(), up=set(), coarsest=set(), short_down=False, short_up=False)
    for k in range(nlev - 1):                # down(k), then up(k) on the way back        :443-445, 453-455
        H = tail_n(Ht, k)
        dw, uw = down_waves(H), up_waves(H)
        r["down"] |= {w[4] for w in dw}
        r["up"] |= {w[4] for w in uw}
        r["short_down"] |= any(w[2] - w[1] < w[3] for w in dw)
        r["short_up"] |= any(w[2] - w[1] < w[3] for w in uw)
    r["coarsest"] |= {w[4] for w in coarsest_waves(tail_n(Ht, nlev - 1))}  #              :448
    return r


def reached(shapes):
    tot = dict(down=set(), up=set(), coarsest=set(), short_down=False, short_up=False)
    for s in shapes:
        for key, v in fast_bodies(*s).items():
            tot[key] = tot[key] | v
    return tot


ALL_UP = {(0, 1), (1, 1), (0, 2), (0, 3), (1, 3), (0, 4)}


def test_partition_covers_every_row_once():
    """Every height the entry points admit: the waves' row ranges tile the interior rows exactly once, in order,
    and no wave has more rows than the body it is sent to was compiled for."""
    for H in range(3, MAX_N + 1):
        for waves, lo, hi in ((up_waves(H), 1, H - 1), (coarsest_waves(H), 1, H - 1)) + (
                ((down_waves(H), 1, (H + 1) // 2 - 1),) if H & 1 and H >= 5 else ()):
            rows = [y for w in waves for y in range(w[1], w[2])]
            assert rows == list(range(lo, hi)), (H, waves)
            for w in waves:
                body = w[4][1] if isinstance(w[4], tuple) else w[4]
                assert w[2] - w[1] <= body and w[3] <= body, (H, w)
    for Ht in range(3, MAX_N + 1):
        H = 2 * Ht - 1
        for waves, lo, hi in ((ext_down_waves(Ht), 1, Ht - 1), (ext_up_waves(H), 1, H - 1)):
            assert [y for w in waves for y in range(w[1], w[2])] == list(range(lo, hi)), (Ht, waves)
            assert all(w[2] - w[1] <= w[4] and w[3] <= w[4] for w in waves), (Ht, waves)
        assert all((w[1] - 1) % 2 == 0 for w in ext_up_waves(H))  # "even: y0 - 1 is even on every wave"  :805


def test_unreachable_up_bodies():
    """(PAR, PER) = (1, 2) and (1, 4) are compiled (up_par<1>'s switch) but no height reaches them: wv * per is even
    for an even per.  Every other body is reachable, three rows per wave only for 35 <= H <= 50."""
    seen = set()
    for H in range(3, MAX_N + 1):
        seen |= {w[4] for w in up_waves(H)}
    assert seen == ALL_UP and (1, 2) not in seen and (1, 4) not in seen
    assert [H for H in range(3, MAX_N + 1) if up_waves(H)[0][3] == 3] == list(range(35, 51))
    assert {H for H in range(35, 51) if dim_ok(H, 2)} >= {37, 41, 45, 49}


def test_new_shapes_reach_every_body():
    got = reached(TAIL_SHAPES)
    assert got["up"] == ALL_UP, ALL_UP - got["up"]
    assert got["coarsest"] == {1, 2, 3, 4}, got["coarsest"]
    assert got["down"] == {1, DOWN_ROWS} == {1, 2}
    assert got["short_down"] and got["short_up"]
    # a coarsest level with an even node count (4, 6, 8 below a finer level; 64 alone) and tails with Ht != Wt
    ends = {(tail_n(Ht, nlev - 1), nlev > 1) for Ht, _, nlev in TAIL_SHAPES}
    assert {(4, True), (6, True), (4, False), (6, False), (64, False)} <= ends, ends
    assert {8, 6} <= {tail_n(Wt, nlev - 1) for _, Wt, nlev in TAIL_SHAPES}
    assert sum(Ht != Wt for Ht, Wt, _ in TAIL_SHAPES) >= 6
    # three rows per wave at both window parities needs two or more waves: every such shape has 12 or more
    assert all(len(up_waves(H)) >= 12 for H in (37, 41, 45, 49))


def test_new_ext_shapes_reach_every_row_count():
    ups = {ext_up_waves(Hx)[0][3] for Hx, _, _ in EXT_SHAPES}
    assert ups == {2, 4, 6, 8}, ups
    downs = {ext_down_waves((Hx + 1) // 2)[0][3] for Hx, _, _ in EXT_SHAPES}
    assert downs == {1, 2, 3, 4}, downs
    # 97 rows: 6 of the compiled 8 rows per wave, and the last wave's window is clipped in the middle (y < y1, :861)
    w = ext_up_waves(97)
    assert w[0][3] == 6 and w[-1][2] - w[-1][1] == 5 and len(w) == 16
    for Hx, Wx, nlev in EXT_SHAPES:
        assert dim_ok((Hx + 1) // 2, nlev) and dim_ok((Wx + 1) // 2, nlev), (Hx, Wx, nlev)
    assert any(Hx != Wx for Hx, Wx, _ in EXT_SHAPES)


# test_gpu_mg.test_coarse_tail_kernel's (Nt, nlev), all square, and the level-X rows of test_coarse_tail_ext_bitwise
OLD_TAIL_SHAPES = [(5, 5, 2), (9, 9, 3), (17, 17, 3), (33, 33, 5), (65, 65, 6), (65, 65, 2)]
OLD_EXT_ROWS = [129, 129, 129, 65, 17, 9, 65, 129]


def test_what_the_power_of_two_shapes_reached():
    """The record of the gap: 5, 9, 17, 33 and 65 nodes a side never run three rows per wave (either parity), never a
    coarsest level of three or four rows per wave or of an even node count, never a tail with Ht != Wt; the extended
    tail never runs 6 rows per wave."""
    got = reached(OLD_TAIL_SHAPES)
    assert got["up"] == {(0, 1), (1, 1), (0, 2), (0, 4)} and ALL_UP - got["up"] == {(0, 3), (1, 3)}
    assert got["coarsest"] == {1, 2}
    assert got["down"] == {1, 2} and got["short_down"] and got["short_up"]
    assert all(tail_n(Ht, nlev - 1) & 1 and Ht == Wt for Ht, Wt, nlev in OLD_TAIL_SHAPES)
    assert {ext_up_waves(H)[0][3] for H in OLD_EXT_ROWS} == {2, 4, 8}


# ----------------------------------------------------------------------------- the oracle assertions fire
def _problem(T, Ht=49, Wt=49, nlev=5, B=2):
    mg = orc.OracleMultigrid(Wt - 1, "poisson", npdt(T), levels=nlev, rows=Ht - 1, w=(W0, W1))
    rng = np.random.default_rng(Ht + Wt)
    f = rng.standard_normal((B, Ht, Wt)).astype(npdt(T))
    f[:, 0, :] = f[:, -1, :] = f[:, :, 0] = f[:, :, -1] = 0
    return mg, f, B


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
def test_oracle_rejects_a_dropped_coarse_row(T, monkeypatch):
    """Wave 1 of the 49-row level owns rows 4..6 (three rows, odd window parity: up_rows<1, 3>) and builds x on rows
    3..7 from the coarse rows 1..4.  A body that loses the last of them (c = 3 of its C = 4) gets row 7 of x wrong,
    and with it row 6 of the output."""
    wv, y0, y1, per, body = up_waves(49)[1]
    assert (y0, y1, per, body) == (4, 7, 3, (1, 3))
    Ib, C = (y0 - 1) >> 1, (1 + 3 + 2) // 2 + 1            # Ib, C of up_rows                 :309, 315
    lost, row = Ib + C - 1, y0 - 1 + 3 + 2 - 1             # coarse row 4, window row 7
    assert (lost, row) == (4, 7)
    mg, f, B = _problem(T)
    ref = tail_oracle(mg, 0, f, None, B, nu1=1, nu2=1, q2=False)
    good = orc.prolong

    def faulty(e, pidc, ptab, w1=1.0):
        out = good(e, pidc, ptab, w1)
        if e.shape[-2] == 25:
            e2 = e.copy()
            e2[:, lost, :] = 0
            out[:, row, :] = good(e2, pidc, ptab, w1)[:, row, :]
        return out
    monkeypatch.setattr(orc, "prolong", faulty)
    bad = tail_oracle(mg, 0, f, None, B, nu1=1, nu2=1, q2=False)
    assert np.array_equal(bad[:, :4], ref[:, :4]) and not np.array_equal(bad[:, 6], ref[:, 6])
    with pytest.raises(AssertionError, match="scaled max err"):
        close(bad[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, "dropped coarse row")


@pytest.mark.parametrize("T", [torch.float32, torch.float64])
@pytest.mark.parametrize("Ht,Wt,nlev", [(49, 49, 5), (6, 8, 1), (64, 64, 1)])
def test_oracle_rejects_a_skipped_coarsest_column(T, Ht, Wt, nlev):
    """A coarsest phase that never stores its last interior column (an even-width level's column W - 2, say)."""
    mg, f, B = _problem(T, Ht, Wt, nlev)
    ref = tail_oracle(mg, 0, f, None, B, nu1=1, nu2=1, q2=False)
    last = mg.levels[-1]
    good = last.sweep

    def faulty(v, ff):
        out = good(v, ff)
        out[:, :, -2] = v[:, :, -2]
        return out
    last.sweep = faulty
    bad = tail_oracle(mg, 0, f, None, B, nu1=1, nu2=1, q2=False)
    with pytest.raises(AssertionError, match="scaled max err"):
        close(bad[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], T, "skipped coarsest column")
