"""The footprint harness (tests/footprint.py) itself, on the CPU: the mask builder against the level allocator's view
arithmetic, the four assertions driven by numpy stand-ins for a kernel (a correct one passes, each kind of fault is
reported by the assertion that is meant to catch it), the descriptor table's coverage of the library's entry points,
and the halo-copy cases against a numpy model of their record tables.  Nothing is launched."""
import numpy as np
import pytest

import footprint as fp


def test_masks_match_the_level_view():
    """nodes / interior / boundary / ring partition the frame as _Level.view() lays it out (33 x 321 fp64 and
    35 x 323 fp32: pad columns, ghost rows between samples, slack)"""
    for H, W, B, esz in ((33, 321, 2, 8), (35, 323, 3, 4), (3, 3, 1, 8)):
        g = fp.Geo(H, W, B, esz)
        assert g.numel == B * g.bs + 256 and g.bs >= (H + 2) * g.ld and g.ld >= W + 2 + g.off
        raw = np.arange(g.numel)
        view = raw[:B * g.bs].reshape(B, H + 2, g.ld)[:, 1:H + 1, g.off:g.off + W]     # _Level.view()
        assert np.array_equal(np.flatnonzero(g.nodes()), np.sort(view.ravel()))
        assert np.array_equal(np.flatnonzero(g.interior()), np.sort(view[:, 1:-1, 1:-1].ravel()))
        assert g.boundary().sum() == B * (H * W - (H - 2) * (W - 2))
        assert g.ring().sum() == B * ((H + 2) * (W + 2) - H * W) and not (g.ring() & g.nodes()).any()
        assert not g.nodes()[B * g.bs:].any()
        assert g.where(int(view[B - 1, 2, 1])) == f"sample {B - 1} row 2 column 1"
        assert g.where(B * g.bs + 3) == "slack element 3"
        p = g.pid()
        assert p.B == 1 and p.ld == g.ld and p.off == g.off and p.numel == (H + 2) * g.ld + 256


def test_poison_and_canaries():
    g = fp.Geo(5, 7, 2, 4)
    rng = np.random.default_rng(0)
    nodes = rng.standard_normal((2, 5, 7)).astype(np.float32)
    f = fp.field_in("f", g, np.float32, nodes)
    assert (f.z[~g.nodes()] == 0).all() and np.isnan(f.p[~g.nodes()]).all()
    assert np.array_equal(f.z[g.nodes()], nodes.ravel()) and np.array_equal(f.p[g.nodes()], nodes.ravel())
    r = fp.field_in("r", g, np.float32, nodes, keep=g.ring())
    assert (r.p[g.ring()] == 0).all() and np.isnan(r.p[~g.nodes() & ~g.ring()]).all()
    o = fp.field_out("o", g, np.float64, g.interior())
    assert (o.z.view(np.uint8) == fp.C1).all() and (o.p.view(np.uint8) == fp.C2).all() and np.isfinite(o.z).all()
    ids = rng.integers(0, 16, (5, 7))
    m = fp.pid_in("pid", g.pid(), ids, 16, rng)
    assert m.p.max() < 16 and (m.z[~g.pid().nodes()] == 0).all() and (m.p[~g.pid().nodes()] != 0).any()
    assert np.array_equal(m.p[g.pid().nodes()], ids.ravel())


# a numpy stand-in for a framed kernel: out(interior) = 2 u + f; `fault` breaks it in one way
H, W, B = 7, 11, 2


def stand_in_case():
    g = fp.Geo(H, W, B, 8)
    rng = np.random.default_rng(1)
    c = fp.Case("stand_in", "f64", f"{H}x{W}")
    c.add(fp.field_in("u", g, np.float64, rng.standard_normal((B, H, W))))
    c.add(fp.field_in("f", g, np.float64, rng.standard_normal((B, H, W))))
    c.add(fp.field_out("out", g, np.float64, g.interior()))
    return c, g


def stand_in(g, fault=None):
    def launch(case, bufs):
        u, f, out = bufs["u"], bufs["f"], bufs["out"]
        rows, cols = np.arange(1, H - 1), np.arange(1, W - 1)
        if fault == "skipped":
            cols = cols[:-1]                                   # the last interior column is never stored
        i = g.index(rows, cols).ravel()
        out[i] = 2 * u[i] + f[i]
        if fault == "0 * pad":                                 # the last column's result adds 0 * (ghost column W)
            j = g.index(rows, [W - 2]).ravel()
            out[j] = out[j] + 0 * u[j + 2]
        elif fault == "ghost column":
            out[g.index([3], [W]).ravel()] = 1.0
        elif fault == "pad column":
            out[g.index([3], [W + 5]).ravel()] = 1.0
        elif fault == "slack":
            out[B * g.bs + 17] = 1.0
        elif fault == "boundary node":
            out[g.index([0], [4]).ravel()[-1]] = 1.0           # (only in the last sample)
        elif fault == "input":
            f[g.index([2], [2]).ravel()] += 1.0
        return bufs
    return launch


def test_correct_stand_in_passes():
    c, g = stand_in_case()
    after = fp.run_case(c, stand_in(g))
    assert np.array_equal(after["Z"]["out"][g.interior()], after["P"]["out"][g.interior()])


@pytest.mark.parametrize("fault,kind,operand", [
    ("ghost column", "a", "out"), ("pad column", "a", "out"), ("slack", "a", "out"), ("boundary node", "a", "out"),
    ("input", "b", "f"), ("0 * pad", "c", "out"), ("skipped", "d", "out")])
def test_fault_is_reported_by_its_assertion(fault, kind, operand):
    c, g = stand_in_case()
    with pytest.raises(fp.FootprintError) as e:
        fp.run_case(c, stand_in(g, fault))
    assert (e.value.kind, e.value.operand) == (kind, operand), str(e.value)


def test_in_place_and_loose_operands():
    """An in-place operand's canary is its own content (an update that moves nothing is a skipped store); a loose
    write set may be written in part, but what is written must not depend on the poison."""
    g = fp.Geo(H, W, B, 8)
    rng = np.random.default_rng(2)
    x = fp.field_inout("x", g, np.float64, rng.standard_normal((B, H, W)), g.interior())
    ws = fp.flat_out("ws", 8, np.float64, np.arange(8) < 6, loose=True)
    i = g.index(np.arange(1, H - 1), np.arange(1, W - 1)).ravel()

    def run(move, wsval, nws=3):
        out = {}
        for key, b0, w0 in (("Z", x.z, ws.z), ("P", x.p, ws.p)):
            xb, wb = b0.copy(), w0.copy()
            xb[i] += move
            wb[:nws] = wsval(key)
            out[key] = {"x": xb, "ws": wb}
        fp.check([x, ws], out["Z"], out["P"])
    run(1.0, lambda k: 2.0)
    for move, wsval, nws, kind in ((0.0, lambda k: 2.0, 3, "d"), (1.0, lambda k: 2.0 if k == "Z" else np.nan, 3, "c"),
                                   (1.0, lambda k: 2.0, 7, "a")):
        with pytest.raises(fp.FootprintError) as e:
            run(move, wsval, nws)
        assert e.value.kind == kind


def test_join_rects_leave_nodes_uncovered():
    for Hh, Ww in ((5, 5), (33, 321), (35, 323), (321, 9)):
        rects, fine, coarse = fp.join_rects(Hh, Ww)
        Hc = (Hh + 1) // 2
        assert 1 <= len(rects) <= 4
        for I0, I1, c0, c1 in rects:     # the entry point's own rules (include/feanet_hip.h)
            assert 1 <= I0 < I1 <= Hc - 1 and c0 % 2 == 1 and 1 <= c0 < c1 <= Ww - 1 and (c1 % 2 == 1 or c1 == Ww - 1)
        inner = np.zeros((Hh, Ww), bool)
        inner[1:-1, 1:-1] = True
        assert fine.any() and not (fine & ~inner).any() and (inner & ~fine).any(), "must not cover the grid"
        assert coarse.any() and not coarse[0].any() and not coarse[-1].any() and not coarse[:, 0].any() and \
            not coarse[:, -1].any()
    assert len(fp.join_rects(33, 321)[0]) == 2


def test_covers_every_framed_entry_point():
    """Every mg_* and pcg_* name of _lib._SIGS, the four fea_pcg_*_f64f32 names and the two fea_dd_copy_* names of
    _lib._EXTRA have a footprint descriptor: a new entry point cannot ship without one."""
    from feanet_amd import _lib
    want = [n for n in _lib._SIGS if n.startswith(("mg_", "pcg_"))]
    want += [n for n in _lib._EXTRA if n.endswith("_f64f32") or n.startswith("fea_dd_copy_")]
    assert len(want) >= 35
    assert sorted(fp.DESC) == sorted(want)
    for name, names in {**fp.PCG_ARGS, **fp.MIXED_ARGS}.items():
        sig = _lib._SIGS[name] if name in _lib._SIGS else _lib._EXTRA[name][0]
        assert len(names.split()) + 1 == len(sig), name


@pytest.mark.parametrize("entry", sorted(fp.DESC))
def test_cases_are_well_formed(entry):
    """Every case of the table builds; its calls name existing operands and match the signature's length; every
    output has a write set inside its buffer, disjoint from the slack a framed output ends with."""
    from feanet_amd import _lib
    d = fp.DESC[entry]
    for suf in d.sufs:
        cs = fp.cases(entry, suf)
        assert cs
        for c in cs:
            names = {o.name for o in c.ops}
            assert c.calls
            for sym, args in c.calls:
                key = sym[4:-4] if sym[4:-4] in _lib._SIGS else sym
                sig = _lib._SIGS[key] if key in _lib._SIGS else _lib._EXTRA[sym][0]
                assert len(args) + 1 == len(sig), (c, sym)
                for a in args:
                    if isinstance(a, fp.Ref):
                        assert a.name in names, (c, a.name)
                    if isinstance(a, fp.Refs):
                        assert all(n is None or n in names for n in a.names), c
            assert any(o.role != "in" for o in c.ops), c
            for o in c.ops:
                if o.role != "in" and o.geo is not None:
                    assert not o.mask[o.geo.B * o.geo.bs:].any() and not (o.mask & ~o.geo.nodes()).any(), (c, o.name)


def dd_model(case, bufs):
    """numpy model of fea_dd_copy_blocks / fea_dd_copy_rects reading the case's record table"""
    size = {n: a.size * a.itemsize for n, a in bufs.items()}
    addr = {"src": 1 << 40, "dst": 1 << 41}

    def elem(a, esz):      # address -> (buffer, element index)
        n = "dst" if a >= addr["dst"] else "src"
        o = a - addr[n]
        assert 0 <= o < size[n] and o % esz == 0
        return bufs[n], o // esz
    for sym, args in case.calls:
        tab, n, esz = args[0].make(addr).tobytes(), args[1], args[2]
        for i in range(n):
            if sym == "fea_dd_copy_blocks":
                frame, stage, ld = np.frombuffer(tab, np.int64, 3, 32 * i)
                rows, cols = np.frombuffer(tab, np.int32, 2, 32 * i + 24)
                (fb, f0), (sb, s0) = elem(frame, esz), elem(stage, esz)
                for r in range(rows):
                    if args[3]:
                        sb[s0 + r * cols:s0 + (r + 1) * cols] = fb[f0 + r * ld:f0 + r * ld + cols]
                    else:
                        fb[f0 + r * ld:f0 + r * ld + cols] = sb[s0 + r * cols:s0 + (r + 1) * cols]
            else:
                dst, src, dld, sld, rows, cols = np.frombuffer(tab, np.int64, 6, 48 * i)
                (db, d0), (sb, s0) = elem(dst, esz), elem(src, esz)
                for r in range(rows):
                    db[d0 + r * dld:d0 + r * dld + cols] = sb[s0 + r * sld:s0 + r * sld + cols]
    return bufs


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_dd_cases_against_the_record_model(suf):
    """49 blocks / 33 rectangles (one past a launch's table), a record without rows, one block past 256 * 256
    elements: the cases' expected values and write sets are those of the records they pass."""
    for entry in fp.DD_NAMES:
        for c in fp.cases(entry, suf):
            n = c.calls[0][1][1]
            assert n == (49 if entry.endswith("blocks") else 33)
            rec = fp.dd_layout(entry, n)
            assert rec[0][2] * rec[0][3] > 256 * 256 and rec[1][2] == 0
            assert len({(h, w) for _, _, h, w in rec}) > 10
            fp.run_case(c, dd_model)
            dst = next(o for o in c.ops if o.name == "dst")
            assert dst.mask.sum() == sum(h * w for _, _, h, w in rec) and not dst.mask.all()


# ----------------------------------------------------------------------------- task-height ladders
def test_pick_rb_restatement_matches_the_abi():
    """The coverage guard's restatement of pick_rb against what the ABI exposes: fea_pcg_parts is nstrips x the row
    tasks of ONE sample at pick_rb's height, over a sweep of shapes that reaches every height; and the cycle join's
    partial count (fea_mg_join_norm_parts, which takes B because its height depends on it) differs between the
    ladder's rungs 1, 4 and 16."""
    from feanet_amd import _lib
    L = _lib.lib()
    heights = set()
    for esz in (4, 8):
        for H in (3, 5, 33, 129, 1025, 4097, 4099, 8193, 16385, 32769, 65537, 100001):
            for W in (3, 33, 163, 257, 259, 321, 515, 1025, 4097):
                ns = fp.nstrips(W, esz)
                rb = fp.pick_rb(1, ns, H - 2)
                heights.add(rb)
                assert L.fea_pcg_parts(H, W, esz) == ns * -(-(H - 2) // rb), (H, W, esz, rb)
        per = [L.fea_mg_join_norm_parts(B, fp.LADDER_H, fp.LADDER_W, esz) for B in (1, 4, 16)]
        assert len(set(per)) == 3 and min(per) > 0, per
    assert heights == {2, 4, 8, 16, 32}
    assert [fp.pick_rb(1, 1, H - 2) for H in (4097, 8193, 16385, 32769, 65537)] == [2, 4, 8, 16, 32]
    assert fp.pick_rb(1, 1, 131073 - 2, 64) == 64


def test_ladders_reach_their_heights():
    """five distinct heights on the batch ladder, six for the two kernels whose cap is 64 rows; a ladder that lost a
    height (kTargetWaves or kRB changed) says so"""
    for entry in fp.DESC:
        if entry in fp.BATCH_FREE or entry in fp.DD_NAMES:
            continue
        for esz in (4, 8):
            hs = fp.ladder_heights(entry, esz)
            if entry.startswith(("pcg_", "fea_pcg_")):
                assert set(hs) == {2}
            else:
                assert hs == [2, 4, 8, 16, 32] + ([64] if entry in fp.CAP64 else [])
    assert sorted(fp.CAP64) == ["mg_cycle_join", "mg_sweep_restrict"]
    old = fp.K_TARGET_WAVES
    try:
        fp.K_TARGET_WAVES = 4096
        with pytest.raises(AssertionError, match="re-pick the ladder"):
            fp.ladder_heights("mg_sweep", 8)
    finally:
        fp.K_TARGET_WAVES = old


# a numpy stand-in for a framed kernel with a fused norm, run in row tasks whose height grows with the batch:
# out(interior) = 2 u + f, norm[b] = sqrt(sum of u^2 over the interior), one partial per task in ws
LH, LW = 19, 9


def ladder_case(B):
    g = fp.Geo(LH, LW, B, 8)
    rng = np.random.default_rng(B)
    c = fp.Case("stand_in", "f64", f"{LH}x{LW} B={B}")
    c.B, c.norm_n, c.nan_op = B, (LH - 2) * (LW - 2), "u"
    c.add(fp.field_in("u", g, np.float64, rng.standard_normal((B, LH, LW))))
    c.add(fp.field_in("f", g, np.float64, rng.standard_normal((B, LH, LW))))
    c.add(fp.field_out("out", g, np.float64, g.interior()))
    c.add(fp.flat_out("ws", 10 * B + 3, np.float64, np.arange(10 * B + 3) < 10 * B, loose=True, norm="ws"))
    c.add(fp.flat_out("norm", B + 2, np.float64, np.arange(B + 2) < B, sample=fp.rows(1), norm="norm"))
    return c, g


def ladder_stand_in(fault=None):
    def launch(case, bufs):
        B = case.B
        g = fp.Geo(LH, LW, B, 8)
        u, f, out, ws, norm = (bufs[n] for n in ("u", "f", "out", "ws", "norm"))
        rb = 2 * B                                           # the task height: 2, 4, 8 rows on the rungs 1, 2, 4
        cols = np.arange(1, LW - 1)
        for b in range(B):
            starts = list(range(1, LH - 1, rb))
            for t, r0 in enumerate(starts):
                rows = np.arange(r0, min(r0 + rb, LH - 1))
                i = g.index(rows, cols)[b].ravel()
                out[i] = 2 * u[i] + f[i]
                if fault == "height" and t:                  # a task's first row takes its halo row from the wrong place
                    j = g.index(rows[:1], cols)[b].ravel()
                    out[j] += 1e-9 * u[j - g.ld]
                sq = u[i] ** 2
                ws[b * len(starts) + t] = np.nansum(sq) if fault == "nan dropped" else sq.sum()
            if fault == "leak" and b + 1 < B:                # 0 * (a node of the next sample)
                j = g.index([2], [2])
                out[j[b]] += 0 * u[j[b + 1]]
            norm[b] = np.sqrt(ws[b * len(starts):(b + 1) * len(starts)].sum())
            if fault == "norm height":
                norm[b] *= 1 + 1e-9 * rb
        return bufs
    return launch


def test_correct_ladder_stand_in_passes():
    report = fp.run_ladder(lambda B: ladder_case(B)[0], (1, 2, 4), fp.HostBackend(ladder_stand_in()))
    assert [n for _, n in report] == [3, 9, 5, 9]           # partials per sample: B=4 (top), B=1, B=2, last alone
    fp.isolation(ladder_case(3)[0], fp.HostBackend(ladder_stand_in()))


@pytest.mark.parametrize("fault,kind,operand", [("height", "h", "out"), ("norm height", "h", "norm"),
                                                ("leak", "s", "out"), ("nan dropped", "n", "norm")])
def test_ladder_fault_is_reported_by_its_assertion(fault, kind, operand):
    """a result that depends on the task height, a norm that does, a leak between samples and a NaN that a norm
    drops each raise the error kind meant for them"""
    with pytest.raises(fp.FootprintError) as e:
        fp.run_ladder(lambda B: ladder_case(B)[0], (1, 2, 4), fp.HostBackend(ladder_stand_in(fault)))
    assert (e.value.kind, e.value.operand) == (kind, operand), str(e.value)


def test_prefix_rungs_hold_the_top_rungs_samples():
    """derive(): a lower rung's per-sample operands are the top rung's samples block by block (ghost rows and
    padding included), shared operands whole; flat [B, per] operands and the gathered source's rank-major blocks
    follow their own layouts"""
    be = fp.HostBackend(None)
    for entry, shape, mode in (("mg_pack", (33, 321), ""), ("mg_mid_down_gathered", (13, 13), "k 1 T 4 4"),
                               ("pcg_update", (33, 321), ""), ("fea_pcg_update_f64f32", (33, 321), "")):
        suf = "f64"
        top = fp.build_case(entry, suf, shape + (3,), True if entry != "mg_pack" else False, mode)
        tb = be.initial(top)
        for src in ((0,), (0, 1), (2,)):
            c = fp.build_case(entry, suf, shape + (len(src),), True if entry != "mg_pack" else False, mode)
            b = be.initial(c)
            fp.derive(top, tb, c, b, src)
            for op, t in zip(c.ops, top.ops):
                if op.role == "out":
                    continue
                if op.sample is None:
                    assert np.array_equal(b[op.name], tb[op.name])
                    continue
                assert op.name in ("src", "bc", "gsrc", "scalars", "sb") or op.geo is not None, op.name
                for i, s in enumerate(src):
                    assert np.array_equal(b[op.name][op.sample(c.B, i)], tb[op.name][t.sample(3, s)], equal_nan=True)
        if entry == "mg_mid_down_gathered":       # [Pr * Pc][B][gcr][gcc]
            gs = next(o for o in top.ops if o.name == "gsrc")
            v = gs.z.reshape(4, 3, 6 * 6)
            assert np.array_equal(gs.z[gs.sample(3, 1)], v[:, 1].ravel())
