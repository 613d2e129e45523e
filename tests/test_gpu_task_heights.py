"""Every framed and Krylov entry point at every row-task height, and the isolation of a batch's samples.

The host picks the rows per wave task (rb) from the batch size and the shape (pick_rb, balanced_rb, join_config), and
"results are bitwise independent of the task height" (csrc/hnet_ops.hip, csrc/framed_ops.hip).  tests/footprint.py
drives the height with one strip and a tall grid: at H = 4097, W = 33 the batches B = 1, 2, 4, 8, 16 reach
rb = 2, 4, 8, 16, 32, and B = 32 reaches 64 in the two kernels whose cap is 64 rows (fea_mg_sweep_restrict,
fea_mg_cycle_join; B = 16 also crosses the join's kJoinBatchPow2).  A case is built once for the top rung and stays on
the GPU; every lower rung is a prefix of its samples, one more holds the last sample alone, and

  * sample b's field outputs, send blocks and sb values are the SAME BYTES in every rung that contains it;
  * the Krylov partial sums are the same bytes on every rung (pcg_geom takes the height of ONE sample);
  * the residual norms (fea_mg_residual_norm, also over a range; the fused norms of fea_mg_sweep_restrict and
    fea_mg_cycle_join, appended in the call or deferred) are sums of the same non-negative squares in another order:
    bitwise equal where two rungs have the same number of partials per sample, and otherwise within 2 n u relative,
    n the nodes summed and u = 2^-53: every kernel accumulates its norm in double (`double ssq` / `double s` per lane,
    wave_sum(double), k_norm_final / k_norm_append in double), whatever the field type;
  * nothing outside the write set is stored and no input moves, on every rung (assertions (a), (b) of footprint.check).

W = 163 (two fp64 strips, the second ragged; 161 for the two-level kernels, whose second coarse grid needs it) repeats
the rungs B = 1, 2, 4.  Entry points whose geometry ignores B
(mid, hmid, the tails, pack, unpack) run the prefix check at their DESC shapes with B = 1, 2, 3.

Isolation, on the B = 4 rung and on every DESC case with B >= 2, for sample j first, middle and last: with every node
of sample j a quiet NaN in every per-sample input (its scalars row included) every other sample's outputs, norms and
partial sets keep their bytes; with ONE NaN at an interior node, every norm the call produces for sample j is
non-finite (a diverged sample never reports a finite residual).

Both streaming modes: FEANET_NT_BYTES=0 runs the nontemporal instantiations on every rung, 1 TiB the cached ones."""
import time

import numpy as np
import pytest
import torch

import footprint as fp

pytestmark = pytest.mark.gpu

STREAM = {"nt": "0", "cached": str(1 << 40)}
PARAMS = [(e, suf, two) for e in sorted(fp.DESC) if e not in fp.DD_NAMES for suf in fp.DESC[e].sufs
          for two in ((False, True) if fp.DESC[e].two else (False,))]


def ladder_build(entry, suf, H, W, two, mode):
    return lambda B: fp.build_case(entry, suf, (H, W, B), two, mode)


@pytest.mark.parametrize("stream", sorted(STREAM))
@pytest.mark.parametrize("entry,suf,two", PARAMS, ids=[f"{e}-{s}-{'16' if t else '1'}" for e, s, t in PARAMS])
def test_task_heights(entry, suf, two, stream, monkeypatch):
    monkeypatch.setenv("FEANET_NT_BYTES", STREAM[stream])
    t0 = time.perf_counter()
    be = fp.DeviceBackend()
    d = fp.DESC[entry]
    esz = 4 if suf == "f32" else 8
    failed, lines = [], []

    def attempt(what, fn):
        try:
            r = fn()
            lines.append(f"  {what}: " + (", ".join(f"{lab} ({n} partials)" if n else lab for lab, n in r) if r else
                                          "ok"))
        except fp.FootprintError as e:
            failed.append(f"{what}: {e}")
    if entry in fp.BATCH_FREE:
        for shape, tw, mode in d.params():
            if tw == two:
                H, W, _ = shape
                attempt(f"{H}x{W} {mode} prefixes B=1,2,3 + isolation",
                        lambda: fp.run_ladder(ladder_build(entry, suf, H, W, two, mode), fp.SMALL_RUNGS, be, 3))
    else:
        rungs = fp.rungs_of(entry)
        hs = fp.ladder_heights(entry, esz)
        for mode in d.modes:
            attempt(f"{fp.LADDER_H}x{fp.LADDER_W} {mode} heights {hs}",
                    lambda: fp.run_ladder(ladder_build(entry, suf, fp.LADDER_H, fp.LADDER_W, two, mode), rungs, be, 4))
            W2 = fp.ladder_w2(entry)
            attempt(f"{fp.LADDER_H}x{W2} {mode} heights {fp.ladder_heights(entry, esz, W2, (1, 2, 4))}",
                    lambda: fp.run_ladder(ladder_build(entry, suf, fp.LADDER_H, W2, two, mode), (1, 2, 4), be, None))
        for shape, tw, mode in d.params():
            if tw == two and shape[2] >= 2:
                c = fp.build_case(entry, suf, shape, two, mode)
                attempt(f"{c} isolation", lambda: fp.isolation(c, be))
    print(f"{entry}_{suf} {'16 patterns' if two else 'one pattern'} {stream}: {time.perf_counter() - t0:.2f} s\n" +
          "\n".join(lines))
    assert not failed, f"{len(failed)} failures:\n" + "\n".join(failed)


def test_device_comparison_tells_samples_apart():
    """A control of the device-resident path (the host tests drive the same code with numpy): a rung derived from
    sample 1 of the top rung agrees with sample 1 and is reported ('h') against sample 0; a sample poisoned with NaN
    differs from its clean run ('s' when compared as if it were another sample's)."""
    be = fp.DeviceBackend()
    build = ladder_build("mg_sweep_restrict", "f64", 33, 321, True, "hist")
    top, one = build(3), build(1)
    before = be.initial(top)
    after = be.launch(top, be.clone(before))
    fp.check_ab(top, before, after)
    b1 = be.initial(one)
    fp.derive(top, before, one, b1, (1,))
    a1 = be.launch(one, be.clone(b1))
    for norms in (False, True):
        fp.compare_samples("h", "sample 1 alone", one, a1, 0, top, after, 1, norms)
        with pytest.raises(fp.FootprintError) as e:
            fp.compare_samples("h", "sample 1 against sample 0", one, a1, 0, top, after, 0, norms)
        assert e.value.kind == "h" and e.value.operand == ("norm_hist" if norms else "u_out"), str(e.value)
    bufs = be.clone(before)
    u = next(o for o in top.ops if o.name == "u")
    bufs["u"][torch.as_tensor(fp.sample_nodes(u.geo, 2), device="cuda")] = float("nan")
    got = be.launch(top, bufs)
    fp.compare_samples("s", "sample 1 next to a NaN sample", top, got, 1, top, after, 1)
    with pytest.raises(fp.FootprintError) as e:
        fp.compare_samples("s", "the NaN sample itself", top, got, 2, top, after, 2)
    assert e.value.kind == "s"
    assert not np.isfinite(fp.norm_values(top, got, 2)["norm_hist"])
    assert np.isfinite(fp.norm_values(top, got, 1)["norm_hist"])


# ----------------------------------------------------------------------------- solver level
def _rhs(rng, B, H, W, T):
    return torch.from_numpy(rng.standard_normal((B, 1, H, W))).cuda().to(T)


@pytest.mark.parametrize("smoother", ["jac", "hjac"])
@pytest.mark.parametrize("T", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_multigrid_solver_batch_16_against_batch_1(T, smoother):
    """MultigridSolver on 4097 x 33 nodes, vcycle(3): samples 0 and 15 of a batch of 16 are the bytes of the same
    right-hand sides solved alone.  The two plans differ in every task height and in the join's path (balanced
    heights at B = 1, the power of two at B = 16)."""
    from feanet_amd.solver import MultigridSolver
    rows, n, B = 4096, 32, 16
    rng = np.random.default_rng(16)
    kw = dict(rows=rows, dtype=T)
    if smoother == "hjac":
        kw.update(smoother="hjac", hnet=(0.2 * rng.standard_normal((3, 3, 3))).astype(np.float32))
    f = _rhs(rng, B, rows + 1, n + 1, T)
    sb = MultigridSolver(n, batch=B, **kw)
    sb.set_rhs(f=f)
    sb.load()
    sb.vcycle(3)
    ub = sb.solution()
    assert torch.isfinite(ub).all()
    for b in (0, B - 1):
        s1 = MultigridSolver(n, batch=1, **kw)
        s1.set_rhs(f=f[b:b + 1])
        s1.load()
        s1.vcycle(3)
        u1 = s1.solution()[0]
        bad = (u1.view(torch.int64 if T == torch.float64 else torch.int32) !=
               ub[b].view(torch.int64 if T == torch.float64 else torch.int32))
        assert not bad.any(), f"sample {b}: {int(bad.sum())} nodes differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("T", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_pcg_solver_batch_16_against_batch_1(T):
    """PCGSolver on 4097 x 33 nodes, iterate(3): samples 0 and 15 of a batch of 16 against the same systems alone,
    bitwise (iterate and residual history)."""
    from feanet_amd import PCGSolver
    rows, n, B = 4096, 32, 16
    rng = np.random.default_rng(17)
    f = _rhs(rng, B, rows + 1, n + 1, T)
    sb = PCGSolver(n, rows=rows, dtype=T, batch=B)
    sb.set_rhs(f=f)
    sb.load()
    sb.iterate(3)
    xb, hb = sb.solution(), np.array(sb.history())
    assert torch.isfinite(xb).all() and hb.shape == (4, B)
    I = torch.int64 if T == torch.float64 else torch.int32
    for b in (0, B - 1):
        s1 = PCGSolver(n, rows=rows, dtype=T, batch=1)
        s1.set_rhs(f=f[b:b + 1])
        s1.load()
        s1.iterate(3)
        bad = s1.solution()[0].view(I) != xb[b].view(I)
        assert not bad.any(), f"sample {b}: {int(bad.sum())} nodes differ, first at {bad.nonzero()[0].tolist()}"
        assert np.array_equal(np.array(s1.history())[:, 0], hb[:, b]), f"sample {b}: residual history differs"
