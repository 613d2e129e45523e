"""Domain decomposition (feanet_amd.dd) on the CPU: partition invariants, the
communication schedule, and a world_size 2 / 3 gloo run of the decomposed V-cycle (oracle
operators on each rank's slab) against the oracle's single-grid V-cycle on the global grid."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from feanet_amd.dd import (Partition, _joined_chunk_steps, _partition_for, dd_schedule, default_agglomeration,
                           exchange_depths, global_levels, simulate_validity)  # noqa: F401
from oracle import feanet_oracle as orc


@pytest.mark.parametrize("m,n,P,Ld", [(64, 32, 2, 2), (96, 64, 3, 3), (256, 128, 4, 3), (4096, 4096, 8, 4),
                                      (16384, 8192, 8, 4), (512, 512, 1, 3), (48, 16, 3, 2)])
def test_partition_invariants(m, n, P, Ld):
    part = Partition(m, n, P, Ld)
    for l in range(Ld + 1):
        H = (m >> l) + 1
        owned = []
        for r in range(P):
            p = part.level(l, r)
            owned += list(range(p.s, p.e))
            assert 0 <= p.gr0 and p.gr0 + p.Hloc <= H and p.Hloc % 2 == 1 and p.Hloc >= 3
            assert 1 <= p.lo and p.hi <= p.Hloc - 1
            if l < Ld:
                q = part.level(l + 1, r)
                assert p.gr0 == 2 * q.gr0 and p.Hloc == 2 * q.Hloc - 1  # fine (2I-1, 2I) <-> coarse I locally
                assert p.s == 2 * q.s - 1  # coarse row I owned with its fine rows (2I-1, 2I)
                assert p.e == (2 * q.e - 1 if r < P - 1 else H - 1)
                g = part.ghost(l)
                if r > 0:
                    assert p.lo == g + 1  # ghost rows below the owned rows (+ the kept edge row)
                if r < P - 1:
                    assert p.Hloc - p.hi == g
        assert owned == list(range(1, H - 1)), "interior rows owned exactly once"


def test_partition_rejects_bad_splits():
    with pytest.raises(ValueError):
        Partition(100, 64, 3, 2)
    with pytest.raises(ValueError):
        Partition(64, 64, 8, 3)  # 1 coarse row per rank
    with pytest.raises(ValueError):
        Partition(64, 64, 4, 3)  # 2 coarse rows per rank < 4 ghost rows
    assert Partition(512, 512, 4, 2).ghost(0) == 16


def test_dd_schedule_comm_counts():
    """Communication-avoiding schedule: one batch of neighbour messages + one all-gather per cycle."""
    for Ld in (1, 2, 3, 5):
        steps, end = dd_schedule(Ld, depths=(4, 9))
        kinds = [s[0] for s in steps]
        assert kinds.count("exchange") == (2 if Ld >= 2 else 1)
        assert kinds.count("gather") == kinds.count("coarse") == kinds.count("scatter") == 1
        assert end in ("a", "b")
        for kind, s in (("head", "a"), ("join", "b"), ("tail", "b")):
            st, _ = _joined_chunk_steps(Ld, 1, 1, True, kind, s, (4, 9))
            ex = [x for x in st if x[0] == "exchange"]
            assert len(ex) == {"head": 1 + (Ld >= 2), "join": 1 + (Ld >= 2), "tail": 1}[kind]


@pytest.mark.parametrize("m,n,P,Ld", [(64, 32, 2, 2), (128, 64, 2, 3), (16384, 8192, 8, 4), (16384, 8192, 8, 6)])
def test_exchange_depths_minimal(m, n, P, Ld):
    """The chosen depths keep every program exact; one row less of either does not."""
    part, (D0, D1) = _partition_for(m, n, P, Ld)
    init = lambda d: {(0, "a"): d, (0, "b"): d}

    def progs(D):
        out = [dd_schedule(Ld, 1, 1, True, "a", D)[0]]
        for nj in (0, 1, 2):
            seq, s = [], "a"
            for kind in ["head"] + ["join"] * nj + ["tail"]:
                st, s = _joined_chunk_steps(Ld, 1, 1, True, kind, s, D)
                seq += st
            out.append(seq)
        return out
    assert all(simulate_validity(p, Ld, part.ghost, init(D0)) for p in progs((D0, D1)))
    if D0 > 1:
        assert not all(simulate_validity(p, Ld, part.ghost, init(D0 - 1)) for p in progs((D0 - 1, D1)))
    if Ld >= 2 and D1 > 1:
        assert not all(simulate_validity(p, Ld, part.ghost, init(D0)) for p in progs((D0, D1 - 1)))
    assert D1 <= part.ghost(1) and D0 <= part.ghost(0)


def test_partition_grows_ghosts_when_needed():
    """V(2,2) at Ld = 4 needs more coarse ghost rows than V(1,1): the partition grows G."""
    part, _ = _partition_for(4096, 4096, 8, 4, 2, 2)
    assert part.G > _partition_for(4096, 4096, 8, 4)[0].G
    with pytest.raises(ValueError):
        exchange_depths(4, Partition(4096, 4096, 8, 4, 4).ghost, 2, 2, joined=False)


@pytest.mark.parametrize("m,n,P,Ld,nl", [(512, 512, 4, 2, 3), (1024, 1024, 8, 3, 3), (512, 512, 4, 2, 1),
                                         (16384, 8192, 8, 4, 3)])
def test_exchange_depths_learned_smoother(m, n, P, Ld, nl):
    """The learned smoother's decomposed V-cycle (dd_schedule(smoother='hjac')): every HRelax sweep loses 1 + nl
    ghost lines, so the chosen partition keeps more ghost lines than Jacobi's and the depths are minimal for the
    unjoined program; with nl HNet layers assumed fewer than the kernels apply the same depths fail."""
    part, (D0, D1) = _partition_for(m, n, P, Ld, smoother="hjac", nl=nl)
    init = lambda d: {(0, "a"): d, (0, "b"): d}
    prog = lambda D: dd_schedule(Ld, 1, 1, True, "a", D, "hjac")[0]
    kinds = {st[0] for st in prog((D0, D1))}
    assert {"hsweep_restrict", "prolong_hsweep", "gather", "coarse", "scatter"} <= kinds and "sweep" not in kinds
    assert simulate_validity(prog((D0, D1)), Ld, part.ghost, init(D0), nl)
    assert not simulate_validity(prog((D0 - 1, D1)), Ld, part.ghost, init(D0 - 1), nl)
    if Ld >= 2 and D1 > 1:
        assert not simulate_validity(prog((D0, D1 - 1)), Ld, part.ghost, init(D0), nl)
    jac_part, (J0, _) = _partition_for(m, n, P, Ld)
    assert part.G >= jac_part.G and D0 >= J0 and (nl < 3 or D0 > J0)
    if nl > 1:
        assert not simulate_validity(prog((D0, D1)), Ld, part.ghost, init(D0), nl + 1)


def test_default_agglomeration_learned_smoother():
    """DDSolver's default Ld for the learned smoother: the first level with <= 2^21 nodes (8193^2: Ld = 3, the
    projection's best at 2, 4 and 8 ranks, profiles/r06_dd_hjac), clamped to what the partition allows."""
    L = global_levels(8192, 8192)
    for P, Pc in ((2, 1), (2, 2), (4, 2)):
        assert default_agglomeration(8192, 8192, P, L, max_nodes=1 << 21, Pc=Pc) == 3
    assert default_agglomeration(1024, 1024, 2, global_levels(1024, 1024), max_nodes=1 << 21) == 1


def test_default_agglomeration():
    L = global_levels(16384, 8192)
    Ld = default_agglomeration(16384, 8192, 8, L)
    assert ((16384 >> Ld) + 1) * ((8192 >> Ld) + 1) <= (1 << 20)
    Partition(16384, 8192, 8, Ld)


@pytest.mark.parametrize("P", [2, 4, 8])
def test_c4_agglomeration_level_is_the_measured_best(P):
    """C4 (8193^2 over the bench's 2x1 / 2x2 / 4x2 blocks): the default agglomeration level is the one the
    per-rank projection chose.  Round 6 (tools/dd_projection.py with the coarse sub-cycle timed as GPU graph replays,
    profiles/r06_dd/dd_projection.txt): Ld = 5 (257^2) at 2 / 4 / 8 ranks, 257.2 / 156.6 / 109.1 us against 279.5 /
    161.1 / 111.5 at Ld = 4 and 278.2 / 168.5 / 118.3 at Ld = 6.  (Rounds 3-5 measured Ld = 4 or 5 depending on the
    rank count with the kernels of their time: profiles/r03_dd .. r05_dd.)"""
    from feanet_amd.dd import default_grid
    Pr, Pc = default_grid(P)
    assert default_agglomeration(8192, 8192, Pr, global_levels(8192, 8192), Pc=Pc) == 5


@pytest.mark.parametrize("m,n,P,Pc,want", [(4096, 4096, 2, 1, 4), (4096, 4096, 4, 2, 4), (4096, 4096, 8, 2, 4),
                                            (16384, 16384, 8, 2, 6), (2048, 2048, 2, 1, 3), (8192, 4096, 4, 1, 4)])
def test_default_agglomeration_other_sizes(m, n, P, Pc, want):
    """The agglomeration rule off the one grid it was measured on (8193^2): the first level whose global grid has
    <= 2^18 nodes, capped by what the partition can still split.  These pins fix the rule's behaviour at other
    sizes; they are not measured optima (no communication is modelled)."""
    Pr = P // Pc
    Ld = default_agglomeration(m, n, Pr, global_levels(m, n), Pc=Pc)
    assert Ld == want
    cap = 1 << 18
    Partition(m, n, Pr, Ld)
    assert ((m >> Ld) + 1) * ((n >> Ld) + 1) <= cap or m // (Pr << (Ld + 1)) < 4 or m % (Pr << (Ld + 1))


@pytest.mark.parametrize("msg,want", [
    ("operation not permitted when stream is capturing", True),
    ("HIP error: hipErrorStreamCaptureUnsupported (hipError_t 900)", True),
    ("CUDA error: operation failed due to a previous error during capture: hipErrorStreamCaptureInvalidated", True),
    ("NCCL error: stream is capturing", True),
    ("Trying to backward through the graph a second time", False),
    ("graph replay failed: an illegal memory access was encountered", False),
    ("feanet_amd: fea_dd_copy_blocks failed (invalid arguments) while capturing", False),
    ("NCCL communicator was aborted on rank 3", False),
])
def test_capture_error_classifier(msg, want):
    """Only stream-capture refusals switch the decomposed solver to the segment-wise path; any other error —
    including ones whose text mentions a graph — must propagate (dd._is_capture_error)."""
    from feanet_amd.dd import _is_capture_error
    assert _is_capture_error(RuntimeError(msg)) is want


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, m, n, Ld, port, outdir, grid, problem, hw):
    import dd_oracle
    dd_oracle.run_rank(rank, world, m, n, Ld, port, outdir, grid=grid, kind=problem, hw=hw)


def _hnet():
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multigrid-feanet_amd", "feanet_amd",
                             "weights", "hnet_iso_poisson_33x33.npz"))
    return np.stack([w[f"conv{i}"].reshape(3, 3) for i in range(3)])


@pytest.mark.parametrize("m,n,P,Ld,grid,problem,hjac", [(64, 32, 2, 2, None, "poisson", False),
                                                        (96, 32, 3, 2, None, "poisson", False),
                                                        (128, 64, 2, 3, None, "poisson", False),
                                                        (64, 64, 4, 2, (2, 2), "poisson", False),
                                                        (64, 128, 2, 2, (1, 2), "poisson", False),
                                                        (128, 96, 6, 2, (2, 3), "poisson", False),
                                                        (64, 64, 4, 2, (2, 2), "interface", False),
                                                        (128, 64, 2, 2, None, "poisson", True),
                                                        (64, 64, 4, 2, (2, 2), "interface", True)])
def test_dd_vcycle_gloo_vs_single_grid(tmp_path, m, n, P, Ld, grid, problem, hjac):
    """Row slabs and 2-D blocks (the oracle rank model exchanges x then y: corners via the diagonal neighbours) over gloo,
    world sizes 2..6, against the oracle's single-grid V-cycle on the global grid; also the two-material problem
    (windows of the global pattern maps) and the learned HRelax smoother (DDSolver's exchange depths for it)."""
    import dd_oracle
    hw = _hnet() if hjac else None
    mp.spawn(_worker, args=(P, m, n, Ld, _free_port(), str(tmp_path), grid, problem, hw), nprocs=P, join=True)
    got = np.full((2, m + 1, n + 1), np.nan)
    for r in range(P):
        s, e, sc, ec = map(int, open(os.path.join(tmp_path, f"rank{r}.idx")).read().split())
        got[:, s:e, sc:ec] = np.load(os.path.join(tmp_path, f"rank{r}.npy"))
    f, u = dd_oracle.problem(m, n, 2)
    L = global_levels(m, n)
    mg = orc.OracleMultigrid(n, problem, np.float64, levels=L, rows=None if problem == "interface" else m)
    if hjac:  # MultiGrid(mode='hjac').Step: every sweep an HRelax
        for lv in mg.levels:
            lv.sweep = (lambda ll, o: (lambda v, ff: (lambda j: j + orc.hnet(j - v, ll.geo, hw))(o(v, ff))))(lv, lv.sweep)
    geo, _ = orc.square_geometry((m + 1, n + 1), np.float64)
    mg.set_boundary(geo, u * (1 - geo))
    v = u
    for _ in range(2):
        v = mg.step(v, f)
    inner = got[:, 1:-1, 1:-1]
    assert not np.isnan(inner).any(), "owned blocks do not tile the interior"
    err = np.abs(inner - v[:, 1:-1, 1:-1]).max() / np.abs(v).max()
    assert err < 1e-13, err


def test_partition_2d():
    """2-D blocks: both axes tile the interior exactly once, the column axis pairs fine and coarse
    columns like the rows, default grids split rows at least as finely as columns."""
    from feanet_amd.dd import Partition2D, default_grid
    assert default_grid(8) == (4, 2) and default_grid(4) == (2, 2) and default_grid(2) == (2, 1)
    part = Partition2D(8192, 8192, 4, 2, 4, 3)
    for l in range(5):
        W = (8192 >> l) + 1
        cols = []
        for r in range(8):
            q = part.clevel(l, r)
            if r // 2 == 0:
                cols += list(range(q.s, q.e))
            assert 0 <= q.gr0 and q.gr0 + q.Hloc <= W
            if l < 4:  # intergrid levels need odd extents (the agglomerated level Ld does not)
                assert q.Hloc % 2 == 1
                q1 = part.clevel(l + 1, r)
                assert q.gr0 == 2 * q1.gr0 and q.Hloc == 2 * q1.Hloc - 1
        assert cols == list(range(1, W - 1))


def test_rect_records_decompose_the_dd_copies():
    """dd._rect_records (the fea_dd_copy_rects table behind the agglomeration's copies): the placement view pair
    ([B, Pr, c, Pc, cc] strided views) becomes B * Pr * Pc rectangles of c x cc with the right addresses and pitches;
    a row-slab run ([B, run]) one rectangle of B rows; views without a common unit-stride dimension are refused.
    Checked by replaying the records with numpy on host tensors."""
    import torch
    from feanet_amd.dd import _rect_records
    B, Pr, Pc, c, cc, ld = 2, 3, 4, 5, 6, 40
    field = torch.zeros(B, Pr * c + 3, ld, dtype=torch.float64)
    stage = torch.arange(Pr * Pc * B * c * cc, dtype=torch.float64).reshape(Pr * Pc, B, c, cc)
    dst = field[:, 1:1 + Pr * c, 2:2 + Pc * cc].reshape(B, Pr, c, Pc, cc)
    src = stage.view(Pr, Pc, B, c, cc).permute(2, 0, 3, 1, 4)
    recs = _rect_records(dst, src)
    assert recs.shape == (B * Pr * Pc, 6) and (recs[:, 4:] == [c, cc]).all()
    flat_d, flat_s = field.view(-1).numpy(), stage.view(-1).numpy()
    base_d, base_s, esz = field.data_ptr(), stage.data_ptr(), 8
    for d0, s0, dld, sld, rows, cols in recs:
        for r in range(rows):
            o_d, o_s = (d0 - base_d) // esz + r * dld, (s0 - base_s) // esz + r * sld
            flat_d[o_d:o_d + cols] = flat_s[o_s:o_s + cols]
    assert torch.equal(dst, src)
    run = torch.zeros(B, 50, dtype=torch.float32)
    r2 = _rect_records(run[:, :20], run[:, 30:])
    assert r2.shape == (1, 6) and list(r2[0, 2:]) == [50, 50, B, 20]
    assert _rect_records(field[:, 1:4, 0:1].transpose(1, 2), field[:, 1:4, 2:3].transpose(1, 2)) is None



def _framed(B, H, W, dtype):
    """A framed buffer (as MultigridSolver's levels hold them) on the host whose every element is its own flat index,
    and its layout (footprint.Geo)."""
    import torch
    import footprint as fp
    geo = fp.Geo(H, W, B, torch.empty(0, dtype=dtype).element_size())
    assert geo.numel < 1 << 24  # (exact in fp32 too)
    return torch.arange(geo.numel, dtype=dtype), geo


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_block_and_rows_views_name_the_frame_nodes(dtype):
    """dd._block / dd._rows (every halo region, gather source and scatter view of the decomposed solver): element
    [b, y, x] of the view is node (y0 + y, x0 + x) of sample b as the framed layout places it — column 0 of a row
    128 bytes minus one element into it, whatever the element size (tests/footprint.py's Geo.index, which the
    kernels' write-footprint tests are built on)."""
    import torch
    from feanet_amd.dd import _block, _rows
    dtype = getattr(torch, dtype)
    B, H, W = 2, 11, 21
    t, geo = _framed(B, H, W, dtype)
    for y0, y1, x0, x1 in [(0, H, 0, W), (3, 7, 2, 5), (1, 2, W - 1, W), (H - 3, H, 0, 3)]:
        v = _block(t, B, geo.bs, geo.ld, y0, y1, x0, x1)
        want = torch.from_numpy(geo.index(np.arange(y0, y1), np.arange(x0, x1)))
        assert v.shape == want.shape and torch.equal(v.to(torch.int64), want), (y0, y1, x0, x1)
    for y0, y1 in [(0, H), (3, 5), (H - 1, H)]:
        v = _rows(t, B, geo.bs, geo.ld, y0, y1)
        assert v.shape == (B, (y1 - y0) * geo.ld) and v.is_contiguous() == (B == 1)
        nodes = v.reshape(B, y1 - y0, geo.ld)[:, :, geo.off:geo.off + W]  # whole framed rows: the nodes sit at off
        want = torch.from_numpy(geo.index(np.arange(y0, y1), np.arange(W)))
        assert torch.equal(nodes.to(torch.int64), want), (y0, y1)
        assert int(v[0, 0]) == int(want[0, 0, 0]) - geo.off  # and the run starts where the frame row does


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_staging_records(dtype):
    """dd._Staging's block table (fea_dd_copy_blocks reads it) over [B, rows, cols] block views and [B, run] row
    runs of two samples: one record per view and sample, in order; the frame address is the view's sample b, the
    stage address the running element offset into the buffer, ld the view's row pitch (a run: one row of its own
    length), the last word rows | cols << 32; the records tile the buffer without gaps.  Replayed with numpy, the
    table packs the views in order and unpacks them again."""
    import torch
    from feanet_amd.dd import _block, _rows, _Staging
    dtype = getattr(torch, dtype)
    B, H, W = 2, 11, 21
    t, geo = _framed(B, H, W, dtype)
    views = [_block(t, B, geo.bs, geo.ld, 1, 4, 2, 7), _rows(t, B, geo.bs, geo.ld, 4, 6),
             _block(t, B, geo.bs, geo.ld, 3, 10, W - 3, W), _block(t, B, geo.bs, geo.ld, 5, 6, 5, 6),
             _rows(t, B, geo.bs, geo.ld, H - 1, H)]
    st = _Staging(views, t.device, dtype)
    esz = t.element_size()
    assert st.esz == esz and st.buf.dtype == dtype and st.records.dtype == np.int64
    assert st.records.shape == (len(views) * B, 4)
    off, k = 0, 0
    for v in views:
        rows, cols = (1, v.shape[1]) if v.dim() == 2 else v.shape[1:]
        for b in range(B):
            base, stage, ld, word = (int(x) for x in st.records[k])
            assert base == (v[b, 0] if v.dim() == 2 else v[b, 0, 0]).data_ptr(), k
            assert stage == st.buf[off:].data_ptr(), k
            assert ld == (cols if v.dim() == 2 else v.stride(1)), k
            assert word == rows | (cols << 32) and (word & 0xFFFFFFFF, word >> 32) == (rows, cols), k
            off += rows * cols
            k += 1
    assert off == st.n == sum(v.numel() for v in views) == st.buf.numel()  # no gap, nothing past the end
    # the table replayed: pack, then unpack into a cleared frame
    flat, stage = t.numpy(), st.buf.numpy()
    stage[:] = -1

    def replay(to_stage):
        for base, sa, ld, word in st.records:
            rows, cols = int(word) & 0xFFFFFFFF, int(word) >> 32
            for r in range(rows):
                f0, s0 = (int(base) - t.data_ptr()) // esz + r * int(ld), (int(sa) - st.buf.data_ptr()) // esz + r * cols
                if to_stage:
                    stage[s0:s0 + cols] = flat[f0:f0 + cols]
                else:
                    flat[f0:f0 + cols] = stage[s0:s0 + cols]
    replay(True)
    assert torch.equal(st.buf, torch.cat([v[b].reshape(-1) for v in views for b in range(B)]))
    kept = [v.clone() for v in views]
    t.zero_()
    replay(False)
    assert all(torch.equal(v, w) for v, w in zip(views, kept))
    covered = torch.zeros_like(t, dtype=torch.bool)
    for v in views:
        torch.as_strided(covered, v.shape, v.stride(), v.storage_offset()).fill_(True)
    assert not t[~covered].any()  # and nothing outside the views was written


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_halo_staging_segments(dtype):
    """dd.halo_staging: the send views of all regions grouped per neighbour (peers ascending, a peer's views in item
    order) in one staging buffer, the receive views likewise in another; each neighbour's message is one segment
    (peer, element offset, element count), and the segments tile their buffer without gaps."""
    import torch
    from feanet_amd.dd import _block, halo_staging
    dtype = getattr(torch, dtype)
    B, H, W = 2, 11, 21
    t, geo = _framed(B, H, W, dtype)
    blk = lambda *a: _block(t, B, geo.bs, geo.ld, *a)
    # (peer, direction, send view, receive view): two items' regions towards peers 3, 1 and 2, interleaved
    regs = [(3, (1, 0), blk(7, 9, 1, 20), blk(9, 11, 1, 20)), (1, (0, -1), blk(1, 9, 1, 4), blk(1, 9, 0, 1)),
            (2, (1, -1), blk(7, 9, 1, 3), blk(9, 10, 0, 1)), (3, (1, 0), blk(6, 9, 2, 19), blk(9, 10, 2, 19)),
            (1, (0, -1), blk(2, 8, 1, 2), blk(2, 8, 0, 1))]
    send, recv, seg_s, seg_r = halo_staging(regs)
    assert [q for q, _, _ in seg_s] == [q for q, _, _ in seg_r] == [1, 2, 3]
    for stg, segs, which in ((send, seg_s, 2), (recv, seg_r, 3)):
        order = [r[which] for q in (1, 2, 3) for r in regs if r[0] == q]
        assert [int(a) for a in stg.records[:, 0]] == [v[b, 0, 0].data_ptr() for v in order for b in range(B)]
        at = 0
        for q, o, cnt in segs:
            assert o == at and cnt == sum(r[which].numel() for r in regs if r[0] == q)
            at += cnt
        assert at == stg.n == stg.buf.numel()
        assert stg.buf.dtype == dtype
