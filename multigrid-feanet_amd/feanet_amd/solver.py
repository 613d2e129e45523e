"""MultigridSolver: the MI355X V-cycle over solver-owned framed level buffers.

`MultigridSolver` is the facade named by BASELINE.json's north star; it executes the reference's
V-cycle (FEANet/multigrid.py MultiGrid.iterate :159-185 == M-FEANet-mg_test.ipynb MultiGrid.Step
:27346-27372 == MM_Model_convergence.ipynb rec_V_cycle :132-148 for nu1 = nu2 = 1) with the fused
HIP level kernels of framed_ops.hip:

  down, level 0 :  nu1 sweeps               (fea_mg_sweep)
                   residual + restriction    (fea_mg_residual_restrict)
  down, level l :  zero-guess sweep + residual + restriction in one pass
                   (fea_mg_residual_restrict with u = NULL)
  coarsest      :  nu1 + nu2 sweeps from zero (no exact solve, as the reference)
  up, level l   :  prolongation + correction + post-sweep in one pass (fea_mg_prolong_sweep)

The launch sequence of one V-cycle is built once (a list of C-ABI calls with fixed device
pointers) and replayed as a HIP graph.  Everything stays on the device; the only host syncs
are the ones a caller asks for (e.g. `.item()` on the residual norm, as the reference drivers do).
"""
import itertools
import math
import time
import weakref

import numpy as np
import torch

from . import _lib, mesh_setup as ms, ops
from .graphs import GraphCache
from .schedule import (OMDF, _other, extend_tail, group_hmid, group_mid, group_triples, hjac_schedule, pair_prolongations, pair_restrictions,
                       shift_schedule, vcycle_schedule)


_SOLVERS = weakref.WeakValueDictionary()  # handle -> live MultigridSolver (torch.ops.feanet.mg_step)
_HANDLES = itertools.count(1)


def first_sweep_raw(launches, f0, raw):
    """`launches` with the cycle's first finest-level HRelax launch (the first whose f is level 0's, `f0`, and that
    has a u_raw parameter) reading the un-reset iterate `raw`: the first cycle after load() (M-FEANet-mg_test.ipynb
    :151-153).  None if there is no such launch."""
    for i, rec in enumerate(launches):
        try:
            _lib.arg(rec, "u_raw")
        except TypeError:  # not an HRelax launch (or a device copy of the decomposed solver's lists)
            continue
        if _lib.arg(rec, "f") == f0:
            return launches[:i] + [_lib.replace(rec, u_raw=raw)] + launches[i + 1:]
    return None


def solver_by_handle(h):
    s = _SOLVERS.get(int(h))
    if s is None:
        raise RuntimeError(f"feanet: no live MultigridSolver with handle {h}")
    return s


class _Level:
    """Framed buffers of one level: H x W nodes (H = rows, W = columns)."""

    def __init__(self, m, n, B, dtype, device, pid_np=None, pid_shape=None, pid_phase=None):
        self.m, self.n = m, n
        self.H, self.W = m + 1, n + 1
        self.N = self.W
        self.esz = 4 if dtype == torch.float32 else 8
        self.off = 128 // self.esz - 1  # column of node 0 in a framed row: column 1 starts a 128-byte line
        self.ld, self.bs = _lib.mg_layout(self.H, self.W, self.esz)
        self.B = B
        self.dtype = dtype
        self.device = device
        numel = B * self.bs + 256
        self.f = torch.zeros(numel, dtype=dtype, device=device)
        self.a = torch.zeros(numel, dtype=dtype, device=device)
        self.b = torch.zeros(numel, dtype=dtype, device=device)
        self.zero = None
        self.c = None  # third iterate buffer of the finest level (solve(): the block's start state)
        self.pid = None
        if pid_np is not None:
            p = np.zeros((self.H + 2, self.ld), np.uint8)
            p[1:self.H + 1, self.off:self.off + self.W] = pid_np
            self.pid = torch.from_numpy(p.reshape(-1)).to(device)
            self.pid = torch.cat([self.pid, torch.zeros(256, dtype=torch.uint8, device=device)])
        elif pid_shape is not None:  # (shape, size): built on the device straight into the frame
            self.pid = torch.zeros((self.H + 2) * self.ld + 256, dtype=torch.uint8, device=device)
            ms.interface_pattern_map_device(self.N, pid_shape[0], pid_shape[1], device=device,
                                            out=self.pid.data_ptr() + self.ld + self.off, ld=self.ld)
        elif pid_phase is not None:  # this level's [m, n] uint8 device phase image: likewise, boundary nodes included
            self.pid = torch.zeros((self.H + 2) * self.ld + 256, dtype=torch.uint8, device=device)
            ms.phase_pattern_map_device(pid_phase, out=self.pid.data_ptr() + self.ld + self.off, ld=self.ld)

    def buf(self, name):
        if name in ("zero", "c") and getattr(self, name) is None:
            setattr(self, name, torch.zeros_like(self.a))
        return getattr(self, name)

    def view(self, t):
        """[B, H, W] view of the interior+boundary nodes of a framed buffer (plumbing / tests)."""
        off = 128 // t.element_size() - 1
        return t[:self.B * self.bs].view(self.B, self.H + 2, self.ld)[:, 1:self.H + 1, off:off + self.W]

    def pid_view(self):
        """[H, W] view of the framed pattern map (one byte per node, the fields' row pitch and column offset)."""
        return self.pid[:(self.H + 2) * self.ld].view(self.H + 2, self.ld)[1:self.H + 1, self.off:self.off + self.W]

    def geom(self):
        return (self.B, self.H, self.W, self.ld, self.bs)

    def geom_kw(self):
        """geom() by parameter name, for _lib.launch."""
        return dict(B=self.B, H=self.H, W=self.W, ld=self.ld, bstride=self.bs)


class MultigridSolver:
    """Geometric-multigrid V-cycle for FEANet's structured-quad FE problems on one MI355X.

    Args:
        n: fine-grid intervals per edge (N = n + 1 nodes).  A power of two >= 2 when `rows` is omitted (the
            reference's square); with `rows` given, any n and rows divisible by 2^(L-1) that leave at least 2
            intervals each way on the coarsest level, e.g. MultigridSolver(96, rows=96): 97, 49, 25, 13, 7, 4 nodes.
        rows: intervals in the row direction: a rectangle (Poisson, or the two-material problem with explicit
            pid_maps), or rows = n for a square whose n is not a power of two (default n).
        levels: number of levels L (default int(log2 n), the reference's choice; coarsest n/2^(L-1);
            for a rectangle, the most levels whose coarsest grid has >= 2 intervals each way).
        problem: "poisson" (MeshSquare, one stencil) or "interface" (MeshCenterInterface, 16
            stencils; `prop` coefficients, `shape` 0 circle / 1 rectangle inclusion).
        dtype: torch.float32 or torch.float64.  batch: number of right-hand sides B.
        R, P: restriction / prolongation kernels, [C, 3, 3] with C = 1 or 16 (per-pattern, the
            learned 16-channel operators of FEANet/multigrid.py); default the bilinear kernel
            [[1,2,1],[2,4,2],[1,2,1]]/4 for both (mg_test; == MM's 4 x full-weighting/16).
        w: ratios (w_R, w_P) multiplying restriction/prolongation (FEANet/multigrid.py:170,178).
        nu1, nu2: pre/post sweeps per level; the coarsest level gets nu1 + nu2 sweeps.
        compat: None, or "mm_interface_q2" to reproduce MM_Interface_error.ipynb:141 (pre-smoothing
            applied to the finest grid at every depth).
        graph: replay the V-cycle as a HIP graph (default True).
        coarse_tail: run every level with N <= 65 (below the finest) as one LDS-resident launch
            (fea_mg_coarse_tail); False keeps one launch per level op.
        fuse: run the last pre-sweep of a level fused with its residual + restriction
            (fea_mg_sweep_restrict, one read of u and f); False issues them separately.
        zero_start: every V-cycle starts the finest level from a zero guess too (the replicated coarse
            sub-solve of the domain-decomposed path, feanet_amd.dd).
        smoother: "jac" (weighted Jacobi) or "hjac" (the learned smoother of M-FEANet-mg_test.ipynb,
            HJacIterator.HRelax: Jacobi + HNet correction; `hnet` = its [nl, 3, 3] conv weights, e.g.
            feanet_amd/weights/hnet_iso_poisson_33x33.npz).  "hjac" runs fea_mg_hsweep for every
            relaxation (MultiGrid(mode='hjac').Step semantics); with coarse_tail its levels of <= 65^2 nodes
            that fit in LDS run as one fea_mg_hjac_tail launch.
        join_cycles: vcycle(k) with k >= 2 runs the finest level's post-smooth of each cycle and the
            pre-smooth + residual + restriction of the next as one pass (fea_mg_cycle_join; bitwise
            the same result, 28 instead of 52 B per node between two cycles).  V(1,1) Jacobi only.
        mid: run latency-bound coarse levels (B*H*W <= MID_NODES) up to four per launch
            (fea_mg_mid_down / fea_mg_mid_up, bitwise the per-level kernels); with smoother="hjac", two per
            launch (fea_mg_hmid_down / fea_mg_hmid_up, bitwise the fused per-level HJac kernels).
        pair_levels: two consecutive zero-guess restrictions, and two recomputed-iterate prolongations, left
            to single-level launches run as one each (fea_mg_zero_restrict2 / fea_mg_prolong2, bitwise the two).
        pid_maps: two-material problem only — explicit per-level pattern maps ([H_l, W_l] uint8, one per level)
            instead of the MeshCenterInterface maps of the square: a domain-decomposed rank's window of the
            global level maps (feanet_amd.dd.DDSolver(problem="interface")); allows a rectangular window.
        phase: two-material problem only — the geometry as an element phase image instead of `shape`: [rows, n], one
            value per element, 0 (coefficient prop[0]) or 1 (prop[1]); numpy array or tensor, host or device, bool or
            any integer dtype.  A device image stays on the device: pattern maps and coarse images are built there
            (fea_phase_pattern_map / fea_phase_coarsen).  Every node, boundary nodes included, takes the pattern of
            the elements it touches (mesh_setup.phase_pattern_map), so phase 1 may touch the boundary.  Rectangles
            and sizes that are not powers of two as `rows` / `n` allow; rows and n divisible by 2^(L-1).
        coarsen: how level l+1's image follows from level l's, as a count of phase-1 children per coarse element
            (mesh_setup.phase_min_count).  "majority": ties to the stiffer phase — the reference's rates on smooth
            inclusions, but the stationary cycle can diverge on element-scale noise.  "stiff": stiff if any child
            is — never diverged at contrast 20 in the study of DESIGN, slower on smooth inclusions.  Neither is
            mesh-independent at high contrast (prop=(1, 1000)): solve there with PCGSolver.
        phase_levels: explicit list of L per-level images instead of coarsening (phase_levels[0] must equal `phase`
            if both are given).
        Not supported with a phase image: more than two phases (16 table rows hold exactly 2^4 patterns), one image
        per sample of a batch (the kernels broadcast one map), DDSolver, and the FEANet/ drop-in classes.
    """

    MID_NODES = 20000     # levels with <= this many nodes (B*H*W) may go to the LDS-tile multi-level launches (groups
    #                       of >= 2 consecutive levels above the coarse tail).  Round 6: 20000 (<= 129^2, which forms no
    #                       group above the 65^2 tail, so the standard plans run the streaming two-level kernels on
    #                       every level above it) — metric V-cycle 132.6 -> 128.8 us, C2 35.9 -> 33.6, C4 grid 528 ->
    #                       519, C3 92.0 -> 90.0, C5 level, DD 8-rank projection 108.9 -> 104.6 against 300000 (<= 513^2,
    #                       rounds 2-5), once this round's task heights had sped the two-level kernels up
    #                       (profiles/r06_ab/mid_nodes.txt).  Larger values still select the multi-level launches (bitwise).
    MID_NODES_DOWN = None  # per-direction overrides of MID_NODES (None: MID_NODES)
    MID_NODES_UP = None
    MID_MIN_TILES = 200   # workgroups a multi-level launch should give the 256 CUs
    MID_MAX_REDUNDANCY = 3.0  # staged top-level region / owned nodes (down pass)
    HMID_NODES = 300000   # learned-smoother levels paired into the HJac two-level launches: <= 513^2 nodes
    HMID_MIN_TILES = 64   # workgroups an HJac two-level launch should give the CUs (one per CU: LDS)
    THREE_LEVEL_UP = True     # the three launch-bound levels right above the coarse tail run as one launch going up /
    THREE_LEVEL_DOWN = False  # going down (the register-strip form of fea_mg_mid_up / fea_mg_mid_down, k = 3), bitwise
    #                           the launches they replace (_three_level_ok: which plans; needs mid and pair_levels).  One switch per direction: up wins, down loses — a
    #                           minimum-height task of the down kernel streams 29 rows of its top level in one wave.
    #                           Same-process vcycle(1000), us per cycle, off / down / up / both: metric 129.7 / 130.9 /
    #                           127.9 / 128.6, C2 33.5 / 34.3 / 31.4 / 31.5 (profiles/r07_ab/three_level.txt)
    STRIP2_COLUMNS = {8: 116, 4: 244}  # Ovl2<T>::S and FEA_BAL2_WAVES of csrc/framed_ops.hip (_three_level_ok)
    BAL2_WAVES = 1024
    TAIL_MAX_N = 65       # the coarse tail (one LDS-resident launch) covers the levels of at most this many rows / columns
    TAIL_EXT = True       # the single-level restriction / prolongation right above the coarse tail run inside the
    TAIL_EXT_MIN_BATCH = 64  # tail's launch (fea_mg_coarse_tail_ext: single pattern, V(1,1)) for batches of at least
    #                       this many samples: one workgroup per sample moves the level's traffic through one CU, which
    #                       only pays when the samples fill the chip (C5, 256 x 1025^2 fp32: 1142 -> 1125 us; at B = 1
    #                       the metric cycle 130.1 -> 134.1 us, C2 33.8 -> 37.6; profiles/r06_ab/tail_ext.txt)

    def __init__(self, n, levels=None, problem="poisson", dtype=torch.float64, device=None, batch=1,
                 omega=2.0 / 3.0, size=2.0, prop=(1, 20), shape=0, R=None, P=None, w=(1.0, 1.0),
                 nu1=1, nu2=1, compat=None, graph=True, coarse_tail=True, fuse=True, rows=None, zero_start=False,
                 smoother="jac", hnet=None, join_cycles=True, mid=True, pair_levels=True, pid_maps=None,
                 phase=None, coarsen="majority", phase_levels=None):
        m = n if rows is None else int(rows)
        if rows is None and (n < 2 or (n & (n - 1)) != 0):
            raise ValueError(f"MultigridSolver: n={n} must be a power of two >= 2")
        if m < 2 or n < 2:
            raise ValueError(f"MultigridSolver: need >= 2 intervals each way (got {m} x {n})")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("MultigridSolver: dtype must be torch.float32 or torch.float64")
        if coarsen not in ms.PHASE_RULES:
            raise ValueError(f"MultigridSolver: unknown coarsen rule {coarsen!r}")
        imaged = phase is not None or phase_levels is not None
        if imaged:  # refused before the device is touched; values of a device image after
            if problem != "interface":
                raise ValueError("MultigridSolver: phase / phase_levels are for problem='interface'")
            if pid_maps is not None:
                raise ValueError("MultigridSolver: give phase or pid_maps, not both")
            if shape != 0:
                raise ValueError("MultigridSolver: give phase or shape, not both (a phase image is the geometry)")
            as_array = lambda p: p if torch.is_tensor(p) else np.asarray(p)
            phase = None if phase is None else as_array(phase)
            phase_levels = None if phase_levels is None else [as_array(p) for p in phase_levels]
            if phase_levels is not None and not phase_levels:
                raise ValueError("MultigridSolver: phase_levels is empty")
            for name, img in [("phase", phase)] + [(f"phase_levels[{l}]", p) for l, p in enumerate(phase_levels or [])]:
                if img is None:
                    continue
                if len(img.shape) != 2:
                    raise ValueError(f"MultigridSolver: {name} must be [rows, n] (one value per element), got shape "
                                     f"{tuple(img.shape)}")
                if not (torch.is_tensor(img) and img.is_cuda):
                    ms._phase_image(img.numpy() if torch.is_tensor(img) else img)
            fine = phase if phase is not None else phase_levels[0]
            if tuple(fine.shape) != (m, n):
                raise ValueError(f"MultigridSolver: the phase image is {tuple(fine.shape)}, the grid has {m} x {n} "
                                 "elements (rows x n)")
        self.device = torch.device(device if device is not None else "cuda")
        ops.require_hip(torch.empty(0, device=self.device), "solver device")
        self.n, self.m = n, m
        if levels is None:
            L = 1
            while (n % (1 << L) == 0 and m % (1 << L) == 0 and (n >> L) >= 2 and (m >> L) >= 2):
                L += 1
            self.L = L if rows is not None else int(math.log2(n))
        else:
            self.L = int(levels)
        s_ = 1 << (self.L - 1)
        if self.L < 1 or n % s_ or m % s_ or n // s_ < 2 or m // s_ < 2:
            raise ValueError(f"MultigridSolver: {self.L} levels do not fit a {m} x {n} grid")
        self.dtype = dtype
        self.B = int(batch)
        self.omega = omega
        self.size = size
        self.problem = problem
        self.prop, self.shape = (prop[0], prop[1]), shape
        self._flux_image = None  # flux(): the fine element phase image on the device (built on first use)
        self._explicit_maps = pid_maps is not None
        self.nu1, self.nu2 = int(nu1), int(nu2)
        self.compat = compat
        self.use_graph = graph
        self.fuse = fuse
        self.zero_start = zero_start
        self.join_cycles = join_cycles
        self.mid = bool(mid)
        self.pair_levels = bool(pair_levels)
        if smoother not in ("jac", "hjac"):
            raise ValueError(f"MultigridSolver: unknown smoother {smoother!r}")
        self.smoother = smoother
        if smoother == "hjac":
            if hnet is None:
                raise ValueError("MultigridSolver: smoother='hjac' needs the HNet weights (hnet=[nl, 3, 3])")
            if compat is not None:
                raise ValueError("MultigridSolver: smoother='hjac' follows MultiGrid(mode='hjac').Step only")
            hw = np.asarray(torch.as_tensor(hnet).detach().cpu().float().numpy(), np.float32).reshape(-1, 3, 3)
            if not 1 <= hw.shape[0] <= 3:
                raise ValueError("MultigridSolver: HNet with 1..3 conv layers supported")
        hjac_tail = coarse_tail and smoother == "hjac"
        if smoother == "hjac":
            coarse_tail = False
        npdt = np.float32 if dtype == torch.float32 else np.float64
        multi = problem == "interface"
        if problem not in ("poisson", "interface"):
            raise ValueError(f"MultigridSolver: unknown problem {problem!r}")
        if multi and m != n and pid_maps is None and not imaged:
            raise ValueError("MultigridSolver: the two-material problem is defined on the square only")
        if pid_maps is not None:  # explicit per-level maps (a domain-decomposed rank's window of the global maps)
            if not multi:
                raise ValueError("MultigridSolver: pid_maps is for the two-material problem")
            pid_maps = [np.ascontiguousarray(p, np.uint8) for p in pid_maps]
        ktab = ms.stencil_table(prop if multi else None)
        self.ntab = ktab.shape[0]
        lin = ms.linear_transfer_kernel() / np.float32(4.0)
        R = lin[None] if R is None else np.asarray(torch.as_tensor(R).detach().cpu().float().numpy(), np.float32)
        P = lin[None] if P is None else np.asarray(torch.as_tensor(P).detach().cpu().float().numpy(), np.float32)
        R = R.reshape(-1, 3, 3)
        P = P.reshape(-1, 3, 3)
        if multi:  # per-pattern tables cover every pattern id
            R = np.broadcast_to(R, (self.ntab, 3, 3)) if R.shape[0] == 1 else R
            P = np.broadcast_to(P, (self.ntab, 3, 3)) if P.shape[0] == 1 else P
        elif R.shape[0] != 1 or P.shape[0] != 1:
            raise ValueError("MultigridSolver: the Poisson problem has one pattern; R/P must be [1, 3, 3]")
        w = [float(x) for x in (w.detach().cpu().tolist() if torch.is_tensor(w) else w)]
        self.w = (w[0], w[1])
        dev = self.device
        self.ktab_np = ktab
        self.hw = None
        self.nl = 0
        if smoother == "hjac":
            self.hw = torch.from_numpy(hw.reshape(-1).astype(npdt)).to(dev)
            self.nl = hw.shape[0]
        self.ktab = torch.from_numpy(ktab.reshape(-1, 9).astype(npdt)).to(dev)
        self.omd = torch.from_numpy(ms.omega_over_d(ktab, omega, npdt)).to(dev)
        self.rtab = torch.from_numpy(np.ascontiguousarray(R).reshape(-1, 9).astype(npdt)).to(dev)
        self.ptab = torch.from_numpy(np.ascontiguousarray(P).reshape(-1, 9).astype(npdt)).to(dev)
        self.levels = []
        self.phase_images = self._phase_images(phase, phase_levels, prop, coarsen) if imaged else None
        for l in range(self.L):
            nl, ml = n >> l, m >> l
            if imaged:  # pattern maps straight from the level's image into the frame, on the device
                self.levels.append(_Level(ml, nl, self.B, dtype, dev, pid_phase=self.phase_images[l]))
                continue
            if pid_maps is not None:
                if pid_maps[l].shape != (ml + 1, nl + 1):
                    raise ValueError(f"MultigridSolver: pid_maps[{l}] is {pid_maps[l].shape}, level {l} is "
                                     f"{(ml + 1, nl + 1)}")
                self.levels.append(_Level(ml, nl, self.B, dtype, dev, pid_np=pid_maps[l]))
                continue
            # two-material pattern maps: built on the device (setup_ops.hip), bit-identical to the host
            self.levels.append(_Level(ml, nl, self.B, dtype, dev, pid_shape=(shape, size) if multi else None))
        if imaged:
            self.fine_pid = self.levels[0].pid_view().contiguous()
        elif pid_maps is not None:
            self.fine_pid = torch.from_numpy(pid_maps[0]).to(dev)
        else:
            self.fine_pid = ms.interface_pattern_map_device(n + 1, shape, size, device=dev) if multi else None
        if multi:  # the framed kernels read each node's stiffness row from its own pattern (K symmetric; checked)
            for Lv in self.levels:
                if ms.stencil_mirror_mismatches(ktab, Lv.pid_view()):
                    raise ValueError("MultigridSolver: the stiffness table is not symmetric on this pattern map "
                                     "(the framed two-material kernels need K_ij == K_ji bit for bit)")
        self.tail_from = None
        esz = self.levels[0].esz
        if coarse_tail:
            for l in range(1, self.L):
                Lv = self.levels[l]
                if (Lv.H <= self.TAIL_MAX_N and Lv.W <= self.TAIL_MAX_N
                        and 0 < _lib.coarse_tail_lds_bytes(Lv.H, Lv.W, self.L - l, esz, multi) <= _lib.TAIL_LDS_LIMIT):
                    self.tail_from = l
                    break
        # learned smoother: the levels of <= 65^2 nodes whose f, u and two scratch fields fit in LDS
        self.hjac_tail_from = None
        if hjac_tail:
            for l in range(1, self.L):
                Lv = self.levels[l]
                if (Lv.H <= 65 and Lv.W <= 65
                        and 0 < _lib.hjac_tail_lds_bytes(Lv.H, Lv.W, self.L - l, esz, multi) <= _lib.TAIL_LDS_LIMIT):
                    self.hjac_tail_from = l
                    break
        t_from = self.tail_from if self.tail_from is not None else self.hjac_tail_from
        if t_from is not None and imaged:
            self.tail_pid = torch.cat([self.levels[l].pid_view().reshape(-1) for l in range(t_from, self.L)])
        elif t_from is not None and multi:
            maps = [pid_maps[l].reshape(-1) if pid_maps is not None else
                    ms.interface_pattern_map(self.levels[l].N, shape, size).reshape(-1) for l in range(t_from, self.L)]
            self.tail_pid = torch.from_numpy(np.concatenate(maps)).to(dev)
        else:
            self.tail_pid = None
        self.ws = torch.zeros(max(1, _lib.norm_workspace_bytes(self.B, m + 1, n + 1) // 8), dtype=torch.float64,
                              device=dev)
        self.norm_out = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self._bc = None  # Dirichlet data of set_boundary ([B, 1, H, W]; None: zero)
        self._raw = None  # smoother="hjac": the un-reset iterate load() got, read by the next cycle's first sweep
        self._hjac_first = False
        self._state = "a"
        # joinable solvers rest BETWEEN cycles in a pipelined ("mid-cycle") state after vcycle(k): see
        # _vcycles_pipelined; None = the iterate is materialised in buffer self._state
        self._mid = None
        self._hist = None  # solve(): fused residual-norm history + counters (_ensure_hist)
        self._cnt = None
        self._hist_gen = 0
        self._hist_host = None  # pinned host copy of the history (_read_hist)
        self._trace = False  # solve(): synchronise and time every phase into _solve_log (diagnostics)
        self._solve_log = []
        self._f1_snap = None
        self._sws = None  # solve(): per-cycle partial norm sets of a graph block
        self._bc_version = object()  # identity changes with every set_boundary (third-buffer packing)
        self._c_bc = None
        # Dirichlet data the finest iterate buffers a/b carry: set_boundary takes effect at the next load(),
        # and the third buffer c (a materialised end iterate) is packed with the same data as a/b
        self._ab_bc, self._ab_version = None, self._bc_version
        self._plans = {}
        self._graphs = GraphCache(self.device)
        self.mass = ms.mass_stencil(size / n)
        self.handle = next(_HANDLES)  # torch.ops.feanet.mg_step(u, f, handle, cycles)
        _SOLVERS[self.handle] = self

    def _phase_images(self, phase, phase_levels, prop, coarsen):
        """The L per-level phase images as contiguous uint8 device tensors: `phase_levels`, or `phase` coarsened on
        the device by the rule's child count.  Host images are copied once; a device image never leaves it.  (The
        constructor has checked that rows and n are divisible by 2^(L-1) and that the finest image is [rows, n].)"""
        m, n, L, dev = self.m, self.n, self.L, self.device
        fine = None if phase is None else ms._phase_tensor(phase, dev)
        if phase_levels is None:
            return ms.phase_hierarchy_device(fine, L, prop, coarsen)
        if len(phase_levels) != L:
            raise ValueError(f"MultigridSolver: {len(phase_levels)} phase_levels for {L} levels")
        imgs = [ms._phase_tensor(p, dev) for p in phase_levels]
        for l, p in enumerate(imgs):
            if tuple(p.shape) != (m >> l, n >> l):
                raise ValueError(f"MultigridSolver: phase_levels[{l}] is {tuple(p.shape)}, level {l} has "
                                 f"{(m >> l, n >> l)} elements")
        if fine is not None and not torch.equal(fine, imgs[0]):
            raise ValueError("MultigridSolver: phase_levels[0] differs from phase")
        return imgs

    # ------------------------------------------------------------------ problem data
    @property
    def N(self):
        return self.n + 1

    @property
    def H(self):
        return self.m + 1

    @property
    def W(self):
        return self.n + 1

    def _check_field(self, x, name):
        ops.require_hip(x, name)
        x = x.to(self.dtype)
        H, W = self.H, self.W
        if x.numel() == H * W:
            x = x.reshape(1, 1, H, W).expand(self.B, 1, H, W)
        if tuple(x.shape[-2:]) != (H, W) or x.numel() != self.B * H * W:
            raise ValueError(f"MultigridSolver: {name} must be [{self.B}, 1, {H}, {W}]")
        return x.reshape(self.B, 1, H, W).contiguous()

    def set_rhs(self, f=None, F=None):
        """Set the assembled right-hand side f (= FNet(F), the `forcing_term` of the reference) or
        the nodal source F (FNet applied on the device, FEANet/model.py:49-61)."""
        if (f is None) == (F is None):
            raise ValueError("MultigridSolver.set_rhs: give exactly one of f (assembled) or F (source)")
        if F is not None:
            F = self._check_field(F, "F")
            f = ops.conv3x3(F, torch.from_numpy(self.mass))
        f = self._check_field(f, "f")
        L0 = self.levels[0]
        self._collapse()  # a pipelined next pre-smooth was made with the old right-hand side
        self._pack(f, L0.f, geo=None, bc=None, reset=False)

    def set_boundary(self, bc_value=None, geometry_idx=None):
        """Dirichlet data of the fine level (the `boundary_value` / `geometry_idx` of JacobiBlock).
        The framed kernels implement the square geometry (geo.py:13-30); other geometries go through
        FEANet.jacobi.JacobiBlock's generic operator."""
        if geometry_idx is not None:
            g = self._check_field(geometry_idx, "geometry_idx")
            sq = torch.ones_like(g)
            sq[..., 0, :] = 0
            sq[..., -1, :] = 0
            sq[..., :, 0] = 0
            sq[..., :, -1] = 0
            if not torch.equal(g, sq):
                raise NotImplementedError("MultigridSolver: only the square geometry (geo.py:13-30) is fused")
        self._bc = None if bc_value is None else self._check_field(bc_value, "boundary_value")
        self._bc_version = object()

    def _pack(self, x, dst, geo=None, bc=None, reset=True):
        """x (None: zeros) -> framed dst; reset: x*geo + bc (square geometry), else a raw copy."""
        Lv = self.levels[0]
        bp, bs = (None, 0)
        if bc is not None:
            bp, bs = bc.data_ptr(), self.H * self.W
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.call("mg_pack", self.dtype, None if x is None else x.data_ptr(), dst.data_ptr(), None,
                  0 if reset else -1, bp, bs, *Lv.geom(), stream)

    def load(self, u0=None):
        """Set the fine-grid iterate (reset_boundary applied: u*geo + bc, jacobi.py:27-29)."""
        L0 = self.levels[0]
        bc = self._bc
        if u0 is not None:
            u0 = self._check_field(u0, "u0")
        self._pack(u0, L0.a, bc=bc)
        self._pack(u0, L0.b, bc=bc)  # both ping-pong buffers carry the boundary values
        self._mid = None
        self._ab_bc, self._ab_version = bc, self._bc_version
        if L0.c is not None and self._c_bc is not self._ab_version:
            self._pack(u0, L0.c, bc=bc)  # c only needs the Dirichlet values on its boundary nodes
            self._c_bc = self._ab_version
        self._state = "a"
        if self.smoother == "hjac":
            # HRelax forms J(u) - u with the iterate the driver passed, before reset_boundary
            # (M-FEANet-mg_test.ipynb:151-153; the drivers pass un-reset zeros, :27478-27489): the
            # first sweep of the next V-cycle sees bc - u0 on the boundary nodes
            self._raw = torch.zeros_like(L0.a)
            self._pack(u0, self._raw, reset=False)  # u0 None: zeros
            self._hjac_first = True

    def solution(self):
        """Current fine iterate as a contiguous [B, 1, H, W] tensor."""
        L0 = self.levels[0]
        out = torch.empty((self.B, 1, self.H, self.W), dtype=self.dtype, device=self.device)
        _lib.call("mg_unpack", self.dtype, L0.buf(self._iterate()).data_ptr(), out.data_ptr(), *L0.geom(),
                  ops._stream(out))
        return out

    def flux_image(self):
        """(phase image, k0, k1) of flux(): the device-resident fine image of a phase= solver, element_phase(N, shape,
        size) copied once for a shape= solver, no image and k = 1 for the Poisson problem."""
        from . import flux as fx
        if self.problem != "interface":
            return None, 1.0, 1.0
        if self._flux_image is None:
            if self.phase_images is not None:
                self._flux_image = self.phase_images[0]
            elif self._explicit_maps or self.m != self.n:
                raise ValueError("MultigridSolver.flux: a solver built from pid_maps has no element phase image")
            else:
                self._flux_image = fx.phase_operand(ms.element_phase(self.N, self.shape, self.size), self.m, self.n,
                                                    self.device)
        return (self._flux_image,) + fx.coefficients(self.prop)

    def flux(self, fields=True):
        """Element fluxes q = -k grad u, their means, the mean gradient and the energy u^T K u of the current iterate
        (the buffer solution() reads), as a feanet_amd.flux.FluxResult of device tensors; no host synchronisation."""
        from . import flux as fx
        L0 = self.levels[0]
        img, k0, k1 = self.flux_image()
        return fx.flux_framed(L0.buf(self._iterate()).data_ptr(), self.dtype, self.device, *L0.geom(), phase=img,
                              k0=k0, k1=k1, h=self.size / self.n, fields=fields)

    def energy_forms(self, pair=(0, 1), fields=True):
        """The energy forms between samples pair[0] and pair[1] of the current iterate (the buffer solution() reads),
        split by the phases of flux_image(), as a feanet_amd.flux.EnergyForms with B = 1: A [1, 2, 3], density
        [1, 3, m, n] or None; no host synchronisation.  The default pair needs batch >= 2; pair=(i, i) is one sample
        with itself."""
        from . import flux as fx
        L0 = self.levels[0]
        img = self.flux_image()[0]
        return fx.pair_forms(L0.buf(self._iterate()).data_ptr(), self.dtype, self.device, self.B, L0.geom(), pair, img,
                             fields, "MultigridSolver.energy_forms")

    def residual_norm(self):
        """Per-sample ||(f - K u)[1:-1, 1:-1]||_2 of the current iterate (float64 device tensor [B])."""
        L0 = self.levels[0]
        _lib.call("mg_residual_norm", self.dtype, L0.buf(self._iterate()).data_ptr(), L0.f.data_ptr(),
                  None if L0.pid is None else L0.pid.data_ptr(), self.ktab.data_ptr(), self.ntab,
                  self.norm_out.data_ptr(), self.ws.data_ptr(), *L0.geom(), 0, 0, 0, 0,
                  torch.cuda.current_stream(self.device).cuda_stream)
        return self.norm_out.clone()

    def set_transfer(self, R=None, P=None, w=None):
        """Replace the restriction / prolongation kernels (and the ratios w) of a built solver, for training
        loops that update them between V-cycles (FEANet/multigrid.py:132-157 under an optimizer).

        R / P ([npat or 1, 3, 3], any device) are rounded to float32 like the constructor's and copied into the
        resident tables IN PLACE on the current stream: the launch plans and captured HIP graphs hold the tables'
        addresses, so they stay valid and nothing is reallocated or recaptured.  The ratios are passed by value
        into the launches, so new ratios (w != the current ones) drop the plans and graphs instead; the level
        buffers are kept either way.

        A solver resting in the pipelined state (after vcycle) has not stored its last cycle's end iterate: it
        is recomputed from the pre-smoothed iterate and the level-1 correction with the CURRENT P (_collapse).
        So that state is collapsed first, with the old tables, before any of them changes."""
        if R is not None or P is not None or w is not None:
            self._collapse()
        for src, dst, name in ((R, self.rtab, "R"), (P, self.ptab, "P")):
            if src is None:
                continue
            t = torch.as_tensor(src).detach().to(device=self.device, dtype=torch.float32).reshape(-1, 9)
            if t.shape[0] not in (1, dst.shape[0]):
                raise ValueError(f"MultigridSolver.set_transfer: {name} has {t.shape[0]} patterns, the solver "
                                 f"{dst.shape[0]}")
            dst.copy_(t.to(self.dtype).expand(dst.shape[0], 9))
        if w is not None:
            w = [float(x) for x in (w.detach().cpu().tolist() if torch.is_tensor(w) else w)]
            if (w[0], w[1]) != self.w:
                self.w = (w[0], w[1])
                self._plans.clear()
                self._graphs.clear()

    # ------------------------------------------------------------------ schedule
    def _ptr(self, lvl, name):
        if name == OMDF:  # recomputed in the kernel (u = NULL)
            return None
        return self.levels[lvl].buf(name).data_ptr()

    def _build(self, start):
        """Bind the symbolic schedule (feanet_amd.schedule) to C-ABI calls with device pointers:
        list of (name, args-without-stream) for one V-cycle from buffer `start`, and the end buffer."""
        if self.smoother == "hjac":
            steps, end = hjac_schedule(self.L, self.nu1, self.nu2, "zero" if self.zero_start else start,
                                       tail_from=self.hjac_tail_from, fuse=self.fuse)
            if self.mid and self.fuse:
                steps = group_hmid(steps, self._pick_hmid())
        else:
            steps, end = vcycle_schedule(self.L, self.nu1, self.nu2, self.compat, start, self.tail_from, self.fuse,
                                         top_zero=self.zero_start)
            if self.mid:
                steps = group_mid(steps, lambda lv: self._pick_mid(lv, False), lambda lv: self._pick_mid(lv, True))
            if self.pair_levels:
                if self.mid:
                    steps = group_triples(steps, lambda l: self.THREE_LEVEL_DOWN and self._three_level_ok(l),
                                          lambda l: self.THREE_LEVEL_UP and self._three_level_ok(l))
                ok = lambda l: l + 2 < self.L and self.levels[l + 2].H >= 3 and self.levels[l + 2].W >= 3
                steps = pair_prolongations(pair_restrictions(steps, ok), ok)
            if self._tail_ext_ok():
                steps = extend_tail(steps)
        return [self.bind_step(st) for st in steps], end

    def _three_level_ok(self, l):
        """Levels l, l+1, l+2 may run as one register-strip launch each way (fea_mg_mid_down / fea_mg_mid_up with
        TR = TC = -1): the single-pattern Jacobi V(1,1) cycle from a stored finest iterate, level l+3 the coarse tail's
        first, all three levels launch-bound and the tail not extended over level l+2.  Launch-bound: even at the
        minimum task height (one row of level l+2 per wave task) the top level's two-level restriction has fewer waves
        than the floor the two-level kernels keep — Ovl2::S owned columns per strip and FEA_BAL2_WAVES of
        csrc/framed_ops.hip; at batch 1 levels of at most 513^2."""
        top = self.levels[l]
        strips = -(-(top.W - 2) // self.STRIP2_COLUMNS[top.esz])
        launch_bound = self.B * strips * max(((top.H + 1) // 2 + 1) // 2 - 2, 1) < self.BAL2_WAVES
        return (self.smoother == "jac" and self.ntab == 1 and self.nu1 == 1 and self.nu2 == 1 and self.compat is None
                and not self.zero_start and self.tail_from is not None and l >= 1 and l + 3 == self.tail_from
                and not self._tail_ext_ok() and launch_bound)

    def _tail_ext_ok(self):
        """fea_mg_coarse_tail_ext's scope: the single-pattern V(1,1) tail, the level above it at most 129 wide."""
        t = self.tail_from
        return (self.TAIL_EXT and t is not None and self.B >= self.TAIL_EXT_MIN_BATCH and self.ntab == 1
                and self.nu1 == 1 and self.nu2 == 1 and self.compat is None and self.levels[t - 1].W <= 129 and self.levels[t - 1].H <= 129)

    def _mid_tile(self, up, a, k):
        """Tile size for a multi-level launch over levels a..a+k-1 (down: tile of level a+k; up: of
        level a), or None: the largest power of two whose LDS footprint fits, that gives the chip
        >= MID_MIN_TILES workgroups (or the most it can) and, going down, stages <= MID_MAX_REDUNDANCY
        times the top level's nodes."""
        esz = self.levels[0].esz
        multi = self.ntab > 1
        tl = self.levels[a if up else a + k]
        top = self.levels[a]
        best = None
        for T in ((128, 64, 32, 16, 8) if up else (32, 16, 8, 4, 2)):
            if _lib.mid_lds_bytes(up, k, T, T, esz, multi) <= 0:
                continue
            tiles = self.B * -(-(tl.H - 2) // T) * -(-(tl.W - 2) // T)
            if not up:
                reg = (T << k) + 3 * ((1 << k) - 1)
                if reg * reg * tiles > self.MID_MAX_REDUNDANCY * self.B * top.H * top.W:
                    continue
            best = T
            if tiles >= self.MID_MIN_TILES:
                return T
        return best

    def _hmid_tile(self, up, a):
        """Tile size of an HJac two-level launch over levels a, a+1 (down: tile of level a+2; up: of level a):
        the largest whose LDS footprint fits and that gives >= HMID_MIN_TILES workgroups, else the smallest that
        fits (None: none does)."""
        esz = self.levels[0].esz
        tl = self.levels[a if up else a + 2]
        fit = [T for T in ((64, 32, 16, 8) if up else (16, 8, 4, 2))
               if _lib.hmid_lds_bytes(up, T, self.nl, esz, self.ntab > 1) > 0]
        for T in fit:
            if self.B * -(-(tl.H - 2) // T) * -(-(tl.W - 2) // T) >= self.HMID_MIN_TILES:
                return T
        return fit[-1] if fit else None

    def _pick_hmid(self):
        """(a, T_down, T_up) for the HJac levels paired into two-level launches: streamed coarse levels (a >= 1,
        above the HJac tail) of <= HMID_NODES nodes, paired from the coarse end upward."""
        top = self.hjac_tail_from if self.hjac_tail_from is not None else self.L - 1
        el = [l for l in range(1, top) if self.B * self.levels[l].H * self.levels[l].W <= self.HMID_NODES]
        pairs = []
        hi = len(el)
        while hi >= 2:
            a = el[hi - 2]
            if el[hi - 1] == a + 1 and a + 2 < self.L:
                td, tu = self._hmid_tile(False, a), self._hmid_tile(True, a)
                if td and tu:
                    pairs.append((a, td, tu))
                    hi -= 2
                    continue
            hi -= 1
        return pairs

    def _pick_mid(self, levels, up):
        """Groups (a, k, T) of consecutive latency-bound levels, formed from the coarse end upward."""
        cap = self.MID_NODES_UP if up else self.MID_NODES_DOWN
        cap = self.MID_NODES if cap is None else cap
        el = sorted(l for l in levels
                    if self.B * self.levels[l].H * self.levels[l].W <= cap and l + 1 < self.L)
        groups = []
        hi = len(el)
        while hi >= 2:
            for k in range(min(4, hi), 1, -1):
                a = el[hi - k]
                if el[hi - 1] - a != k - 1:
                    continue
                T = self._mid_tile(up, a, k)
                if T:
                    groups.append((a, k, T))
                    hi -= k
                    break
            else:
                hi -= 1
        return groups

    # the recurring parameter groups of the level entry points, by name (include/feanet_hip.h)
    def _pid(self, l):
        Lv = self.levels[l]
        return None if Lv.pid is None else Lv.pid.data_ptr()

    def _stencil(self, pid):
        return dict(pid=pid, ktab=self.ktab.data_ptr(), omd=self.omd.data_ptr(), ntab=self.ntab)

    def _restriction(self):
        return dict(rtab=self.rtab.data_ptr(), nrtab=self.rtab.shape[0], w0=self.w[0])

    def _prolongation(self):
        return dict(ptab=self.ptab.data_ptr(), nptab=self.ptab.shape[0], w1=self.w[1])

    def _hnet(self):
        return dict(hw=self.hw.data_ptr(), nlayers=self.nl)

    def _coarse_pitch(self, l):
        """Row pitch and sample stride of level l + 1 (and of level l + 2: _coarse_pitch2)."""
        return dict(ldc=self.levels[l + 1].ld, bstridec=self.levels[l + 1].bs)

    def _coarse_pitch2(self, l):
        return dict(ldc2=self.levels[l + 2].ld, bstridec2=self.levels[l + 2].bs)

    def bind_step(self, st):
        """One schedule step -> (C-ABI function base name, args without the stream)."""
        lv = self.levels
        launch, pid, sten = _lib.launch, self._pid, self._stencil
        rest, prol, cp, cp2 = self._restriction, self._prolongation, self._coarse_pitch, self._coarse_pitch2

        def ptr(l, name):
            return None if name is None else self._ptr(l, name)

        def geom(l):
            return lv[l].geom_kw()

        def pids(a, n):
            return _lib.PtrArray([pid(j) for j in range(a, a + n)]) if self.ntab > 1 else None

        def fs(a, n):
            return _lib.PtrArray([lv[j].f.data_ptr() for j in range(a, a + n)])

        def tail(t):  # the LDS-resident tails take every level's pattern map and the tables without their row counts
            return dict(Ht=lv[t].H, Wt=lv[t].W, nlev=self.L - t, ld_t=lv[t].ld, bs_t=lv[t].bs,
                        pid_levels=None if self.tail_pid is None else self.tail_pid.data_ptr(),
                        ktab=self.ktab.data_ptr(), omd=self.omd.data_ptr(), ntab=self.ntab, rtab=self.rtab.data_ptr(),
                        ptab=self.ptab.data_ptr(), w0=self.w[0], w1=self.w[1], nu1=self.nu1, nu2=self.nu2, B=lv[t].B)

        kind, l = st[0], st[1]
        f = lv[l].f.data_ptr()
        if kind == "sweep":
            return launch("mg_sweep", u=ptr(l, st[2]), f=f, out=ptr(l, st[3]), **sten(pid(l)), **geom(l))
        if kind == "hsweep":
            return launch("mg_hsweep", u=ptr(l, st[2]), u_raw=None, f=f, out=ptr(l, st[3]), **sten(pid(l)),
                          **self._hnet(), **geom(l))
        if kind == "resid_restrict":
            return launch("mg_residual_restrict", u=ptr(l, st[2]), f=f, v_out=ptr(l, st[3]), fc=lv[l + 1].f.data_ptr(),
                          **sten(pid(l)), **rest(), **geom(l), **cp(l))
        if kind == "resid_restrict2":
            return launch("mg_zero_restrict2", f=f, fc=lv[l + 1].f.data_ptr(), fc2=lv[l + 2].f.data_ptr(),
                          pidc=pid(l + 1), **sten(pid(l)), **rest(), **geom(l), **cp(l), **cp2(l))
        if kind == "resid_restrict3":  # the register-strip form: TR = -1 (unit-height tasks), TC = -1
            return launch("mg_mid_down", f=fs(l, 4), k=3, B=self.B, H=lv[l].H, W=lv[l].W, **sten(pids(l, 4)),
                          **rest(), TR=-1, TC=-1)
        if kind == "prolong_sweep3":
            return launch("mg_mid_up", f=fs(l, 3), e=ptr(l + 3, st[2]), out=ptr(l, st[3]), k=3, B=self.B, H=lv[l].H,
                          W=lv[l].W, **sten(pids(l, 4)), **prol(), TR=-1, TC=-1)
        if kind == "sweep_restrict":
            return launch("mg_sweep_restrict", u=ptr(l, st[2]), f=f, u_out=ptr(l, st[3]), fc=lv[l + 1].f.data_ptr(),
                          **sten(pid(l)), **rest(), **geom(l), **cp(l), norm_ws=None, norm_hist=None, norm_cnt=None)
        if kind == "prolong_sweep":
            return launch("mg_prolong_sweep", u=ptr(l, st[2]), ec=ptr(l + 1, st[3]), f=f, out=ptr(l, st[4]),
                          pidc=pid(l + 1), **sten(pid(l)), **prol(), **geom(l), **cp(l))
        if kind == "prolong_sweep2":
            return launch("mg_prolong2", fc=lv[l + 1].f.data_ptr(), ec2=ptr(l + 2, st[2]), f=f, out=ptr(l, st[3]),
                          pidc=pid(l + 1), pidc2=pid(l + 2), **sten(pid(l)), **prol(), **geom(l), **cp(l), **cp2(l))
        if kind == "prolong_add":
            return launch("mg_prolong_add", u=ptr(l, st[2]), ec=ptr(l + 1, st[3]), out=ptr(l, st[4]), pidc=pid(l + 1),
                          **prol(), **geom(l), **cp(l))
        if kind == "mid_down":
            a, k, T = st[1], st[2], st[3]
            TR, TC = T if isinstance(T, tuple) else (T, T)
            return launch("mg_mid_down", f=fs(a, k + 1), k=k, B=self.B, H=lv[a].H, W=lv[a].W,
                          **sten(pids(a, k + 1)), **rest(), TR=TR, TC=TC)
        if kind == "mid_up":
            a, k, csrc, dst, T = st[1:6]
            TR, TC = T if isinstance(T, tuple) else (T, T)
            return launch("mg_mid_up", f=fs(a, k), e=ptr(a + k, csrc), out=ptr(a, dst), k=k, B=self.B, H=lv[a].H,
                          W=lv[a].W, **sten(pids(a, k + 1)), **prol(), TR=TR, TC=TC)
        if kind == "coarse_tail":
            return launch("mg_coarse_tail", f_t=f, v_t=ptr(l, st[2]), q2=int(self.compat == "mm_interface_q2"),
                          **tail(l))
        if kind == "coarse_tail_ext":
            x, t = l, l + 1
            return launch("mg_coarse_tail_ext", f_x=f, v_x=ptr(x, st[2]), Hx=lv[x].H, Wx=lv[x].W, ld_x=lv[x].ld,
                          bs_x=lv[x].bs, nlev=self.L - t, ktab=self.ktab.data_ptr(), omd=self.omd.data_ptr(),
                          ntab=self.ntab, rtab=self.rtab.data_ptr(), ptab=self.ptab.data_ptr(), w0=self.w[0],
                          w1=self.w[1], B=lv[x].B)
        if kind == "hsweep_restrict":
            return launch("mg_hsweep_restrict", u=ptr(l, st[2]), u_raw=None, f=f, out=ptr(l, st[3]),
                          fc=lv[l + 1].f.data_ptr(), **sten(pid(l)), **self._hnet(), **rest(), **geom(l), **cp(l))
        if kind == "prolong_hsweep":
            return launch("mg_prolong_hsweep", u=ptr(l, st[2]), u_raw=None, ec=ptr(l + 1, st[3]), f=f,
                          out=ptr(l, st[4]), pidc=pid(l + 1), **sten(pid(l)), **self._hnet(), **prol(), **geom(l),
                          **cp(l))
        if kind == "hmid_down":
            a, da, da1, T = st[1:5]
            us = _lib.PtrArray([ptr(a, da), ptr(a + 1, da1)])
            return launch("mg_hmid_down", f=fs(a, 3), u=us, B=self.B, H=lv[a].H, W=lv[a].W, **sten(pids(a, 3)),
                          **self._hnet(), **rest(), T=T)
        if kind == "hmid_up":
            a, u0, u1, esrc, dst, T = st[1:7]
            us = _lib.PtrArray([ptr(a, u0), ptr(a + 1, u1)])
            return launch("mg_hmid_up", f=fs(a, 2), u=us, e=ptr(a + 2, esrc), out=ptr(a, dst), B=self.B, H=lv[a].H,
                          W=lv[a].W, **sten(pids(a, 3)), **self._hnet(), **prol(), T=T)
        if kind == "hjac_tail":
            return launch("mg_hjac_tail", f_t=f, u_t=ptr(l, st[2]), **self._hnet(), **tail(l))
        raise ValueError(f"MultigridSolver: unknown schedule step {kind!r}")

    def _plan(self, start):
        if start not in self._plans:
            self._plans[start] = self._build(start)
        return self._plans[start]

    def _launch(self, plan):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for name, args in plan:
            if name == "norm_append":  # dtype-free entry point
                _lib.call_raw(name, *args, stream)
            else:
                _lib.call(name, self.dtype, *args, stream)

    def _joinable(self):
        return (self.join_cycles and self.smoother == "jac" and self.nu1 == 1 and self.nu2 == 1 and
                self.compat is None and not self.zero_start and self.fuse and self.L >= 2)

    def _join_call(self, pre, ec_ptr, norm=False, out=None, norm_ws=None):
        """fea_mg_cycle_join: PS(0) of the cycle whose pre-smoothed iterate is in `pre`, fused with the
        next cycle's SR(0); the new pre-smoothed iterate lands in the other buffer.  norm: also append the
        residual norm of the cycle's end iterate to the solve history (solve())."""
        L0, L1 = self.levels[0], self.levels[1]
        out = out or _other(pre)
        if norm_ws is not None:
            norms = dict(norm_ws=norm_ws, norm_hist=None, norm_cnt=None)
        elif norm:
            norms = dict(norm_ws=self.ws.data_ptr(), norm_hist=self._hist.data_ptr(), norm_cnt=self._cnt.data_ptr())
        else:
            norms = dict(norm_ws=None, norm_hist=None, norm_cnt=None)
        return _lib.launch("mg_cycle_join", u=self._ptr(0, pre), ec=ec_ptr, f=L0.f.data_ptr(), u_out=self._ptr(0, out),
                           fc=L1.f.data_ptr(), pidc=self._pid(1), **self._stencil(self._pid(0)),
                           **self._prolongation(), **self._restriction(), **L0.geom_kw(), **self._coarse_pitch(0),
                           **norms)

    def _run_graph(self, key, issue):
        """issue()'s launches under `key`: eager the first time (lazy buffers and pointer arrays exist afterwards),
        captured as a HIP graph the second, replayed after (GraphCache); always eager without use_graph."""
        self._graphs.run(key, issue, self.use_graph)

    def joined_program(self, k):
        """vcycle(k) with joined cycle boundaries as [(segment key, launches)] plus the end buffer:
        the first cycle's SR(0), k-1 segments (coarse part + cycle join) and the last coarse part +
        PS(0).  (Also used by bench.py to time the join kernel inside the cycle.)"""
        s0 = self._state
        plan, _ = self._plan(s0)
        head, mid = plan[0], plan[1:-1]
        ec_ptr = _lib.arg(plan[-1], "ec")  # level-1 correction the finest prolongation reads (same every cycle)
        prog = [(("head", s0), [head])]
        pre = _other(s0)
        for _ in range(k - 1):
            prog.append((("join", pre), mid + [self._join_call(pre, ec_ptr)]))
            pre = _other(pre)
        tail = self._plan(_other(pre))[0][-1]  # PS(0): pre -> _other(pre)
        prog.append((("tail", pre), mid + [tail]))
        return prog, _other(pre)

    GRAPH_CYCLES = 32  # max joined cycles per HIP graph

    @staticmethod
    def graph_blocks(njoin, G):
        """Block sizes the njoin cycle joins of vcycle(njoin + 1) are replayed in: as many blocks of G
        (a power of two) as fit, then the binary decomposition of the remainder, largest first."""
        blocks = [G] * (njoin // G)
        r = njoin % G
        b = G
        while r:
            b //= 2
            if r >= b:
                blocks.append(b)
                r -= b
        return blocks

    @staticmethod
    def pipe_blocks(njoin, G):
        """Block sizes of vcycle(njoin): as many blocks of G as fit, then the remainder as ONE block (one graph
        per remainder size, at most G of them): a call of k <= G cycles is a single graph launch, so its fixed
        cost (the submission of the first graph, the gap in front of every further graph) is paid once."""
        return [G] * (njoin // G) + ([njoin % G] if njoin % G else [])

    def _ensure_c(self):
        """The finest level's third buffer with the Dirichlet values of the iterate buffers a/b on its boundary
        nodes (its interior is always written before it is read; a set_boundary() not yet followed by a load()
        does not show, as in the unjoined solver)."""
        L0 = self.levels[0]
        if L0.c is None or self._c_bc is not self._ab_version:
            L0.buf("c")
            self._pack(None, L0.c, bc=self._ab_bc)
            self._c_bc = self._ab_version

    def _post_smooth(self, src, dst):
        """Level 0's last post-smooth PS(0) (prolongation + correction + sweep, the plan's last launch) reading the
        pre-smoothed iterate in buffer `src` and writing the cycle's end iterate to `dst`."""
        return _lib.replace(self._plan("a")[0][-1], u=self._ptr(0, src), out=self._ptr(0, dst))

    def _collapse(self):
        """Leave the pipelined state: the last cycle's end iterate recomputed (PS(0) from the join's
        inputs) into the buffer of the now-discarded next pre-smooth, which becomes the resting state."""
        m = self._mid
        if m is None:
            return
        self._launch([self._post_smooth(m["last"], m["pre"])])
        self._state = m["pre"]
        self._mid = None

    def _iterate(self):
        """Name of the finest-level buffer holding the current iterate.  In the pipelined state the
        last cycle's end iterate v is not stored (the cycle join went on to the next pre-smooth): it is
        recomputed once by the last post-smooth PS(0) from the join's inputs, still intact — the
        pre-smoothed iterate `last` and the level-1 correction — into buffer c (bitwise the unjoined
        cycle's result)."""
        m = self._mid
        if m is None:
            return self._state
        if not m["mat"]:
            self._ensure_c()
            self._launch([self._post_smooth(m["last"], "c")])
            m["mat"] = True
        return "c"

    def _vcycles_pipelined(self, k):
        """k V-cycles as k x [levels >= 1 of a cycle + the cycle join] (fea_mg_cycle_join: post-smooth of
        the cycle and pre-smooth + residual + restriction of the next, 28 instead of 52 B per fine node).
        The solver rests between calls in the pipelined state the join leaves — the NEXT cycle's
        pre-smoothed iterate in `pre`, its restricted residual in f_1 — so consecutive calls pay neither a
        separate first pre-smooth nor a last post-smooth: every call, whatever k, runs exactly k cycles'
        work at the steady-state rate.  From a loaded iterate the first call opens the pipeline with that
        pre-smooth (fea_mg_sweep_restrict).  The end iterate is materialised only when asked for
        (_iterate).  Replayed as few HIP graphs: blocks of GRAPH_CYCLES joins plus one block of the rest
        (pipe_blocks), keyed by (pipeline opened?, buffer, size)."""
        plan, _ = self._plan("a")
        mid = plan[1:-1]  # levels >= 1 (they never touch the finest level's iterate buffers)
        ec_ptr = _lib.arg(plan[-1], "ec")  # level-1 correction the finest prolongation reads (same every cycle)
        if self._mid is None:
            s0 = self._state
            head = [self._plan(s0)[0][0]]
            pre = _other(s0)
        else:
            head, pre = [], self._mid["pre"]
        G = max(1, self.GRAPH_CYCLES)
        G = 1 << (G.bit_length() - 1)
        for nb in self.pipe_blocks(k, G):
            def issue(head=head, pre=pre, nb=nb):
                launches = list(head)
                for _ in range(nb):
                    launches += mid + [self._join_call(pre, ec_ptr)]
                    pre = _other(pre)
                self._launch(launches)
            self._run_graph(("pipe", bool(head), pre, nb), issue)
            if nb % 2:
                pre = _other(pre)
            head = []
        self._mid = {"pre": pre, "last": _other(pre), "mat": False}

    def vcycle(self, k=1):
        """Run k V-cycles on the resident iterate (asynchronous; no host sync)."""
        if k < 1:
            return
        if self._joinable() and not self._hjac_first:
            self._vcycles_pipelined(k)
            return
        self._vcycles_plain(k)

    def _vcycles_plain(self, k):
        """k unjoined V-cycles (one replay of the whole-cycle plan each) from the materialised iterate."""
        self._collapse()
        for _ in range(k):
            plan, end = self._plan(self._state)
            if self._hjac_first:  # the first sweep of the first cycle after load() reads the un-reset iterate
                self._hjac_first = False
                first = first_sweep_raw(plan, self.levels[0].f.data_ptr(), self._raw.data_ptr())
                self._launch(plan if first is None else first)
            else:
                self._run_graph(self._state, lambda: self._launch(plan))
            self._state = end

    # ------------------------------------------------------------------ full multigrid (nested iteration)
    FMG_MAX_COARSEST = 10  # interior nodes of the coarsest level fmg() accepts (4 x 7 nodes: the largest measured)

    def fmg_base_cycles(self):
        """Default number of cycles (nu1 + nu2 sweeps each) on the coarsest level of fmg(): 1 when that level has one
        interior node (two sweeps solve it to 1/9), else 8."""
        Lc = self.levels[-1]
        return 1 if (Lc.H - 2) * (Lc.W - 2) == 1 else 8

    def _fmg_check(self, cycles, interp, base_cycles):
        if self.smoother != "jac":
            raise ValueError("MultigridSolver.fmg: smoother='hjac' is not supported (Jacobi V-cycles only)")
        if self.compat is not None:
            raise ValueError(f"MultigridSolver.fmg: compat={self.compat!r} is not supported")
        if self.zero_start:
            raise ValueError("MultigridSolver.fmg: zero_start solvers have no stored iterate to start a cycle from")
        if interp not in ("cubic", "bilinear"):
            raise ValueError(f"MultigridSolver.fmg: interp must be 'cubic' or 'bilinear', not {interp!r}")
        if int(cycles) < 1 or (base_cycles is not None and int(base_cycles) < 1):
            raise ValueError("MultigridSolver.fmg: cycles and base_cycles must be >= 1")
        Lc = self.levels[-1]
        if (Lc.H - 2) * (Lc.W - 2) > self.FMG_MAX_COARSEST:
            raise ValueError(f"MultigridSolver.fmg: the coarsest level ({Lc.H} x {Lc.W} nodes) is not solved by a few "
                             f"sweeps; the hierarchy needs more levels (at most {self.FMG_MAX_COARSEST} interior nodes "
                             "on the coarsest)")

    def _fmg_tail(self, s):
        """First level of the coarse tail in a V-cycle of the sub-hierarchy s .. L-1, or None: the solver's own tail,
        or below it the levels s+1 .. L-1 where they fit in LDS."""
        if self.tail_from is None or s + 1 > self.L - 1:
            return None
        t = max(self.tail_from, s + 1)
        if t > self.tail_from:
            Lv = self.levels[t]
            need = _lib.coarse_tail_lds_bytes(Lv.H, Lv.W, self.L - t, Lv.esz, self.ntab > 1)
            if not 0 < need <= _lib.TAIL_LDS_LIMIT:
                return None
        return t

    def _fmg_subplan(self, s, start):
        """One V-cycle of the sub-hierarchy s .. L-1 from level s's stored iterate in buffer `start`: (launches, end
        buffer).  The schedule of L - s levels shifted by s, with each grouping of _build where its own predicate
        holds (all of them bitwise the launches they replace).  Two kernels that sum a coarse value in different
        orders (last-bit differences) are placed the same way in every solver, so that the pass gives the same bits
        whichever performance switches the solver was built with: level s, the one with the stored iterate, always
        runs its last pre-sweep fused with the residual + restriction (fea_mg_sweep_restrict), whatever `fuse`; the
        levels below it, which pre-sweep more than once only with nu1 >= 2, always sweep and restrict in separate
        launches — the arithmetic of the coarse tail, which is bitwise those and not the fused kernel.  For a fused
        solver with nu1 <= 1 that is the ordinary plan at s = 0."""
        if s == 0 and self.fuse and self.nu1 <= 1:
            return self._plan(start)
        key = ("fmg", s, start)
        if key not in self._plans:
            t = self._fmg_tail(s)
            steps, end = vcycle_schedule(self.L - s, self.nu1, self.nu2, None, start, None if t is None else t - s,
                                         True)
            steps = shift_schedule(steps, s)
            # nu1 >= 2: the levels below s sweep and restrict in separate launches, as the coarse tail computes them
            steps = [x for st in steps for x in
                     ([("sweep", st[1], st[2], st[3]), ("resid_restrict", st[1], st[3], None)]
                      if st[0] == "sweep_restrict" and st[1] > s else [st])]
            if self.mid:
                steps = group_mid(steps, lambda lv: self._pick_mid(lv, False), lambda lv: self._pick_mid(lv, True))
            if self.pair_levels:
                if self.mid and t == self.tail_from:
                    steps = group_triples(steps, lambda l: self.THREE_LEVEL_DOWN and self._three_level_ok(l),
                                          lambda l: self.THREE_LEVEL_UP and self._three_level_ok(l))
                ok = lambda l: l + 2 < self.L and self.levels[l + 2].H >= 3 and self.levels[l + 2].W >= 3
                steps = pair_prolongations(pair_restrictions(steps, ok), ok)
            if t == self.tail_from and self._tail_ext_ok():
                steps = extend_tail(steps)
            plan = [self.bind_step(st) for st in steps]
            if t is not None and t > self.tail_from and self.tail_pid is not None:
                # a tail that starts below tail_from: its levels' maps start further into tail_pid
                off = sum(self.levels[j].H * self.levels[j].W for j in range(self.tail_from, t))
                plan = [_lib.replace(rec, pid_levels=self.tail_pid.data_ptr() + off) if rec[0] == "mg_coarse_tail"
                        else rec for rec in plan]
            self._plans[key] = (plan, end)
        return self._plans[key]

    def _fmg_boundary(self, l, name, bc):
        """fea_fmg_boundary on buffer `name` of level l: the Dirichlet data `bc` of the finest level sampled at this
        level's nodes (bc None: zeros)."""
        Lv = self.levels[l]
        return _lib.launch("fmg_boundary", bc=None if bc is None else bc.data_ptr(),
                           bc_bstride=0 if bc is None else self.H * self.W, stride=1 << l,
                           dst=Lv.buf(name).data_ptr(), **Lv.geom_kw())

    def fmg_program(self, cycles=1, interp="cubic", base_cycles=None):
        """The launches of fmg() in order, as [(phase, level, launches)] with phase "restrict", "base" or "level",
        and the finest-level buffer the result lands in.  (tools/fmg_timing.py times the phases.)"""
        self._fmg_check(cycles, interp, base_cycles)
        cycles = int(cycles)
        base_cycles = self.fmg_base_cycles() if base_cycles is None else int(base_cycles)
        lv, L, bc = self.levels, self.L, self._bc
        order = 3 if interp == "cubic" else 1
        prog = []
        # the right-hand sides f_1 .. f_(L-1) = P^T f_(l-1)
        chain = [_lib.launch("fmg_restrict", f=lv[l].f.data_ptr(), fc=lv[l + 1].f.data_ptr(), **lv[l].geom_kw(),
                             **self._coarse_pitch(l)) for l in range(L - 1)]
        if chain:
            prog.append(("restrict", 0, chain))

        def cycles_from(s, n):  # n V-cycles of the sub-hierarchy s .. L-1 from buffer a; the end buffer
            out, cur = [], "a"
            for _ in range(n):
                plan, cur = self._fmg_subplan(s, cur)
                out += plan
            return out, cur

        # coarsest level: its Dirichlet data, then base_cycles cycles from a zero interior (zeroed by the caller)
        top = L - 1
        launches = [self._fmg_boundary(top, "a", bc), self._fmg_boundary(top, "b", bc)]
        if top == 0 and lv[0].c is not None:
            launches.append(self._fmg_boundary(0, "c", bc))
        body, cur = cycles_from(top, base_cycles)
        prog.append(("base", top, launches + body))
        for s in range(L - 2, -1, -1):
            launches = [self._fmg_boundary(s, "a", bc), self._fmg_boundary(s, "b", bc)]
            if s == 0 and lv[0].c is not None:
                launches.append(self._fmg_boundary(0, "c", bc))
            launches.append(_lib.launch("fmg_prolong", u=None, ec=lv[s + 1].buf(cur).data_ptr(),
                                        out=lv[s].a.data_ptr(), **lv[s].geom_kw(), **self._coarse_pitch(s),
                                        order=order))
            # a level below the finest carries zero boundary values in every cycle that corrects with it
            launches += [self._fmg_boundary(s + 1, "a", None), self._fmg_boundary(s + 1, "b", None)]
            body, cur = cycles_from(s, cycles)
            prog.append(("level", s, launches + body))
        return prog, cur

    def fmg(self, cycles=1, interp="cubic", base_cycles=None):
        """Full-multigrid start (nested iteration; asynchronous, like vcycle): the problem of set_rhs / set_boundary
        solved on the coarsest level (`base_cycles` cycles of nu1 + nu2 sweeps from zero; default
        fmg_base_cycles()), then for every finer level the solution interpolated up as that level's guess
        (interp "cubic" or "bilinear": fea_fmg_prolong) and `cycles` V-cycles of the levels from there down, with
        the solver's own nu1, nu2, R, P and w.  Coarse right-hand sides are f_(l+1) = P^T f_l
        (fea_fmg_restrict), coarse Dirichlet data the fine data injected at the coarse boundary nodes
        (fea_fmg_boundary; taken off again before the level serves as a correction level).  Leaves the finest iterate
        resident as load() does: vcycle, solve's loop, solution and residual_norm continue from it.  The result is
        the same bits whichever of coarse_tail, mid, pair_levels and fuse the solver was built with.  The whole
        program replays as one HIP graph per (cycles, interp, base_cycles).  About 4/3 of `cycles` fine V-cycles of
        work; one pass with cubic interpolation ends below the discretisation error."""
        prog, end = self.fmg_program(cycles, interp, base_cycles)
        self._mid = None  # whatever iterate was in flight is replaced
        launches = [rec for _, _, recs in prog for rec in recs]
        coarsest = self.levels[-1]
        base_cycles = self.fmg_base_cycles() if base_cycles is None else int(base_cycles)

        def issue():
            coarsest.a.zero_()  # the zero interior the base cycles start from (a few nodes; a memset node)
            self._launch(launches)
        # the launches hold the Dirichlet field's address: graphs of an earlier set_boundary are dropped
        self._graphs.discard(lambda k: isinstance(k, tuple) and k[:1] == ("fmg",) and k[4] is not self._bc_version)
        self._run_graph(("fmg", int(cycles), interp, base_cycles, self._bc_version, self.levels[0].c is not None),
                        issue)
        self._ab_bc, self._ab_version = self._bc, self._bc_version
        if self.levels[0].c is not None:
            self._c_bc = self._ab_version
        self._state = end

    def step(self, u, f, cycles=1):
        """Functional form of MultiGrid.Step / MultiGrid.iterate: `cycles` V-cycles from u with rhs f,
        returns the new fine iterate — through the custom op torch.ops.feanet.mg_step (MultiGrid.iterate's
        fused path takes the same op)."""
        from . import torch_ops  # noqa: F401  (registers torch.ops.feanet.mg_step)
        return torch.ops.feanet.mg_step(u, f, self.handle, int(cycles))

    def _step(self, u, f, cycles=1):
        """Body of feanet::mg_step.  One cycle from a freshly loaded iterate, read at once, runs the unjoined
        plan (SR(0) + coarse levels + PS(0), 52 B per fine node): the pipelined form would add a cycle join's
        next pre-smooth and a recomputed post-smooth that nothing reads.  More cycles run joined."""
        if cycles < 1:
            raise ValueError("MultigridSolver.step: cycles must be >= 1")
        self._mid = None  # whatever a previous call left in flight is replaced by u below
        self.set_rhs(f=f)
        self.load(u)
        if cycles == 1:
            self._vcycles_plain(1)
        else:
            self.vcycle(cycles)
        return self.solution()

    def solve(self, u0=None, f=None, F=None, eps=1e-6, max_cycles=100, bc_value=None, fmg=False):
        """Driver loop of the reference notebooks (M-FEANet-mg_test.ipynb:27426-27436,
        MM_Model_convergence.ipynb:196-203): V-cycles until max_b ||r_b|| <= eps (at most max_cycles;
        stops after a non-finite norm, :27434-27436).  Returns (u [B,1,N,N], residual history: list of
        per-sample numpy arrays, first entry = the initial residual).

        Joinable solvers (V(1,1) Jacobi) run the device-resident loop of _solve_joined: the residual
        norm of every cycle comes out of the cycle join (fused, no extra pass) and the host looks at the
        history once per block of cycles.  The result — iterate and history — is that of the per-cycle
        loop (bitwise the same iterate; norms summed in another fixed order).

        fmg=True (u0 must be None) starts from the full-multigrid pass fmg() instead of load(u0): history[0] is
        the residual after that pass, and the per-cycle loop runs from there."""
        if fmg and u0 is not None:
            raise ValueError("MultigridSolver.solve: fmg=True computes its own start (u0 must be None)")
        if bc_value is not None:
            self.set_boundary(bc_value)
        if f is not None or F is not None:
            self.set_rhs(f=f, F=F)
        if fmg:
            self.fmg()
        else:
            self.load(u0)
        if not fmg and self._joinable() and not self._hjac_first and self.use_graph:
            return self._solve_joined(eps, max_cycles, u0)
        hist = [self.residual_norm().cpu().numpy()]
        while hist[-1].max() > eps and len(hist) <= max_cycles:
            self.vcycle()
            hist.append(self.residual_norm().cpu().numpy())
            if not np.all(np.isfinite(hist[-1])):
                break
        return self.solution(), hist

    SOLVE_BLOCK_MAX = 64  # cycles per host check of the solve loop

    def _ensure_hist(self, rows):
        """Device history of fused residual norms (rows of B) and the join's counters; captured solve
        graphs hold these pointers, so a reallocation retires them (new generation in their keys)."""
        if self._hist is None or self._hist.shape[0] < rows:
            self._hist = torch.zeros((max(1024, rows), self.B), dtype=torch.float64, device=self.device)
            self._cnt = torch.zeros(2, dtype=torch.int32, device=self.device)
            self._hist_gen += 1

    def _read_hist(self, r0, r1):
        """History rows r0..r1-1 to the host: one async copy into pinned memory, then a stream sync."""
        n = (r1 - r0) * self.B
        if self._hist_host is None or self._hist_host.numel() < self._hist.numel():
            self._hist_host = torch.empty(self._hist.numel(), dtype=torch.float64, pin_memory=True)
        out = self._hist_host[:n]
        out.copy_(self._hist[r0:r1].reshape(-1), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return out.numpy().reshape(r1 - r0, self.B).copy()

    def _set_cnt(self, row):
        """Join counters for the next norm-fused launch: arrival count 0, history row `row` (device-side
        fills, no host synchronisation)."""
        self._cnt[0].fill_(0)
        self._cnt[1].fill_(row)

    def _solve_joined(self, eps, max_cycles, u0=None):
        """The solve loop on the device.  State between blocks ("mid-cycle"): the pre-smoothed iterate of
        the next cycle in a finest-level buffer S, its restricted residual in f_1 — what a cycle join
        leaves.  A block runs nb x [levels >= 1 of a cycle + the norm-fused cycle join] (graph blocks of
        graph_blocks(nb)), its joins ping-ponging between the two finest-level buffers other than S (a
        third buffer, so S survives the block untouched); join i appends ||r|| of the iterate at the end
        of cycle i to the device history.  The host reads the block's norms once and
          * stops at the first cycle j with max_b ||r_b|| <= eps (or a non-finite norm), as the reference;
          * if j is the block's last cycle, its end iterate v_j (never stored by the join) is recomputed by
            the last post-smooth PS(0) from the join's inputs, still intact: bitwise the unjoined result;
          * if j is earlier (the contraction beat the prediction), the block is re-run from S to j (f_1 of
            S from a copy taken at the block's start).
        The initial norm comes from the first pre-smooth (fea_mg_sweep_restrict with the fused norm).
        Block sizes: 3 cycles, then the predicted count to eps from the last contraction ratio plus its
        last increase (V-cycle contraction grows towards its asymptotic rate; the extrapolation is bounded
        so the prediction errs short: another block costs one host round trip, an overshoot a re-run)."""
        self._ensure_hist(max_cycles + 2)
        L0, L1 = self.levels[0], self.levels[1]
        self._ensure_c()

        def stop(h):
            return (not np.all(np.isfinite(h))) or h.max() <= eps

        if max_cycles < 1:
            return self.solution(), [self.residual_norm().cpu().numpy()]
        s0 = self._state
        plan, _ = self._plan(s0)
        head, mid = plan[0], plan[1:-1]
        ec_ptr = _lib.arg(plan[-1], "ec")
        gen = self._hist_gen
        assert head[0] == "mg_sweep_restrict", head[0]
        # pre-smooth + initial norm (row 0): opens the first block's graph
        head_launch = _lib.replace(head, norm_ws=self.ws.data_ptr(), norm_hist=self._hist.data_ptr(),
                                   norm_cnt=self._cnt.data_ptr())
        self._set_cnt(0)
        S = _other(s0)
        # deferred norms: each joined cycle of a graph block writes its partial sums to its own set, one
        # reduction launch per graph block appends the block's rows
        per = _lib.join_norm_parts(self.B, L0.H, L0.W, L0.esz)
        stride = per * self.B
        Gmax = self.SOLVE_BLOCK_MAX
        if self._sws is None or self._sws.numel() < Gmax * stride:
            self._sws = torch.zeros(Gmax * stride, dtype=torch.float64, device=self.device)
            self._hist_gen += 1  # captured solve graphs hold the old workspace pointer
            gen = self._hist_gen
        log = self._solve_log = []
        trace = self._trace

        def mark(what):
            if trace:
                torch.cuda.synchronize(self.device)
                log.append((what, time.perf_counter()))
        mark("head")

        def run_joins(S, nb, with_head=False):
            """nb norm-fused cycles from start buffer S (after the first pre-smooth if with_head), one graph
            per block of up to SOLVE_BLOCK_MAX cycles; returns (last read buffer, last written)."""
            X, Y = [x for x in "abc" if x != S]
            p, t, last = S, X, None
            for blk in ([nb] if nb <= Gmax else self.graph_blocks(nb, Gmax)):
                # (first read, first write, second write) fixes the whole buffer sequence of the block
                def issue(with_head=with_head, p=p, t=t, blk=blk):
                    launches = [head_launch] if with_head else []
                    for i in range(blk):  # cycle i of the graph block: partial sums into set i
                        launches += mid + [self._join_call(p, ec_ptr, out=t,
                                                           norm_ws=self._sws.data_ptr() + 8 * i * stride)]
                        p, t = t, (Y if t == X else X)
                    launches.append(_lib.launch("norm_append", ws=self._sws.data_ptr(), stride=stride, per=per,
                                                B=self.B, nrows=blk, hist=self._hist.data_ptr(),
                                                cnt=self._cnt.data_ptr()))
                    self._launch(launches)
                self._run_graph(("sblock", with_head, p, t, Y if t == X else X, blk, gen), issue)
                with_head = False
                for _ in range(blk):
                    last, p, t = p, t, (Y if t == X else X)
            return last, p

        hist = None
        c = 0
        q = None
        while True:
            h = float(hist[-1].max()) if hist is not None else float("inf")
            if eps <= 0.0 or (q is not None and not 0.0 < q < 1.0):
                nb = self.SOLVE_BLOCK_MAX
            elif q is None:
                nb = 3
            else:
                nb = int(math.ceil(math.log(eps / h) / math.log(q))) if h > eps else 1
            nb = max(1, min(nb, self.SOLVE_BLOCK_MAX, max_cycles - c))
            if nb > 1 and hist is not None:  # f_1 of the start state: the joins overwrite it, a re-run
                if self._f1_snap is None:      # needs it back (the first block re-runs from u0 instead)
                    self._f1_snap = torch.empty_like(L1.f)
                self._f1_snap.copy_(L1.f)
            last_read, end = run_joins(S, nb, with_head=hist is None)
            mark("joins")
            log.append(("block", c, nb))
            if hist is None:
                rows = self._read_hist(0, 1 + nb)
                hist = [rows[0]]
                if stop(hist[0]):  # the loaded guess already meets eps: no cycle at all
                    self.load(u0)
                    return self.solution(), hist
                new = rows[1:]
            else:
                new = self._read_hist(c + 1, c + 1 + nb)
            mark("read")
            j = next((i for i in range(nb) if stop(new[i])), None)
            if j is not None and j < nb - 1:  # converged inside the block: re-run S -> cycle c + j + 1
                if c == 0:
                    self.load(u0)
                    self._set_cnt(0)
                else:
                    L1.f.copy_(self._f1_snap)
                    self._set_cnt(c + 1)
                last_read, end = run_joins(S, j + 1, with_head=c == 0)
                log.append(("rerun", c, j + 1))
                mark("rerun")
            keep = nb if j is None else j + 1
            hist += [new[i] for i in range(keep)]
            c += keep
            S = end
            if j is not None or c >= max_cycles:
                break
            rs = [float(hist[i + 1].max() / hist[i].max()) for i in (len(hist) - 3, len(hist) - 2)
                  if i >= 0 and hist[i].max() > 0]
            q = rs[-1] if rs else None
            if len(rs) == 2 and q is not None:
                # V-cycle contraction grows towards its asymptote: extrapolate the last step (bounded), so
                # the prediction is not systematically one cycle short
                q = min(q + max(0.0, rs[1] - rs[0]), 1.15 * q)
        # v of the last cycle: PS(0) from the last join's inputs (its pre-smoothed iterate `last_read`, the
        # level-1 correction untouched since), into a ping-pong buffer of the unjoined plans
        D = _other(last_read)
        self._run_graph(("tail", last_read, D), lambda: self._launch([self._post_smooth(last_read, D)]))
        self._state = D
        mark("tail")
        u = self.solution()
        mark("solution")
        return u, hist

    # ------------------------------------------------------------------ accounting
    def bytes_per_vcycle(self, k=1):
        """Algorithmic HBM bytes per V-cycle as executed (DESIGN.md §3 accounting).  Joinable solvers run
        every cycle as [levels >= 1 + one fea_mg_cycle_join] (pipelined, _vcycles_pipelined)."""
        esz = self.levels[0].esz
        plan = self._plan("a")[0]
        if not self._joinable():
            return self._plan_bytes(plan)
        L0, L1 = self.levels[0], self.levels[1]
        nodes = L0.B * (L0.H - 2) * (L0.W - 2)
        coarse = L1.B * (L1.H - 2) * (L1.W - 2)
        pb = 1 if self.problem == "interface" else 0
        join = nodes * (3 * esz + pb) + coarse * (2 * esz + pb)
        return self._plan_bytes(plan[1:-1]) + join

    def _plan_bytes(self, plan):
        esz = self.levels[0].esz
        pb = 1 if self.problem == "interface" else 0
        total = 0
        for rec in plan:
            name = rec[0]
            if name in ("mg_coarse_tail", "mg_hjac_tail"):
                continue
            if name == "mg_coarse_tail_ext":  # read f_X twice (down, up), write v_X (the tail itself: LDS)
                H, W, B = (_lib.arg(rec, p) for p in ("Hx", "Wx", "B"))
                total += 3 * esz * B * (H - 2) * (W - 2)
                continue
            B, H, W = (_lib.arg(rec, p) for p in ("B", "H", "W"))
            if name == "mg_hsweep":  # read u (NULL: zero guess) and f (+ pattern), write out
                total += B * (H - 2) * (W - 2) * (esz * (3 if _lib.arg(rec, "u") is not None else 2) + pb)
                continue
            if name in ("mg_hsweep_restrict", "mg_prolong_hsweep"):
                nodes = B * (H - 2) * (W - 2)
                coarse = B * ((H + 1) // 2 - 2) * ((W + 1) // 2 - 2)
                if name == "mg_hsweep_restrict":  # read u (or not), f; write out, f_c
                    total += nodes * (esz * (3 if _lib.arg(rec, "u") is not None else 2) + pb) + coarse * esz
                else:  # read u, f, e; write out
                    total += nodes * (3 * esz + pb) + coarse * (esz + pb)
                continue
            if name in ("mg_hmid_down", "mg_hmid_up"):
                n = []
                for _ in range(3):
                    n.append(B * (H - 2) * (W - 2))
                    H, W = (H + 1) // 2, (W + 1) // 2
                if name == "mg_hmid_down":  # read f_a; write u_a, f_(a+1), u_(a+1), f_(a+2)
                    total += esz * (2 * n[0] + 2 * n[1] + n[2]) + pb * (n[0] + n[1])
                else:  # read u_a, f_a, u_(a+1), f_(a+1), e; write u_a
                    total += esz * (3 * n[0] + 2 * n[1] + n[2]) + pb * (n[0] + n[1] + n[2])
                continue
            if name in ("mg_mid_down", "mg_mid_up"):
                k = _lib.arg(rec, "k")
                sizes = []
                for _ in range(k + 1):
                    sizes.append(B * (H - 2) * (W - 2))
                    H, W = (H + 1) // 2, (W + 1) // 2
                if name == "mg_mid_down":  # read f_a, write f_{a+1..a+k}
                    total += esz * sum(sizes) + pb * sum(sizes[:-1])
                else:  # read f_a..f_{a+k-1}, u_{a+k}; write u_a
                    total += esz * (sum(sizes) + sizes[0]) + pb * sum(sizes)
                continue
            if name == "mg_zero_restrict2":  # read f_l (+ pattern), write f_{l+1}, f_{l+2}
                n0 = B * (H - 2) * (W - 2)
                H, W = (H + 1) // 2, (W + 1) // 2
                n1 = B * (H - 2) * (W - 2)
                n2 = B * ((H + 1) // 2 - 2) * ((W + 1) // 2 - 2)
                total += n0 * (esz + pb) + (n1 + n2) * esz
                continue
            if name == "mg_prolong2":  # read f_l, f_{l+1} (+ patterns), e_{l+2}; write u_l
                n0 = B * (H - 2) * (W - 2)
                H, W = (H + 1) // 2, (W + 1) // 2
                n1 = B * (H - 2) * (W - 2)
                n2 = B * ((H + 1) // 2 - 2) * ((W + 1) // 2 - 2)
                total += n0 * (2 * esz + pb) + n1 * (esz + pb) + n2 * (esz + pb)
                continue
            nodes = B * (H - 2) * (W - 2)
            coarse = B * ((H + 1) // 2 - 2) * ((W + 1) // 2 - 2)
            if name == "mg_sweep":
                total += nodes * (esz * (3 if _lib.arg(rec, "u") is not None else 2) + pb)
            elif name == "mg_residual_restrict":
                u, v_out = _lib.arg(rec, "u"), _lib.arg(rec, "v_out")
                total += nodes * (esz * (2 if u is not None else 1) + pb) + coarse * esz
                if u is None and v_out is not None:
                    total += nodes * esz  # v written
            elif name == "mg_sweep_restrict":
                total += nodes * (3 * esz + pb) + coarse * esz
            elif name == "mg_prolong_sweep":  # u = NULL: the iterate is recomputed from f
                total += nodes * ((3 if _lib.arg(rec, "u") is not None else 2) * esz + pb) + coarse * (esz + pb)
            elif name == "mg_prolong_add":
                total += nodes * 2 * esz + coarse * (esz + pb)
        return total
