/*
 * feanet_fmg.h — C ABI of the full-multigrid (nested iteration) transfers of libfeanet_hip.so, next to
 * feanet_hip.h, whose conventions hold here too: T is float (_f32) or double (_f64); all data pointers are DEVICE
 * pointers owned by the caller; calls are asynchronous on `stream`; 0 on success, FEA_EINVAL (-1) for invalid
 * arguments (nothing is launched), otherwise the hipError_t of the launch; stateless, re-entrant, safe inside
 * stream capture.
 *
 * All three work on FRAMED level buffers (family (2) of feanet_hip.h: node (r, c) of sample b at
 * base[b*bstride + (r+1)*ld + (A-1) + c], fea_mg_layout() for ld / bstride).  Where a coarse level is involved,
 * H and W are odd and the coarse level has (H+1)/2 x (W+1)/2 nodes in its own framed layout (ldc, bstridec).
 * The reference has no full-multigrid start; what a driver does with these is shown in INTEGRATION.md and
 * MultigridSolver.fmg (feanet_amd/solver.py).
 */
#ifndef FEANET_FMG_H
#define FEANET_FMG_H

#include "feanet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = u + I(ec) on the interior nodes of the H x W level: the interpolation of a coarse SOLUTION.  ec is the
 * (H+1)/2 x (W+1)/2 level including its boundary nodes, which are data (the coarse Dirichlet values); at least
 * 2 x 2 coarse nodes (H, W >= 3, odd).  u == NULL: zero.  out == u is legal (u is read at the node itself only);
 * out == ec and u == ec are rejected.
 * order = 1: bilinear (1/2, 1/2).  order = 3: tensor-product cubic — between coarse nodes i and i+1
 * (-1, 9, 9, -1)/16 of i-1 .. i+2, next to a boundary the one-sided (5, 15, -5, 1)/16 of the four nodes nearest
 * it; a direction with fewer than 4 coarse nodes falls back to 1/2, 1/2; coincident nodes copy; columns inside
 * each coarse row first, then across four coarse rows (the exact expression: csrc/fmg_ops.hip).
 * Writes: out's interior nodes only.  Its boundary nodes, ghost ring and pad are never written, and nothing the
 * ghost ring or pad of ec or u holds reaches a written value.  The result does not depend on B. */
int fea_fmg_prolong_f32(const float* u, const float* ec, float* out, int B, int H, int W, int ld, long long bstride,
                        int ldc, long long bstridec, int order, void* stream);
int fea_fmg_prolong_f64(const double* u, const double* ec, double* out, int B, int H, int W, int ld,
                        long long bstride, int ldc, long long bstridec, int order, void* stream);

/* fc = R f on the coarse interior with the fixed R = [[1,2,1],[2,4,2],[1,2,1]]/4, the transpose of the bilinear
 * interpolation: the coarse load vector of a fine one.  No stencil, no table, no iterate; bitwise
 * fea_mg_residual_restrict with an all-zero u, rtab = R and w0 = 1.  H, W >= 5, odd.  fc == f is rejected.
 * Writes: fc's interior nodes only. */
int fea_fmg_restrict_f32(const float* f, float* fc, int B, int H, int W, int ld, long long bstride, int ldc,
                         long long bstridec, void* stream);
int fea_fmg_restrict_f64(const double* f, double* fc, int B, int H, int W, int ld, long long bstride, int ldc,
                         long long bstridec, void* stream);

/* The 2 (H + W) - 4 boundary nodes of framed dst: node (r, c) takes bc[b * bc_bstride + (r * stride) * Wf +
 * c * stride] of the contiguous fine field bc ([B, 1, (H-1)*stride + 1, Wf], Wf = (W-1)*stride + 1; bc_bstride
 * elements between samples, 0 = one field for all), or zero when bc == NULL.  stride >= 1.  Injects the Dirichlet
 * data of the fine level onto a coarse one, and takes it off again.
 * Writes: dst's boundary nodes only. */
int fea_fmg_boundary_f32(const float* bc, long long bc_bstride, int stride, float* dst, int B, int H, int W, int ld,
                         long long bstride, void* stream);
int fea_fmg_boundary_f64(const double* bc, long long bc_bstride, int stride, double* dst, int B, int H, int W, int ld,
                         long long bstride, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_FMG_H */
