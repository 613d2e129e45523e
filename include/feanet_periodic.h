/*
 * feanet_periodic.h — C ABI of the two-material multigrid kernels on a TORUS (libfeanet_hip.so): an [m, n] element
 * image is the periodic cell, node (r, c) is the upper-left node of element (r, c), every index is taken modulo
 * (m, n) and every node is an unknown (definitions: DESIGN §18).  Conventions of feanet_hip.h: all data pointers are
 * DEVICE pointers owned by the caller; calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 * default); 0 on success, FEA_EINVAL (-1) for invalid arguments (nothing is launched), otherwise the hipError_t of the
 * launch; stateless, re-entrant, safe inside stream capture.
 *
 * Torus layout of a field of type T (float / double): node (r, c) of sample b at x[b * bstride + r * ld + c],
 * 0 <= r < m, 0 <= c < n; ld >= n and bstride >= m * ld, both multiples of 16 / sizeof(T); the base 16-byte aligned.
 * There is no ghost ring.  Every entry point writes exactly the m x n nodes of its output and no result depends on
 * the pad columns n .. ld-1 or the slack between samples.
 * pid: one pattern byte per node (interface_pattern_map's ids, 0 .. 15, built from the wrapped image), row pitch ldp
 * bytes, shared by the B samples; ldp a multiple of 4 and at least n rounded up to 16 / sizeof(T); 4-byte aligned.
 * ktab: the 16 x 9 stencil table in T; omd: 16 values omega / ktab[p][4] in T.
 * The operator, with taps t = 3 (dr + 1) + (dc + 1):  (K u)(r, c) = sum_t ktab[pid(r, c)][8 - t] u(r + dr, c + dc)
 * (the own-row mirrored form; equal to the neighbours' rows on a torus, tests/test_periodic_host.py).
 * What a driver does with these is shown in INTEGRATION.md and feanet_amd/periodic.py.
 */
#ifndef FEANET_PERIODIC_H
#define FEANET_PERIODIC_H

#include "feanet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Partial sums fea_per_apply_* / fea_per_reduce_* write per sample and quantity for an m x n torus of elem_size 4 or 8
 * (one per wave task; the task grid is the one a single sample would get, so it does not depend on B); -1: unsupported
 * size. */
long long fea_per_parts(int m, int n, int elem_size);

/* out = u + omd[pid] (f - K u), one weighted Jacobi sweep.  u NULL: the zero guess, out = omd[pid] f.  out must not
 * be u (nor overlap it). */
int fea_per_sweep_f32(const float* u, const float* f, float* out, const uint8_t* pid, long long ldp, const float* ktab,
                      const float* omd, int B, int m, int n, int ld, long long bstride, void* stream);
int fea_per_sweep_f64(const double* u, const double* f, double* out, const uint8_t* pid, long long ldp,
                      const double* ktab, const double* omd, int B, int m, int n, int ld, long long bstride,
                      void* stream);

/* fc(I, J) = sum over dr, dc in {-1, 0, 1} of k[dr][dc] (f - K u)(2 I + dr, 2 J + dc), k = [1 2 1; 2 4 2; 1 2 1] / 4,
 * on the (m / 2) x (n / 2) torus fc (pitch ldc, sample pitch bstridec, the same layout rules); the residual never goes
 * to memory.  m and n must be even.  u NULL: the zero guess, the residual is f. */
int fea_per_residual_restrict_f32(const float* u, const float* f, float* fc, const uint8_t* pid, long long ldp,
                                  const float* ktab, int B, int m, int n, int ld, long long bstride, int ldc,
                                  long long bstridec, void* stream);
int fea_per_residual_restrict_f64(const double* u, const double* f, double* fc, const uint8_t* pid, long long ldp,
                                  const double* ktab, int B, int m, int n, int ld, long long bstride, int ldc,
                                  long long bstridec, void* stream);

/* u += P ec in place, P the transpose of the restriction above: ec is the (m / 2) x (n / 2) coarse torus, u the m x n
 * fine one; m and n must be even. */
int fea_per_prolong_add_f32(const float* ec, float* u, int B, int m, int n, int ld, long long bstride, int ldc,
                            long long bstridec, void* stream);
int fea_per_prolong_add_f64(const double* ec, double* u, int B, int m, int n, int ld, long long bstride, int ldc,
                            long long bstridec, void* stream);

/* y = K p.  part NULL, or doubles part[(b * 2 + q) * per + i], 0 <= i < per = fea_per_parts(m, n, sizeof(T)): the
 * partial sums of p . y (q = 0) and of y (q = 1) of sample b.  y must not be p. */
int fea_per_apply_f32(const float* p, float* y, double* part, const uint8_t* pid, long long ldp, const float* ktab,
                      int B, int m, int n, int ld, long long bstride, void* stream);
int fea_per_apply_f64(const double* p, double* y, double* part, const uint8_t* pid, long long ldp, const double* ktab,
                      int B, int m, int n, int ld, long long bstride, void* stream);

/* part[b * per + i]: the partial sums of a . b over the m x n nodes of sample b, or of a alone (b NULL). */
int fea_per_reduce_f32(const float* a, const float* b, double* part, int B, int m, int n, int ld, long long bstride,
                       void* stream);
int fea_per_reduce_f64(const double* a, const double* b, double* part, int B, int m, int n, int ld, long long bstride,
                       void* stream);

/* sums[j] = part[j * per .. j * per + per - 1] summed in a fixed order, 0 <= j < count (count = B quantities of a
 * reduce, 2 B of an apply).  Writes: those count doubles. */
int fea_per_final(const double* part, long long per, double* sums, int count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_PERIODIC_H */
