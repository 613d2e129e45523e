/*
 * feanet_coef.h — C ABI of the matrix-free multigrid kernels on a TORUS whose elements each carry their own
 * coefficient (libfeanet_hip.so; definitions: DESIGN §19).  The cell, the node numbering, the torus layout of a field
 * and every convention are those of feanet_periodic.h: device pointers owned by the caller, asynchronous on `stream`,
 * 0 on success, FEA_EINVAL (-1) for invalid arguments (nothing is launched), otherwise the hipError_t of the launch;
 * stateless, re-entrant, safe inside stream capture.  Prolongation, the reductions, the final sum and the partial-sum
 * count are feanet_periodic.h's (fea_per_prolong_add, fea_per_reduce, fea_per_final, fea_per_parts): they never look
 * at a coefficient.
 *
 * k: the coefficient field in T, one positive finite value per element, element (R, C) at k[R * ldk + C], 0 <= R < m,
 * 0 <= C < n; ldk >= n a multiple of 16 / sizeof(T); the base 16-byte aligned; shared by the B samples.  No result
 * depends on the pad columns n .. ldk-1.
 * Node (r, c) touches the elements NW (r-1, c-1), NE (r-1, c), SW (r, c-1), SE (r, c), indices wrapped.  With the
 * eight differences d_X = u(r, c) - u(neighbour X) and t_NW = (d_N + d_W) + 2 d_NW, t_NE = (d_N + d_E) + 2 d_NE,
 * t_SW = (d_S + d_W) + 2 d_SW, t_SE = (d_S + d_E) + 2 d_SE the operator is
 *     (K u)(r, c) = ((k_NW t_NW + k_NE t_NE) + (k_SW t_SW + k_SE t_SE)) * (1/6),
 * the diagonal d = (2/3) ((k_NW + k_NE) + (k_SW + k_SE)).  K applied to a constant is exactly zero.
 * m and n are at least 2.
 */
#ifndef FEANET_COEF_H
#define FEANET_COEF_H

#include "feanet_periodic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEA_COEF_ARITHMETIC 0
#define FEA_COEF_HARMONIC 1
#define FEA_COEF_GEOMETRIC 2

/* out = u + (omega / d) (f - K u), one weighted Jacobi sweep, one division per node.  u NULL: the zero guess,
 * out = (omega / d) f.  out must not overlap u or f. */
int fea_coef_sweep_f32(const float* u, const float* f, float* out, const float* k, long long ldk, double omega, int B,
                       int m, int n, int ld, long long bstride, void* stream);
int fea_coef_sweep_f64(const double* u, const double* f, double* out, const double* k, long long ldk, double omega,
                       int B, int m, int n, int ld, long long bstride, void* stream);

/* y = K p.  part NULL, or doubles part[(b * 2 + q) * per + i], 0 <= i < per = fea_per_parts(m, n, sizeof(T)): the
 * partial sums of p . y (q = 0) and of y (q = 1) of sample b (the layout of fea_per_apply).  y must not overlap p. */
int fea_coef_apply_f32(const float* p, float* y, double* part, const float* k, long long ldk, int B, int m, int n,
                       int ld, long long bstride, void* stream);
int fea_coef_apply_f64(const double* p, double* y, double* part, const double* k, long long ldk, int B, int m, int n,
                       int ld, long long bstride, void* stream);

/* fc = R (f - K u) on the (m / 2) x (n / 2) torus fc, R the full weighting of fea_per_residual_restrict; the residual
 * never goes to memory.  m and n must be even.  u NULL: the zero guess, the residual is f.  fc must not overlap u or
 * f. */
int fea_coef_residual_restrict_f32(const float* u, const float* f, float* fc, const float* k, long long ldk, int B,
                                   int m, int n, int ld, long long bstride, int ldc, long long bstridec,
                                   void* stream);
int fea_coef_residual_restrict_f64(const double* u, const double* f, double* fc, const double* k, long long ldk, int B,
                                   int m, int n, int ld, long long bstride, int ldc, long long bstridec,
                                   void* stream);

/* kc(I, J) = the mean of k(2 I .. 2 I + 1, 2 J .. 2 J + 1) under `rule`: FEA_COEF_ARITHMETIC
 * ((a + b) + (c + d)) / 4 in T; FEA_COEF_HARMONIC 4 / ((1/a + 1/b) + (1/c + 1/d)) and FEA_COEF_GEOMETRIC
 * exp(((log a + log b) + (log c + log d)) / 4), both in double and rounded to T once (a, b the upper row, c, d the
 * lower).  kc is (m / 2) x (n / 2) with pitch ldkc under k's rules; m and n must be even; kc must not overlap k. */
int fea_coef_coarsen_f32(const float* k, long long ldk, float* kc, long long ldkc, int m, int n, int rule,
                         void* stream);
int fea_coef_coarsen_f64(const double* k, long long ldk, double* kc, long long ldkc, int m, int n, int rule,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_COEF_H */
