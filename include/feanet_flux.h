/*
 * feanet_flux.h — C ABI of the element flux fields and their per-sample sums (libfeanet_hip.so), next to
 * feanet_hip.h, whose conventions hold here too: all data pointers are DEVICE pointers owned by the caller; calls
 * are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default); 0 on success, FEA_EINVAL (-1) for
 * invalid arguments (nothing is launched), otherwise the hipError_t of the launch; stateless, re-entrant, safe
 * inside stream capture.
 *
 * Grid axes: axis 0 is the row index r (coordinate r h), axis 1 the column index c (coordinate c h).  Element
 * (R, C), 0 <= R < He = H-1, 0 <= C < We = W-1, has the nodes a = u[R][C], b = u[R][C+1], c = u[R+1][C],
 * d = u[R+1][C+1] and the coefficient k = phase[R][C] ? k1 : k0.  In the field type T:
 *     sc = (b - a) + (d - c)      sr = (c - a) + (d - b)      w = (a - b) - (c - d)
 *     g_c = sc i2h                g_r = sr i2h                (i2h = 1 / (2h): the element's mean gradient)
 *     q_c = -k g_c                q_r = -k g_r
 *     e   = k ((sc sc + sr sr) 0.25 + w w (1/6))              (= k u_e^T Ke u_e of the Q1 Laplace element; h-free)
 * What a driver does with these is shown in INTEGRATION.md and feanet_amd/flux.py.
 */
#ifndef FEANET_FLUX_H
#define FEANET_FLUX_H

#include "feanet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEA_FLUX_NSUMS 5 /* per-sample sums over all elements, in this order: q_r, q_c, g_r, g_c, e */

/* Partial sums fea_flux_* writes per sample and quantity for an H x W node grid of elem_size 4 or 8 (one per wave
 * task; the task grid is the one a single sample would get, so it does not depend on B); -1: unsupported size. */
long long fea_flux_parts(int H, int W, int elem_size);

/* u: level-0 framed fields (fea_mg_layout: ld, bstride), B samples; all H x W nodes are used, boundary nodes
 * included; no result depends on the ghost ring, the pad columns or the slack between samples.
 * phase: one byte per element (non-zero counts as 1), row pitch ldp >= We bytes, shared by the B samples; NULL:
 * k = k0 everywhere.  k0, k1 and h (> 0, finite) are rounded to T once.
 * q: NULL (sums only) or the flux fields: component 0 is q_r, component 1 is q_c, element (R, C) of sample b and
 * component j at q[b * qbstride + j * cstride + R * ldq + C]; ldq >= We, cstride >= He * ldq, qbstride >= 2 * cstride,
 * all three multiples of 16 / sizeof(T); q 16-byte aligned and not overlapping u.
 * Writes: exactly the He x We elements of each component (q's pad columns stay), and
 * part[(b * FEA_FLUX_NSUMS + k) * per + i], 0 <= i < per = fea_flux_parts(H, W, sizeof(T)): doubles. */
int fea_flux_f32(const float* u, const uint8_t* phase, long long ldp, double k0, double k1, double h, float* q,
                 long long ldq, long long cstride, long long qbstride, double* part, int B, int H, int W, int ld,
                 long long bstride, void* stream);
int fea_flux_f64(const double* u, const uint8_t* phase, long long ldp, double k0, double k1, double h, double* q,
                 long long ldq, long long cstride, long long qbstride, double* part, int B, int H, int W, int ld,
                 long long bstride, void* stream);

/* sums[b * FEA_FLUX_NSUMS + k] = the `per` partials of sample b and quantity k summed in index order (the raw sums
 * over all elements; means and the factor h^2 of the energy's volume are the host's).  Writes: those B * 5 doubles. */
int fea_flux_final(const double* part, long long per, double* sums, int B, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_FLUX_H */
