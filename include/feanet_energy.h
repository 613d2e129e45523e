/*
 * feanet_energy.h — C ABI of the bilinear energy form between two nodal fields, split by phase, with its element
 * density (libfeanet_hip.so), next to feanet_flux.h, whose conventions, grid axes, element nodes a, b, c, d and
 * quantities hold here too: all data pointers are DEVICE pointers owned by the caller; calls are asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = default); 0 on success, FEA_EINVAL (-1) for invalid arguments
 * (nothing is launched), otherwise the hipError_t of the launch; stateless, re-entrant, safe inside stream capture.
 *
 * With sc_x, sr_x, w_x of feanet_flux.h for a field x, in the field type T:
 *     d(u, v) = (sc_u sc_v + sr_u sr_v) 0.25 + (w_u w_v) (1/6)      (= u_e^T Ke v_e of the Q1 Laplace element)
 * d carries neither the coefficient k nor the node spacing h: a(u, v) = sum_p k_p sum_{e in phase p} d(u, v).
 * What a driver does with these is shown in INTEGRATION.md and feanet_amd/flux.py (energy_forms).
 */
#ifndef FEANET_ENERGY_H
#define FEANET_ENERGY_H

#include "feanet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-pair sums over all elements of a phase, in this order: d(u,u) over phase 0, d(u,u) over phase 1, d(u,v) over
 * phase 0, d(u,v) over phase 1, d(v,v) over phase 0, d(v,v) over phase 1 */
#define FEA_ENERGY_NSUMS 6

/* Partial sums fea_energy_* writes per pair and quantity for an H x W node grid of elem_size 4 or 8 (one per wave
 * task; the task grid is the one a single sample would get, so it does not depend on B); -1: unsupported size. */
long long fea_energy_parts(int H, int W, int elem_size);

/* u, v: level-0 framed fields (fea_mg_layout: ld); pair b is u + b * ubstride with v + b * vbstride, 0 <= b < B, and
 * ubstride, vbstride >= (H + 2) * ld.  u == v is allowed (the three forms are then the same bits); the two load cases
 * of one batch are v = u + bstride with B = 1.  All H x W nodes are used, boundary nodes included; no result depends
 * on the ghost ring, the pad columns or the slack between samples.
 * phase: one byte per element (non-zero counts as 1), row pitch ldp >= We bytes, shared by the B pairs; NULL: every
 * element is phase 0 and the phase-1 sums are 0.
 * dens: NULL (sums only) or the element densities: component 0 is d(u,u), 1 is d(u,v), 2 is d(v,v); element (R, C)
 * of pair b and component j at dens[b * dbstride + j * cstride + R * ldd + C]; ldd >= We, cstride >= He * ldd,
 * dbstride >= 3 * cstride, all three multiples of 16 / sizeof(T); dens 16-byte aligned and overlapping neither u nor v.
 * Writes: exactly the He x We elements of each component (dens' pad columns stay), and
 * part[(b * FEA_ENERGY_NSUMS + k) * per + i], 0 <= i < per = fea_energy_parts(H, W, sizeof(T)): doubles. */
int fea_energy_f32(const float* u, const float* v, const uint8_t* phase, long long ldp, float* dens, long long ldd,
                   long long cstride, long long dbstride, double* part, int B, int H, int W, int ld,
                   long long ubstride, long long vbstride, void* stream);
int fea_energy_f64(const double* u, const double* v, const uint8_t* phase, long long ldp, double* dens, long long ldd,
                   long long cstride, long long dbstride, double* part, int B, int H, int W, int ld,
                   long long ubstride, long long vbstride, void* stream);

/* sums[b * FEA_ENERGY_NSUMS + k] = the `per` partials of pair b and quantity k summed in index order (the raw sums;
 * the coefficients and the volume are the host's).  Writes: those B * 6 doubles. */
int fea_energy_final(const double* part, long long per, double* sums, int B, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_ENERGY_H */
