/*
 * feanet_phase.h — C ABI of the two-material set-up from an element phase image (libfeanet_hip.so), next to
 * feanet_hip.h, whose conventions hold here too: all data pointers are DEVICE pointers owned by the caller; calls
 * are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default); 0 on success, FEA_EINVAL (-1) for
 * invalid arguments (nothing is launched), otherwise the hipError_t of the launch; stateless, re-entrant, safe
 * inside stream capture.
 *
 * A phase image holds one byte per ELEMENT, 0 or 1 (any non-zero byte counts as 1): the material of the two-phase
 * problem (coefficients prop[0], prop[1]).  He x We elements make (He+1) x (We+1) nodes.  Two phases only: the 16
 * rows of a stencil table (FEA_MAX_PATTERNS) hold exactly the 2^4 patterns of a node's four quadrant elements.
 * What a driver does with these is shown in INTEGRATION.md and MultigridSolver(phase=...) (feanet_amd/solver.py).
 */
#ifndef FEANET_PHASE_H
#define FEANET_PHASE_H

#include "feanet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pid[r * ldpid + c] = pattern id (0..15) of node (r, c), 0 <= r <= He, 0 <= c <= We, from its quadrant elements
 * e1 = (r-1, c), e2 = (r-1, c-1), e3 = (r, c-1), e4 = (r, c) of phase[er * ldp + ec] (the numbering of
 * fea_interface_pattern_map); an element outside the image counts as phase 0.  Unlike fea_interface_pattern_map,
 * BOUNDARY nodes get the pattern of the elements they touch too, so the stencil table stays symmetric
 * (K_ij == K_ji) on every image, whatever touches the boundary.  ldp >= We, ldpid >= We + 1 (bytes).
 * Writes: exactly those (He+1) x (We+1) bytes.  pid may point into a framed pattern map (base + ld + off): its
 * ghost ring and pad columns are not written.  One thread per node; no address outside the image is formed. */
int fea_phase_pattern_map(const uint8_t* phase, long long ldp, int He, int We, uint8_t* pid, long long ldpid,
                          void* stream);

/* coarse[I * ldc + J] = 1 if at least min_count of the elements (2I, 2J), (2I, 2J+1), (2I+1, 2J), (2I+1, 2J+1) of
 * `fine` are phase 1, else 0.  He, We >= 2 and even (the fine image); the coarse one is He/2 x We/2.  min_count in
 * 1..4; ldf >= We, ldc >= We/2 (bytes).  coarse == fine is rejected.
 * Writes: exactly the He/2 x We/2 bytes of coarse. */
int fea_phase_coarsen(const uint8_t* fine, long long ldf, int He, int We, uint8_t* coarse, long long ldc,
                      int min_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEANET_PHASE_H */
