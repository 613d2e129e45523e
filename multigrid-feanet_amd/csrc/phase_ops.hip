// phase_ops.hip — on-device set-up of the two-material problem from an element phase image (include/feanet_phase.h).
//
// The reference builds its pattern maps for two geometries only (MeshCenterInterface's centred disc / square,
// setup_ops.hip).  Here the geometry is data: one byte per element, 0 or 1.
//   k_phase_pattern_map: node (r, c) of the (He+1) x (We+1) node grid has the quadrant elements
//       e1 = (r-1, c), e2 = (r-1, c-1), e3 = (r, c-1), e4 = (r, c)        (setup_ops.hip, FEANet/mesh.py:78-93)
//     and an element outside the image counts as phase 0.  EVERY node gets the pattern of the elements it touches,
//     boundary nodes included: the reference's pattern 0 on the boundary breaks the symmetry K_ij == K_ji of the
//     one-row-per-node stencil table as soon as phase 1 touches the boundary (DESIGN: the phase image section).
//   k_phase_coarsen: a coarse element is phase 1 when at least min_count of its 2 x 2 children are.
// Set-up kernels, not a hot path: plain byte loads and stores, one thread per output byte, rows walked by a
// grid-stride loop so that any height fits the grid.
#include "fea_common.h"
#include "feanet_phase.h"

namespace fea {

// bits e1 + 2 e2 + 4 e3 + 8 e4 -> pattern id (inverse of FEANet/mesh.py:23-26; setup_ops.hip holds its own copy)
__constant__ uint8_t kPhaseBitsToId[16] = {0, 4, 5, 7, 3, 11, 8, 12, 2, 9, 10, 13, 6, 15, 14, 1};

constexpr int kPhaseMaxDim = 1 << 20;  // elements per side
constexpr int kPhaseMaxRowsGrid = 32768;

__global__ __launch_bounds__(256) void k_phase_pattern_map(const uint8_t* __restrict__ phase, long long ldp, int He,
                                                           int We, uint8_t* __restrict__ pid, long long ldpid) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > We) return;
  const bool left = c >= 1, right = c < We;  // element columns c-1 / c exist
  for (int r = blockIdx.y; r <= He; r += gridDim.y) {
    const bool up = r >= 1, down = r < He;   // element rows r-1 / r exist
    // a pointer is formed only under the guard of the element it reads
    int e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    if (up && right) e1 = phase[(long long)(r - 1) * ldp + c] != 0;
    if (up && left) e2 = phase[(long long)(r - 1) * ldp + (c - 1)] != 0;
    if (down && left) e3 = phase[(long long)r * ldp + (c - 1)] != 0;
    if (down && right) e4 = phase[(long long)r * ldp + c] != 0;
    pid[(long long)r * ldpid + c] = kPhaseBitsToId[e1 + 2 * e2 + 4 * e3 + 8 * e4];
  }
}

__global__ __launch_bounds__(256) void k_phase_coarsen(const uint8_t* __restrict__ fine, long long ldf, int Hc, int Wc,
                                                       uint8_t* __restrict__ coarse, long long ldc, int min_count) {
  const int J = blockIdx.x * blockDim.x + threadIdx.x;
  if (J >= Wc) return;
  for (int I = blockIdx.y; I < Hc; I += gridDim.y) {
    const uint8_t* p = fine + (long long)(2 * I) * ldf + 2 * J;  // rows 2I, 2I+1 < He; columns 2J, 2J+1 < We
    const int cnt = (p[0] != 0) + (p[1] != 0) + (p[ldf] != 0) + (p[ldf + 1] != 0);
    coarse[(long long)I * ldc + J] = cnt >= min_count ? 1 : 0;
  }
}

}  // namespace fea

using namespace fea;

extern "C" int fea_phase_pattern_map(const uint8_t* phase, long long ldp, int He, int We, uint8_t* pid,
                                     long long ldpid, void* stream) {
  if (!phase || !pid || He < 1 || We < 1 || He > kPhaseMaxDim || We > kPhaseMaxDim || ldp < We ||
      ldpid < (long long)We + 1)
    return FEA_EINVAL;
  const dim3 grid((We + 1 + 255) / 256, std::min(He + 1, kPhaseMaxRowsGrid));
  k_phase_pattern_map<<<grid, 256, 0, (hipStream_t)stream>>>(phase, ldp, He, We, pid, ldpid);
  return launch_status();
}

extern "C" int fea_phase_coarsen(const uint8_t* fine, long long ldf, int He, int We, uint8_t* coarse, long long ldc,
                                 int min_count, void* stream) {
  if (!fine || !coarse || fine == coarse || He < 2 || We < 2 || (He & 1) || (We & 1) || He > kPhaseMaxDim ||
      We > kPhaseMaxDim || ldf < We || ldc < We / 2 || min_count < 1 || min_count > 4)
    return FEA_EINVAL;
  const int Hc = He / 2, Wc = We / 2;
  const dim3 grid((Wc + 255) / 256, std::min(Hc, kPhaseMaxRowsGrid));
  k_phase_coarsen<<<grid, 256, 0, (hipStream_t)stream>>>(fine, ldf, Hc, Wc, coarse, ldc, min_count);
  return launch_status();
}
