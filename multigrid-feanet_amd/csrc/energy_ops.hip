// energy_ops.hip — the bilinear energy form d(u, v) = u_e^T Ke v_e between two level-0 FRAMED fields, summed per
// phase, with its element density (include/feanet_energy.h; layout and strip x row-march decomposition: framed_ops.hip /
// framed_strip.h; the kernel shape is flux_ops.hip's).
//
//   energy  d(u,u), d(u,v), d(v,v) per element (optional store), partials of their sums over phase 0 and phase 1
//           2 * 8 + 1 B per fp64 node for the sums, 2 * 8 + 1 + 24 B with the densities
//   final   one workgroup per (pair, quantity) sums its partials in index order
//
// A lane owns VEC node columns c and computes the elements whose RIGHT node is its own column, C = c - 1; the left
// node of its first element comes by DPP from the lane below, for both fields (lane 0: one scalar load of column
// c0 - 1, a node: strip 0 starts at column 1).  Its VEC elements start at C = s SW + VEC lane, a multiple of VEC, so a
// store to dens is one aligned 16-byte store, and the node loads keep the framed alignment.  Strips and row tasks are
// k_flux's (energy_geom == flux_geom: strips over node columns 1 .. W-1, row tasks of the height ONE sample gets, the
// last task takes node row H-1 as well), so a pair's partial set is the same bits in any batch.
// Two node rows of each field live in registers; the next rows' loads are issued before the arithmetic.  Every lane
// accumulates in double, every wave writes one double per quantity (fixed butterfly order).  No LDS, no atomics, no
// branch on data: the phase is one select on the phase byte, elements right of the grid are selected out of the sums
// and masked out of the stores, so nothing depends on the pad columns the vector loads touch.
// d is ONE function of its two fields; its products commute bit for bit, so d(u, v) and d(v, u) are the same bits and
// u == v gives three equal results.
#include "framed_strip.h"
#include "feanet_energy.h"

namespace fea {

template <typename T>
struct EnergyArgs {
  const T* u;
  const T* v;
  const uint8_t* phase;
  long long ldp;
  T* dens;
  long long ldd, cs, dbs;
  double* part;
  long long per;
  int H, W, ld;
  long long ubs, vbs;
  int nstrips, ntr, rb;
};

// one node row of a lane: l = column cl - 1 (lane 0 only), x[0 .. V-1] = own columns
template <typename T, int V>
struct EnergyRow {
  T x[V];
  T l;
};

template <typename T, int V>
__device__ __forceinline__ EnergyRow<T, V> energy_load(const T* __restrict__ rp, int lane) {
  EnergyRow<T, V> r;
  vload<T, V>(rp + V * lane, r.x);
  r.l = T(0);
  if (lane == 0) r.l = rp[-1];  // exec-masked: the other lanes take their left node from the lane below
  return r;
}

// the window row of a lane: w[0] = column cl - 1, w[1 .. V] = own columns
template <typename T, int V>
__device__ __forceinline__ void energy_window(const EnergyRow<T, V>& r, T (&w)[V + 1]) {
  w[0] = shr1(r.x[V - 1], r.l);
#pragma unroll
  for (int k = 0; k < V; ++k) w[k + 1] = r.x[k];
}

// sc, sr, w of one element of one field (feanet_flux.h)
template <typename T>
struct ElemDiffs {
  T sc, sr, w;
};
template <typename T>
__device__ __forceinline__ ElemDiffs<T> elem_diffs(T a, T b, T c, T d) {
  return {(b - a) + (d - c), (c - a) + (d - b), (a - b) - (c - d)};
}
template <typename T>
__device__ __forceinline__ T energy_d(const ElemDiffs<T>& x, const ElemDiffs<T>& y) {
  return (x.sc * y.sc + x.sr * y.sr) * T(0.25) + (x.w * y.w) * T(1.0 / 6.0);
}

template <typename T, bool FIELDS, bool PHASE, bool NT>
__global__ __launch_bounds__(256) void k_energy(EnergyArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int H = g.H, We = g.W - 1;
  const int c0 = 1 + id.s * F::SW;
  const int r0 = 1 + id.t * g.rb;
  const int r1 = id.t == g.ntr - 1 ? H : min(r0 + g.rb, H - 1);  // node rows r0 .. r1-1; the last task: up to H-1
  const int C0 = c0 - 1 + V * lane;                              // first own element column, a multiple of V
  const T* __restrict__ ub = g.u + (long long)id.b * g.ubs + F::OFF + c0;
  const T* __restrict__ vb = g.v + (long long)id.b * g.vbs + F::OFF + c0;
  const int ld = g.ld;
  auto rowo = [&](int r) { return (long long)(min(r, H - 1) + 1) * ld; };
  double s[FEA_ENERGY_NSUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  T ut[V + 1], vt[V + 1];
  energy_window<T, V>(energy_load<T, V>(ub + rowo(r0 - 1), lane), ut);
  energy_window<T, V>(energy_load<T, V>(vb + rowo(r0 - 1), lane), vt);
  EnergyRow<T, V> unx = energy_load<T, V>(ub + rowo(r0), lane);
  EnergyRow<T, V> vnx = energy_load<T, V>(vb + rowo(r0), lane);
  for (int r = r0; r < r1; ++r) {
    // (row H-1 again behind the last row: never used)
    const EnergyRow<T, V> unn = energy_load<T, V>(ub + rowo(r + 1), lane);
    const EnergyRow<T, V> vnn = energy_load<T, V>(vb + rowo(r + 1), lane);
    const int R = r - 1;
    int ph[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      ph[k] = 0;
      if constexpr (PHASE)
        if (C0 + k < We) ph[k] = g.phase[(long long)R * g.ldp + C0 + k];
    }
    T ubw[V + 1], vbw[V + 1];
    energy_window<T, V>(unx, ubw);
    energy_window<T, V>(vnx, vbw);
    T duu[V], duv[V], dvv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const ElemDiffs<T> x = elem_diffs(ut[k], ut[k + 1], ubw[k], ubw[k + 1]);
      const ElemDiffs<T> y = elem_diffs(vt[k], vt[k + 1], vbw[k], vbw[k + 1]);
      duu[k] = energy_d(x, x);
      duv[k] = energy_d(x, y);
      dvv[k] = energy_d(y, y);
      const bool in = C0 + k < We;
      const bool p0 = in && ph[k] == 0;
      s[0] += p0 ? (double)duu[k] : 0.0;
      s[2] += p0 ? (double)duv[k] : 0.0;
      s[4] += p0 ? (double)dvv[k] : 0.0;
      if constexpr (PHASE) {
        const bool p1 = in && ph[k] != 0;
        s[1] += p1 ? (double)duu[k] : 0.0;
        s[3] += p1 ? (double)duv[k] : 0.0;
        s[5] += p1 ? (double)dvv[k] : 0.0;
      }
    }
    if constexpr (FIELDS) {
      T* dp = g.dens + (long long)id.b * g.dbs + (long long)R * g.ldd + C0;
      store_masked<T, V, NT>(dp, duu, C0, g.W);  // element columns C0 + k <= We - 1 (store_masked: cl + k <= W - 2)
      store_masked<T, V, NT>(dp + g.cs, duv, C0, g.W);
      store_masked<T, V, NT>(dp + 2 * g.cs, dvv, C0, g.W);
    }
#pragma unroll
    for (int k = 0; k <= V; ++k) {
      ut[k] = ubw[k];
      vt[k] = vbw[k];
    }
    unx = unn;
    vnx = vnn;
  }
  const long long slot = (long long)id.b * FEA_ENERGY_NSUMS * g.per + (long long)id.t * g.nstrips + id.s;
#pragma unroll
  for (int k = 0; k < FEA_ENERGY_NSUMS; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < FEA_ENERGY_NSUMS; ++k) g.part[slot + k * g.per] = s[k];
  }
}

// One workgroup per (pair, quantity): its `per` partials summed in index order (the scheme of k_flux_final).
__global__ __launch_bounds__(256) void k_energy_final(const double* __restrict__ part, long long per,
                                                     double* __restrict__ sums) {
  __shared__ double sh[256];
  const double* p = part + blockIdx.x * per;
  double s = 0.0;
  for (long long i = threadIdx.x; i < per; i += 256) s += p[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

}  // namespace fea

// the task grid of fea_flux: the Krylov kernels' row tasks (pcg_geom), strips over node columns 1 .. W-1
template <typename T>
static void energy_geom(int H, int W, int& nstrips, int& rb, int& ntr) {
  nstrips = div_up(W - 1, Frame<T>::SW);
  rb = pick_rb(1, nstrips, H - 2);
  ntr = div_up(H - 2, rb);
}

extern "C" long long fea_energy_parts(int H, int W, int elem_size) {
  if (!mg_dims_ok(H, W) || (elem_size != 4 && elem_size != 8)) return -1;
  int ns, rb, ntr;
  if (elem_size == 8) energy_geom<double>(H, W, ns, rb, ntr);
  else energy_geom<float>(H, W, ns, rb, ntr);
  return (long long)ns * ntr;
}

template <typename T>
static int energy(const T* u, const T* v, const uint8_t* phase, long long ldp, T* dens, long long ldd,
                  long long cstride, long long dbstride, double* part, int B, int H, int W, int ld, long long ubs,
                  long long vbs, void* stream) {
  constexpr int V = Frame<T>::VEC;
  if (!u || !v || !part || B < 1 || !layout_ok<T>(H, W, ld, ubs) || !layout_ok<T>(H, W, ld, vbs)) return FEA_EINVAL;
  const int He = H - 1, We = W - 1;
  if (phase && ldp < We) return FEA_EINVAL;
  if (dens) {
    if (ldd < We || ldd % V || cstride % V || dbstride % V || cstride < (long long)He * ldd ||
        dbstride < 3 * cstride || (uintptr_t)dens % 16)
      return FEA_EINVAL;
    const uintptr_t d0 = (uintptr_t)dens, d1 = d0 + (uintptr_t)B * dbstride * sizeof(T);
    const uintptr_t u0 = (uintptr_t)u, u1 = u0 + (uintptr_t)B * ubs * sizeof(T);
    const uintptr_t v0 = (uintptr_t)v, v1 = v0 + (uintptr_t)B * vbs * sizeof(T);
    if ((d0 < u1 && u0 < d1) || (d0 < v1 && v0 < d1)) return FEA_EINVAL;
  }
  EnergyArgs<T> g{};
  g.u = u; g.v = v; g.phase = phase; g.ldp = ldp;
  g.dens = dens; g.ldd = ldd; g.cs = cstride; g.dbs = dbstride; g.part = part;
  g.H = H; g.W = W; g.ld = ld; g.ubs = ubs; g.vbs = vbs;
  energy_geom<T>(H, W, g.nstrips, g.rb, g.ntr);
  g.per = (long long)g.nstrips * g.ntr;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  const bool nt = dens && (long long)B * dbstride * (long long)sizeof(T) > nt_bytes();
  with_flags(
      [&](auto fields, auto ph, auto ntc) {
        if constexpr (fields.value || !ntc.value)  // sums only: nothing to stream
          k_energy<T, fields.value, ph.value, ntc.value><<<grid, 256, 0, (hipStream_t)stream>>>(g);
      },
      dens != nullptr, phase != nullptr, nt);
  return launch_status();
}

#define FEA_ENERGY_API(SUF, T)                                                                                       \
  extern "C" int fea_energy_##SUF(const T* u, const T* v, const uint8_t* phase, long long ldp, T* dens,              \
                                  long long ldd, long long cstride, long long dbstride, double* part, int B, int H,  \
                                  int W, int ld, long long ubstride, long long vbstride, void* stream) {             \
    return energy<T>(u, v, phase, ldp, dens, ldd, cstride, dbstride, part, B, H, W, ld, ubstride, vbstride, stream); \
  }
FEA_ENERGY_API(f32, float)
FEA_ENERGY_API(f64, double)

extern "C" int fea_energy_final(const double* part, long long per, double* sums, int B, void* stream) {
  if (!part || !sums || per < 1 || B < 1) return FEA_EINVAL;
  k_energy_final<<<B * FEA_ENERGY_NSUMS, 256, 0, (hipStream_t)stream>>>(part, per, sums);
  return launch_status();
}
