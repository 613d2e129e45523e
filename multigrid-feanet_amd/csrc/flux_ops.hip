// flux_ops.hip — element flux fields and their per-sample sums from a level-0 FRAMED field (include/feanet_flux.h;
// layout and strip x row-march decomposition: framed_ops.hip / framed_strip.h).
//
//   flux    q = -k grad u at the element centroids (optional store), partials of sum q_r, q_c, g_r, g_c, e
//           8 + 1 B per fp64 node for the sums, 8 + 1 + 16 B with the fields
//   final   one workgroup per (sample, quantity) sums its partials in index order
//
// A lane owns VEC node columns c and computes the elements whose RIGHT node is its own column, C = c - 1; the left
// node of its first element comes by DPP from the lane below (lane 0: one scalar load of column c0 - 1, a node: strip
// 0 starts at column 1).  Its VEC elements start at C = s SW + VEC lane, a multiple of VEC, so its store to q is one
// aligned 16-byte store, and the node loads keep the framed alignment.  Strips cover node columns 1 .. W-1: one more
// column than the Krylov kernels' interior, so there are ceil((W-1) / SW) of them (W - 2 a multiple of SW: the last
// strip holds the boundary column alone).  Row tasks are the Krylov kernels' (pcg_geom: node rows 1 .. H-2 in tasks of
// the height ONE sample would get, so a sample's partial set, and with it every sum, is the same bits in any batch);
// a task owns the elements R = r - 1 of its node rows, and the last task takes node row H-1 as well.
// Two node rows live in registers; the next row's loads are issued before the arithmetic.  Every lane accumulates in
// double, every wave writes one double per quantity (fixed butterfly order).  No LDS, no atomics, no branch on data:
// k is one select on the phase byte, elements right of the grid are selected out of the sums and masked out of the
// stores, so nothing depends on the pad columns the vector loads touch.
#include "framed_strip.h"
#include "feanet_flux.h"

#include <cmath>

namespace fea {

template <typename T>
struct FluxArgs {
  const T* u;
  const uint8_t* phase;
  long long ldp;
  T k0, k1, i2h;
  T* q;
  long long ldq, cs, qbs;
  double* part;
  long long per;
  int H, W, ld;
  long long bs;
  int nstrips, ntr, rb;
};

// one node row of a lane: a[0] = column cl - 1, a[1 .. V] = own columns
template <typename T, int V>
struct FluxRow {
  T x[V];
  T l;
};

template <typename T, int V>
__device__ __forceinline__ FluxRow<T, V> flux_load(const T* __restrict__ rp, int lane) {
  FluxRow<T, V> r;
  vload<T, V>(rp + V * lane, r.x);
  r.l = T(0);
  if (lane == 0) r.l = rp[-1];  // exec-masked: the other lanes take their left node from the lane below
  return r;
}

template <typename T, bool FIELDS, bool PHASE, bool NT>
__global__ __launch_bounds__(256) void k_flux(FluxArgs<T> g) {
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
  const T* __restrict__ ub = g.u + (long long)id.b * g.bs + F::OFF + c0;
  const int ld = g.ld;
  auto rowp = [&](int r) { return ub + (long long)(min(r, H - 1) + 1) * ld; };
  const T k0 = g.k0, k1 = g.k1, i2h = g.i2h;
  double s_qr = 0.0, s_qc = 0.0, s_gr = 0.0, s_gc = 0.0, s_e = 0.0;

  FluxRow<T, V> top = flux_load<T, V>(rowp(r0 - 1), lane);
  FluxRow<T, V> nx = flux_load<T, V>(rowp(r0), lane);
  T tw[V + 1];
  tw[0] = shr1(top.x[V - 1], top.l);
#pragma unroll
  for (int k = 0; k < V; ++k) tw[k + 1] = top.x[k];
  for (int r = r0; r < r1; ++r) {
    const FluxRow<T, V> nn = flux_load<T, V>(rowp(r + 1), lane);  // (row H-1 again behind the last row: never used)
    const int R = r - 1;
    int ph[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      ph[k] = 0;
      if constexpr (PHASE)
        if (C0 + k < We) ph[k] = g.phase[(long long)R * g.ldp + C0 + k];
    }
    T bw[V + 1];
    bw[0] = shr1(nx.x[V - 1], nx.l);
#pragma unroll
    for (int k = 0; k < V; ++k) bw[k + 1] = nx.x[k];
    T qr[V], qc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const T a = tw[k], b = tw[k + 1], c = bw[k], d = bw[k + 1];
      const T kk = ph[k] != 0 ? k1 : k0;
      const T sc = (b - a) + (d - c);
      const T sr = (c - a) + (d - b);
      const T w = (a - b) - (c - d);
      const T gc = sc * i2h;
      const T gr = sr * i2h;
      qc[k] = -kk * gc;
      qr[k] = -kk * gr;
      const T e = kk * ((sc * sc + sr * sr) * T(0.25) + w * w * T(1.0 / 6.0));
      const bool in = C0 + k < We;
      s_qr += in ? (double)qr[k] : 0.0;
      s_qc += in ? (double)qc[k] : 0.0;
      s_gr += in ? (double)gr : 0.0;
      s_gc += in ? (double)gc : 0.0;
      s_e += in ? (double)e : 0.0;
    }
    if constexpr (FIELDS) {
      T* qp = g.q + (long long)id.b * g.qbs + (long long)R * g.ldq + C0;
      store_masked<T, V, NT>(qp, qr, C0, g.W);  // element columns C0 + k <= We - 1 (store_masked: cl + k <= W - 2)
      store_masked<T, V, NT>(qp + g.cs, qc, C0, g.W);
    }
#pragma unroll
    for (int k = 0; k <= V; ++k) tw[k] = bw[k];
    nx = nn;
  }
  const long long slot = (long long)id.b * FEA_FLUX_NSUMS * g.per + (long long)id.t * g.nstrips + id.s;
  s_qr = wave_sum(s_qr);
  s_qc = wave_sum(s_qc);
  s_gr = wave_sum(s_gr);
  s_gc = wave_sum(s_gc);
  s_e = wave_sum(s_e);
  if (lane == 0) {
    g.part[slot] = s_qr;
    g.part[slot + g.per] = s_qc;
    g.part[slot + 2 * g.per] = s_gr;
    g.part[slot + 3 * g.per] = s_gc;
    g.part[slot + 4 * g.per] = s_e;
  }
}

// One workgroup per (sample, quantity): its `per` partials summed in index order (the scheme of k_norm_final).
__global__ __launch_bounds__(256) void k_flux_final(const double* __restrict__ part, long long per,
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

// the task grid: the Krylov kernels' row tasks (pcg_geom), strips over node columns 1 .. W-1
template <typename T>
static void flux_geom(int H, int W, int& nstrips, int& rb, int& ntr) {
  nstrips = div_up(W - 1, Frame<T>::SW);
  rb = pick_rb(1, nstrips, H - 2);
  ntr = div_up(H - 2, rb);
}

extern "C" long long fea_flux_parts(int H, int W, int elem_size) {
  if (!mg_dims_ok(H, W) || (elem_size != 4 && elem_size != 8)) return -1;
  int ns, rb, ntr;
  if (elem_size == 8) flux_geom<double>(H, W, ns, rb, ntr);
  else flux_geom<float>(H, W, ns, rb, ntr);
  return (long long)ns * ntr;
}

template <typename T>
static int flux(const T* u, const uint8_t* phase, long long ldp, double k0, double k1, double h, T* q, long long ldq,
                long long cstride, long long qbstride, double* part, int B, int H, int W, int ld, long long bs,
                void* stream) {
  constexpr int V = Frame<T>::VEC;
  if (!u || !part || B < 1 || !layout_ok<T>(H, W, ld, bs) || !std::isfinite(h) || !(h > 0.0)) return FEA_EINVAL;
  const int He = H - 1, We = W - 1;
  if (phase && ldp < We) return FEA_EINVAL;
  if (q) {
    if (ldq < We || ldq % V || cstride % V || qbstride % V || cstride < (long long)He * ldq ||
        qbstride < 2 * cstride || (uintptr_t)q % 16)
      return FEA_EINVAL;
    const uintptr_t u0 = (uintptr_t)u, u1 = u0 + (uintptr_t)B * bs * sizeof(T);
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)B * qbstride * sizeof(T);
    if (q0 < u1 && u0 < q1) return FEA_EINVAL;
  }
  FluxArgs<T> g{};
  g.u = u; g.phase = phase; g.ldp = ldp; g.k0 = (T)k0; g.k1 = (T)k1; g.i2h = (T)(1.0 / (2.0 * h));
  g.q = q; g.ldq = ldq; g.cs = cstride; g.qbs = qbstride; g.part = part;
  g.H = H; g.W = W; g.ld = ld; g.bs = bs;
  flux_geom<T>(H, W, g.nstrips, g.rb, g.ntr);
  g.per = (long long)g.nstrips * g.ntr;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  const bool nt = q && (long long)B * qbstride * (long long)sizeof(T) > nt_bytes();
  with_flags(
      [&](auto fields, auto ph, auto ntc) {
        if constexpr (fields.value || !ntc.value)  // sums only: nothing to stream
          k_flux<T, fields.value, ph.value, ntc.value><<<grid, 256, 0, (hipStream_t)stream>>>(g);
      },
      q != nullptr, phase != nullptr, nt);
  return launch_status();
}

#define FEA_FLUX_API(SUF, T)                                                                                         \
  extern "C" int fea_flux_##SUF(const T* u, const uint8_t* phase, long long ldp, double k0, double k1, double h,     \
                                T* q, long long ldq, long long cstride, long long qbstride, double* part, int B,     \
                                int H, int W, int ld, long long bstride, void* stream) {                             \
    return flux<T>(u, phase, ldp, k0, k1, h, q, ldq, cstride, qbstride, part, B, H, W, ld, bstride, stream);         \
  }
FEA_FLUX_API(f32, float)
FEA_FLUX_API(f64, double)

extern "C" int fea_flux_final(const double* part, long long per, double* sums, int B, void* stream) {
  if (!part || !sums || per < 1 || B < 1) return FEA_EINVAL;
  k_flux_final<<<B * FEA_FLUX_NSUMS, 256, 0, (hipStream_t)stream>>>(part, per, sums);
  return launch_status();
}
