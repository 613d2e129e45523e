// periodic_ops.hip — the two-material multigrid kernels on a torus (include/feanet_periodic.h; definitions:
// DESIGN §18).
//
//   sweep              out = u + omd (f - K u), or omd f from the zero guess
//   apply              y = K p, optionally with the partials of p . y and of sum y
//   reduce             partials of a . b or of sum a
//   residual_restrict  fc = R (f - K u), the residual stays in registers
//   prolong_add        u += R^T ec
//   final              one workgroup per quantity sums its partials in a fixed order
//
// Layout, decomposition, row helpers, task decoding and the host checks: torus_strip.h.  What is this file's own: a
// node's nine weights are its own row of the stencil table in LDS (kapply's two-material form, mirrored taps), found
// through the pattern map, and the sweep is jacobi(): the expressions of the framed kernels, written once.
// residual_restrict and prolong_add take one thread per coarse / fine node with modulo indexing at every size (the
// first version: the coarse levels are launch-bound, the fine ones re-read their neighbourhood from the caches).  A
// strip form of residual_restrict (the residual rows of a coarse row in registers, one residual per row by DPP) was
// measured at 4096^2: 56.0 us against 97.5 in fp32, but 194.5 against 134.9 in fp64, at 158 VGPRs.
#include "torus_strip.h"
#include "feanet_periodic.h"

namespace fea {

constexpr int kPerTab = 16;  // pattern rows of the stencil table

template <typename T>
struct PerArgs {
  const T* u;
  const T* f;
  T* out;
  const uint8_t* pid;
  long long ldp;
  const T* ktab;
  const T* omd;
  double* part;
  long long per;
  int m, n, ld;
  long long bs;
  int mc, nc, ldc;
  long long bsc;
  int nstrips, ntr, rb;
  int B;  // the one-thread-per-node kernels' batch bound
};

// the own columns' table-row byte offsets (pad bytes are clamped to a row of the table; their results are masked)
template <typename T, int V>
__device__ __forceinline__ PRow<V> per_pids(const uint8_t* __restrict__ pp, int cl, int n) {
  PRow<V> p;
  int o[V];
#pragma unroll
  for (int k = 0; k < V; ++k) o[k] = 0;
  if (cl < n) pload<V>(pp + cl, o);
#pragma unroll
  for (int k = 0; k < V + 3; ++k) p.a[k] = 0;
#pragma unroll
  for (int k = 0; k < V; ++k) p.a[k + 1] = (o[k] & (kPerTab - 1)) * tab_row_bytes<T>();
  return p;
}

// SWEEP: out = u + omd (f - K u) (ZERO: omd f); else y = K u, PART: with the partials of u . y and of sum y
template <typename T, bool SWEEP, bool ZERO, bool PART>
__global__ __launch_bounds__(256) void k_per_stencil(PerArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  __shared__ T tab[kPerTab * kTabStride];
  load_tables<T>(tab, g.ktab, g.omd, kPerTab, (T*)nullptr, (const T*)nullptr, 0);
  __syncthreads();
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const TorusTask k = torus_task<T>(id, g.m, g.n, g.rb);
  const int m = g.m, n = g.n, ld = g.ld, cl = k.cl;
  const T ks[9] = {};
  T* __restrict__ ob = g.out + (long long)k.b * g.bs;
  double s0 = 0.0, s1 = 0.0;
  if constexpr (ZERO) {
    const T* __restrict__ fb = g.f + (long long)k.b * g.bs;
    for (int r = k.r0; r < k.r1; ++r) {
      T fv[V], o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) fv[j] = T(0);
      if (cl < n) vload<T, V>(fb + (long long)r * ld + cl, fv);
      const PRow<V> pb = per_pids<T, V>(g.pid + (long long)r * g.ldp, cl, n);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = tabv(tab, pb.a[j + 1], 9) * fv[j];
      if (cl < n) torus_store<T, V>(ob + (long long)r * ld + cl, o, cl, n);
    }
  } else {
    const T* __restrict__ ub = g.u + (long long)k.b * g.bs;
    auto rowp = [&](int r) { return ub + (long long)torus_wrap(r, m) * ld; };
    Row<T, V> wa = torus_window<T, V>(torus_load<T, V>(rowp(k.r0 - 1), cl, k.cL, n, k.lane), cl, n);
    Row<T, V> wb = torus_window<T, V>(torus_load<T, V>(rowp(k.r0), cl, k.cL, n, k.lane), cl, n);
    TorusRaw<T, V> rc = torus_load<T, V>(rowp(k.r0 + 1), cl, k.cL, n, k.lane);
    for (int r = k.r0; r < k.r1; ++r) {
      // (behind the task's last row: the row is loaded again and never used)
      const TorusRaw<T, V> rd = torus_load<T, V>(rowp(min(r + 2, k.r1)), cl, k.cL, n, k.lane);
      T fv[V], o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) fv[j] = T(0);
      if constexpr (SWEEP)
        if (cl < n) vload<T, V>(g.f + (long long)k.b * g.bs + (long long)r * ld + cl, fv);
      const PRow<V> pb = per_pids<T, V>(g.pid + (long long)r * g.ldp, cl, n);
      const Row<T, V> wc = torus_window<T, V>(rc, cl, n);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if constexpr (SWEEP) o[j] = jacobi<T, V, true>(wa, wb, wc, pb, pb, pb, j, fv[j], ks, T(0), tab);
        else o[j] = kapply<T, V, true>(wa, wb, wc, pb, pb, pb, j, ks, tab);
        if constexpr (PART) {
          const bool in = cl + j < n;
          s0 += in ? (double)wb.a[j + 1] * (double)o[j] : 0.0;
          s1 += in ? (double)o[j] : 0.0;
        }
      }
      if (cl < n) torus_store<T, V>(ob + (long long)r * ld + cl, o, cl, n);
      wa = wb;
      wb = wc;
      rc = rd;
    }
  }
  if constexpr (PART) {
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (k.lane == 0) {
      const long long slot = (long long)k.b * 2 * g.per + (long long)k.t * g.nstrips + k.s;
      g.part[slot] = s0;
      g.part[slot + g.per] = s1;
    }
  }
}

// partials of a . b (DOT) or of sum a over the task's nodes; a = g.u, b = g.f
template <typename T, bool DOT>
__global__ __launch_bounds__(256) void k_per_reduce(PerArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const TorusTask k = torus_task<T>(id, g.m, g.n, g.rb);
  const int n = g.n, cl = k.cl;
  double s = 0.0;
  for (int r = k.r0; r < k.r1; ++r) {
    const long long o = (long long)k.b * g.bs + (long long)r * g.ld + cl;
    T a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = T(0);
    if (cl < n) {
      vload<T, V>(g.u + o, a);
      if constexpr (DOT) vload<T, V>(g.f + o, b);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double v = DOT ? (double)a[j] * (double)b[j] : (double)a[j];
      s += cl + j < n ? v : 0.0;
    }
  }
  s = wave_sum(s);
  if (k.lane == 0) g.part[(long long)k.b * g.per + (long long)k.t * g.nstrips + k.s] = s;
}

// (f - K u) at node (r, c), wrapped indices, the taps in kapply's order
template <typename T, bool ZERO>
__device__ __forceinline__ T per_residual_at(const PerArgs<T>& g, const T* __restrict__ ub, const T* __restrict__ fb,
                                             const T* tab, int r, int c) {
  const T fv = fb[(long long)r * g.ld + c];
  if constexpr (ZERO) return fv;
  const int pc = (g.pid[(long long)r * g.ldp + c] & (kPerTab - 1)) * tab_row_bytes<T>();
  const int ru = r == 0 ? g.m - 1 : r - 1, rd = r == g.m - 1 ? 0 : r + 1;
  const int cw = c == 0 ? g.n - 1 : c - 1, ce = c == g.n - 1 ? 0 : c + 1;
  const T* a = ub + (long long)ru * g.ld;
  const T* b = ub + (long long)r * g.ld;
  const T* d = ub + (long long)rd * g.ld;
  T acc = tabv(tab, pc, 8) * a[cw];
  acc += tabv(tab, pc, 7) * a[c];
  acc += tabv(tab, pc, 6) * a[ce];
  acc += tabv(tab, pc, 5) * b[cw];
  acc += tabv(tab, pc, 4) * b[c];
  acc += tabv(tab, pc, 3) * b[ce];
  acc += tabv(tab, pc, 2) * d[cw];
  acc += tabv(tab, pc, 1) * d[c];
  acc += tabv(tab, pc, 0) * d[ce];
  return fv - acc;
}

template <typename T, bool ZERO>
__global__ __launch_bounds__(256) void k_per_residual_restrict(PerArgs<T> g) {
  __shared__ T tab[kPerTab * kTabStride];
  load_tables<T>(tab, g.ktab, (const T*)nullptr, kPerTab, (T*)nullptr, (const T*)nullptr, 0);
  __syncthreads();
  TorusCoarse k;
  if (!torus_coarse(g, k)) return;
  const T* __restrict__ ub = ZERO ? nullptr : g.u + k.b * g.bs;
  const T* __restrict__ fb = g.f + k.b * g.bs;
  const T q = T(0.25), h = T(0.5);
  T acc = q * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r0, k.c0);
  acc += h * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r0, k.c1);
  acc += q * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r0, k.c2);
  acc += h * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r1, k.c0);
  acc += per_residual_at<T, ZERO>(g, ub, fb, tab, k.r1, k.c1);
  acc += h * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r1, k.c2);
  acc += q * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r2, k.c0);
  acc += h * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r2, k.c1);
  acc += q * per_residual_at<T, ZERO>(g, ub, fb, tab, k.r2, k.c2);
  g.out[k.b * g.bsc + (long long)k.I * g.ldc + k.J] = acc;
}

// u += R^T ec: one thread per fine node; ec = g.u (coarse), u = g.out (fine)
template <typename T>
__global__ __launch_bounds__(256) void k_per_prolong_add(PerArgs<T> g) {
  const long long per_b = (long long)g.m * g.n;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long b = i / per_b;
  if (b >= g.B) return;
  const long long rem = i - b * per_b;
  const int r = (int)(rem / g.n), c = (int)(rem - (long long)r * g.n);
  const int I0 = r >> 1, J0 = c >> 1;
  const int I1 = I0 + 1 == g.mc ? 0 : I0 + 1, J1 = J0 + 1 == g.nc ? 0 : J0 + 1;
  const T* __restrict__ e0 = g.u + b * g.bsc + (long long)I0 * g.ldc;
  const T* __restrict__ e1 = g.u + b * g.bsc + (long long)I1 * g.ldc;
  T e;
  if (!(r & 1)) e = (c & 1) ? T(0.5) * (e0[J0] + e0[J1]) : e0[J0];
  else e = (c & 1) ? T(0.25) * ((e0[J0] + e0[J1]) + (e1[J0] + e1[J1])) : T(0.5) * (e0[J0] + e1[J0]);
  T* up = g.out + b * g.bs + (long long)r * g.ld + c;
  *up = *up + e;
}

// One workgroup per quantity: its `per` partials, each thread its own in index order, then a fixed tree
// (the scheme of k_flux_final).
__global__ __launch_bounds__(256) void k_per_final(const double* __restrict__ part, long long per,
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

template <typename T>
static bool per_layout_ok(int m, int n, int ld, long long bs) { return torus_layout_ok<T>(m, n, ld, bs, 1); }
template <typename T>
static bool per_pid_ok(const uint8_t* pid, long long ldp, int n) {
  constexpr int V = Frame<T>::VEC;
  return pid && (uintptr_t)pid % 4 == 0 && ldp % 4 == 0 && ldp >= (long long)div_up(n, V) * V;
}

template <typename T>
static PerArgs<T> per_args(int m, int n, int ld, long long bs) {
  PerArgs<T> g{};
  torus_geom<T>(g, m, n, ld, bs);
  return g;
}

extern "C" long long fea_per_parts(int m, int n, int elem_size) {
  if (!torus_dim_ok(m, 1) || !torus_dim_ok(n, 1) || (elem_size != 4 && elem_size != 8)) return -1;
  return elem_size == 8 ? per_args<double>(m, n, 0, 0).per : per_args<float>(m, n, 0, 0).per;
}

template <typename T>
static int per_sweep(const T* u, const T* f, T* out, const uint8_t* pid, long long ldp, const T* ktab, const T* omd,
                     int B, int m, int n, int ld, long long bs, void* stream) {
  if (B < 1 || !per_layout_ok<T>(m, n, ld, bs) || !torus_aligned(f) || !torus_aligned(out) ||
      (u && !torus_aligned(u)) || !per_pid_ok<T>(pid, ldp, n) || !ktab || !omd)
    return FEA_EINVAL;
  const long long N = (long long)B * bs;
  if ((u && torus_overlap(u, N, out, N)) || torus_overlap(f, N, out, N)) return FEA_EINVAL;
  PerArgs<T> g = per_args<T>(m, n, ld, bs);
  g.u = u; g.f = f; g.out = out; g.pid = pid; g.ldp = ldp; g.ktab = ktab; g.omd = omd;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (u) k_per_stencil<T, true, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_per_stencil<T, true, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

template <typename T>
static int per_apply(const T* p, T* y, double* part, const uint8_t* pid, long long ldp, const T* ktab, int B, int m,
                     int n, int ld, long long bs, void* stream) {
  const long long N = (long long)B * bs;
  if (B < 1 || !per_layout_ok<T>(m, n, ld, bs) || !torus_aligned(p) || !torus_aligned(y) ||
      !per_pid_ok<T>(pid, ldp, n) || !ktab || torus_overlap(p, N, y, N))
    return FEA_EINVAL;
  PerArgs<T> g = per_args<T>(m, n, ld, bs);
  g.u = p; g.out = y; g.part = part; g.pid = pid; g.ldp = ldp; g.ktab = ktab;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (part) k_per_stencil<T, false, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_per_stencil<T, false, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

template <typename T>
static int per_reduce(const T* a, const T* b, double* part, int B, int m, int n, int ld, long long bs, void* stream) {
  if (B < 1 || !per_layout_ok<T>(m, n, ld, bs) || !torus_aligned(a) || (b && !torus_aligned(b)) || !part)
    return FEA_EINVAL;
  PerArgs<T> g = per_args<T>(m, n, ld, bs);
  g.u = a; g.f = b; g.part = part;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (b) k_per_reduce<T, true><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_per_reduce<T, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

template <typename T>
static int per_residual_restrict(const T* u, const T* f, T* fc, const uint8_t* pid, long long ldp, const T* ktab, int B,
                                 int m, int n, int ld, long long bs, int ldc, long long bsc, void* stream) {
  if (B < 1 || !per_layout_ok<T>(m, n, ld, bs) || (m & 1) || (n & 1) || !per_layout_ok<T>(m / 2, n / 2, ldc, bsc) ||
      !torus_aligned(f) || !torus_aligned(fc) || (u && !torus_aligned(u)) || !per_pid_ok<T>(pid, ldp, n) || !ktab)
    return FEA_EINVAL;
  PerArgs<T> g = per_args<T>(m, n, ld, bs);
  g.u = u; g.f = f; g.out = fc; g.pid = pid; g.ldp = ldp; g.ktab = ktab;
  g.mc = m / 2; g.nc = n / 2; g.ldc = ldc; g.bsc = bsc;
  dim3 grid;
  if (!torus_node_grid(B, (long long)g.mc * g.nc, grid)) return FEA_EINVAL;
  g.B = B;
  if (u) hipLaunchKernelGGL((k_per_residual_restrict<T, false>), grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((k_per_residual_restrict<T, true>), grid, dim3(256), 0, (hipStream_t)stream, g);
  return launch_status();
}

template <typename T>
static int per_prolong_add(const T* ec, T* u, int B, int m, int n, int ld, long long bs, int ldc, long long bsc,
                           void* stream) {
  if (B < 1 || !per_layout_ok<T>(m, n, ld, bs) || (m & 1) || (n & 1) || !per_layout_ok<T>(m / 2, n / 2, ldc, bsc) ||
      !torus_aligned(ec) || !torus_aligned(u))
    return FEA_EINVAL;
  PerArgs<T> g = per_args<T>(m, n, ld, bs);
  g.u = ec; g.out = u;
  g.mc = m / 2; g.nc = n / 2; g.ldc = ldc; g.bsc = bsc;
  dim3 grid;
  if (!torus_node_grid(B, (long long)m * n, grid)) return FEA_EINVAL;
  g.B = B;
  hipLaunchKernelGGL((k_per_prolong_add<T>), grid, dim3(256), 0, (hipStream_t)stream, g);
  return launch_status();
}

#define FEA_PER_API(SUF, T)                                                                                           \
  extern "C" int fea_per_sweep_##SUF(const T* u, const T* f, T* out, const uint8_t* pid, long long ldp, const T* ktab, \
                                     const T* omd, int B, int m, int n, int ld, long long bstride, void* stream) {    \
    return per_sweep<T>(u, f, out, pid, ldp, ktab, omd, B, m, n, ld, bstride, stream);                                \
  }                                                                                                                   \
  extern "C" int fea_per_residual_restrict_##SUF(const T* u, const T* f, T* fc, const uint8_t* pid, long long ldp,    \
                                                 const T* ktab, int B, int m, int n, int ld, long long bstride,       \
                                                 int ldc, long long bstridec, void* stream) {                         \
    return per_residual_restrict<T>(u, f, fc, pid, ldp, ktab, B, m, n, ld, bstride, ldc, bstridec, stream);           \
  }                                                                                                                   \
  extern "C" int fea_per_prolong_add_##SUF(const T* ec, T* u, int B, int m, int n, int ld, long long bstride,         \
                                           int ldc, long long bstridec, void* stream) {                               \
    return per_prolong_add<T>(ec, u, B, m, n, ld, bstride, ldc, bstridec, stream);                                    \
  }                                                                                                                   \
  extern "C" int fea_per_apply_##SUF(const T* p, T* y, double* part, const uint8_t* pid, long long ldp,               \
                                     const T* ktab, int B, int m, int n, int ld, long long bstride, void* stream) {   \
    return per_apply<T>(p, y, part, pid, ldp, ktab, B, m, n, ld, bstride, stream);                                    \
  }                                                                                                                   \
  extern "C" int fea_per_reduce_##SUF(const T* a, const T* b, double* part, int B, int m, int n, int ld,              \
                                      long long bstride, void* stream) {                                              \
    return per_reduce<T>(a, b, part, B, m, n, ld, bstride, stream);                                                   \
  }
FEA_PER_API(f32, float)
FEA_PER_API(f64, double)

extern "C" int fea_per_final(const double* part, long long per, double* sums, int count, void* stream) {
  if (!part || !sums || per < 1 || count < 1) return FEA_EINVAL;
  k_per_final<<<count, 256, 0, (hipStream_t)stream>>>(part, per, sums);
  return launch_status();
}
