// coef_ops.hip — the matrix-free multigrid kernels on a torus whose elements each carry their own coefficient
// (include/feanet_coef.h; definitions: DESIGN §19).
//
//   sweep              out = u + (omega / d) (f - K u), or (omega / d) f from the zero guess
//   apply              y = K p, optionally with the partials of p . y and of sum y
//   residual_restrict  fc = R (f - K u), the residual stays in registers
//   coarsen            kc = the mean of each 2 x 2 block of k under one of three rules
//
// Layout, decomposition, row helpers, task decoding and the host checks: torus_strip.h.  What is this file's own: next
// to the node window marches a two-row window of k, the element rows r - 1 and r of node row r, one new vector load per
// node row.  A node needs the elements of its own column and of the column to the west, so the west element comes by
// DPP from the lane on the left and lane 0 loads column cl - 1 (n - 1 at column 0); no east value and no column 0 of
// k is needed.  There is no table, no LDS, no atomics.  K u is coef_apply() everywhere (sweep, apply,
// residual_restrict), one source expression, so a value is the same bits at every task height and in any batch.  Pad
// columns of k are loaded with their vector like those of u and f, and every value computed from them is selected out.
#include "torus_strip.h"
#include "feanet_coef.h"

namespace fea {

template <typename T>
struct CoefArgs {
  const T* u;
  const T* f;
  T* out;
  const T* k;
  long long ldk;
  T omega;
  double* part;
  long long per;
  int m, n, ld;
  long long bs;
  int mc, nc, ldc;
  long long bsc;
  int nstrips, ntr, rb;
  int B;  // the one-thread-per-node kernel's batch bound
};

// (K u) at a node from its value c, its eight neighbours and its four elements: the one expression of DESIGN §19
template <typename T>
__device__ __forceinline__ T coef_apply(T c, T n, T s, T w, T e, T nw, T ne, T sw, T se, T knw, T kne, T ksw, T kse) {
  const T dn = c - n, ds = c - s, dw = c - w, de = c - e;
  const T dnw = c - nw, dne = c - ne, dsw = c - sw, dse = c - se;
  const T tnw = (dn + dw) + T(2) * dnw;
  const T tne = (dn + de) + T(2) * dne;
  const T tsw = (ds + dw) + T(2) * dsw;
  const T tse = (ds + de) + T(2) * dse;
  constexpr T sixth = T(1) / T(6);
  return ((knw * tnw + kne * tne) + (ksw * tsw + kse * tse)) * sixth;
}

// omega / d of a node, d = (2/3) ((k_NW + k_NE) + (k_SW + k_SE)): the one division of a swept node
template <typename T>
__device__ __forceinline__ T coef_omd(T omega, T knw, T kne, T ksw, T kse) {
  constexpr T two3 = T(2) / T(3);
  const T d = two3 * ((knw + kne) + (ksw + kse));
  return omega / d;
}

// one element row of a lane: a[0] = the element west of the first own column, a[1 .. V] the own columns' elements
template <typename T, int V>
struct KRow {
  T a[V + 1];
};
template <typename T, int V>
struct KRaw {
  T x[V];
  T hl;
};

template <typename T, int V>
__device__ __forceinline__ KRaw<T, V> coef_kload(const T* __restrict__ kp, int cl, int cL, int n, int lane) {
  KRaw<T, V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.x[k] = T(0);
  if (cl < n) vload<T, V>(kp + cl, r.x);  // columns cl .. cl+V-1 <= ldk-1 (ldk a multiple of V)
  r.hl = T(0);
  if (lane == 0) r.hl = kp[cL];
  return r;
}

template <typename T, int V>
__device__ __forceinline__ KRow<T, V> coef_kwindow(const KRaw<T, V>& r) {
  KRow<T, V> w;
#pragma unroll
  for (int k = 0; k < V; ++k) w.a[k + 1] = r.x[k];
  w.a[0] = shr1(r.x[V - 1], r.hl);
  return w;
}

// SWEEP: out = u + (omega / d) (f - K u) (ZERO: (omega / d) f); else y = K u, PART: with the partials of u . y and of
// sum y
template <typename T, bool SWEEP, bool ZERO, bool PART>
__global__ __launch_bounds__(256) void k_coef_stencil(CoefArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const TorusTask t = torus_task<T>(id, g.m, g.n, g.rb);
  const int m = g.m, n = g.n, ld = g.ld, lane = t.lane, r0 = t.r0, r1 = t.r1, cl = t.cl, cL = t.cL;
  T* __restrict__ ob = g.out + (long long)t.b * g.bs;
  auto krowp = [&](int r) { return g.k + (long long)torus_wrap(r, m) * g.ldk; };
  KRow<T, V> ka = coef_kwindow<T, V>(coef_kload<T, V>(krowp(r0 - 1), cl, cL, n, lane));
  KRaw<T, V> kr = coef_kload<T, V>(krowp(r0), cl, cL, n, lane);
  double s0 = 0.0, s1 = 0.0;
  if constexpr (ZERO) {
    const T* __restrict__ fb = g.f + (long long)t.b * g.bs;
    for (int r = r0; r < r1; ++r) {
      // (behind the task's last row: the row is loaded again and never used)
      const KRaw<T, V> kn = coef_kload<T, V>(krowp(min(r + 1, r1)), cl, cL, n, lane);
      T fv[V], o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) fv[j] = T(0);
      if (cl < n) vload<T, V>(fb + (long long)r * ld + cl, fv);
      const KRow<T, V> kb = coef_kwindow<T, V>(kr);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = coef_omd<T>(g.omega, ka.a[j], ka.a[j + 1], kb.a[j], kb.a[j + 1]) * fv[j];
      if (cl < n) torus_store<T, V>(ob + (long long)r * ld + cl, o, cl, n);
      ka = kb;
      kr = kn;
    }
  } else {
    const T* __restrict__ ub = g.u + (long long)t.b * g.bs;
    auto rowp = [&](int r) { return ub + (long long)torus_wrap(r, m) * ld; };
    Row<T, V> wa = torus_window<T, V>(torus_load<T, V>(rowp(r0 - 1), cl, cL, n, lane), cl, n);
    Row<T, V> wb = torus_window<T, V>(torus_load<T, V>(rowp(r0), cl, cL, n, lane), cl, n);
    TorusRaw<T, V> rc = torus_load<T, V>(rowp(r0 + 1), cl, cL, n, lane);
    for (int r = r0; r < r1; ++r) {
      // (behind the task's last row: the rows are loaded again and never used)
      const TorusRaw<T, V> rd = torus_load<T, V>(rowp(min(r + 2, r1)), cl, cL, n, lane);
      const KRaw<T, V> kn = coef_kload<T, V>(krowp(min(r + 1, r1)), cl, cL, n, lane);
      T fv[V], o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) fv[j] = T(0);
      if constexpr (SWEEP)
        if (cl < n) vload<T, V>(g.f + (long long)t.b * g.bs + (long long)r * ld + cl, fv);
      const Row<T, V> wc = torus_window<T, V>(rc, cl, n);
      const KRow<T, V> kb = coef_kwindow<T, V>(kr);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T acc = coef_apply<T>(wb.a[j + 1], wa.a[j + 1], wc.a[j + 1], wb.a[j], wb.a[j + 2], wa.a[j], wa.a[j + 2],
                                    wc.a[j], wc.a[j + 2], ka.a[j], ka.a[j + 1], kb.a[j], kb.a[j + 1]);
        if constexpr (SWEEP) {
          const T w = coef_omd<T>(g.omega, ka.a[j], ka.a[j + 1], kb.a[j], kb.a[j + 1]);
          o[j] = w * (fv[j] - acc) + wb.a[j + 1];
        } else {
          o[j] = acc;
        }
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
      ka = kb;
      kr = kn;
    }
  }
  if constexpr (PART) {
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) {
      const long long slot = (long long)t.b * 2 * g.per + (long long)t.t * g.nstrips + t.s;
      g.part[slot] = s0;
      g.part[slot + g.per] = s1;
    }
  }
}

// (f - K u) at node (r, c), wrapped indices
template <typename T, bool ZERO>
__device__ __forceinline__ T coef_residual_at(const CoefArgs<T>& g, const T* __restrict__ ub,
                                              const T* __restrict__ fb, int r, int c) {
  const T fv = fb[(long long)r * g.ld + c];
  if constexpr (ZERO) return fv;
  const int ru = r == 0 ? g.m - 1 : r - 1, rd = r == g.m - 1 ? 0 : r + 1;
  const int cw = c == 0 ? g.n - 1 : c - 1, ce = c == g.n - 1 ? 0 : c + 1;
  const T* a = ub + (long long)ru * g.ld;
  const T* b = ub + (long long)r * g.ld;
  const T* d = ub + (long long)rd * g.ld;
  const T* ka = g.k + (long long)ru * g.ldk;
  const T* kb = g.k + (long long)r * g.ldk;
  const T acc = coef_apply<T>(b[c], a[c], d[c], b[cw], b[ce], a[cw], a[ce], d[cw], d[ce], ka[cw], ka[c], kb[cw], kb[c]);
  return fv - acc;
}

template <typename T, bool ZERO>
__global__ __launch_bounds__(256) void k_coef_residual_restrict(CoefArgs<T> g) {
  TorusCoarse k;
  if (!torus_coarse(g, k)) return;
  const T* __restrict__ ub = ZERO ? nullptr : g.u + k.b * g.bs;
  const T* __restrict__ fb = g.f + k.b * g.bs;
  const T q = T(0.25), h = T(0.5);
  T acc = q * coef_residual_at<T, ZERO>(g, ub, fb, k.r0, k.c0);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, k.r0, k.c1);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, k.r0, k.c2);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, k.r1, k.c0);
  acc += coef_residual_at<T, ZERO>(g, ub, fb, k.r1, k.c1);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, k.r1, k.c2);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, k.r2, k.c0);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, k.r2, k.c1);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, k.r2, k.c2);
  g.out[k.b * g.bsc + (long long)k.I * g.ldc + k.J] = acc;
}

// one thread per coarse element
template <typename T>
__global__ __launch_bounds__(256) void k_coef_coarsen(const T* __restrict__ k, long long ldk, T* __restrict__ kc,
                                                      long long ldkc, int mc, int nc, int rule) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)mc * nc) return;
  const int I = (int)(i / nc), J = (int)(i - (long long)I * nc);
  const T* p = k + (long long)(2 * I) * ldk + 2 * J;
  const T a = p[0], b = p[1], c = p[ldk], d = p[ldk + 1];
  T v;
  if (rule == FEA_COEF_ARITHMETIC) {
    v = ((a + b) + (c + d)) * T(0.25);
  } else if (rule == FEA_COEF_HARMONIC) {
    v = (T)(4.0 / ((1.0 / (double)a + 1.0 / (double)b) + (1.0 / (double)c + 1.0 / (double)d)));
  } else {
    v = (T)exp(((log((double)a) + log((double)b)) + (log((double)c) + log((double)d))) * 0.25);
  }
  kc[(long long)I * ldkc + J] = v;
}

}  // namespace fea

template <typename T>
static bool coef_layout_ok(int m, int n, int ld, long long bs) { return torus_layout_ok<T>(m, n, ld, bs, 2); }
template <typename T>
static bool coef_k_ok(const T* k, long long ldk, int n) {
  return torus_aligned(k) && ldk >= n && ldk % Frame<T>::VEC == 0;
}

template <typename T>
static CoefArgs<T> coef_args(int m, int n, int ld, long long bs, const T* k, long long ldk) {
  CoefArgs<T> g{};
  torus_geom<T>(g, m, n, ld, bs);
  g.k = k; g.ldk = ldk;
  return g;
}

template <typename T>
static int coef_sweep(const T* u, const T* f, T* out, const T* k, long long ldk, double omega, int B, int m, int n,
                      int ld, long long bs, void* stream) {
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || !torus_aligned(f) || !torus_aligned(out) ||
      (u && !torus_aligned(u)) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs;
  if ((u && torus_overlap(u, N, out, N)) || torus_overlap(f, N, out, N)) return FEA_EINVAL;
  CoefArgs<T> g = coef_args<T>(m, n, ld, bs, k, ldk);
  g.u = u; g.f = f; g.out = out; g.omega = (T)omega;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (u) k_coef_stencil<T, true, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_coef_stencil<T, true, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

template <typename T>
static int coef_apply_launch(const T* p, T* y, double* part, const T* k, long long ldk, int B, int m, int n, int ld,
                             long long bs, void* stream) {
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || !torus_aligned(p) || !torus_aligned(y) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs;
  if (torus_overlap(p, N, y, N)) return FEA_EINVAL;
  CoefArgs<T> g = coef_args<T>(m, n, ld, bs, k, ldk);
  g.u = p; g.out = y; g.part = part;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (part) k_coef_stencil<T, false, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_coef_stencil<T, false, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

template <typename T>
static int coef_residual_restrict(const T* u, const T* f, T* fc, const T* k, long long ldk, int B, int m, int n, int ld,
                                  long long bs, int ldc, long long bsc, void* stream) {
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || (m & 1) || (n & 1) ||
      !torus_layout_ok<T>(m / 2, n / 2, ldc, bsc, 1) || !torus_aligned(f) || !torus_aligned(fc) ||
      (u && !torus_aligned(u)) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs, Nc = (long long)B * bsc;
  if ((u && torus_overlap(u, N, fc, Nc)) || torus_overlap(f, N, fc, Nc)) return FEA_EINVAL;
  CoefArgs<T> g = coef_args<T>(m, n, ld, bs, k, ldk);
  g.u = u; g.f = f; g.out = fc;
  g.mc = m / 2; g.nc = n / 2; g.ldc = ldc; g.bsc = bsc;
  dim3 grid;
  if (!torus_node_grid(B, (long long)g.mc * g.nc, grid)) return FEA_EINVAL;
  g.B = B;
  if (u) hipLaunchKernelGGL((k_coef_residual_restrict<T, false>), grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((k_coef_residual_restrict<T, true>), grid, dim3(256), 0, (hipStream_t)stream, g);
  return launch_status();
}

template <typename T>
static int coef_coarsen(const T* k, long long ldk, T* kc, long long ldkc, int m, int n, int rule, void* stream) {
  if (!torus_dim_ok(m, 2) || !torus_dim_ok(n, 2) || (m & 1) || (n & 1) || !coef_k_ok<T>(k, ldk, n) ||
      !coef_k_ok<T>(kc, ldkc, n / 2) || rule < FEA_COEF_ARITHMETIC || rule > FEA_COEF_GEOMETRIC)
    return FEA_EINVAL;
  if (torus_overlap(k, (long long)m * ldk, kc, (long long)(m / 2) * ldkc)) return FEA_EINVAL;
  dim3 grid;
  if (!torus_node_grid(1, (long long)(m / 2) * (n / 2), grid)) return FEA_EINVAL;
  hipLaunchKernelGGL((k_coef_coarsen<T>), grid, dim3(256), 0, (hipStream_t)stream, k, ldk, kc, ldkc, m / 2, n / 2,
                     rule);
  return launch_status();
}

#define FEA_COEF_API(SUF, T)                                                                                          \
  extern "C" int fea_coef_sweep_##SUF(const T* u, const T* f, T* out, const T* k, long long ldk, double omega, int B, \
                                      int m, int n, int ld, long long bstride, void* stream) {                        \
    return coef_sweep<T>(u, f, out, k, ldk, omega, B, m, n, ld, bstride, stream);                                     \
  }                                                                                                                   \
  extern "C" int fea_coef_apply_##SUF(const T* p, T* y, double* part, const T* k, long long ldk, int B, int m, int n, \
                                      int ld, long long bstride, void* stream) {                                      \
    return coef_apply_launch<T>(p, y, part, k, ldk, B, m, n, ld, bstride, stream);                                    \
  }                                                                                                                   \
  extern "C" int fea_coef_residual_restrict_##SUF(const T* u, const T* f, T* fc, const T* k, long long ldk, int B,    \
                                                  int m, int n, int ld, long long bstride, int ldc,                   \
                                                  long long bstridec, void* stream) {                                 \
    return coef_residual_restrict<T>(u, f, fc, k, ldk, B, m, n, ld, bstride, ldc, bstridec, stream);                  \
  }                                                                                                                   \
  extern "C" int fea_coef_coarsen_##SUF(const T* k, long long ldk, T* kc, long long ldkc, int m, int n, int rule,     \
                                        void* stream) {                                                               \
    return coef_coarsen<T>(k, ldk, kc, ldkc, m, n, rule, stream);                                                     \
  }
FEA_COEF_API(f32, float)
FEA_COEF_API(f64, double)
