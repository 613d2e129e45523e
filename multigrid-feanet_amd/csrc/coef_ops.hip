// coef_ops.hip — the matrix-free multigrid kernels on a torus whose elements each carry their own coefficient
// (include/feanet_coef.h; definitions: DESIGN §19).
//
//   sweep              out = u + (omega / d) (f - K u), or (omega / d) f from the zero guess
//   apply              y = K p, optionally with the partials of p . y and of sum y
//   residual_restrict  fc = R (f - K u), the residual stays in registers
//   coarsen            kc = the mean of each 2 x 2 block of k under one of three rules
//
// Layout and decomposition are periodic_ops.hip's: [B, m, ld] without a ghost ring, a wave owns a strip of 64 * VEC
// node columns and a task of rb rows (the row tasks ONE sample gets), a lane owns VEC columns, three node rows sit in
// a register window that marches down and the row after the next is loaded before the arithmetic; left and right
// neighbours come by DPP, the columns next to the strip and column 0 are explicit loads.  Next to the node window
// marches a two-row window of k: the element rows r - 1 and r of node row r, one new vector load per node row.  A node
// needs the elements of its own column and of the column to the west, so the west element comes by DPP from the lane
// on the left and lane 0 loads column cl - 1 (n - 1 at column 0); no east value and no column 0 of k is needed.
// There is no table, no LDS, no atomics.  K u is coef_apply() everywhere (sweep, apply, residual_restrict), one source
// expression, so a value is the same bits at every task height and in any batch.  Pad columns of u, f and k are loaded
// with their vector but every value computed from them is selected out; nothing outside the m x n nodes is written.
// residual_restrict takes one thread per coarse node with modulo indexing, as fea_per_residual_restrict does.
#include "framed_strip.h"
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

// one node row of a lane: x = own columns, hl / hr = the strip's outer neighbours (lanes 0 / 63), w0 = column 0
template <typename T, int V>
struct CoefRaw {
  T x[V];
  T hl, hr, w0;
};

template <typename T, int V>
__device__ __forceinline__ CoefRaw<T, V> coef_load(const T* __restrict__ rp, int cl, int cL, int n, int lane) {
  CoefRaw<T, V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.x[k] = T(0);
  if (cl < n) vload<T, V>(rp + cl, r.x);  // columns cl .. cl+V-1 <= ld-1 (ld a multiple of V)
  r.hl = T(0);
  r.hr = T(0);
  if (lane == 0) r.hl = rp[cL];  // exec-masked scalar loads
  if (lane == kWave - 1 && cl + V < n) r.hr = rp[cl + V];
  r.w0 = rp[0];
  return r;
}

// the node window row: a[0] = left of the first own column, a[1 .. V] own, a[V+1] = right of the last own column; the
// right neighbour of column n-1 is column 0
template <typename T, int V>
__device__ __forceinline__ Row<T, V> coef_window(const CoefRaw<T, V>& r, int cl, int n) {
  Row<T, V> w;
#pragma unroll
  for (int k = 0; k < V; ++k) w.a[k + 1] = r.x[k];
  w.a[0] = shr1(r.x[V - 1], r.hl);
  w.a[V + 1] = shl1(r.x[0], r.hr);
  w.a[V + 2] = T(0);
#pragma unroll
  for (int k = 0; k < V; ++k)
    if (cl + k == n - 1) w.a[k + 2] = r.w0;
  return w;
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

template <typename T, int V>
__device__ __forceinline__ void coef_store(T* p, const T (&o)[V], int cl, int n) {
  if (cl + V <= n) {
    vstore<T, V, false>(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (cl + k < n) p[k] = o[k];
  }
}

__device__ __forceinline__ int coef_wrap(int r, int m) { return r < 0 ? r + m : (r >= m ? r - m : r); }

// SWEEP: out = u + (omega / d) (f - K u) (ZERO: (omega / d) f); else y = K u, PART: with the partials of u . y and of
// sum y
template <typename T, bool SWEEP, bool ZERO, bool PART>
__global__ __launch_bounds__(256) void k_coef_stencil(CoefArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int m = g.m, n = g.n, ld = g.ld, lane = lane_id();
  const int r0 = id.t * g.rb, r1 = min(r0 + g.rb, m);
  const int cl = id.s * F::SW + V * lane;
  const int cL = (cl == 0 ? n : cl) - 1;  // only lane 0 reads it: cl < n there
  T* __restrict__ ob = g.out + (long long)id.b * g.bs;
  auto krowp = [&](int r) { return g.k + (long long)coef_wrap(r, m) * g.ldk; };
  KRow<T, V> ka = coef_kwindow<T, V>(coef_kload<T, V>(krowp(r0 - 1), cl, cL, n, lane));
  KRaw<T, V> kr = coef_kload<T, V>(krowp(r0), cl, cL, n, lane);
  double s0 = 0.0, s1 = 0.0;
  if constexpr (ZERO) {
    const T* __restrict__ fb = g.f + (long long)id.b * g.bs;
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
      if (cl < n) coef_store<T, V>(ob + (long long)r * ld + cl, o, cl, n);
      ka = kb;
      kr = kn;
    }
  } else {
    const T* __restrict__ ub = g.u + (long long)id.b * g.bs;
    auto rowp = [&](int r) { return ub + (long long)coef_wrap(r, m) * ld; };
    Row<T, V> wa = coef_window<T, V>(coef_load<T, V>(rowp(r0 - 1), cl, cL, n, lane), cl, n);
    Row<T, V> wb = coef_window<T, V>(coef_load<T, V>(rowp(r0), cl, cL, n, lane), cl, n);
    CoefRaw<T, V> rc = coef_load<T, V>(rowp(r0 + 1), cl, cL, n, lane);
    for (int r = r0; r < r1; ++r) {
      // (behind the task's last row: the rows are loaded again and never used)
      const CoefRaw<T, V> rd = coef_load<T, V>(rowp(min(r + 2, r1)), cl, cL, n, lane);
      const KRaw<T, V> kn = coef_kload<T, V>(krowp(min(r + 1, r1)), cl, cL, n, lane);
      T fv[V], o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) fv[j] = T(0);
      if constexpr (SWEEP)
        if (cl < n) vload<T, V>(g.f + (long long)id.b * g.bs + (long long)r * ld + cl, fv);
      const Row<T, V> wc = coef_window<T, V>(rc, cl, n);
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
      if (cl < n) coef_store<T, V>(ob + (long long)r * ld + cl, o, cl, n);
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
      const long long slot = (long long)id.b * 2 * g.per + (long long)id.t * g.nstrips + id.s;
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
  const long long per_b = (long long)g.mc * g.nc;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long b = i / per_b;
  if (b >= g.B) return;
  const long long rem = i - b * per_b;
  const int I = (int)(rem / g.nc), J = (int)(rem - (long long)I * g.nc);
  const T* __restrict__ ub = ZERO ? nullptr : g.u + b * g.bs;
  const T* __restrict__ fb = g.f + b * g.bs;
  const int r1 = 2 * I, c1 = 2 * J;
  const int r0 = r1 == 0 ? g.m - 1 : r1 - 1, r2 = r1 + 1;  // m, n even: 2 I + 1 <= m - 1
  const int c0 = c1 == 0 ? g.n - 1 : c1 - 1, c2 = c1 + 1;
  const T q = T(0.25), h = T(0.5);
  T acc = q * coef_residual_at<T, ZERO>(g, ub, fb, r0, c0);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, r0, c1);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, r0, c2);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, r1, c0);
  acc += coef_residual_at<T, ZERO>(g, ub, fb, r1, c1);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, r1, c2);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, r2, c0);
  acc += h * coef_residual_at<T, ZERO>(g, ub, fb, r2, c1);
  acc += q * coef_residual_at<T, ZERO>(g, ub, fb, r2, c2);
  g.out[b * g.bsc + (long long)I * g.ldc + J] = acc;
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

static inline bool coef_dim_ok(int n) { return n >= 2 && n <= (1 << 20); }

template <typename T>
static bool coef_layout_ok(int m, int n, int ld, long long bs) {
  constexpr int V = Frame<T>::VEC;
  return coef_dim_ok(m) && coef_dim_ok(n) && ld >= n && ld % V == 0 && bs >= (long long)m * ld && bs % V == 0;
}
static inline bool coef_aligned(const void* p) { return p && (uintptr_t)p % 16 == 0; }
template <typename T>
static bool coef_k_ok(const T* k, long long ldk, int n) {
  return coef_aligned(k) && ldk >= n && ldk % Frame<T>::VEC == 0;
}
// two ranges of na and nb elements of T
template <typename T>
static bool coef_overlap(const T* a, long long na, const T* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(T);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(T);
  return a0 < b1 && b0 < a1;
}

// strips over the node columns 0 .. n-1, row tasks of the height ONE sample gets: fea_per_parts' rule
template <typename T>
static CoefArgs<T> coef_args(int m, int n, int ld, long long bs, const T* k, long long ldk) {
  CoefArgs<T> g{};
  g.m = m; g.n = n; g.ld = ld; g.bs = bs; g.k = k; g.ldk = ldk;
  g.nstrips = div_up(n, Frame<T>::SW);
  g.rb = pick_rb(1, g.nstrips, m);
  g.ntr = div_up(m, g.rb);
  g.per = (long long)g.nstrips * g.ntr;
  return g;
}

template <typename T>
static int coef_sweep(const T* u, const T* f, T* out, const T* k, long long ldk, double omega, int B, int m, int n,
                      int ld, long long bs, void* stream) {
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || !coef_aligned(f) || !coef_aligned(out) ||
      (u && !coef_aligned(u)) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs;
  if ((u && coef_overlap(u, N, out, N)) || coef_overlap(f, N, out, N)) return FEA_EINVAL;
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
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || !coef_aligned(p) || !coef_aligned(y) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs;
  if (coef_overlap(p, N, y, N)) return FEA_EINVAL;
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
  if (B < 1 || !coef_layout_ok<T>(m, n, ld, bs) || (m & 1) || (n & 1) || ldc < n / 2 || ldc % Frame<T>::VEC ||
      bsc < (long long)(m / 2) * ldc || bsc % Frame<T>::VEC || !coef_aligned(f) || !coef_aligned(fc) ||
      (u && !coef_aligned(u)) || !coef_k_ok<T>(k, ldk, n))
    return FEA_EINVAL;
  const long long N = (long long)B * bs, Nc = (long long)B * bsc;
  if ((u && coef_overlap(u, N, fc, Nc)) || coef_overlap(f, N, fc, Nc)) return FEA_EINVAL;
  CoefArgs<T> g = coef_args<T>(m, n, ld, bs, k, ldk);
  g.u = u; g.f = f; g.out = fc;
  g.mc = m / 2; g.nc = n / 2; g.ldc = ldc; g.bsc = bsc;
  const long long blocks = ((long long)B * g.mc * g.nc + 255) / 256;
  if (blocks > 0x7fffffffll) return FEA_EINVAL;
  g.B = B;
  const dim3 grid((unsigned)blocks);
  if (u) hipLaunchKernelGGL((k_coef_residual_restrict<T, false>), grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((k_coef_residual_restrict<T, true>), grid, dim3(256), 0, (hipStream_t)stream, g);
  return launch_status();
}

template <typename T>
static int coef_coarsen(const T* k, long long ldk, T* kc, long long ldkc, int m, int n, int rule, void* stream) {
  if (!coef_dim_ok(m) || !coef_dim_ok(n) || (m & 1) || (n & 1) || !coef_k_ok<T>(k, ldk, n) ||
      !coef_k_ok<T>(kc, ldkc, n / 2) || rule < FEA_COEF_ARITHMETIC || rule > FEA_COEF_GEOMETRIC)
    return FEA_EINVAL;
  if (coef_overlap(k, (long long)m * ldk, kc, (long long)(m / 2) * ldkc)) return FEA_EINVAL;
  const long long blocks = ((long long)(m / 2) * (n / 2) + 255) / 256;
  if (blocks > 0x7fffffffll) return FEA_EINVAL;
  hipLaunchKernelGGL((k_coef_coarsen<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k, ldk, kc, ldkc,
                     m / 2, n / 2, rule);
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
