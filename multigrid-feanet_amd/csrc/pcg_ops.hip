// pcg_ops.hip — Krylov vector operations of the multigrid-preconditioned conjugate gradient (feanet_amd.pcg) on
// level-0 FRAMED buffers (layout and strip x row-march decomposition: framed_ops.hip / framed_strip.h).
//
//   residual   r = f - K x                         (interior; boundary nodes of r zeroed)      + partials of r.r
//   dot        partials of r.z                                                                 16 B / fp64 node
//   direction  p_out = z + beta p_in               (interior; p ping-pongs)                    + partials of p.Kp, 24 B
//   update     x += alpha p,  r -= alpha K p       (in place, pointwise; K p recomputed)       + partials of r.r, 40 B
//   scalar     one workgroup per sample sums its partials in index order and advances the sample's scalar block
//              (FEA_PCG_*: rz, pAp, alpha, beta, ||r||, done flag, iteration count, history row)
//
// K acts on interior nodes with kapply (the tap order and mirrored table reads of the cycle kernels), so K p is the
// same bits as the residual the V-cycle forms.  The direction kernel rebuilds the new direction on its window's halo
// columns and rows from z and p_in (same expression as the stored value, -ffp-contract=on), which is why p_out must
// not be p_in.  Every wave writes one partial sum (double, fixed butterfly order) to
// part[(b * ntr + t) * nstrips + s]; the task height is chosen as for one sample, so a sample's partial set — and
// with it every reduced scalar — is the same bits whatever the batch it runs in.  No atomics, nothing allocates or
// synchronises, safe under stream capture.
//
// Mixed precision (fea_pcg_*_f64f32): the Krylov state stays in fp64, the preconditioner runs on an fp32 framed
// hierarchy.  The same fp64 task grid addresses the fp32 level-0 field through Frame<float>::OFF and its own ld / bs
// (column 1 of both frames is 128-byte aligned; a lane's two columns are one aligned 8-byte access there):
//   narrow     r32 = float(r s_b)                  (interior; s_b from the sample's ||r0||)    12 B / node
//   dot        partials of r.widen(z32)                                                        12 B
//   direction  p_out = widen(z32) + beta p_in      (window rows of z32 loaded in fp32, widened) 20 B
//   update     as above, also r32 = float(r_new s_b)                                           44 B
// s_b is one power of two per sample, fixed for the solve (sb[b], written by the narrowing of load()), so products
// with it are exact and CG does not see it.  Only interior nodes of r32 are ever written.
#include "framed_strip.h"

namespace fea {

constexpr int kPcgResidual = 0, kPcgDirection = 1, kPcgUpdate = 2;

template <typename T>
struct PcgArgs {
  const T* v;   // the field K acts on: x (residual), z (direction), p (update)
  const T* v2;  // direction: p_in
  const T* f;   // residual: right-hand side
  T* out;       // residual: r;  direction: p_out
  T* x;         // update
  T* r;         // update
  const uint8_t* pid;
  const T* ktab;
  int ntab;
  const double* sc;  // per-sample scalar blocks (FEA_PCG_NSCALARS doubles each)
  double* part;
  int H, W, ld;
  long long bs;
  int nstrips, ntr, rb;
  // mixed precision (T = double): the fp32 level-0 field of the preconditioner in its own frame
  const float* z32;  // direction, dot: the preconditioner's end iterate
  float* r32;        // narrow, update: the preconditioner's right-hand side
  const double* sb;  // update: per-sample scale s_b (narrow: written through sbw)
  double* sbw;
  int ld32;
  long long bs32;
};

// MIX: the f64f32 form — the direction's z, the update's second residual store live in the fp32 frame
template <typename T, bool MULTI, int MODE, bool NT, bool MIX = false>
__global__ __launch_bounds__(256) void k_pcg(PcgArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  static_assert(!MIX || (std::is_same<T, double>::value && MODE != kPcgResidual), "f64f32: direction and update");
  constexpr bool kMixDir = MIX && MODE == kPcgDirection;
  using ZT = typename std::conditional<kMixDir, float, T>::type;  // element type of the field z is read from
  __shared__ T tab[MULTI ? FEA_MAX_PATTERNS * kTabStride : 1];
  if constexpr (MULTI) {
    load_tables<T>(tab, g.ktab, nullptr, g.ntab, nullptr, nullptr, 0);
    __syncthreads();
  }
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int H = g.H, W = g.W;
  const int c0 = 1 + id.s * F::SW;
  const int r0 = 1 + id.t * g.rb;
  const int r1 = min(r0 + g.rb, H - 1);
  const int cl = c0 + V * lane;  // first own column
  T ks[9];
  if constexpr (!MULTI) {
#pragma unroll
    for (int d = 0; d < 9; ++d) ks[d] = g.ktab[d];
  }
  const long long poff = F::OFF + c0;
  const long long boff = (long long)id.b * g.bs + poff;
  const T* __restrict__ va = kMixDir ? nullptr : g.v + boff;
  const T* __restrict__ vb = MODE == kPcgDirection ? g.v2 + boff : nullptr;
  // the strip's first column in the fp32 frame, and that frame's row offsets
  const long long boff32 = MIX ? (long long)id.b * g.bs32 + Frame<float>::OFF + c0 : 0;
  const int ld32 = MIX ? g.ld32 : 0;
  auto rowo32 = [&](int r) -> long long { return (long long)(min(r, H) + 1) * ld32; };
  const uint8_t* __restrict__ pb = MULTI ? g.pid + poff : nullptr;
  const int ld = g.ld;
  auto rowo = [&](int r) -> long long { return (long long)(min(r, H) + 1) * ld; };
  const long long pslot = ((long long)id.b * g.ntr + id.t) * g.nstrips + id.s;
  const double* sc = g.sc ? g.sc + (long long)id.b * FEA_PCG_NSCALARS : nullptr;
  T coef = T(0);  // beta (direction) / alpha (update): formed in double, applied in T
  if constexpr (MODE == kPcgDirection) coef = (T)sc[FEA_PCG_BETA];
  if constexpr (MODE == kPcgUpdate) coef = (T)sc[FEA_PCG_ALPHA];
  double sbv = 1.0;
  if constexpr (MIX && MODE == kPcgUpdate) sbv = g.sb[id.b];
  double s = 0.0;

  if constexpr (MODE == kPcgUpdate) {
    // a frozen sample (alpha = 0): x and r (and r32) stay as they are, whatever p holds; its r.r is summed again in
    // the same order, so the history row repeats bit for bit
    if (sc[FEA_PCG_DONE] != 0.0) {
      const T* rb_ = g.r + boff;
      for (int r = r0; r < r1; ++r) {
        T rv[V];
        vload<T, V>(rb_ + rowo(r) + V * lane, rv);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (cl + k <= W - 2) s += (double)rv[k] * (double)rv[k];
      }
      s = wave_sum(s);
      if (lane == 0) g.part[pslot] = s;
      return;
    }
  }
  if constexpr (MODE == kPcgResidual) {
    // boundary nodes of r: rows 0 and H-1 by the first / last row task, columns 0 and W-1 by the first / last strip
    T* ob = g.out + boff;
    const T zv[V] = {};
    if (id.t == 0) store_masked<T, V, false>(ob + rowo(0) + V * lane, zv, cl, W);
    if (id.t == g.ntr - 1) store_masked<T, V, false>(ob + rowo(H - 1) + V * lane, zv, cl, W);
    const int ra = id.t == 0 ? 0 : r0, re = id.t == g.ntr - 1 ? H : r1;
    T* o0 = g.out + (long long)id.b * g.bs + F::OFF;
    if (id.s == 0 && lane == 0)
      for (int r = ra; r < re; ++r) o0[rowo(r)] = T(0);
    if (id.s == g.nstrips - 1 && lane == 0)
      for (int r = ra; r < re; ++r) o0[rowo(r) + W - 1] = T(0);
  }

  // a window row of the field K acts on; the direction's is z + beta p_in on every window column
  // (f64f32: z's window row is loaded and shifted in fp32 — the same lanes' columns, half the bytes — then widened)
  struct RawV {
    RawRow<ZT, V> a;
    RawRow<T, V> b;
  };
  auto raw_v = [&](int r) {
    RawV w;
    if constexpr (kMixDir) w.a = raw_row<float, V>(g.z32 + boff32 + rowo32(r), lane);
    else w.a = raw_row<T, V>(va + rowo(r), lane);
    if constexpr (MODE == kPcgDirection) w.b = raw_row<T, V>(vb + rowo(r), lane);
    return w;
  };
  auto fin_v = [&](const RawV& w) {
    Row<T, V> a;
    if constexpr (kMixDir) {
      const Row<float, V> z = finish(w.a);
#pragma unroll
      for (int j = 0; j < V + 3; ++j) a.a[j] = (T)z.a[j];
    } else {
      a = finish(w.a);
    }
    if constexpr (MODE == kPcgDirection) {
      const Row<T, V> b = finish(w.b);
#pragma unroll
      for (int j = 0; j < V + 3; ++j) a.a[j] = a.a[j] + coef * b.a[j];
    }
    return a;
  };
  Row<T, V> w0 = fin_v(raw_v(r0 - 1));
  Row<T, V> w1 = fin_v(raw_v(r0));
  RawV nx = raw_v(r0 + 1);
  PRow<V> p0{}, p1{}, p2{};
  RawP<V> px{};
  if constexpr (MULTI) {
    p0 = finish_p<T>(raw_prow<V>(pb + rowo(r0 - 1), lane));
    p1 = finish_p<T>(raw_prow<V>(pb + rowo(r0), lane));
    px = raw_prow<V>(pb + rowo(r0 + 1), lane);
  }
  for (int r = r0; r < r1; ++r) {
    const RawV nn = raw_v(r + 2);
    RawP<V> pn{};
    if constexpr (MULTI) pn = raw_prow<V>(pb + rowo(r + 2), lane);
    const long long ro = boff + rowo(r) + V * lane;
    T fv[V], xv[V];
    if constexpr (MODE == kPcgResidual) vload<T, V>(g.f + ro, fv);
    if constexpr (MODE == kPcgUpdate) {
      vload<T, V>(g.r + ro, fv);
      vload<T, V>(g.x + ro, xv);
    }
    const Row<T, V> w2 = fin_v(nx);
    if constexpr (MULTI) p2 = finish_p<T>(px);
    T o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const T kv = kapply<T, V, MULTI>(w0, w1, w2, p0, p1, p2, k, ks, tab);
      const bool in = cl + k <= W - 2;
      if constexpr (MODE == kPcgResidual) {
        o[k] = fv[k] - kv;
        if (in) s += (double)o[k] * (double)o[k];
      } else if constexpr (MODE == kPcgDirection) {
        o[k] = w1.a[k + 1];
        if (in) s += (double)o[k] * (double)kv;
      } else {
        o[k] = fv[k] - coef * kv;
        xv[k] = xv[k] + coef * w1.a[k + 1];
        if (in) s += (double)o[k] * (double)o[k];
      }
    }
    if constexpr (MODE == kPcgUpdate) {
      store_masked<T, V, NT>(g.r + ro, o, cl, W);
      store_masked<T, V, NT>(g.x + ro, xv, cl, W);
      if constexpr (MIX) {
        float nv[V];
#pragma unroll
        for (int k = 0; k < V; ++k) nv[k] = (float)(o[k] * sbv);
        store_masked<float, V, NT>(g.r32 + boff32 + rowo32(r) + V * lane, nv, cl, W);
      }
    } else {
      store_masked<T, V, NT>(g.out + ro, o, cl, W);
    }
    w0 = w1;
    w1 = w2;
    nx = nn;
    if constexpr (MULTI) {
      p0 = p1;
      p1 = p2;
      px = pn;
    }
  }
  s = wave_sum(s);
  if (lane == 0) g.part[pslot] = s;
}

// partials of r.z over the interior (pointwise: no window); Z = float: z in the fp32 frame (f64f32)
template <typename T, typename Z = T>
__global__ __launch_bounds__(256) void k_pcg_dot(PcgArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  constexpr bool MIX = !std::is_same<Z, T>::value;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int H = g.H, W = g.W;
  const int r0 = 1 + id.t * g.rb;
  const int r1 = min(r0 + g.rb, H - 1);
  const int cl = 1 + id.s * F::SW + V * lane;
  const long long boff = (long long)id.b * g.bs + F::OFF + cl;
  const T* __restrict__ a = g.v + boff;
  const Z* __restrict__ b;
  if constexpr (MIX) b = g.z32 + (long long)id.b * g.bs32 + Frame<Z>::OFF + cl;
  else b = g.v2 + boff;
  const int ldz = MIX ? g.ld32 : g.ld;
  double s = 0.0;
  for (int r = r0; r < r1; ++r) {
    const long long ro = (long long)(r + 1) * g.ld;
    T av[V];
    Z bv[V];
    vload<T, V>(a + ro, av);
    vload<Z, V>(b + (long long)(r + 1) * ldz, bv);
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (cl + k <= W - 2) s += (double)av[k] * (double)bv[k];
  }
  s = wave_sum(s);
  if (lane == 0) g.part[((long long)id.b * g.ntr + id.t) * g.nstrips + id.s] = s;
}

// The per-sample scale of the f64f32 path: the power of two that puts ||r0|| s_b in [1, 2); 1 for ||r0|| = 0 or not
// finite.  Formed from the exponent field (subnormal ||r0||: 2^1023; ||r0|| >= 2^1023: 2^-1022, so s_b is a normal
// number), the same bits in every wave.
__device__ __forceinline__ double pcg_scale(double rn) {
  const long long ex = (__double_as_longlong(rn) >> 52) & 0x7ff;
  if (!(rn > 0.0) || ex == 0x7ff) return 1.0;
  const long long e = 2046 - ex;
  return __longlong_as_double((e < 1 ? 1ll : e) << 52);
}

// r32 = float(r s_b) on the interior (pointwise), s_b from the sample's FEA_PCG_RNORM; the sample's first task stores it
template <bool NT>
__global__ __launch_bounds__(256) void k_pcg_narrow(PcgArgs<double> g) {
  using F = Frame<double>;
  constexpr int V = F::VEC;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int H = g.H, W = g.W;
  const int r0 = 1 + id.t * g.rb;
  const int r1 = min(r0 + g.rb, H - 1);
  const int cl = 1 + id.s * F::SW + V * lane;
  const double sbv = pcg_scale(g.sc[(long long)id.b * FEA_PCG_NSCALARS + FEA_PCG_RNORM]);
  if (id.s == 0 && id.t == 0 && lane == 0) g.sbw[id.b] = sbv;
  const double* __restrict__ a = g.v + (long long)id.b * g.bs + F::OFF + cl;
  float* __restrict__ o = g.r32 + (long long)id.b * g.bs32 + Frame<float>::OFF + cl;
  for (int r = r0; r < r1; ++r) {
    double av[V];
    float nv[V];
    vload<double, V>(a + (long long)(r + 1) * g.ld, av);
#pragma unroll
    for (int k = 0; k < V; ++k) nv[k] = (float)(av[k] * sbv);
    store_masked<float, V, NT>(o + (long long)(r + 1) * g.ld32, nv, cl, W);
  }
}

// One workgroup per sample: the sample's `per` partials summed in index order (the scheme of k_norm_final), then
// the step's update of its scalar block by one lane with ordinary stores.
__global__ __launch_bounds__(256) void k_pcg_scalar(const double* __restrict__ part, long long per,
                                                   double* __restrict__ scalars, double* __restrict__ hist,
                                                   int hist_rows, int B, int step) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  const double* p = part + b * per;
  double s = 0.0;
  for (long long i = threadIdx.x; i < per; i += 256) s += p[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double sum = sh[0];
  double* S = scalars + (long long)b * FEA_PCG_NSCALARS;
  double done = S[FEA_PCG_DONE];
  auto append = [&](double rn) {
    const long long row = (long long)S[FEA_PCG_ROW];
    if (row >= 0 && row < hist_rows) hist[row * B + b] = rn;
    S[FEA_PCG_ROW] = (double)(row + 1);
  };
  if (step == FEA_PCG_STEP_INIT) {  // sum = r0.r0
    const double rn = sqrt(sum);
    const double thresh = S[FEA_PCG_RTOL] >= 0.0 ? S[FEA_PCG_RTOL] * rn : S[FEA_PCG_EPS];
    S[FEA_PCG_RZ] = S[FEA_PCG_RZ_PREV] = S[FEA_PCG_PAP] = S[FEA_PCG_ALPHA] = S[FEA_PCG_BETA] = 0.0;
    S[FEA_PCG_RNORM] = rn;
    S[FEA_PCG_DONE] = !isfinite(rn) ? (double)FEA_PCG_BREAKDOWN : rn <= thresh ? (double)FEA_PCG_CONVERGED : 0.0;
    S[FEA_PCG_ITERS] = 0.0;
    S[FEA_PCG_THRESH] = thresh;
    S[FEA_PCG_ROW] = 0.0;
    append(rn);
  } else if (step == FEA_PCG_STEP_RZ) {  // sum = r.z
    if (done == 0.0 && !isfinite(sum)) S[FEA_PCG_DONE] = done = (double)FEA_PCG_BREAKDOWN;
    if (done != 0.0) {
      S[FEA_PCG_BETA] = 0.0;
    } else {
      const double prev = S[FEA_PCG_RZ];
      S[FEA_PCG_RZ_PREV] = prev;
      S[FEA_PCG_RZ] = sum;
      S[FEA_PCG_BETA] = (S[FEA_PCG_ITERS] > 0.0 && prev != 0.0) ? sum / prev : 0.0;
    }
  } else if (step == FEA_PCG_STEP_PAP) {  // sum = p.Kp
    if (done == 0.0) {
      S[FEA_PCG_PAP] = sum;
      if (!(sum > 0.0) || !isfinite(sum)) S[FEA_PCG_DONE] = done = (double)FEA_PCG_BREAKDOWN;
    }
    S[FEA_PCG_ALPHA] = done != 0.0 ? 0.0 : S[FEA_PCG_RZ] / sum;
  } else {  // FEA_PCG_STEP_RR: sum = r.r after the update
    const double rn = sqrt(sum);
    if (done == 0.0) {
      S[FEA_PCG_ITERS] += 1.0;
      if (!isfinite(rn)) S[FEA_PCG_DONE] = (double)FEA_PCG_BREAKDOWN;
      else if (rn <= S[FEA_PCG_THRESH]) S[FEA_PCG_DONE] = (double)FEA_PCG_CONVERGED;
    }
    S[FEA_PCG_RNORM] = rn;
    append(rn);
  }
}

}  // namespace fea

// the task grid of the Krylov kernels: the height a single sample would get, so partial sets do not depend on B
template <typename T>
static void pcg_geom(int H, int W, int& nstrips, int& rb, int& ntr) {
  nstrips = mg_nstrips<T>(W);
  rb = pick_rb(1, nstrips, H - 2);
  ntr = div_up(H - 2, rb);
}

template <typename T>
static PcgArgs<T> pcg_args(int H, int W, int ld, long long bs) {
  PcgArgs<T> g{};
  g.H = H;
  g.W = W;
  g.ld = ld;
  g.bs = bs;
  pcg_geom<T>(H, W, g.nstrips, g.rb, g.ntr);
  return g;
}

template <typename T>
static inline bool pcg_nt(int B, long long bs) { return (long long)B * bs * (long long)sizeof(T) > nt_bytes(); }

extern "C" long long fea_pcg_parts(int H, int W, int elem_size) {
  if (!mg_dims_ok(H, W) || (elem_size != 4 && elem_size != 8)) return -1;
  int ns, rb, ntr;
  if (elem_size == 8) pcg_geom<double>(H, W, ns, rb, ntr);
  else pcg_geom<float>(H, W, ns, rb, ntr);
  return (long long)ns * ntr;
}

extern "C" int fea_pcg_scalar_step(const double* part, long long per, double* scalars, double* hist, int hist_rows,
                                   int B, int step, void* stream) {
  if (!part || !scalars || !hist || per <= 0 || hist_rows <= 0 || B <= 0 || step < FEA_PCG_STEP_INIT ||
      step > FEA_PCG_STEP_RR)
    return FEA_EINVAL;
  k_pcg_scalar<<<B, 256, 0, (hipStream_t)stream>>>(part, per, scalars, hist, hist_rows, B, step);
  return launch_status();
}

template <typename T, int MODE, bool MIX = false>
static void pcg_launch(const PcgArgs<T>& g, int B, void* stream) {
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  hipStream_t s = (hipStream_t)stream;
  const bool nt = pcg_nt<T>(B, g.bs);
  if (g.ntab > 1) {
    if (nt) k_pcg<T, true, MODE, true, MIX><<<grid, 256, 0, s>>>(g);
    else k_pcg<T, true, MODE, false, MIX><<<grid, 256, 0, s>>>(g);
  } else {
    if (nt) k_pcg<T, false, MODE, true, MIX><<<grid, 256, 0, s>>>(g);
    else k_pcg<T, false, MODE, false, MIX><<<grid, 256, 0, s>>>(g);
  }
}

template <typename T>
static int pcg_residual(const T* x, const T* f, T* r, const uint8_t* pid, const T* ktab, int ntab, double* part, int B,
                        int H, int W, int ld, long long bs, void* stream) {
  if (!x || !f || !r || !part || B <= 0 || !layout_ok<T>(H, W, ld, bs) || !tab_ok(ktab, ntab, pid) || r == x)
    return FEA_EINVAL;
  PcgArgs<T> g = pcg_args<T>(H, W, ld, bs);
  g.v = x; g.f = f; g.out = r; g.pid = pid; g.ktab = ktab; g.ntab = ntab; g.part = part;
  pcg_launch<T, kPcgResidual>(g, B, stream);
  return launch_status();
}

template <typename T>
static int pcg_direction(const T* z, const T* p_in, T* p_out, const uint8_t* pid, const T* ktab, int ntab,
                         const double* scalars, double* part, int B, int H, int W, int ld, long long bs,
                         void* stream) {
  if (!z || !p_in || !p_out || !scalars || !part || B <= 0 || !layout_ok<T>(H, W, ld, bs) ||
      !tab_ok(ktab, ntab, pid) || p_out == p_in || p_out == z)
    return FEA_EINVAL;
  PcgArgs<T> g = pcg_args<T>(H, W, ld, bs);
  g.v = z; g.v2 = p_in; g.out = p_out; g.pid = pid; g.ktab = ktab; g.ntab = ntab; g.sc = scalars;
  g.part = part;
  pcg_launch<T, kPcgDirection>(g, B, stream);
  return launch_status();
}

template <typename T>
static int pcg_update(const T* p, T* x, T* r, const uint8_t* pid, const T* ktab, int ntab, const double* scalars,
                      double* part, int B, int H, int W, int ld, long long bs, void* stream) {
  if (!p || !x || !r || !scalars || !part || B <= 0 || !layout_ok<T>(H, W, ld, bs) || !tab_ok(ktab, ntab, pid) ||
      x == p || r == p || x == r)
    return FEA_EINVAL;
  PcgArgs<T> g = pcg_args<T>(H, W, ld, bs);
  g.v = p; g.x = x; g.r = r; g.pid = pid; g.ktab = ktab; g.ntab = ntab; g.sc = scalars; g.part = part;
  pcg_launch<T, kPcgUpdate>(g, B, stream);
  return launch_status();
}

template <typename T>
static int pcg_dot(const T* r, const T* z, double* part, int B, int H, int W, int ld, long long bs, void* stream) {
  if (!r || !z || !part || B <= 0 || !layout_ok<T>(H, W, ld, bs)) return FEA_EINVAL;
  PcgArgs<T> g = pcg_args<T>(H, W, ld, bs);
  g.v = r; g.v2 = z; g.part = part;
  k_pcg_dot<T><<<mg_grid(B, g.ntr, g.nstrips), 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

#define FEA_PCG_API(SUF, T)                                                                                        \
  extern "C" int fea_pcg_residual_##SUF(const T* x, const T* f, T* r, const uint8_t* pid, const T* ktab, int ntab,   \
                                        double* part, int B, int H, int W, int ld, long long bs, void* stream) {    \
    return pcg_residual<T>(x, f, r, pid, ktab, ntab, part, B, H, W, ld, bs, stream);                               \
  }                                                                                                                \
  extern "C" int fea_pcg_direction_##SUF(const T* z, const T* p_in, T* p_out, const uint8_t* pid, const T* ktab,    \
                                         int ntab, const double* scalars, double* part, int B, int H, int W,       \
                                         int ld, long long bs, void* stream) {                                     \
    return pcg_direction<T>(z, p_in, p_out, pid, ktab, ntab, scalars, part, B, H, W, ld, bs, stream);               \
  }                                                                                                                \
  extern "C" int fea_pcg_update_##SUF(const T* p, T* x, T* r, const uint8_t* pid, const T* ktab, int ntab,          \
                                      const double* scalars, double* part, int B, int H, int W, int ld,            \
                                      long long bs, void* stream) {                                                \
    return pcg_update<T>(p, x, r, pid, ktab, ntab, scalars, part, B, H, W, ld, bs, stream);                        \
  }                                                                                                                \
  extern "C" int fea_pcg_dot_##SUF(const T* r, const T* z, double* part, int B, int H, int W, int ld,              \
                                   long long bs, void* stream) {                                                   \
    return pcg_dot<T>(r, z, part, B, H, W, ld, bs, stream);                                                        \
  }
FEA_PCG_API(f32, float)
FEA_PCG_API(f64, double)

// ---------------------------------------------------------------------------
// f64f32: fp64 Krylov fields (ld, bs) next to the preconditioner's fp32 level-0 field (ld32, bs32)
// ---------------------------------------------------------------------------
static inline bool pcg_mix_ok(int B, int H, int W, int ld, long long bs, int ld32, long long bs32) {
  return B > 0 && layout_ok<double>(H, W, ld, bs) && layout_ok<float>(H, W, ld32, bs32);
}

static PcgArgs<double> pcg_mix_args(int H, int W, int ld, long long bs, int ld32, long long bs32) {
  PcgArgs<double> g = pcg_args<double>(H, W, ld, bs);
  g.ld32 = ld32;
  g.bs32 = bs32;
  return g;
}

extern "C" int fea_pcg_narrow_f64f32(const double* r, float* r32, const double* scalars, double* sb, int B, int H,
                                     int W, int ld, long long bs, int ld32, long long bs32, void* stream) {
  if (!r || !r32 || !scalars || !sb || !pcg_mix_ok(B, H, W, ld, bs, ld32, bs32) || (const void*)r32 == (const void*)r ||
      sb == scalars)
    return FEA_EINVAL;
  PcgArgs<double> g = pcg_mix_args(H, W, ld, bs, ld32, bs32);
  g.v = r; g.r32 = r32; g.sc = scalars; g.sbw = sb;
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  if (pcg_nt<double>(B, bs)) k_pcg_narrow<true><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  else k_pcg_narrow<false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

extern "C" int fea_pcg_dot_f64f32(const double* r, const float* z32, double* part, int B, int H, int W, int ld,
                                  long long bs, int ld32, long long bs32, void* stream) {
  if (!r || !z32 || !part || !pcg_mix_ok(B, H, W, ld, bs, ld32, bs32)) return FEA_EINVAL;
  PcgArgs<double> g = pcg_mix_args(H, W, ld, bs, ld32, bs32);
  g.v = r; g.z32 = z32; g.part = part;
  k_pcg_dot<double, float><<<mg_grid(B, g.ntr, g.nstrips), 256, 0, (hipStream_t)stream>>>(g);
  return launch_status();
}

extern "C" int fea_pcg_direction_f64f32(const float* z32, const double* p_in, double* p_out, const uint8_t* pid,
                                        const double* ktab, int ntab, const double* scalars, double* part, int B,
                                        int H, int W, int ld, long long bs, int ld32, long long bs32, void* stream) {
  if (!z32 || !p_in || !p_out || !scalars || !part || !pcg_mix_ok(B, H, W, ld, bs, ld32, bs32) ||
      !tab_ok(ktab, ntab, pid) || p_out == p_in || (const void*)p_out == (const void*)z32)
    return FEA_EINVAL;
  PcgArgs<double> g = pcg_mix_args(H, W, ld, bs, ld32, bs32);
  g.z32 = z32; g.v2 = p_in; g.out = p_out; g.pid = pid; g.ktab = ktab; g.ntab = ntab; g.sc = scalars;
  g.part = part;
  pcg_launch<double, kPcgDirection, true>(g, B, stream);
  return launch_status();
}

extern "C" int fea_pcg_update_f64f32(const double* p, double* x, double* r, float* r32, const uint8_t* pid,
                                     const double* ktab, int ntab, const double* scalars, const double* sb,
                                     double* part, int B, int H, int W, int ld, long long bs, int ld32,
                                     long long bs32, void* stream) {
  const void* n = r32;
  if (!p || !x || !r || !r32 || !scalars || !sb || !part || !pcg_mix_ok(B, H, W, ld, bs, ld32, bs32) ||
      !tab_ok(ktab, ntab, pid) || x == p || r == p || x == r || n == p || n == x || n == r)
    return FEA_EINVAL;
  PcgArgs<double> g = pcg_mix_args(H, W, ld, bs, ld32, bs32);
  g.v = p; g.x = x; g.r = r; g.r32 = r32; g.pid = pid; g.ktab = ktab; g.ntab = ntab; g.sc = scalars; g.sb = sb;
  g.part = part;
  pcg_launch<double, kPcgUpdate, true>(g, B, stream);
  return launch_status();
}
