// fmg_ops.hip — the transfers of the full-multigrid start (include/feanet_fmg.h) on the framed layout
// (framed_ops.hip): the interpolation of a coarse SOLUTION to the next finer level, the restriction of a right-hand
// side without a stencil, and the injection of Dirichlet data onto a level's boundary nodes.
//
// fea_fmg_prolong: out = u + I(ec) on the interior nodes of the H x W level, ec the (H+1)/2 x (W+1)/2 level with
// its boundary nodes (the coarse Dirichlet values).  One direction, n coarse nodes e[0..n-1], fine node 2j+1
// between coarse j and j+1 (0 <= j <= n-2), four taps and four weights:
//     t1 = e[j]   t2 = e[j+1]   t0 = j == 0 ? e[3] : e[j-1]   t3 = j == n-2 ? e[n-4] : e[j+2]
//     cubic, 0 < j < n-2 :  (w0, w1, w2, w3) = (-1,  9,  9, -1) / 16
//     cubic, j == 0      :                     ( 1,  5, 15, -5) / 16     (5, 15, -5, 1)/16 of e[0..3]
//     cubic, j == n-2    :                     (-5, 15,  5,  1) / 16     (1, -5, 15, 5)/16 of e[n-4..n-1]
//     order 1, or n < 4  :                     ( 0, 1/2, 1/2, 0),  t0 = t3 = 0 (nothing is read for them)
//     v = w0 * t0;  v += w1 * t1;  v += w2 * t2;  v += w3 * t3;          (four statements, each product fused
//                                                                          with its own add: -ffp-contract=on)
// so the rows and columns next to the boundary differ from the others in their weights and in ONE tap only (the
// far node of the one-sided formula takes the place of the node beyond the boundary): weights and a select, no
// branch.  A fine node 2j coincides with coarse j and copies it.  Columns first: every coarse row a is interpolated
// along its columns into h_a (the statements above with the column's j; coincident columns copy), then across the
// rows: fine row 2a+1 takes the statements above on h of the rows (t0..t3 of j = a), fine row 2a copies h_a.
// Last,  out = u + v  (u == NULL: out = v).  Every value is one fixed expression of its node, so the result does
// not depend on the task height, the strip or the batch.
//
// Work decomposition: the strip / row march of k_mg_prolong.  A lane owns VEC fine columns (cl odd, cl + VEC - 1),
// i.e. the coarse columns j0+1 .. j0+VEC/2 with j0 = (cl-1)/2, which it loads with one vector load; the coarse
// columns j0-1, j0 and j0+VEC/2+1 come from the neighbouring lanes by DPP (one lane further to the left than
// crow_term needs), the wave's edges from three scalar halo loads, the far taps e[3] and e[n-4] from two
// wave-uniform loads.  A task marches down its fine rows two at a time with a window of four column-interpolated
// coarse rows in registers (h of t0..t3); each step loads ONE new coarse row and the two fine rows of u, issued a
// step ahead of the arithmetic.  No LDS.  Only indices inside ec's H x W nodes are ever used in a stored value:
// ghost ring and pad may hold anything (they are read by the lanes past the grid, whose values are dropped).
//
// fea_fmg_restrict: fc = R f, R = [[1,2,1],[2,4,2],[1,2,1]]/4 — restrict9() on three f rows, the statements of
// fea_mg_residual_restrict with u = 0, rtab = R, w0 = 1 (f - K 0 = f and 1 * x = x exactly), so bitwise that.
#include "framed_strip.h"

#include "feanet_fmg.h"

namespace fea {

template <typename T>
struct FmgArgs {
  const T* u;
  const T* ec;
  T* out;
  int H, W, ld;
  long long bs;
  int Hc, Wc, ldc;
  long long bsc;
  int nstrips, ntr, rb;
  int cubx, cuby;  // cubic along the columns / across the rows (order 3 and >= 4 coarse nodes that way)
};

// the four weights at coarse interval j of n coarse nodes (header comment)
template <typename T>
struct W4 {
  T w[4];
};
template <typename T>
__device__ __forceinline__ W4<T> fmg_weights(bool cubic, int j, int n) {
  const bool lo = j == 0, hi = j == n - 2;
  W4<T> r;
  r.w[0] = cubic ? (lo ? T(1) / 16 : hi ? T(-5) / 16 : T(-1) / 16) : T(0);
  r.w[1] = cubic ? (lo ? T(5) / 16 : hi ? T(15) / 16 : T(9) / 16) : T(0.5);
  r.w[2] = cubic ? (lo ? T(15) / 16 : hi ? T(5) / 16 : T(9) / 16) : T(0.5);
  r.w[3] = cubic ? (lo ? T(-5) / 16 : hi ? T(1) / 16 : T(-1) / 16) : T(0);
  return r;
}
template <typename T>
__device__ __forceinline__ T interp4(const W4<T>& w, T t0, T t1, T t2, T t3) {
  T v = w.w[0] * t0;
  v += w.w[1] * t1;
  v += w.w[2] * t2;
  v += w.w[3] * t3;
  return v;
}

// a coarse row as loaded: the lane's own columns, the halo values of the wave's edge lanes, the two far taps
template <typename T, int Q>
struct RawE {
  T x[Q];
  T h1, h2, fl, fr;
};

template <typename T, bool HASU, bool NT>
__global__ __launch_bounds__(256) void k_fmg_prolong(FmgArgs<T> g) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  constexpr int Q = V / 2;
  const TaskId id = decode_task(g.nstrips, g.ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int H = g.H, W = g.W, Hc = g.Hc, Wc = g.Wc;
  const int c0 = 1 + id.s * F::SW;
  const int r0 = 1 + id.t * g.rb;  // odd
  const int r1 = min(r0 + g.rb, H - 1);
  const int cl = c0 + V * lane;  // odd
  const int j0 = (cl - 1) / 2;
  const bool cubx = g.cubx != 0, cuby = g.cuby != 0;
  const int ld = g.ld, ldc = g.ldc;
  const long long boff = (long long)id.b * g.bs + F::OFF + c0;
  const T* ub = HASU ? g.u + boff : nullptr;  // may alias out: every node is read by the lane that writes it
  T* ob = g.out + boff;
  const T* __restrict__ e0 = g.ec + (long long)id.b * g.bsc + F::OFF;  // column 0 of ec's rows
  const int bc0 = (c0 + 1) / 2;  // lane 0's first own coarse column
  const int fl_c = min(3, Wc - 1), fr_c = max(Wc - 4, 0);
  auto rowo = [&](int r) -> long long { return (long long)(min(r, H) + 1) * ld; };

  // per-column weights and far-tap selects (fixed for the task)
  W4<T> wx[Q];
  bool xlo[Q], xhi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    wx[q] = fmg_weights<T>(cubx, j0 + q, Wc);
    xlo[q] = j0 + q == 0;
    xhi[q] = j0 + q == Wc - 2;
  }

  auto raw = [&](int a) {  // coarse row a, clamped into the level's rows
    const int ac = max(min(a, Hc - 1), 0);
    const T* __restrict__ rp = e0 + (long long)(ac + 1) * ldc;
    const T* __restrict__ ep = rp + bc0;
    RawE<T, Q> r;
    vload<T, Q>(ep + Q * lane, r.x);
    r.h1 = ep[lane < 32 ? -1 : kWave * Q];
    r.h2 = ep[-2];
    r.fl = rp[fl_c];
    r.fr = rp[fr_c];
    return r;
  };
  // the row interpolated along its columns, at the lane's V fine columns
  struct HRow {
    T v[V];
  };
  auto colinterp = [&](const RawE<T, Q>& r) {
    T e[Q + 3];  // coarse columns j0-1 .. j0+Q+1
#pragma unroll
    for (int q = 0; q < Q; ++q) e[q + 2] = r.x[q];
    e[1] = shr1(r.x[Q - 1], r.h1);
    e[0] = Q == 1 ? shr1(e[1], r.h2) : shr1(r.x[Q == 1 ? 0 : Q - 2], r.h2);
    e[Q + 2] = shl1(r.x[0], r.h1);
    HRow h;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const T t0 = cubx ? (xlo[q] ? r.fl : e[q]) : T(0);
      const T t3 = cubx ? (xhi[q] ? r.fr : e[q + 3]) : T(0);
      h.v[2 * q] = interp4<T>(wx[q], t0, e[q + 1], e[q + 2], t3);
      h.v[2 * q + 1] = e[q + 2];
    }
    return h;
  };
  auto s0row = [&](int a) { return a == 0 ? 3 : a - 1; };
  auto s3row = [&](int a) { return a == Hc - 2 ? Hc - 4 : a + 2; };
  auto loadu = [&](int y, T (&uv)[V]) {
    if constexpr (HASU) vload<T, V>(ub + rowo(y) + V * lane, uv);
  };
  auto emit = [&](int y, const T (&v)[V], const T (&uv)[V]) {
    T o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = HASU ? uv[k] + v[k] : v[k];
    store_masked<T, V, NT>(ob + rowo(y) + V * lane, o, cl, W);
  };

  const int a0 = (r0 - 1) / 2;
  HRow H0 = colinterp(raw(s0row(a0)));
  HRow H1 = colinterp(raw(a0));
  HRow H2 = colinterp(raw(a0 + 1));
  HRow H3 = colinterp(raw(s3row(a0)));
  T u0[V], u1[V];
  loadu(r0, u0);
  loadu(r0 + 1, u1);
  for (int y = r0; y < r1; y += 2) {
    const int a = (y - 1) / 2;
    // the next step's loads, ahead of this step's arithmetic
    const RawE<T, Q> rn = raw(s3row(a + 1));
    T n0[V], n1[V];
    loadu(y + 2, n0);
    loadu(y + 3, n1);
    const W4<T> wy = fmg_weights<T>(cuby, a, Hc);  // wave-uniform
    T v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const T t0 = cuby ? H0.v[k] : T(0);
      const T t3 = cuby ? H3.v[k] : T(0);
      v[k] = interp4<T>(wy, t0, H1.v[k], H2.v[k], t3);
    }
    emit(y, v, u0);
    if (y + 1 < r1) emit(y + 1, H2.v, u1);
    H0 = H1;
    H1 = H2;
    H2 = H3;
    H3 = colinterp(rn);
    if constexpr (HASU) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        u0[k] = n0[k];
        u1[k] = n1[k];
      }
    }
  }
}

// fc = R f on the coarse interior: task = (strip, coarse rows [I0, I1)), fine rows 2 I0 - 1 .. 2 I1 - 1 are read
template <typename T>
__global__ __launch_bounds__(256) void k_fmg_restrict(const T* __restrict__ f, T* __restrict__ fc, int H, int W, int ld,
                                                      long long bs, int Hc, int Wc, int ldc, long long bsc, int nstrips,
                                                      int ntr, int rb) {
  using F = Frame<T>;
  constexpr int V = F::VEC;
  constexpr int Q = V / 2;
  const TaskId id = decode_task(nstrips, ntr);
  if (!id.valid) return;
  const int lane = lane_id();
  const int c0 = 1 + id.s * F::SW;
  const int I0 = 1 + id.t * (rb / 2);
  const int I1 = min(I0 + rb / 2, Hc - 1);
  const T rs[9] = {T(0.25), T(0.5), T(0.25), T(0.5), T(1), T(0.5), T(0.25), T(0.5), T(0.25)};
  const int dz[1] = {0};
  const T* __restrict__ fb = f + (long long)id.b * bs + F::OFF + c0;
  const int bc0 = (c0 + 1) / 2;
  T* __restrict__ cb = fc + (long long)id.b * bsc + F::OFF + bc0 + Q * lane;
  const int Jl = bc0 + Q * lane;
  auto rowo = [&](int r) -> long long { return (long long)(min(r, H) + 1) * ld; };
  auto rr = [&](int y) { return raw_row<T, V>(fb + rowo(y), lane); };

  Row<T, V> Ra = finish(rr(2 * I0 - 1));
  RawRow<T, V> nb = rr(2 * I0), nc = rr(2 * I0 + 1);
  for (int I = I0; I < I1; ++I) {
    const Row<T, V> Rb = finish(nb), Rc = finish(nc);
    nb = rr(2 * I + 2);  // the next coarse row's fine rows, ahead of the arithmetic
    nc = rr(2 * I + 3);
    T o[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q)  // fine columns cl + 2q .. cl + 2q + 2 = window columns 2q + 1 ..
      o[q] = restrict9<T, false>(rs, (const T*)nullptr, Ra.a, Rb.a, Rc.a, 2 * q + 1, dz, dz, dz, 0);
    store_masked<T, Q, false>(cb + (long long)(I + 1) * ldc, o, Jl, Wc);
    Ra = Rc;
  }
}

// the 2 (H + W) - 4 boundary nodes of dst: bc sampled at `stride`, or zero
template <typename T>
__global__ __launch_bounds__(256) void k_fmg_boundary(const T* __restrict__ bc, long long bc_bs, int stride,
                                                      T* __restrict__ dst, int H, int W, int ld, long long bs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= 2 * (H + W) - 4) return;
  int r, c;
  if (i < W) {
    r = 0;
    c = i;
  } else if (i < 2 * W) {
    r = H - 1;
    c = i - W;
  } else {
    const int k = i - 2 * W;
    r = 1 + k / 2;
    c = (k & 1) ? W - 1 : 0;
  }
  const long long Wf = (long long)(W - 1) * stride + 1;
  const T v = bc ? bc[(long long)b * bc_bs + (long long)r * stride * Wf + (long long)c * stride] : T(0);
  dst[(long long)b * bs + (long long)(r + 1) * ld + Frame<T>::OFF + c] = v;
}

}  // namespace fea

// the coarse level of an interpolation: (H+1)/2 x (W+1)/2 nodes, at least 2 each way (no interior needed: its
// boundary nodes are data), in its own framed layout
template <typename T>
static inline bool fmg_coarse_ok(int H, int W, int ldc, long long bsc) {
  if (!mg_odd(H, W)) return false;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  return Hc >= 2 && Wc >= 2 && ldc >= mg_ld<T>(Wc) && ldc % Frame<T>::A == 0 && bsc >= (long long)(Hc + 2) * ldc;
}

template <typename T>
static int fmg_prolong(const T* u, const T* ec, T* out, int B, int H, int W, int ld, long long bs, int ldc,
                       long long bsc, int order, void* stream) {
  if (!ec || !out || B <= 0 || !layout_ok<T>(H, W, ld, bs) || !fmg_coarse_ok<T>(H, W, ldc, bsc)) return FEA_EINVAL;
  if ((order != 1 && order != 3) || out == ec || u == ec) return FEA_EINVAL;
  FmgArgs<T> g{};
  g.u = u; g.ec = ec; g.out = out; g.H = H; g.W = W; g.ld = ld; g.bs = bs;
  g.Hc = (H + 1) / 2; g.Wc = (W + 1) / 2; g.ldc = ldc; g.bsc = bsc;
  g.nstrips = mg_nstrips<T>(W);
  g.rb = pick_rb(B, g.nstrips, H - 2);
  g.ntr = div_up(H - 2, g.rb);
  g.cubx = order == 3 && g.Wc >= 4;
  g.cuby = order == 3 && g.Hc >= 4;
  const bool nt = (long long)B * bs * (long long)sizeof(T) > nt_bytes();
  const dim3 grid = mg_grid(B, g.ntr, g.nstrips);
  hipStream_t s = (hipStream_t)stream;
  with_flags([&](auto hasu, auto ntc) { k_fmg_prolong<T, hasu(), ntc()><<<grid, 256, 0, s>>>(g); }, u != nullptr, nt);
  return launch_status();
}

template <typename T>
static int fmg_restrict(const T* f, T* fc, int B, int H, int W, int ld, long long bs, int ldc, long long bsc,
                        void* stream) {
  if (!f || !fc || f == fc || B <= 0 || !layout_ok<T>(H, W, ld, bs) || !fmg_coarse_ok<T>(H, W, ldc, bsc))
    return FEA_EINVAL;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  if (Hc < 3 || Wc < 3) return FEA_EINVAL;  // no coarse interior
  const int nstrips = mg_nstrips<T>(W);
  const int rb = pick_rb(B, nstrips, H - 2);
  const int ntr = div_up(Hc - 2, rb / 2);
  k_fmg_restrict<T><<<mg_grid(B, ntr, nstrips), 256, 0, (hipStream_t)stream>>>(f, fc, H, W, ld, bs, Hc, Wc, ldc, bsc,
                                                                               nstrips, ntr, rb);
  return launch_status();
}

template <typename T>
static int fmg_boundary(const T* bc, long long bc_bs, int stride, T* dst, int B, int H, int W, int ld, long long bs,
                        void* stream) {
  if (!dst || B <= 0 || B > 65535 || !layout_ok<T>(H, W, ld, bs) || stride < 1 || bc_bs < 0 || dst == bc)
    return FEA_EINVAL;
  k_fmg_boundary<T><<<dim3(div_up(2 * (H + W) - 4, 256), B), 256, 0, (hipStream_t)stream>>>(bc, bc_bs, stride, dst, H,
                                                                                          W, ld, bs);
  return launch_status();
}

#define FEA_FMG_ENTRY(T, SUF)                                                                                          \
  extern "C" int fea_fmg_prolong_##SUF(const T* u, const T* ec, T* out, int B, int H, int W, int ld,                   \
                                       long long bstride, int ldc, long long bstridec, int order, void* stream) {      \
    return fmg_prolong<T>(u, ec, out, B, H, W, ld, bstride, ldc, bstridec, order, stream);                             \
  }                                                                                                                    \
  extern "C" int fea_fmg_restrict_##SUF(const T* f, T* fc, int B, int H, int W, int ld, long long bstride, int ldc,    \
                                        long long bstridec, void* stream) {                                            \
    return fmg_restrict<T>(f, fc, B, H, W, ld, bstride, ldc, bstridec, stream);                                        \
  }                                                                                                                    \
  extern "C" int fea_fmg_boundary_##SUF(const T* bc, long long bc_bstride, int stride, T* dst, int B, int H, int W,    \
                                        int ld, long long bstride, void* stream) {                                     \
    return fmg_boundary<T>(bc, bc_bstride, stride, dst, B, H, W, ld, bstride, stream);                                 \
  }
FEA_FMG_ENTRY(float, f32)
FEA_FMG_ENTRY(double, f64)
