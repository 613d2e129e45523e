// torus_strip.h — what the kernel families on the torus layout share (periodic_ops.hip: a pattern map and a stencil
// table; coef_ops.hip: a coefficient per element).
//
// Torus layout: [B, m, ld] without a ghost ring; every index wraps.  sweep, apply and reduce use the strip x row-march
// decomposition of the framed kernels (framed_strip.h): a wave owns a strip of 64 * VEC node columns and a task of rb
// rows, a lane owns VEC columns (one 16-byte load per row), three node rows sit in a register window that marches
// down and the row after the next is loaded before the arithmetic.  Left and right neighbours come by DPP inside the
// wave; the columns next to the strip (lane 0: column cl - 1, or n - 1 at column 0; lane 63: column cl + VEC) and
// column 0, the right neighbour of column n - 1 wherever that column lies in the strip, are explicit loads.  Rows wrap
// in the row pointer.  On a 2 x k level the row above and the row below are the same row, and on an m x 2 level the
// left and the right neighbour are the same node: the window then simply holds the node twice and both taps are added.
// The row tasks are those ONE sample gets (torus_geom, the one statement of that rule: it fixes the number of partial
// sums, fea_per_parts), so a sample's partial sums are the same bits in any batch.  Pad columns are loaded with their
// vector but every value taken from them is selected out; nothing outside the m x n nodes is written.
// residual_restrict takes one thread per coarse node with modulo indexing at every size.
//
// The march itself stays in each family's stencil kernel, on these helpers: one march around an operator type was
// built and measured, and cost fea_per_sweep_f32 2 % at 4096^2.
#pragma once
#include "framed_strip.h"

namespace fea {

// one node row of a lane: x = own columns, hl / hr = the strip's outer neighbours (lanes 0 / 63), w0 = column 0
template <typename T, int V>
struct TorusRaw {
  T x[V];
  T hl, hr, w0;
};

template <typename T, int V>
__device__ __forceinline__ TorusRaw<T, V> torus_load(const T* __restrict__ rp, int cl, int cL, int n, int lane) {
  TorusRaw<T, V> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.x[k] = T(0);
  if (cl < n) vload<T, V>(rp + cl, r.x);  // columns cl .. cl+V-1 <= ld-1 (ld a multiple of V)
  r.hl = T(0);
  r.hr = T(0);
  if (lane == 0) r.hl = rp[cL];                           // exec-masked scalar loads
  if (lane == kWave - 1 && cl + V < n) r.hr = rp[cl + V];
  r.w0 = rp[0];
  return r;
}

// the window row: a[0] = left of the first own column, a[1 .. V] own, a[V+1] = right of the last own column; the right
// neighbour of column n-1 is column 0
template <typename T, int V>
__device__ __forceinline__ Row<T, V> torus_window(const TorusRaw<T, V>& r, int cl, int n) {
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

template <typename T, int V>
__device__ __forceinline__ void torus_store(T* p, const T (&o)[V], int cl, int n) {
  if (cl + V <= n) {
    vstore<T, V, false>(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (cl + k < n) p[k] = o[k];
  }
}

__device__ __forceinline__ int torus_wrap(int r, int m) { return r < 0 ? r + m : (r >= m ? r - m : r); }

struct TorusTask {
  int b, s, t, r0, r1, cl, cL, lane;
};
template <typename T>
__device__ __forceinline__ TorusTask torus_task(const TaskId& id, int m, int n, int rb) {
  TorusTask k;
  k.b = id.b;
  k.s = id.s;
  k.t = id.t;
  k.lane = lane_id();
  k.r0 = id.t * rb;
  k.r1 = min(k.r0 + rb, m);
  k.cl = id.s * Frame<T>::SW + Frame<T>::VEC * k.lane;
  k.cL = (k.cl == 0 ? n : k.cl) - 1;  // only lane 0 reads it: cl = c0 < n there
  return k;
}

// residual_restrict's thread: sample b, coarse node (I, J) and the wrapped fine rows r0 .. r2 and columns c0 .. c2
// around it.  The nine weighted residuals stay in each kernel (one body around a callable residual cost
// fea_coef_residual_restrict_f32 two register brackets).
struct TorusCoarse {
  long long b;
  int I, J, r0, r1, r2, c0, c1, c2;
};
template <typename A>
__device__ __forceinline__ bool torus_coarse(const A& g, TorusCoarse& k) {
  const long long per_b = (long long)g.mc * g.nc;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  k.b = i / per_b;
  if (k.b >= g.B) return false;
  const long long rem = i - k.b * per_b;
  k.I = (int)(rem / g.nc);
  k.J = (int)(rem - (long long)k.I * g.nc);
  k.r1 = 2 * k.I;
  k.c1 = 2 * k.J;
  k.r0 = k.r1 == 0 ? g.m - 1 : k.r1 - 1;
  k.r2 = k.r1 + 1;  // m, n even: 2 I + 1 <= m - 1
  k.c0 = k.c1 == 0 ? g.n - 1 : k.c1 - 1;
  k.c2 = k.c1 + 1;
  return true;
}

}  // namespace fea

// ------------------------------------------------------------------ host side: the checks and the task rule
// [B, m, ld] fields: extents lo .. 2^20 (lo = 1, or 2 where an element needs two distinct node rows and columns)
static inline bool torus_dim_ok(int n, int lo) { return n >= lo && n <= (1 << 20); }
template <typename T>
static bool torus_layout_ok(int m, int n, int ld, long long bs, int lo) {
  constexpr int V = Frame<T>::VEC;
  return torus_dim_ok(m, lo) && torus_dim_ok(n, lo) && ld >= n && ld % V == 0 && bs >= (long long)m * ld && bs % V == 0;
}
static inline bool torus_aligned(const void* p) { return p && (uintptr_t)p % 16 == 0; }
// two ranges of na and nb elements of T
template <typename T>
static bool torus_overlap(const T* a, long long na, const T* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(T);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(T);
  return a0 < b1 && b0 < a1;
}

// one thread per node of B samples of `nodes` nodes
static inline bool torus_node_grid(int B, long long nodes, dim3& grid) {
  const long long blocks = (B * nodes + 255) / 256;
  if (blocks > 0x7fffffffll) return false;
  grid = dim3((unsigned)blocks);
  return true;
}

// The geometry fields of PerArgs / CoefArgs.  Strips over the node columns 0 .. n-1, row tasks of the height ONE
// sample gets; per = the partial sums of one quantity of one sample.
template <typename T, typename A>
static void torus_geom(A& g, int m, int n, int ld, long long bs) {
  g.m = m; g.n = n; g.ld = ld; g.bs = bs;
  g.nstrips = div_up(n, Frame<T>::SW);
  g.rb = pick_rb(1, g.nstrips, m);
  g.ntr = div_up(m, g.rb);
  g.per = (long long)g.nstrips * g.ntr;
}
