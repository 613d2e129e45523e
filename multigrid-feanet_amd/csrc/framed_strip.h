// framed_strip.h — the strip helpers of the framed level kernels (framed_ops.hip, pcg_ops.hip): the framed
// layout, 16-byte row loads with DPP neighbours, the 3-row stencil window (kapply) and the Jacobi emit on it
// (jacobi), the 9-tap restriction (restrict9), the masked row store, the task decode, the coefficient tables in
// LDS and the launch geometry.  Layout and work decomposition: see framed_ops.hip.
#pragma once
#include <cstdlib>

#include "fea_common.h"

#include <type_traits>
#include <utility>

namespace fea {

template <typename T>
struct Frame {
  static constexpr int A = 128 / (int)sizeof(T);
  static constexpr int OFF = A - 1;
  static constexpr int VEC = 16 / (int)sizeof(T);
  static constexpr int SW = kWave * VEC;
};
constexpr int kRB = 32;     // fine rows per task (even: tasks start on odd rows)
constexpr int kWaves = 4;   // waves (tasks) per block
constexpr int kTabStride = 10;  // LDS table row: 9 stencil weights + omega/d
// Pattern windows (PRow, CRow::o, the prolongation's pe) hold BYTE offsets of a pattern's LDS table row
// (pattern * kTabStride * sizeof(T)), so a table read is one ds_read at that address
// plus the tap as an immediate offset, with no per-read index scaling
template <typename T>
__host__ __device__ constexpr int tab_row_bytes() { return kTabStride * (int)sizeof(T); }
template <typename T>
__device__ __forceinline__ T tabv(const T* t, int off, int d) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(t) + off + d * (int)sizeof(T));
}
// The restricted field f_c (a quarter of the level's bytes) is stored with normal stores (vstore<T, Q>) even
// when the level's own stores stream past the caches: the next kernel (the coarse level's restriction)
// reads it straight back, from the Infinity Cache instead of HBM.

static inline int div_up(int a, int b) { return (a + b - 1) / b; }

template <typename T>
static inline int mg_nstrips(int W) { return div_up(W - 2, Frame<T>::SW); }

// row pitch (elements) of a framed grid with W columns
template <typename T>
static inline int mg_ld(int W) {
  using F = Frame<T>;
  // room for the last strip's loads: plain strips (k * SW + halo) and the overlapped strips of
  // k_mg_sweep_restrict / k_mg_cycle_join (start <= W - 2, 64*VEC columns)
  // (any strip starts at a column <= W - 2, so W + 2*SW columns cover every variant's last loads)
  const int need = F::OFF + 2 + std::max(mg_nstrips<T>(W) * F::SW + F::VEC, W + 2 * F::SW);
  return div_up(need, F::A) * F::A;
}

// sample pitch of an H x W framed grid: H rows plus the ghost rows -1 and H
template <typename T>
static inline long long mg_bstride(int H, int W) { return (long long)(H + 2) * mg_ld<T>(W); }

// ---------------------------------------------------------------------------
// vector access helpers
// ---------------------------------------------------------------------------
template <typename T, int V>
struct VecOf;
template <>
struct VecOf<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <>
struct VecOf<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct VecOf<float, 2> { typedef float type __attribute__((ext_vector_type(2))); };

template <typename T, int V, bool NTL = false>
__device__ __forceinline__ void vload(const T* p, T (&x)[V]) {
  if constexpr (V == 1) {
    x[0] = *p;
  } else {
    const auto* q = reinterpret_cast<const typename VecOf<T, V>::type*>(p);
    typename VecOf<T, V>::type v;
    if constexpr (NTL)
      v = __builtin_nontemporal_load(q);
    else
      v = *q;
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] = v[k];
  }
}

// NT: nontemporal (streaming) store — used on levels too large to be re-read from cache.  A
// compile-time flag: with a runtime flag the two stores are merged before inlining and the
// nontemporal hint is lost.
template <typename T, int V, bool NT = false>
__device__ __forceinline__ void vstore(T* p, const T (&x)[V]) {
  constexpr bool nt = NT;
  if constexpr (V == 1) {
    if constexpr (nt)
      __builtin_nontemporal_store(x[0], p);
    else
      *p = x[0];
  } else {
    typename VecOf<T, V>::type v;
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = x[k];
    auto* q = reinterpret_cast<typename VecOf<T, V>::type*>(p);
    if constexpr (nt)
      __builtin_nontemporal_store(v, q);
    else
      *q = v;
  }
}

// V pattern bytes -> ints
template <int V>
__device__ __forceinline__ void pload(const uint8_t* p, int (&o)[V]) {
  if constexpr (V == 1) {
    o[0] = p[0];
  } else if constexpr (V == 2) {
    const unsigned v = *reinterpret_cast<const unsigned short*>(p);
    o[0] = v & 0xff;
    o[1] = v >> 8;
  } else {
    const unsigned v = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (v >> (8 * k)) & 0xff;
  }
}

// A row segment of one lane: a[0] = column c-1 (L), a[1..V] = own columns, a[V+1] = c+V (R),
// a[V+2] = c+V+1 (RR).
template <typename T, int V>
struct Row {
  T a[V + 3];
};
template <int V>
struct PRow {  // LDS table row byte offsets (pattern * tab_row_bytes<T>()) for the same columns
  int a[V + 3];
};

// Rows are loaded in two halves so a load can be issued one iteration ahead of its use:
// raw_*() issues the 16-byte vector load of the lane's columns plus the 16-byte halo load
// (lane 0: columns c0-V..c0-1, lane 63: c0+SW..), finish() builds the window row with DPP.
template <typename T, int V>
struct RawRow {
  T x[V], h[V];
};
template <int V>
struct RawP {
  int x[V], h[V];
};

template <typename T, int V, bool NTL = false>
__device__ __forceinline__ RawRow<T, V> raw_row(const T* __restrict__ rp, int lane) {
  RawRow<T, V> r;
  vload<T, V, NTL>(rp + V * lane, r.x);
  // halo: only the two edge lanes load (exec-masked), the other lanes' h is never read
#pragma unroll
  for (int k = 0; k < V; ++k) r.h[k] = T(0);
  if (lane == 0 || lane == kWave - 1) vload<T, V>(rp + (lane == 0 ? -V : kWave * V), r.h);
  return r;
}

template <typename T, int V>
__device__ __forceinline__ Row<T, V> finish(const RawRow<T, V>& r) {
  Row<T, V> w;
#pragma unroll
  for (int k = 0; k < V; ++k) w.a[k + 1] = r.x[k];
  w.a[0] = shr1(r.x[V - 1], r.h[V - 1]);
  w.a[V + 1] = shl1(r.x[0], r.h[0]);
  w.a[V + 2] = shl1(r.x[1 % V], r.h[1 % V]);
  return w;
}

template <int V>
__device__ __forceinline__ RawP<V> raw_prow(const uint8_t* __restrict__ pp, int lane) {
  RawP<V> r;
  pload<V>(pp + V * lane, r.x);
#pragma unroll
  for (int k = 0; k < V; ++k) r.h[k] = 0;
  if (lane == 0 || lane == kWave - 1) pload<V>(pp + (lane == 0 ? -V : kWave * V), r.h);
  return r;
}

template <typename T, int V>
__device__ __forceinline__ PRow<V> finish_p(const RawP<V>& r) {
  PRow<V> w;
#pragma unroll
  for (int k = 0; k < V; ++k) w.a[k + 1] = r.x[k] * tab_row_bytes<T>();
  w.a[0] = shr1(r.x[V - 1], r.h[V - 1]) * tab_row_bytes<T>();
  w.a[V + 1] = shl1(r.x[0], r.h[0]) * tab_row_bytes<T>();
  w.a[V + 2] = shl1(r.x[1 % V], r.h[1 % V]) * tab_row_bytes<T>();
  return w;
}

// (K u) at own column k (k = 0..V, k = V is the R column) from the 3-row window.
// Two-material (MULTI): KNet applies tap t with the weight of the NEIGHBOUR's pattern (split, then convolve:
// FEANet/model.py:22-30); K is a symmetric FE stiffness, so that weight is bit for bit the mirrored tap 8 - t of the
// CENTRE's pattern (stencil_table(); MultigridSolver checks it on every level's map, mesh_setup
// .stencil_mirror_mismatches).  All nine weights then come from one table row — one base address, adjacent
// offsets — instead of three rows picked by the window's neighbour patterns; taps are summed in the same order, so
// every value is the same bits as with the neighbours' rows.
template <typename T, int V, bool MULTI>
__device__ __forceinline__ T kapply(const Row<T, V>& w0, const Row<T, V>& w1, const Row<T, V>& w2,
                                    const PRow<V>& p0, const PRow<V>& p1, const PRow<V>& p2, int k,
                                    const T (&ks)[9], const T* tab) {
  T acc;
  if constexpr (MULTI) {
    const int pc = p1.a[k + 1];
    acc = tabv(tab, pc, 8) * w0.a[k];
    acc += tabv(tab, pc, 7) * w0.a[k + 1];
    acc += tabv(tab, pc, 6) * w0.a[k + 2];
    acc += tabv(tab, pc, 5) * w1.a[k];
    acc += tabv(tab, pc, 4) * w1.a[k + 1];
    acc += tabv(tab, pc, 3) * w1.a[k + 2];
    acc += tabv(tab, pc, 2) * w2.a[k];
    acc += tabv(tab, pc, 1) * w2.a[k + 1];
    acc += tabv(tab, pc, 0) * w2.a[k + 2];
  } else {
    acc = ks[0] * w0.a[k];
    acc += ks[1] * w0.a[k + 1];
    acc += ks[2] * w0.a[k + 2];
    acc += ks[3] * w1.a[k];
    acc += ks[4] * w1.a[k + 1];
    acc += ks[5] * w1.a[k + 2];
    acc += ks[6] * w2.a[k];
    acc += ks[7] * w2.a[k + 1];
    acc += ks[8] * w2.a[k + 2];
  }
  return acc;
}

// One Jacobi-swept value, omd (f - K x) + x, at own column k of the window rows a, b, c (the shared emit of the
// sweep, the prolongation kernels and the two-level prolongation's coarse stage).  The last line is one source
// expression on purpose: -ffp-contract=on fuses within an expression only, so splitting it changes the bits.
template <typename T, int N, bool MULTI>
__device__ __forceinline__ T jacobi(const Row<T, N>& a, const Row<T, N>& b, const Row<T, N>& c, const PRow<N>& pa,
                                    const PRow<N>& pb, const PRow<N>& pc, int k, T f, const T (&ks)[9], T om,
                                    const T* tab) {
  const T acc = kapply<T, N, MULTI>(a, b, c, pa, pb, pc, k, ks, tab);
  const T omk = MULTI ? tabv(tab, pb.a[k + 1], 9) : om;
  return omk * (f - acc) + b.a[k + 1];
}

// Coarse value of the 9-tap restriction from three residual rows in grid order: the sum over (ky, kx) of
// R[ky][kx] r_ky[o + kx], nine statements in this order (each product fuses with its own add only).  MULTI: each
// tap with the weight of its fine node's pattern; pa, pb, pc hold the rows' table-row offsets, the same columns
// from index po on.
template <typename T, bool MULTI, int NR, int NP>
__device__ __forceinline__ T restrict9(const T (&rs)[9], const T* rtb, const T (&ra)[NR], const T (&rb)[NR],
                                       const T (&rc)[NR], int o, const int (&pa)[NP], const int (&pb)[NP],
                                       const int (&pc)[NP], int po) {
  T acc;
  if constexpr (!MULTI) {
    acc = rs[0] * ra[o];
    acc += rs[1] * ra[o + 1];
    acc += rs[2] * ra[o + 2];
    acc += rs[3] * rb[o];
    acc += rs[4] * rb[o + 1];
    acc += rs[5] * rb[o + 2];
    acc += rs[6] * rc[o];
    acc += rs[7] * rc[o + 1];
    acc += rs[8] * rc[o + 2];
  } else {
    acc = tabv(rtb, pa[po], 0) * ra[o];
    acc += tabv(rtb, pa[po + 1], 1) * ra[o + 1];
    acc += tabv(rtb, pa[po + 2], 2) * ra[o + 2];
    acc += tabv(rtb, pb[po], 3) * rb[o];
    acc += tabv(rtb, pb[po + 1], 4) * rb[o + 1];
    acc += tabv(rtb, pb[po + 2], 5) * rb[o + 2];
    acc += tabv(rtb, pc[po], 6) * rc[o];
    acc += tabv(rtb, pc[po + 1], 7) * rc[o + 1];
    acc += tabv(rtb, pc[po + 2], 8) * rc[o + 2];
  }
  return acc;
}

template <typename T>
struct MgArgs {
  const T* u;
  const T* f;
  T* out;
  T* out2;
  const T* ec;
  const uint8_t* pid;
  const uint8_t* pidc;
  const T* ktab;
  const T* omd;
  const T* rtab;
  const T* ptab;
  double* part;
  int ntab, nrtab, nptab;
  T w;
  T w2;  // second ratio (cycle join: w1 of the prolongation)
  int H, W, ld;  // rows, columns of the (local) grid
  long long bs;
  int Hc, Wc, ldc;
  long long bsc;
  int Hc2, Wc2, ldc2;  // the level below the coarse one (k_mg_zero_restrict2: its right-hand side in out2;
  long long bsc2;      //   k_mg_prolong2: its correction in ec2, its pattern map in pidc2)
  const T* ec2;
  const uint8_t* pidc2;
  int nstrips, ntr;  // strips per row, row tasks per sample
  int rb;            // fine rows per row task (even)
  int rlo, rhi;      // row range of the residual norm
  int clo, chi;      // column range of the residual norm
  int nt;            // 1: nontemporal stores (level larger than FEANET_NT_BYTES); 2: also loads (sweep, join)
  int rev;           // decode_task_lin: deal the launch's tasks in reverse order (last task first)
  int flip;          // cycle join: every task streams in the other direction (even tasks bottom-up, odd top-down)
  // (rev and flip are always 0 — nothing sets them any more; the kernels read them, so dropping them changes device code)
  // cycle join over up to 4 rectangles (nrect > 0; a domain-decomposed rank's border strips, then its interior):
  // rectangle r = coarse rows [rI0[r], rI1[r]) x fine columns [rc0[r], rc1[r]) (odd bounds, coarse column J owned
  // with its fine columns 2J-1, 2J), its nstrips rns[r], its row tasks rnt[r]; the launch's tasks per sample are
  // rectangle by rectangle, rt[r] the first of rectangle r
  int nrect;
  int rI0[4], rI1[4], rc0[4], rc1[4], rns[4], rt[5];
  // zero-guess restrictions of a domain-decomposed rank (k_mg_zero_restrict, k_mg_zero_restrict2): the output level's
  // block [gr0, gr1) x [gc0, gc1) (local rows / columns) also goes to gsend[b][r - gr0][c - gc0] — the all-gather's
  // send buffer of the agglomeration, written by the kernel that computes it instead of a copy launch after it
  T* gsend;
  int gr0, gr1, gc0, gc1;
};

// the agglomeration send-buffer store of a zero-guess restriction (MgArgs::gsend), node (r, c) of the output level
template <typename T>
__device__ __forceinline__ void gather_store(const MgArgs<T>& g, int b, int r, int c, T v) {
  if (g.gsend && r >= g.gr0 && r < g.gr1 && c >= g.gc0 && c < g.gc1)
    g.gsend[((long long)b * (g.gr1 - g.gr0) + (r - g.gr0)) * (g.gc1 - g.gc0) + (c - g.gc0)] = v;
}

struct TaskId {
  int b, s, t;
  bool valid;
};

__device__ __forceinline__ TaskId decode_task(int nstrips, int ntr) {
  const int nsg = (nstrips + kWaves - 1) / kWaves;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int per_b = ntr * nsg;
  TaskId id;
  id.b = bid / per_b;
  const int rem = bid - id.b * per_b;
  id.t = rem / nsg;
  const int sg = rem - id.t * nsg;
  id.s = sg * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: scalar
  id.valid = id.s < nstrips;
  return id;
}

// Loads ktab/omd (stride 10) and optionally a second 9-wide table into LDS.
template <typename T>
__device__ __forceinline__ void load_tables(T* tab, const T* ktab, const T* omd, int ntab, T* tab2,
                                            const T* t2, int n2) {
  for (int i = threadIdx.x; i < ntab * kTabStride; i += blockDim.x) {
    const int p = i / kTabStride, d = i - p * kTabStride;
    tab[i] = (d == 9) ? (omd ? omd[p] : T(0)) : ktab[p * 9 + d];
  }
  if (tab2)
    for (int i = threadIdx.x; i < n2 * kTabStride; i += blockDim.x) {
      const int p = i / kTabStride, d = i - p * kTabStride;
      tab2[i] = (d == 9) ? T(0) : t2[p * 9 + d];
    }
}

// V values of one row, columns cl .. cl+V-1, of a grid W columns wide: one vector store, or the columns left of the
// boundary column W-1 one by one.  Fine rows (V = VEC, the level's W) and restricted rows (V = VEC/2, Wc) alike.
template <typename T, int V, bool NT>
__device__ __forceinline__ void store_masked(T* p, const T (&o)[V], int cl, int W) {
  if (cl + V - 1 <= W - 2) {
    vstore<T, V, NT>(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (cl + k <= W - 2) p[k] = o[k];
  }
}

}  // namespace fea

using namespace fea;

// Grid sizes: H, W >= 3; the intergrid kernels additionally need odd H and W (coarse (H+1)/2).
static inline bool mg_dim_ok(int n) { return n >= 3 && n <= (1 << 20) + 1; }
static inline bool mg_dims_ok(int H, int W) { return mg_dim_ok(H) && mg_dim_ok(W); }
static inline bool mg_odd(int H, int W) { return (H & 1) && (W & 1); }

// Rows per wave task: the largest even count (<= kRB) that still gives >= kTargetWaves waves, so small
// levels are spread over the chip instead of being marched row by row by a few waves (1024 / 4096 / 8192
// measured slower than 2048 on levels 1-2, profiles/r02_ab).
constexpr int kTargetWaves = 2048;  // 8 waves per CU
static int target_waves() { return kTargetWaves; }
static inline int pick_rb(int B, int nstrips, int rows, int maxrb = kRB) {
  const int tw = target_waves();
  for (int rb = maxrb; rb > 2; rb /= 2)
    if ((long long)B * nstrips * div_up(rows, rb) >= tw) return rb;
  return 2;
}

// Levels whose fields exceed this many bytes stream their stores past the caches (measured on the
// 4097^2 fp64 sweep: 64.8 us with nontemporal stores vs 84.6 us without).  64 MiB: the three fields
// of a 2049^2 fp64 level (~36 MB each) stay in the 256 MiB Infinity Cache between the level's
// restriction and prolongation (V-cycle 201 -> 196 us with 64 instead of 32 MiB, A/B on MI355X).
static long long nt_bytes() {
  const char* e = getenv("FEANET_NT_BYTES");
  return e ? atoll(e) : (64ll << 20);
}

template <typename T>
static MgArgs<T> mg_args(int H, int W, int ld, long long bs, int B) {
  MgArgs<T> g{};
  g.nt = (long long)B * bs * (long long)sizeof(T) > nt_bytes();
  g.H = H;
  g.W = W;
  g.ld = ld;
  g.bs = bs;
  g.nstrips = mg_nstrips<T>(W);
  g.rb = pick_rb(B, g.nstrips, H - 2);
  g.ntr = div_up(H - 2, g.rb);
  g.rlo = 1;
  g.rhi = H - 1;
  g.clo = 1;
  g.chi = W - 1;
  return g;
}

template <typename T>
static inline bool layout_ok(int H, int W, int ld, long long bs) {
  return mg_dims_ok(H, W) && ld >= mg_ld<T>(W) && ld % Frame<T>::A == 0 && bs >= (long long)(H + 2) * ld;
}

static inline dim3 mg_grid(int B, int ntr, int nstrips) {
  return dim3((unsigned)(B * ntr * div_up(nstrips, kWaves)));
}
