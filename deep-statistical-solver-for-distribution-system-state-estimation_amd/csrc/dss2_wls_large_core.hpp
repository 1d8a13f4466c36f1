// The blocked fp64 WLS solve with the gain matrix in global memory, shared by csrc/dss2_wls_large.hip (the plain estimator),
// csrc/dss2_wls_robust.hip (the Huber M-estimator's large form) and csrc/dss2_wls_bad_data.hip (the blocked bad-data kernel): the workspace layout, the LDS carve, the rows' assembly, the blocked
// Cholesky and back substitution, the Gauss-Newton loop (wl_gauss_newton), the ONE kernel body on this layout (wls_blocked_kernel: the
// two estimators are two instantiations of it), and the host side -- the entries' size check, grid and workspace check, and their
// launch path (wl_launch).  The layout and every step are described in the header of dss2_wls_large.hip; nothing here depends on which
// kernel runs it.  The steps find a slice's rows through a rows object (WlRows below: this layout), so that dss2_wls_banded.hpp runs
// them on a band of the gain matrix.
#pragma once
#include "dss2_wls_core.hpp"

namespace dss2 {

constexpr int WL_T = 256;                // threads of a workgroup
constexpr int WL_NB = 16;                // columns of a block column
constexpr int WL_TILE = 8;               // the trailing update's register tile is WL_TILE x WL_TILE
constexpr int WL_MAX_NODES = 256;        // two workgroups of the largest graph share the LDS of a CU
constexpr int WL_GROUPS = 512;

typedef double wl_d2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr size_t wl_row_off(int r) {
  return (size_t)(WL_NB * WL_NB) * ((size_t)(r / WL_NB) * (r / WL_NB + 1) / 2) + (size_t)(r % WL_NB) * WL_NB * (r / WL_NB + 1);
}
__host__ __device__ constexpr size_t wl_graph_doubles(int n) {       // block rows of ns + 1 rows, the lower triangle of blocks
  return (size_t)(WL_NB * WL_NB) * ((size_t)((2 * n + WL_NB) / WL_NB) * ((2 * n + WL_NB) / WL_NB + 1) / 2);
}
__host__ __device__ constexpr int wl_pstride(int n) { return (2 * n + 1 + WL_TILE - 1) / WL_TILE * WL_TILE; }
// (S: the panel's stride.  The dense rows' is wl_pstride(n); a band's is shorter, dss2_wls_banded.hpp)
__host__ __device__ constexpr size_t wl_lds_doubles(int n, int S) { return (size_t)WL_NB * S + WL_NB * WL_NB + WL_NB + 4 * (size_t)n; }
__host__ __device__ constexpr size_t wl_lds_bytes(int n, int S) { return wl_lds_doubles(n, S) * 8 + 16 + ((size_t)n + 15) / 16 * 16; }
__host__ __device__ constexpr size_t wl_lds_doubles(int n) { return wl_lds_doubles(n, wl_pstride(n)); }
__host__ __device__ constexpr size_t wl_lds_bytes(int n) { return wl_lds_bytes(n, wl_pstride(n)); }
static_assert(2 * wl_lds_bytes(WL_MAX_NODES) <= (size_t)kMaxLdsBytes, "two workgroups of the largest graph per CU");
static_assert(WL_NB == 16 && WL_TILE == 8 && WL_NB % WL_TILE == 0, "the unrolled loops and the readlane indices assume 16 and 8");

struct WlLds { double* Pt; double* Ld; double* invd; double* u; double* du; int* ctl; unsigned char* slk; int S; };
__device__ __forceinline__ WlLds wl_carve(unsigned char* smem, int n, int S) {
  WlLds l;
  l.S = S;
  l.Pt = reinterpret_cast<double*>(smem);
  l.Ld = l.Pt + (size_t)WL_NB * l.S;
  l.invd = l.Ld + WL_NB * WL_NB;
  l.u = l.invd + WL_NB;
  l.du = l.u + 2 * n;
  l.ctl = reinterpret_cast<int*>(smem + wl_lds_doubles(n, S) * 8);
  l.slk = smem + wl_lds_doubles(n, S) * 8 + 16;
  return l;
}
__device__ __forceinline__ WlLds wl_carve(unsigned char* smem, int n) { return wl_carve(smem, n, wl_pstride(n)); }

// Where the steps below find the ROWS of a slice A.  WlRows is the lower triangle of blocks above; WbRows (dss2_wls_banded.hpp) keeps a
// band of block columns per block row.  Both give
//   doubles(n)     the slice's length for n buses (wl_form zeroes it)
//   at(A, r)       row r < ns as a pointer to its column 0: at(A, r)[c] is G[r, c] for every column c the row stores
//   rhs(A, ns)     the right-hand side b, ns entries
//   left(j0)       the first column that the rows of the block row at j0 store
//   below(j0, w, ns)  the PANEL of the block column j0 .. j0 + w: the rows `first` .. `end` - 1 that have entries in these columns, and
//                  the b row, which counts as row `end`; at(A, i) as above, pt(i) the row's place in a row of Pt
// The slice travels beside the object as a `double* __restrict__`, and n and ns come in as arguments, so that WlRows has no state: the
// dense kernels then compile to what they were (the blocked bad-data kernel sits at 256 registers and spilled with n kept in the object).
struct WlPanelRows {
  int first, end;
  __device__ __forceinline__ double* at(double* A, int i) const { return A + wl_row_off(i); }      // (the b row is row ns of the slice)
  __device__ __forceinline__ int pt(int i) const { return i; }
};
struct WlRows {
  __device__ __forceinline__ size_t doubles(int n) const { return wl_graph_doubles(n); }
  __device__ __forceinline__ double* at(double* A, int r) const { return A + wl_row_off(r); }
  __device__ __forceinline__ double* rhs(double* A, int ns) const { return A + wl_row_off(ns); }
  __device__ __forceinline__ int left(int) const { return 0; }
  __device__ __forceinline__ WlPanelRows below(int j0, int w, int ns) const { return WlPanelRows{j0 + w, ns}; }
};

// lane `lane`'s x in every lane (`lane` is a constant after unrolling: two v_readlane_b32)
__device__ __forceinline__ double wl_lane(double x, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// A <- 0, then every row by its owner.  Starts with a barrier (u, slk and whatever read A before are done with).  `mask` is the
// removal mask of dss2_wls_core.hpp (WsNoMask, the default, compiles to nothing: the plain and the Huber kernel).
template <class Rows, class Wt = WsNoWeight, class Mask = WsNoMask>
__device__ __forceinline__ void wl_form(const dss2_wls_solve_args& a, const WsGraph& g, double* __restrict__ A, const Rows rows, int ns, int tid, const Wt& wt = Wt(),
                                        const Mask& mask = Mask()) {
  const size_t pairs = rows.doubles(g.n) / 2;
  __syncthreads();
  for (size_t p = tid; p < pairs; p += WL_T) reinterpret_cast<wl_d2*>(A)[p] = wl_d2{0.0, 0.0};
  __syncthreads();
  for (int r = tid; r < ns; r += WL_T) ws_accumulate_row_at(a, g, r, rows.at(A, r), rows.rhs(A, ns), mask, wt);
}

// Wave 0: the diagonal block at (j0, j0), w columns wide, factorised in registers; lane i < w holds row i.  Returns whether every pivot
// was > 0 and finite (uniform over the wave).
template <class Rows>
__device__ __forceinline__ bool wl_factor_diag(double* __restrict__ A, const Rows rows, const WlLds& l, int j0, int w, int lane) {
  const bool mine = lane < w;
  double* grow = rows.at(A, j0 + (mine ? lane : 0)) + j0;
  double row[WL_NB];
#pragma unroll
  for (int k = 0; k < WL_NB; ++k) row[k] = (mine && k <= lane) ? grow[k] : 0.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < WL_NB; ++j) {
    const double d = wl_lane(row[j], j);
    const bool good = d > 0.0 && d < INFINITY;
    if (j < w) ok = ok && good;
    const double s = good ? sqrt(d) : 1.0;
    row[j] = lane == j ? s : row[j] / s;              // (0 in the lanes above the diagonal)
#pragma unroll
    for (int k = j + 1; k < WL_NB; ++k) {
      const double lkj = wl_lane(row[j], k);
      if (lane >= k) row[k] -= row[j] * lkj;
    }
  }
  if (lane < WL_NB) {
    double dg = 1.0;
#pragma unroll
    for (int k = 0; k < WL_NB; ++k) {
      const bool in = mine && k <= lane;
      l.Ld[lane * WL_NB + k] = in ? row[k] : 0.0;
      if (in) grow[k] = row[k];
      if (k == lane) dg = row[k];
    }
    l.invd[lane] = 1.0 / dg;                          // (1 beyond the block's width)
  }
  return ok;
}

// The panel below the diagonal block: thread i solves row i (p.first .. p.end, the b row included) against Ld.  Beyond the block's width
// (the last block column only) A holds zeros and Ld is 0: those entries stay 0.
template <class Panel>
__device__ __forceinline__ void wl_panel(double* __restrict__ A, const Panel p, const WlLds& l, int j0, int tid) {
  for (int i = p.first + tid; i <= p.end; i += WL_T) {
    wl_d2* prow = reinterpret_cast<wl_d2*>(p.at(A, i) + j0);
    double x[WL_NB];
#pragma unroll
    for (int k = 0; k < WL_NB / 2; ++k) { const wl_d2 v = prow[k]; x[2 * k] = v.x; x[2 * k + 1] = v.y; }
#pragma unroll
    for (int j = 0; j < WL_NB; ++j) {
      x[j] *= l.invd[j];
#pragma unroll
      for (int m = j + 1; m < WL_NB; ++m) x[m] -= x[j] * l.Ld[m * WL_NB + j];
    }
#pragma unroll
    for (int k = 0; k < WL_NB / 2; ++k) prow[k] = wl_d2{x[2 * k], x[2 * k + 1]};
#pragma unroll
    for (int k = 0; k < WL_NB; ++k) l.Pt[(size_t)k * l.S + p.pt(i)] = x[k];
  }
}

// A[i, c] -= sum_j Pt[j][i] Pt[j][c] for j1 <= c <= i <= ns, c < ns, on 8 x 8 tiles: tile p = ti (ti + 1) / 2 + tj, tj <= ti
// (j1 = rw.first, ns = rw.end: the panel's rows, the b row last)
template <class Panel>
__device__ __forceinline__ void wl_trailing(double* __restrict__ A, const Panel rw, const WlLds& l, int tid) {
  const int j1 = rw.first, ns = rw.end;
  const int ntr = (ns + 1 - j1 + WL_TILE - 1) / WL_TILE, ntiles = ntr * (ntr + 1) / 2;
  for (int p = tid; p < ntiles; p += WL_T) {
    int ti = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
    while (ti * (ti + 1) / 2 > p) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= p) ++ti;
    const int tj = p - ti * (ti + 1) / 2;
    const int i0 = j1 + WL_TILE * ti, c0 = j1 + WL_TILE * tj;
    double acc[WL_TILE][WL_TILE];
#pragma unroll
    for (int q = 0; q < WL_TILE; ++q)
#pragma unroll
      for (int c = 0; c < WL_TILE; ++c) acc[q][c] = 0.0;
#pragma unroll 4
    for (int j = 0; j < WL_NB; ++j) {
      const wl_d2* pr2 = reinterpret_cast<const wl_d2*>(l.Pt + (size_t)j * l.S + rw.pt(i0));
      const wl_d2* pc2 = reinterpret_cast<const wl_d2*>(l.Pt + (size_t)j * l.S + rw.pt(c0));
      double pr[WL_TILE], pc[WL_TILE];
#pragma unroll
      for (int q = 0; q < WL_TILE / 2; ++q) {
        const wl_d2 v = pr2[q], c = pc2[q];
        pr[2 * q] = v.x; pr[2 * q + 1] = v.y; pc[2 * q] = c.x; pc[2 * q + 1] = c.y;
      }
#pragma unroll
      for (int q = 0; q < WL_TILE; ++q)
#pragma unroll
        for (int c = 0; c < WL_TILE; ++c) acc[q][c] += pr[q] * pc[c];
    }
    if (tj < ti && i0 + WL_TILE - 1 <= ns) {            // a whole tile below the diagonal
#pragma unroll
      for (int q = 0; q < WL_TILE; ++q) {
        wl_d2* arow = reinterpret_cast<wl_d2*>(rw.at(A, i0 + q) + c0);
#pragma unroll
        for (int c = 0; c < WL_TILE / 2; ++c) {
          wl_d2 v = arow[c];
          v.x -= acc[q][2 * c]; v.y -= acc[q][2 * c + 1];
          arow[c] = v;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < WL_TILE; ++q) {
        const int i = i0 + q;
        if (i > ns) continue;
        double* arow = rw.at(A, i);
#pragma unroll
        for (int c = 0; c < WL_TILE; ++c)
          if (c0 + c <= i && c0 + c < ns) arow[c0 + c] -= acc[q][c];
      }
    }
  }
}

// Cholesky of A WITH the b row (row ns), which leaves as y = L^-1 b.  Wave 0's return value says whether every pivot was good.
template <class Rows>
__device__ __forceinline__ bool wl_factor(double* __restrict__ A, const Rows rows, const WlLds& l, int ns, int tid) {
  bool ok = true;
  for (int j0 = 0; j0 < ns; j0 += WL_NB) {
    const int w = ns - j0 < WL_NB ? ns - j0 : WL_NB;
    __syncthreads();                                   // the rows' owners, or the previous trailing update, have written the block
    if (tid < 64) ok = wl_factor_diag(A, rows, l, j0, w, tid) && ok;
    __syncthreads();
    const auto below = rows.below(j0, w, ns);
    wl_panel(A, below, l, j0, tid);
    __syncthreads();
    if (j0 + w < ns) wl_trailing(A, below, l, tid);
  }
  return ok;
}

// L^T du = y, block column by block column from the last; starts and ends with a barrier
template <class Rows>
__device__ __forceinline__ void wl_back_substitute(double* __restrict__ A, const Rows rows, const WlLds& l, int ns, int tid) {
  __syncthreads();
  const double* y = rows.rhs(A, ns);
  for (int c = tid; c < ns; c += WL_T) l.du[c] = y[c];
  __syncthreads();
  for (int j0 = (ns - 1) / WL_NB * WL_NB; j0 >= 0; j0 -= WL_NB) {
    const int w = ns - j0 < WL_NB ? ns - j0 : WL_NB;
    if (tid < 64) {                                    // the diagonal block: lane c owns column c of it and du[j0 + c]
      const bool mine = tid < w;
      double Lc[WL_NB], dg = 1.0;
#pragma unroll
      for (int j = 0; j < WL_NB; ++j) {
        Lc[j] = (mine && j >= tid && j < w) ? rows.at(A, j0 + j)[j0 + tid] : 0.0;
        if (mine && j == tid) dg = Lc[j];
      }
      const double inv = 1.0 / dg;
      double yv = mine ? l.du[j0 + tid] : 0.0;
#pragma unroll
      for (int j = WL_NB - 1; j >= 0; --j) {
        if (j < w) {
          const double xj = wl_lane(yv * inv, j);
          if (tid < j) yv -= Lc[j] * xj;
          else if (tid == j) yv = xj;
        }
      }
      if (mine) l.du[j0 + tid] = yv;
    }
    __syncthreads();
    for (int c = rows.left(j0) + tid; c < j0; c += WL_T) {   // the columns left of the block: rows of A, coalesced over c
      double s = l.du[c];
      for (int j = 0; j < w; ++j) s -= rows.at(A, j0 + j)[c] * l.du[j0 + j];
      l.du[c] = s;
    }
    __syncthreads();
  }
}

// ws_gauss_newton's counterpart on this layout: Gauss-Newton from the state in LDS, at most a.max_iter iterations (the trip count is
// fixed; a graph that has stopped skips the body, uniformly over its workgroup).  Adds the updates applied to t.iters, sets t.status
// (1, then 0 or 2) and t.last.  wt.at(it) is the weighting of iteration `it`, `mask` the removal mask.  Ends with a barrier, after which
// l.ctl = {stop, apply} of the last iteration run: stop without apply is a failed factorisation.
template <class Rows, class Wt, class Mask = WsNoMask>
__device__ __forceinline__ void wl_gauss_newton(const dss2_wls_solve_args& a, const WsGraph& g, double* __restrict__ A, const Rows rows, const WlLds& l, int ns,
                                                int tid, WsTally& t, const Wt& wt, const Mask& mask = Mask()) {
  t.status = 1;
  bool active = true;                                  // uniform over the workgroup
  for (int it = 0; it < a.max_iter; ++it) {
    if (active) {
      wl_form(a, g, A, rows, ns, tid, wt.at(it), mask);
      const bool ok = wl_factor(A, rows, l, ns, tid);
      wl_back_substitute(A, rows, l, ns, tid);
      ws_decide(a, l.du, l.ctl, ns, tid, ok, t);
      __syncthreads();
      if (l.ctl[1]) for (int r = tid; r < ns; r += WL_T) l.u[r] += l.du[r];
      active = l.ctl[0] == 0;
    }
  }
  __syncthreads();
}

// The kernel on this layout: one workgroup of WL_T threads per graph and workspace slice, the workgroups stride over the graphs.
// A graph's n (ws_range) sets its carve, its panel stride and every trip count; LDS and the slice were sized for the bound.
// Args is dss2_wls_large_args (the plain estimator) or dss2_wls_robust_args (the Huber one), as for wls_lds_kernel.
template <class Args>
__global__ void __launch_bounds__(WL_T) wls_blocked_kernel(const Args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wl_smem[];
  const dss2_wls_solve_args& a = ws_solve_block(b);
  // the slice is sized by nodes_per_graph (with a graph_ptr: the bound); a graph uses the rows 0 .. 2 n of it, whose offsets depend on the row alone
  double* A = static_cast<double*>(b.workspace) + (size_t)blockIdx.x * wl_graph_doubles(a.nodes_per_graph);
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  auto wt = ws_weighting(b);
  using Wt = decltype(wt);
  const int64_t n_graphs = ws_n_graphs(a);
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    const WsRange rg = ws_range(a, gr);
    if (!rg.ok) {                                      // uniform over the workgroup
      if (tid == 0) {
        ws_refuse(a, gr);
        if constexpr (Wt::robust) b.n_downweighted[gr] = 0;
      }
      continue;
    }
    const int n = rg.n, ns = 2 * n;
    const WlLds l = wl_carve(wl_smem, n);
    if constexpr (Wt::robust) wt.cnt = reinterpret_cast<int*>(l.Pt);   // the panel is idle after the last factorisation: n ints of its 16 (2 n + 1) doubles
    const WsGraph g = ws_graph(rg.base, n, vlv, l.u, l.slk);
    const WsLds start = {nullptr, nullptr, l.u, l.du, l.ctl, l.slk};
    ws_load_start<WL_T>(a, g, start, tid);
    WsTally t = {0, 1, 0.0};
    wl_gauss_newton(a, g, A, WlRows(), l, ns, tid, t, wt);
    if constexpr (Wt::robust) wt.n_down = b.n_downweighted + gr;
    ws_finish<WL_T>(a, g, gr, l.du, ns, tid, t, wt);   // (the objective's per-bus parts go through du)
  }
}

// ---- host side: the grid and the size check of the entries that run on this layout (`who` names the entry in the message)
inline int64_t wl_grid(const dss2_wls_solve_args& a) {
  const int64_t n_graphs = ws_n_graphs(a);
  int64_t grid = WL_GROUPS;
  if (a.max_groups > 0 && a.max_groups < grid) grid = a.max_groups;
  return n_graphs < grid ? n_graphs : grid;
}
inline int wl_check_size(const dss2_wls_solve_args& a, const char* who) {
  if (int rc = ws_check_batch(a, who)) return rc;
  if (a.nodes_per_graph > WL_MAX_NODES) {
    set_error("%s: %d buses per graph: at most %d (a block column's panel of the gain matrix lives in LDS)", who, a.nodes_per_graph, WL_MAX_NODES);
    return 2;
  }
  return 0;
}
inline size_t wl_workspace_bytes(int nodes_per_graph, int64_t groups) {
  if (nodes_per_graph <= 0 || nodes_per_graph > WL_MAX_NODES || groups <= 0) return 0;
  return (size_t)groups * wl_graph_doubles(nodes_per_graph) * 8;
}
// the checks of a large entry's workspace and of the rest of its arguments, after wl_check_size; 0 or 2
inline int wl_check_workspace(const dss2_wls_solve_args& a, const void* workspace, uint64_t workspace_bytes, const char* who) {
  if (a.max_groups < 0) { set_error("%s: bad leading dimension or max_groups", who); return 2; }
  const int n = a.nodes_per_graph;
  const int64_t grid = wl_grid(a);
  const size_t need = wl_workspace_bytes(n, grid);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) { set_error("%s: the workspace is null or not 16-byte aligned", who); return 2; }
  if (workspace_bytes < need) {
    set_error("%s: the workspace has %llu bytes, %lld workgroups of %d buses need %llu", who, (unsigned long long)workspace_bytes,
              (long long)grid, n, (unsigned long long)need);
    return 2;
  }
  return ws_check_rest(a, who);
}
// The launch of kernel K on this layout, after the entry's checks (ws_launch's counterpart; the flag is K's own here too).  extra_lds:
// what K keeps behind the carve of the bound.
template <auto K, class Args>
inline int wl_launch(const Args& b, const char* who, hipStream_t s, size_t extra_lds = 0) {
  const dss2_wls_solve_args& a = b.solve;
  static std::atomic<uint32_t> done{0};
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(K), done, who)) return rc;
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  hipLaunchKernelGGL(K, dim3((unsigned)wl_grid(a)), dim3(WL_T), wl_lds_bytes(a.nodes_per_graph) + extra_lds, s, b);
  return check_launch(who);
}

}  // namespace dss2
