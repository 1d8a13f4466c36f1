// The banded form of the blocked WLS solve (dss2_wls_large_core.hpp): the same kernel steps -- wl_form, wl_factor, wl_back_substitute,
// wl_gauss_newton, ws_decide -- on rows that keep only a band of the gain matrix, for graphs whose buses were numbered for a small
// bandwidth (estimator.band_order: Cuthill-McKee).  G couples the buses within two branches of each other; with hb >= max (r - c) over
// its non-zeros and Wb = ceil(hb / 16), the Cholesky factor has no entry outside the band either, so
//
//   workspace slice   block row R (rows 16 R .. 16 R + 15) keeps the block columns R - Wb .. R: every row is W = 16 (Wb + 1) doubles,
//                     row r at r W, its column c at c - 16 (R - Wb) -- also where R < Wb (the columns before 0 are never touched).
//                     Behind the nb = ceil(ns / 16) block rows: the right-hand side b, 16 nb doubles.  256 nb (Wb + 1) + 16 nb doubles.
//   factorisation     block column J: the diagonal block as before; the panel is the rows of block rows J + 1 .. J + Wb (at most
//                     16 Wb) and the b row; the trailing update runs over the tiles of those rows alone.
//   substitution      a block row of L^T reaches 16 Wb columns to the left, no further.
//   LDS               Pt: 16 rows of S = 16 Wb + 8 doubles (a panel row's place is its distance from the panel's first row; the b
//                     row comes last); Ld, invd, u, du, ctl, slk as in the dense form.  wb_lds_bytes(n, Wb) <= the LDS of a
//                     workgroup is the cap on (n, hb), DSS2_WLS_BAND_LDS_BYTES; the host mirrors the formula (estimator.py).
//
// Three kernels run on this layout: wls_banded_kernel<dss2_wls_large_args> (the plain estimator, csrc/dss2_wls_large.hip),
// wls_banded_kernel<dss2_wls_robust_args> (the Huber one, csrc/dss2_wls_robust.hip) and wls_bad_data_banded_kernel (csrc/dss2_wls_bad_data.hip,
// with the selected inverse of dss2_wls_banded_invert.hpp); each enters through its dense form's C function when half_bandwidth > 0.
//
// THE GUARD.  The row owners write G[r, c] at at(r)[c]; a column left of the band would land in another row.  Which columns a row has is
// a matter of the graph alone, so it is checked once per graph before anything is assembled (wb_fits: every bus against the lowest
// bus within two branches of it).  A graph that does not fit is not assembled: status 2, no iteration, its start as its state.
#pragma once
#include "dss2_wls_large_core.hpp"

namespace dss2 {

static_assert(DSS2_WLS_BAND_BLOCK == WL_NB && DSS2_WLS_BAND_LDS_BYTES == kMaxLdsBytes, "the header's constants are this layout's");
constexpr int WB_GROUPS = DSS2_WLS_BAND_GROUPS;

__host__ __device__ constexpr int wb_blocks(int hb) { return (hb + WL_NB - 1) / WL_NB; }
__host__ __device__ constexpr int wb_pstride(int Wb) { return WL_NB * Wb + WL_TILE; }
__host__ __device__ constexpr size_t wb_graph_doubles(int n, int Wb) {
  return (size_t)((2 * n + WL_NB - 1) / WL_NB) * ((size_t)(WL_NB * WL_NB) * (Wb + 1) + WL_NB);
}
__host__ __device__ constexpr size_t wb_lds_bytes(int n, int Wb) { return wl_lds_bytes(n, wb_pstride(Wb)); }

struct WbRows;
struct WbPanelRows {
  const WbRows& rows; int ns, first, end;
  __device__ __forceinline__ double* at(double* A, int i) const;
  __device__ __forceinline__ int pt(int i) const { return i - first; }
};
struct WbRows {                     // WlRows' counterpart (dss2_wls_large_core.hpp): W = 16 (Wb + 1), shift = 16 Wb
  int W, shift;
  __device__ __forceinline__ size_t doubles(int n) const { return wb_graph_doubles(n, shift / WL_NB); }
  __device__ __forceinline__ double* at(double* A, int r) const { return A + (size_t)r * W + shift - (r & ~(WL_NB - 1)); }
  __device__ __forceinline__ double* rhs(double* A, int ns) const { return A + (size_t)((ns + WL_NB - 1) / WL_NB * WL_NB) * W; }
  __device__ __forceinline__ int left(int j0) const { return j0 > shift ? j0 - shift : 0; }
  __device__ __forceinline__ WbPanelRows below(int j0, int w, int ns) const {
    const int first = j0 + w;
    return WbPanelRows{*this, ns, first, first + shift < ns ? first + shift : ns};
  }
};
__device__ __forceinline__ double* WbPanelRows::at(double* A, int i) const { return i == end ? rows.rhs(A, ns) : rows.at(A, i); }

// Whether every non-zero of G lies in the band: bus li's rows 2 li, 2 li + 1 (one block row) against the lowest bus within two branches.
// The answer goes through ctl[2] (every thread that objects stores the same 1; HIP's __syncthreads_or would cost 256 bytes of static LDS
// on top of a carve that may take all of it).  Uniform over the workgroup; two barriers.
__device__ __forceinline__ bool wb_fits(const dss2_wls_solve_args& a, const WsGraph& g, int* __restrict__ ctl, int shift, int tid) {
  if (tid == 0) ctl[2] = 0;
  __syncthreads();
  for (int li = tid; li < g.n; li += WL_T) {
    int lowest = li;
    const int64_t gi = g.base + li;
    for (int k = a.inc_rowptr[gi]; k < a.inc_rowptr[gi + 1]; ++k) {
      int e, lo; bool is_from;
      if (!ws_slot(a, g, k, e, lo, is_from)) continue;
      lowest = lo < lowest ? lo : lowest;
      const int64_t gj = g.base + lo;
      for (int q = a.inc_rowptr[gj]; q < a.inc_rowptr[gj + 1]; ++q) {
        int e2, lo2; bool f2;
        if (ws_slot(a, g, q, e2, lo2, f2)) lowest = lo2 < lowest ? lo2 : lowest;
      }
    }
    if (2 * lowest < ((2 * li) & ~(WL_NB - 1)) - shift) ctl[2] = 1;
  }
  __syncthreads();
  return ctl[2] == 0;
}

// wls_blocked_kernel on the band: one workgroup of WL_T threads per graph and slice, the workgroups stride over the graphs.  Equal-size
// graphs only (the host refuses a graph_ptr).  Args is dss2_wls_large_args (the plain estimator) or dss2_wls_robust_args (the Huber one:
// ws_weighting gives its WsHuber), as for wls_blocked_kernel.  The Huber form's per-bus counts of q < 1 cannot pass through the panel as
// they do there -- 16 (16 Wb + 8) doubles hold fewer than n ints once the band is narrow -- so they pass through the head of the slice,
// which is idle after the last factorisation (also for a graph that does not fit: the one thing written to its slice).
template <class Args>
__global__ void __launch_bounds__(WL_T) wls_banded_kernel(const Args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wb_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const int n = a.nodes_per_graph, ns = 2 * n, Wb = wb_blocks(a.half_bandwidth);
  double* A = static_cast<double*>(b.workspace) + (size_t)blockIdx.x * wb_graph_doubles(n, Wb);
  const WbRows rows = {WL_NB * (Wb + 1), WL_NB * Wb};
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  auto wt = ws_weighting(b);
  using Wt = decltype(wt);
  const WlLds l = wl_carve(wb_smem, n, wb_pstride(Wb));
  if constexpr (Wt::robust) wt.cnt = reinterpret_cast<int*>(A);
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    const WsGraph g = ws_graph(gr * n, n, vlv, l.u, l.slk);
    const WsLds start = {nullptr, nullptr, l.u, l.du, l.ctl, l.slk};
    ws_load_start<WL_T>(a, g, start, tid);
    WsTally t = {0, 2, 0.0};
    if (wb_fits(a, g, l.ctl, rows.shift, tid)) wl_gauss_newton(a, g, A, rows, l, ns, tid, t, wt);
    if constexpr (Wt::robust) wt.n_down = b.n_downweighted + gr;
    ws_finish<WL_T>(a, g, gr, l.du, ns, tid, t, wt);
  }
}

// ---- host side: the banded forms' own checks (after ws_check_batch) and their launch, then the one route (wb_route) by which the
// three entries that serve both the blocked and the banded form reach either.  extra_lds: what a kernel keeps behind the carve (the
// bad-data form's fixed block); on the band it counts against the cap on (n, hb).
inline int64_t wb_grid(const dss2_wls_solve_args& a) {
  const int64_t n_graphs = a.n_nodes / a.nodes_per_graph;
  int64_t grid = WB_GROUPS;
  if (a.max_groups > 0 && a.max_groups < grid) grid = a.max_groups;
  return n_graphs < grid ? n_graphs : grid;
}
inline int wb_check(const dss2_wls_solve_args& a, const void* workspace, uint64_t workspace_bytes, const char* who, size_t extra_lds = 0) {
  const int n = a.nodes_per_graph, hb = a.half_bandwidth;
  if (a.graph_ptr) { set_error("%s: the banded form serves equal-size graphs (no graph_ptr)", who); return 2; }
  if (hb < 0) { set_error("%s: half_bandwidth must be >= 0", who); return 2; }
  if (n > (1 << 20) || hb > (1 << 20) || wb_lds_bytes(n, wb_blocks(hb)) + extra_lds > (size_t)DSS2_WLS_BAND_LDS_BYTES) {
    set_error("%s: %d buses per graph at a half-bandwidth of %d states need more than the %d bytes of LDS a workgroup has", who, n, hb,
              DSS2_WLS_BAND_LDS_BYTES);
    return 2;
  }
  if (a.max_groups < 0) { set_error("%s: bad leading dimension or max_groups", who); return 2; }
  const int64_t grid = wb_grid(a);
  const size_t need = (size_t)grid * wb_graph_doubles(n, wb_blocks(hb)) * 8;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) { set_error("%s: the workspace is null or not 16-byte aligned", who); return 2; }
  if (workspace_bytes < need) {
    set_error("%s: the workspace has %llu bytes, %lld workgroups of %d buses at a half-bandwidth of %d need %llu", who,
              (unsigned long long)workspace_bytes, (long long)grid, n, hb, (unsigned long long)need);
    return 2;
  }
  return ws_check_rest(a, who);
}
template <auto K, class Args>
inline int wb_launch(const Args& b, const char* who, hipStream_t s, size_t extra_lds = 0) {
  const dss2_wls_solve_args& a = b.solve;
  static std::atomic<uint32_t> done{0};
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(K), done, who)) return rc;
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  hipLaunchKernelGGL(K, dim3((unsigned)wb_grid(a)), dim3(WL_T), wb_lds_bytes(a.nodes_per_graph, wb_blocks(a.half_bandwidth)) + extra_lds, s, b);
  return check_launch(who);
}

// The route of an entry that serves both forms on rows: half_bandwidth != 0 selects the banded one.  The form's own checks -- the batch,
// then the size and the workspace -- then the entry's parameter check (Check(b, who), or none), then the form's launch of its kernel.
// `who` names the entry and the form in every message; extra_lds as for wb_check and the launches.
template <auto Blocked, auto Banded, auto Check = nullptr, class Args>
inline int wb_route(const Args& b, const char* who_blocked, const char* who_banded, hipStream_t s, size_t extra_lds = 0) {
  const bool banded = b.solve.half_bandwidth != 0;
  const char* who = banded ? who_banded : who_blocked;
  if (banded) {
    if (int rc = ws_check_batch(b.solve, who)) return rc;
    if (int rc = wb_check(b.solve, b.workspace, b.workspace_bytes, who, extra_lds)) return rc;
  } else {
    if (int rc = wl_check_size(b.solve, who)) return rc;             // (ws_check_batch is its first step)
    if (int rc = wl_check_workspace(b.solve, b.workspace, b.workspace_bytes, who)) return rc;
  }
  if constexpr (!std::is_null_pointer_v<decltype(Check)>)
    if (int rc = Check(b, who)) return rc;
  return banded ? wb_launch<Banded>(b, who, s, extra_lds) : wl_launch<Blocked>(b, who, s, extra_lds);
}

}  // namespace dss2
