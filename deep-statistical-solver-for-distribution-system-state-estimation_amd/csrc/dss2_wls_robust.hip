// The Huber M-estimator on the batched WLS estimator's kernels, fp64, gfx950: iteratively re-weighted Gauss-Newton.  Measurement i has
// the weight w_i = c_k R_i^-1 of the plain estimator, the residual r_i = z_i - h_i(u) and t_i = sqrt(w_i) |r_i| at the current iterate;
// its factor is
//     q_i = gamma / t_i   where weighting is on for the iteration (it >= plain_iters) and t_i > gamma,
//     q_i = 1             elsewhere (a NaN and a weight of 0 keep 1),
// and an iteration is the plain one with w_i q_i in place of w_i in G and in b -- H, r and q from the same iterate.  The factor is
// formed where the residual already exists, on the row owners' walk (WsHuber in dss2_wls_core.hpp): every owner that visits a
// measurement recomputes its q from the same inputs in the same order, so nothing is stored during the solve, and the iteration has
// no barrier, no loop and no LDS beyond the plain kernel's.  The start, the slack angles, the pivot test, the decision, the statuses
// and the launch geometry are the plain kernels'; with gamma = +inf the five shared outputs are theirs to the bit.
//
// Two forms, one launch each, one workgroup per graph:
//   wls_robust_kernel<64 / 256>   the gain matrix packed in LDS (dss2_wls_solve.hip's layout and steps), up to 99 buses
//   wls_robust_large_kernel       the gain matrix in a workspace in global memory, blocked Cholesky (dss2_wls_large.hip's), up to 256
//
// After the last iterate, with weighting on: the objective pass (a bus owns its four measurements and the two flows of every branch it
// is the from-end of) writes every q, replaces the term of a measurement with q < 1 by rho's tail 2 gamma t - gamma^2, and counts the
// q < 1; the per-bus counts go through workgroup scratch that is idle by then (the packed array; the panel Pt) and thread 0 adds them.
// No atomics, one writer per value, fixed summation orders.  Every __syncthreads() sits in control flow that is uniform over the
// workgroup; no loop's end depends on the iterate.
#include "dss2_wls_large_core.hpp"

namespace dss2 {

__device__ __forceinline__ WsHuber wr_policy(const dss2_wls_robust_args& b) {
  return WsHuber{b.gamma, b.plain_iters, true, b.bus_q, b.edge_q, nullptr, nullptr};
}

template <int T>
__global__ void __launch_bounds__(T) wls_robust_kernel(const dss2_wls_robust_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wr_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const int n = a.nodes_per_graph, ns = 2 * n;
  const WsLds l = ws_carve(wr_smem, n);
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  WsHuber wt = wr_policy(b);
  wt.cnt = reinterpret_cast<int*>(l.Gp + 2 * n);        // behind the objective's 2 n per-bus parts: n ints, inside the packed array
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    WsGraph g;
    g.base = gr * n; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = l.u; g.slk = l.slk;
    ws_load_start<T>(a, g, l, tid);
    WsTally t = {0, 1, 0.0};
    ws_gauss_newton<T>(a, g, l, ns, tid, WsNoMask(), t, wt);
    for (int r = tid; r < ns; r += T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)l.u[r];
    double jb, je;
    wt.n_down = b.n_downweighted + gr;
    ws_objective<T>(a, g, l.Gp, tid, WsNoMask(), jb, je, wt);     // (its last barrier: the next graph of this workgroup reuses the LDS)
    if (tid == 0) {
      a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
      a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
    }
  }
}

__global__ void __launch_bounds__(WL_T) wls_robust_large_kernel(const dss2_wls_robust_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wr_large_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const int n = a.nodes_per_graph, ns = 2 * n;
  const WlLds l = wl_carve(wr_large_smem, n);
  double* A = static_cast<double*>(b.workspace) + (size_t)blockIdx.x * wl_graph_doubles(n);
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  WsHuber wt = wr_policy(b);
  wt.cnt = reinterpret_cast<int*>(l.Pt);                // the panel is idle after the last factorisation: n ints of its 16 (2 n + 1) doubles
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    WsGraph g;
    g.base = gr * n; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = l.u; g.slk = l.slk;
    const WsLds start = {nullptr, nullptr, l.u, l.du, l.ctl, l.slk};
    ws_load_start<WL_T>(a, g, start, tid);
    WsTally t = {0, 1, 0.0};
    bool active = true;                                // uniform over the workgroup
    for (int it = 0; it < a.max_iter; ++it) {          // (wls_large_kernel's loop, with the weighting of the iteration)
      if (active) {
        wl_form(a, g, A, ns, tid, wt.at(it));
        const bool ok = wl_factor(A, l, ns, tid);
        wl_back_substitute(A, l, ns, tid);
        ws_decide(a, l.du, l.ctl, ns, tid, ok, t);
        __syncthreads();
        if (l.ctl[1]) for (int r = tid; r < ns; r += WL_T) l.u[r] += l.du[r];
        active = l.ctl[0] == 0;
      }
    }
    __syncthreads();
    for (int r = tid; r < ns; r += WL_T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)l.u[r];
    double jb, je;
    wt.n_down = b.n_downweighted + gr;
    ws_objective<WL_T>(a, g, l.du, tid, WsNoMask(), jb, je, wt);  // (its last barrier: the next graph of this workgroup reuses the LDS)
    if (tid == 0) {
      a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
      a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
    }
  }
}

// gamma > 0 (a NaN refused, +inf allowed), plain_iters >= 0, the three outputs; 0 or 2
static int wr_check_params(const dss2_wls_robust_args& b, const char* who) {
  if (!(b.gamma > 0.0)) { set_error("%s: gamma must be > 0", who); return 2; }
  if (b.plain_iters < 0) { set_error("%s: plain_iters must be >= 0", who); return 2; }
  if (!b.bus_q || !b.n_downweighted || (b.solve.n_edges > 0 && !b.edge_q)) { set_error("%s: null argument", who); return 2; }
  return 0;
}

}  // namespace dss2

using namespace dss2;

static int dss2_wls_robust_launch(const dss2_wls_robust_args* bp, void* stream);
extern "C" int dss2_wls_robust(const dss2_wls_robust_args* bp, void* stream) {
  if (!bp) { dss2::set_error("dss2_wls_robust: null argument"); return 2; }
  DSS2_RECORD([b = *bp](void* s_) { return dss2_wls_robust_launch(&b, s_); });
  return dss2_wls_robust_launch(bp, stream);
}
static int dss2_wls_robust_launch(const dss2_wls_robust_args* bp, void* stream) {
  const dss2_wls_robust_args& b = *bp;
  const dss2_wls_solve_args& a = b.solve;
  if (int rc = ws_check_args(a, "wls_robust", 0)) return rc;
  if (int rc = wr_check_params(b, "wls_robust")) return rc;
  const int n = a.nodes_per_graph;
  hipStream_t s = as_stream(stream);
  const int64_t grid = ws_grid(a);
  const size_t lds = ws_bytes(n);
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  if (2 * n <= WS_NARROW_STATES) {
    hipLaunchKernelGGL(wls_robust_kernel<64>, dim3((unsigned)grid), dim3(64), lds, s, b);
  } else {
    static std::atomic<uint32_t> done{0};
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&wls_robust_kernel<256>), done, "wls_robust")) return rc;
    hipLaunchKernelGGL(wls_robust_kernel<256>, dim3((unsigned)grid), dim3(256), lds, s, b);
  }
  return check_launch("wls_robust");
}

static int dss2_wls_robust_large_launch(const dss2_wls_robust_args* bp, void* stream);
extern "C" int dss2_wls_robust_large(const dss2_wls_robust_args* bp, void* stream) {
  if (!bp) { dss2::set_error("dss2_wls_robust_large: null argument"); return 2; }
  DSS2_RECORD([b = *bp](void* s_) { return dss2_wls_robust_large_launch(&b, s_); });
  return dss2_wls_robust_large_launch(bp, stream);
}
static int dss2_wls_robust_large_launch(const dss2_wls_robust_args* bp, void* stream) {
  const dss2_wls_robust_args& b = *bp;
  const dss2_wls_solve_args& a = b.solve;
  if (int rc = wl_check_size(a, "wls_robust_large")) return rc;
  if (int rc = wl_check_workspace(a, b.workspace, b.workspace_bytes, "wls_robust_large")) return rc;
  if (int rc = wr_check_params(b, "wls_robust_large")) return rc;
  hipStream_t s = as_stream(stream);
  static std::atomic<uint32_t> done{0};
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&wls_robust_large_kernel), done, "wls_robust_large")) return rc;
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  hipLaunchKernelGGL(wls_robust_large_kernel, dim3((unsigned)wl_grid(a)), dim3(WL_T), wl_lds_bytes(a.nodes_per_graph), s, b);
  return check_launch("wls_robust_large");
}
