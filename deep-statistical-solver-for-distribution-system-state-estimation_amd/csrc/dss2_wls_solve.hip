// Batched weighted-least-squares state estimation (Gauss-Newton on the normal equations), fp64, gfx950.
//
// The measurement model is gsp_wls_edge's (reference data.py:397-409, 428-435): per bus z = (V, theta, P_inj, Q_inj) with weights
// R^-1, per stored branch (P_from, Q_from); h(u) from the branch equations of data.py:370-376 with shift = 0.  The state u = (v, theta)
// per bus is physical (p.u., rad).  One workgroup solves one graph of n buses (ns = 2 n states), the whole iteration inside ONE launch:
//
//   LDS   G   packed lower triangle of the gain matrix H^T W H, row r at r (r + 1) / 2           ns (ns + 1) / 2 doubles
//         b   the right-hand side H^T W r, stored as ROW ns of the same packed array              ns
//         u   the state                                                                           ns
//         du  the step                                                                            ns
//         ctl {stop, apply}: the decision of an iteration, written by thread 0, read by all after a barrier
//         slk slack flag per bus
//
//   per iteration (trip count = args.max_iter; a graph that has stopped skips the body, uniformly over its workgroup)
//     1. G, b <- 0
//     2. thread r OWNS row r of G and b[r]: it walks every measurement whose Jacobian row is non-zero at state r -- the bus's own four,
//        the flows of its incident branches, the injections of its neighbours -- in a fixed order and adds w H[m, r] H[m, c] for the
//        columns c <= r.  No entry has two writers: no atomics, no barrier between measurements, one summation order.
//        A slack angle's row and column are the identity and its b is 0.
//     3. Cholesky of the packed array WITH the b row (so the b row leaves as y = L^-1 b): per column a barrier, the pivot test (every
//        thread reads the same LDS word), the column scaled, a barrier, the trailing update on a 16 x (T / 16) thread grid.
//        A pivot <= 0 or not finite marks the factorisation failed; the loop runs on to its fixed end.
//     4. back substitution L^T du = y, one barrier per column.
//     5. wave 0 forms max |du|; thread 0 decides (failed -> status 2, state kept; else apply, and status 0 if the step is below tol).
//
// Every __syncthreads() sits in control flow that is uniform over the workgroup; no loop's end depends on the iterate.
// Branch physics is recomputed per visit (fp64 sincos): a bus of degree d costs its two row owners about d + sum of its neighbours' degrees
// branch evaluations, twice -- the grids have d <= 4.  Keeping them in LDS would need a bound on a graph's branch count that the host
// does not have without a read-back.
// The device functions live in dss2_wls_core.hpp, which csrc/dss2_wls_bad_data.hip shares.
#include "dss2_wls_core.hpp"

namespace dss2 {

template <int T>
__global__ void __launch_bounds__(T) wls_solve_kernel(const dss2_wls_solve_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
  const int n = a.nodes_per_graph, ns = 2 * n;
  const WsLds l = ws_carve(ws_smem, n);
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    WsGraph g;
    g.base = gr * n; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = l.u; g.slk = l.slk;
    ws_load_start<T>(a, g, l, tid);
    WsTally t = {0, 1, 0.0};
    ws_gauss_newton<T>(a, g, l, ns, tid, WsNoMask(), t);
    // ---- outputs: the state in fp32, J at the fp64 state (per-bus parts summed by one thread in bus order)
    for (int r = tid; r < ns; r += T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)l.u[r];
    double jb, je;
    ws_objective<T>(a, g, l.Gp, tid, WsNoMask(), jb, je);       // (its last barrier: the next graph of this workgroup reuses the LDS)
    if (tid == 0) {
      a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
      a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
    }
  }
}

}  // namespace dss2

using namespace dss2;

extern "C" size_t dss2_wls_solve_lds_bytes(int nodes_per_graph) {
  return nodes_per_graph > 0 ? ws_bytes(nodes_per_graph) : 0;
}

static int dss2_wls_solve_launch(const dss2_wls_solve_args* ap, void* stream);
extern "C" int dss2_wls_solve(const dss2_wls_solve_args* ap, void* stream) {
  if (!ap) { dss2::set_error("dss2_wls_solve: null argument"); return 2; }
  DSS2_RECORD([a = *ap](void* s_) { return dss2_wls_solve_launch(&a, s_); });
  return dss2_wls_solve_launch(ap, stream);
}
static int dss2_wls_solve_launch(const dss2_wls_solve_args* ap, void* stream) {
  const dss2_wls_solve_args& a = *ap;
  if (int rc = ws_check_args(a, "wls_solve", 0)) return rc;
  const int n = a.nodes_per_graph;
  hipStream_t s = as_stream(stream);
  const int64_t grid = ws_grid(a);
  const size_t lds = ws_bytes(n);
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  if (2 * n <= WS_NARROW_STATES) {
    hipLaunchKernelGGL(wls_solve_kernel<64>, dim3((unsigned)grid), dim3(64), lds, s, a);
  } else {
    static std::atomic<uint32_t> done{0};
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&wls_solve_kernel<256>), done, "wls_solve")) return rc;
    hipLaunchKernelGGL(wls_solve_kernel<256>, dim3((unsigned)grid), dim3(256), lds, s, a);
  }
  return check_launch("wls_solve");
}
