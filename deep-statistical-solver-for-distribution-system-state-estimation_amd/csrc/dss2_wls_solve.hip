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
// The kernel body (wls_lds_kernel), its device functions and the launch path live in dss2_wls_core.hpp, which every WLS kernel shares;
// this file instantiates the plain estimator.
#include "dss2_wls_core.hpp"

using namespace dss2;

extern "C" size_t dss2_wls_solve_lds_bytes(int nodes_per_graph) {
  return nodes_per_graph > 0 ? ws_bytes(nodes_per_graph) : 0;
}

static int wls_solve_launch(const dss2_wls_solve_args* ap, void* stream) {
  using A = dss2_wls_solve_args;
  const A& a = *ap;
  if (int rc = ws_check_args(a, "wls_solve", 0)) return rc;
  return ws_launch<wls_lds_kernel<64, A>, wls_lds_kernel<256, A>>(a, ws_bytes(a.nodes_per_graph), "wls_solve", as_stream(stream));
}
extern "C" int dss2_wls_solve(const dss2_wls_solve_args* ap, void* stream) { return dss2::entry(wls_solve_launch, stream, dss2::copied(ap, "dss2_wls_solve")); }
