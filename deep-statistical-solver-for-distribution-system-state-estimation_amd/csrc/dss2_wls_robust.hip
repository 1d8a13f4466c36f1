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
// Two forms, one launch each, one workgroup per graph -- the plain estimator's two kernel bodies, instantiated on dss2_wls_robust_args
// (ws_weighting in dss2_wls_core.hpp turns them into the WsHuber):
//   wls_lds_kernel<64 / 256, .>   the gain matrix packed in LDS (dss2_wls_core.hpp; dss2_wls_solve.hip's layout and steps), up to 99 buses
//   wls_blocked_kernel<.>         the gain matrix in a workspace in global memory, blocked Cholesky (dss2_wls_large_core.hpp), up to 256
//   wls_banded_kernel<.>          the same on rows that keep a band of G (dss2_wls_banded.hpp; half_bandwidth > 0), beyond 256 buses; it
//                                 enters through dss2_wls_robust_large as the plain banded solve enters through dss2_wls_solve_large
//                                 (wb_route in dss2_wls_banded.hpp, with wr_check_params as the entry's own check)
//
// After the last iterate, with weighting on: the objective pass (a bus owns its four measurements and the two flows of every branch it
// is the from-end of) writes every q, replaces the term of a measurement with q < 1 by rho's tail 2 gamma t - gamma^2, and counts the
// q < 1; the per-bus counts go through workgroup scratch that is idle by then (the packed array; the panel Pt) and thread 0 adds them.
// No atomics, one writer per value, fixed summation orders.  Every __syncthreads() sits in control flow that is uniform over the
// workgroup; no loop's end depends on the iterate.
#include "dss2_wls_banded.hpp"

using namespace dss2;

// gamma > 0 (a NaN refused, +inf allowed), plain_iters >= 0, the three outputs; 0 or 2
static int wr_check_params(const dss2_wls_robust_args& b, const char* who) {
  if (!(b.gamma > 0.0)) { set_error("%s: gamma must be > 0", who); return 2; }
  if (b.plain_iters < 0) { set_error("%s: plain_iters must be >= 0", who); return 2; }
  if (!b.bus_q || !b.n_downweighted || (b.solve.n_edges > 0 && !b.edge_q)) { set_error("%s: null argument", who); return 2; }
  return 0;
}

static int wls_robust_launch(const dss2_wls_robust_args* bp, void* stream) {
  using B = dss2_wls_robust_args;
  const B& b = *bp;
  if (int rc = ws_check_args(b.solve, "wls_robust", 0)) return rc;
  if (int rc = wr_check_params(b, "wls_robust")) return rc;
  // (the wide kernel's uniform launches keep an instantiation without the graph_ptr branch: with it they measured 2.5 % slower)
  if (!b.solve.graph_ptr)
    return ws_launch<wls_lds_kernel<64, B>, wls_lds_kernel<256, B, WsUniformRange>>(b, ws_bytes(b.solve.nodes_per_graph), "wls_robust", as_stream(stream));
  return ws_launch<wls_lds_kernel<64, B>, wls_lds_kernel<256, B>>(b, ws_bytes(b.solve.nodes_per_graph), "wls_robust", as_stream(stream));
}
extern "C" int dss2_wls_robust(const dss2_wls_robust_args* bp, void* stream) { return dss2::entry(wls_robust_launch, stream, dss2::copied(bp, "dss2_wls_robust")); }

static int wls_robust_large_launch(const dss2_wls_robust_args* bp, void* stream) {
  using B = dss2_wls_robust_args;
  return wb_route<wls_blocked_kernel<B>, wls_banded_kernel<B>, wr_check_params>(*bp, "wls_robust_large", "wls_robust_large (banded)", as_stream(stream));
}
extern "C" int dss2_wls_robust_large(const dss2_wls_robust_args* bp, void* stream) {
  return dss2::entry(wls_robust_large_launch, stream, dss2::copied(bp, "dss2_wls_robust_large"));
}
