// What every kernel of the batched fp64 WLS estimator shares.  All four WLS translation units include it, directly or through
// dss2_wls_large_core.hpp and dss2_wls_bad_data_core.hpp: csrc/dss2_wls_solve.hip (the solve alone), csrc/dss2_wls_bad_data.hip (the solve, the covariance,
// normalized residuals and the removal loop), csrc/dss2_wls_large.hip (the solve on a blocked gain matrix in global memory) and
// csrc/dss2_wls_robust.hip (the Huber M-estimator, on both storage forms).  Here live
//   - the device functions: measurements, the row owners' assembly, the packed Cholesky, the decision, the objective;
//   - a graph's range (ws_range: the uniform layout, or graph_ptr with nodes_per_graph as a bound, and the guard of the latter), its
//     prologue (ws_graph) and the plain epilogue (ws_store_state, ws_finish), once for every kernel;
//   - wls_lds_kernel, the ONE kernel body with the gain matrix in LDS: the plain and the Huber estimator are two instantiations of it;
//   - the host side: the argument checks and ws_launch (the launch path of every kernel on the LDS carve).
// The LDS layout, the row ownership and the order of every sum are described in the header of dss2_wls_solve.hip; nothing here
// depends on which kernel runs it.
//
// Every function that reads measurements takes a MASK: mask(id) says whether measurement `id` has been removed (its weight is then 0
// everywhere it enters).  Ids are 4 i + k for bus i (global row), k in V, theta, P, Q, and 4 N + 2 e + k for stored branch e, k in
// P_from, Q_from.  WsNoMask removes nothing and compiles to nothing; WsRemoved looks the id up in a short list in LDS.
//
// Beside it they take a WEIGHTING: a factor q on a measurement's weight that depends on its own residual at the state in LDS.
// WsNoWeight (the default: the callers that know nothing of it) has none and compiles to nothing; WsHuber is the M-estimator's
// q = gamma / t where t = sqrt(w) |r| > gamma (csrc/dss2_wls_robust.hip).  Whoever visits a measurement forms its q from the same
// inputs in the same order: the same bits everywhere, nothing stored during the solve.
#pragma once
#include "dss2_common.hpp"

namespace dss2 {

constexpr int WS_TX = 16;          // trailing update: 16 columns x (T / 16) rows of threads

// LDS carve (bytes from the 16-byte aligned dynamic base), shared by the kernels and dss2_wls_solve_lds_bytes
__host__ __device__ inline size_t ws_doubles(int n) { const size_t ns = 2 * (size_t)n; return ns * (ns + 1) / 2 + 3 * ns; }
__host__ __device__ inline size_t ws_ctl_off(int n) { return (ws_doubles(n) * 8 + 15) / 16 * 16; }
__host__ __device__ inline size_t ws_slk_off(int n) { return ws_ctl_off(n) + 16; }
__host__ __device__ inline size_t ws_bytes(int n) { return ws_slk_off(n) + ((size_t)n + 15) / 16 * 16; }

struct WsNoMask {
  __device__ __forceinline__ bool operator()(int) const { return false; }
};
struct WsRemoved {                  // the ids removed so far: n of them, in LDS
  const int* ids;
  int n;
  __device__ __forceinline__ bool operator()(int id) const {
    bool hit = false;
    for (int q = 0; q < n; ++q) hit = hit || ids[q] == id;
    return hit;
  }
};

struct WsNoWeight {
  static constexpr bool robust = false;
  __device__ __forceinline__ WsNoWeight at(int) const { return *this; }
};
struct WsHuber {
  static constexpr bool robust = true;
  double gamma;
  int plain_iters;                  // the iterations before this one run with q = 1
  bool on;
  double* bus_q; double* edge_q;    // [N, 4], [E, 2]: written by the objective pass (not read before)
  int* cnt;                         // n ints of workgroup scratch for the objective pass's counts of q < 1
  int* n_down;                      // this graph's count (thread 0 writes it)
  __device__ __forceinline__ WsHuber at(int it) const { WsHuber h = *this; h.on = it >= plain_iters; return h; }
  // q of a measurement of weight w and residual r.  Not t > gamma -- a NaN, a weight of 0 -- keeps 1.
  __device__ __forceinline__ double factor(double w, double r) const {
    const double t = sqrt(w) * fabs(r);
    return (on && t > gamma) ? gamma / t : 1.0;
  }
  // rho(t) - t^2 above gamma, rho(t) = 2 gamma t - gamma^2: what a measurement with factor(w, r) < 1 adds to the plain sum w r^2
  __device__ __forceinline__ double excess(double w, double r) const { return 2.0 * gamma * (sqrt(w) * fabs(r)) - gamma * gamma - w * r * r; }
};

// What a kernel body that is a template on its argument struct asks of it: the `solve` block and the weighting.  (cnt and n_down of
// a WsHuber are the kernel's to set: where its scratch lies, which graph it is at.)
__host__ __device__ __forceinline__ const dss2_wls_solve_args& ws_solve_block(const dss2_wls_solve_args& a) { return a; }
template <class Args>
__host__ __device__ __forceinline__ const dss2_wls_solve_args& ws_solve_block(const Args& b) { return b.solve; }
__device__ __forceinline__ WsNoWeight ws_weighting(const dss2_wls_solve_args&) { return WsNoWeight(); }
__device__ __forceinline__ WsNoWeight ws_weighting(const dss2_wls_large_args&) { return WsNoWeight(); }
__device__ __forceinline__ WsHuber ws_weighting(const dss2_wls_robust_args& b) {
  return WsHuber{b.gamma, b.plain_iters, true, b.bus_q, b.edge_q, nullptr, nullptr};
}

// One end's view of a branch: the active and reactive power entering the branch at `self`, and their derivatives with respect to
// (v_self, theta_self, v_other, theta_other).  With delta = theta_self - theta_other this is data.py:370-373 at the from-end and
// data.py:374-376 at the to-end (cos is even, sin is odd).
struct WsBranch { double p, q, dp[4], dq[4]; };

__device__ __forceinline__ WsBranch ws_branch(double vs, double ts, double vo, double to, const float* __restrict__ ep, double kk) {
  const double G = ep[0], B = ep[1], gg = G + (double)ep[2] / 2.0, bb = B + (double)ep[3] / 2.0;
  double s, c;
  sincos(ts - to, &s, &c);
  const double A = G * c + B * s, Q = -G * s + B * c, vv = vs * vo;
  WsBranch f;
  f.p = (-vv * A + gg * (vs * vs)) * kk;
  f.q = (vv * Q - bb * (vs * vs)) * kk;
  f.dp[0] = (-vo * A + 2.0 * gg * vs) * kk; f.dp[1] = -vv * Q * kk; f.dp[2] = -vs * A * kk; f.dp[3] = vv * Q * kk;
  f.dq[0] = (vo * Q - 2.0 * bb * vs) * kk;  f.dq[1] = -vv * A * kk; f.dq[2] = vs * Q * kk;  f.dq[3] = vv * A * kk;
  return f;
}

// double(z) * double(std) + double(mean) where the normalised entry is non-zero, else 0; a weight below 0 counts as 0, and so does
// the weight of a removed measurement (ids id0, id0 + 1, ... in the order of the pairs)
template <int PAIRS, class Mask>
__device__ __forceinline__ void ws_meas(const float* __restrict__ in, const float* __restrict__ mean, const float* __restrict__ stdv,
                                        double (&Z)[PAIRS], double (&R)[PAIRS], const Mask& mask, int id0) {
#pragma unroll
  for (int c = 0; c < PAIRS; ++c) {
    const float z = in[2 * c], r = in[2 * c + 1];
    Z[c] = (z != 0.f) ? (double)z * (double)stdv[2 * c] + (double)mean[2 * c] : 0.0;
    const double w = (r != 0.f) ? (double)r * (double)stdv[2 * c + 1] + (double)mean[2 * c + 1] : 0.0;
    R[c] = w < 0.0 ? 0.0 : w;
    if (mask(id0 + c)) R[c] = 0.0;
  }
}
__device__ __forceinline__ int ws_bus_id(int64_t gi) { return (int)(4 * gi); }
__device__ __forceinline__ int ws_edge_id(const dss2_wls_solve_args& a, int e) { return (int)(4 * a.n_nodes + 2 * (int64_t)e); }

struct WsGraph {                    // what the row owners need of the graph being solved
  int64_t base;                     // first bus
  int n;
  double kk;                        // V_lv^2
  const double* u;                  // LDS state
  const unsigned char* slk;         // LDS slack flags
};
// the graph of n buses from row `base` on (vlv: vminmax_fold's low-voltage base)
__device__ __forceinline__ WsGraph ws_graph(int64_t base, int n, float vlv, const double* u, const unsigned char* slk) {
  WsGraph g;
  g.base = base; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = u; g.slk = slk;
  return g;
}

// Which rows graph gr owns.  Without a graph_ptr: [gr n, (gr + 1) n), n = nodes_per_graph.  With one: [graph_ptr[gr], graph_ptr[gr + 1]),
// and nodes_per_graph is only the BOUND everything was sized by on the host.  The two words are read once per graph and made wave-uniform
// (every wave of the workgroup reads the same two: n is the same in every thread, and so is every trip count derived from it).
// ok = false: the pointer does not describe a graph this launch can hold -- n < 1, n above the bound, rows outside [0, n_nodes) -- and the
// graph is refused (ws_refuse) before anything of it touches LDS or memory.
__host__ __device__ __forceinline__ int64_t ws_n_graphs(const dss2_wls_solve_args& a) {
  return a.graph_ptr ? a.n_graphs : a.n_nodes / a.nodes_per_graph;
}
struct WsRange { int64_t base; int n; bool ok; };
__device__ __forceinline__ int64_t ws_uniform(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ WsRange ws_range(const dss2_wls_solve_args& a, int64_t gr) {
  WsRange r;
  if (a.graph_ptr) {
    const int64_t b0 = ws_uniform(a.graph_ptr[gr]), cnt = ws_uniform(a.graph_ptr[gr + 1]) - b0;
    r.ok = cnt >= 1 && cnt <= (int64_t)a.nodes_per_graph && b0 >= 0 && b0 <= a.n_nodes - cnt;
    r.base = b0; r.n = r.ok ? (int)cnt : 0;
  } else {
    r.base = gr * a.nodes_per_graph; r.n = a.nodes_per_graph; r.ok = true;
  }
  return r;
}
// The range as a kernel body's template parameter, in the style of WsNoMask / WsNoWeight.  WsAnyRange -- the default of every body --
// decides per launch, by the uniform branch of ws_range.  WsUniformRange knows that the launch has no graph_ptr: it is there for the
// one instantiation whose uniform launches measurably slowed with the branch in the body (the wide Huber kernel).
struct WsAnyRange {
  __device__ static __forceinline__ int64_t n_graphs(const dss2_wls_solve_args& a) { return ws_n_graphs(a); }
  __device__ static __forceinline__ WsRange at(const dss2_wls_solve_args& a, int64_t gr) { return ws_range(a, gr); }
};
struct WsUniformRange {
  __device__ static __forceinline__ int64_t n_graphs(const dss2_wls_solve_args& a) { return a.n_nodes / a.nodes_per_graph; }
  __device__ static __forceinline__ WsRange at(const dss2_wls_solve_args& a, int64_t gr) { return WsRange{gr * a.nodes_per_graph, a.nodes_per_graph, true}; }
};
// The five plain outputs of a refused graph (one thread calls it): status 2, nothing done.  No state row is written.
__device__ __forceinline__ void ws_refuse(const dss2_wls_solve_args& a, int64_t gr) {
  a.objective[2 * gr] = 0.0; a.objective[2 * gr + 1] = 0.0;
  a.iterations[gr] = 0; a.status[gr] = 2; a.last_step[gr] = 0.0;
}

// incidence entry k -> stored branch, the other end's LOCAL bus (outside [0, n): an edge that leaves the graph, ignored), orientation
__device__ __forceinline__ bool ws_slot(const dss2_wls_solve_args& a, const WsGraph& g, int k, int& e, int& lo, bool& is_from) {
  const int en = a.inc_ent[k];
  e = en & 0x7fffffff;
  is_from = en >= 0;
  lo = (int)((int64_t)(is_from ? a.eto : a.efrom)[e] - g.base);
  return (unsigned)lo < (unsigned)g.n;
}

__device__ __forceinline__ void ws_add(double* __restrict__ row, int r, const unsigned char* slk, int c, double v) {
  if (c <= r && !((c & 1) && slk[c >> 1])) row[c] += v;
}

// Row r of G and b[r]: every measurement with a non-zero Jacobian entry at state r, in a fixed order.  `row` is the zeroed row r
// (columns 0 .. r, contiguous, LDS or global memory), `bvec` the right-hand side (entry r is written).
template <class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ void ws_accumulate_row_at(const dss2_wls_solve_args& a, const WsGraph& g, int r, double* __restrict__ row,
                                                     double* __restrict__ bvec, const Mask& mask, const Wt& wt = Wt()) {
  const int li = r >> 1, c = r & 1;
  if (c && g.slk[li]) { row[r] = 1.0; bvec[r] = 0.0; return; }     // a slack angle: identity row, held at 0
  const int64_t gi = g.base + li;
  double accb = 0.0;
  {   // the bus's own V (c = 0) or theta (c = 1)
    double Z[4], R[4];
    ws_meas(a.x + gi * a.ldx, a.x_mean, a.x_std, Z, R, mask, ws_bus_id(gi));
    double w = a.w_v * (c ? R[1] : R[0]);
    if constexpr (Wt::robust) w *= wt.factor(w, (c ? Z[1] : Z[0]) - g.u[r]);
    row[r] += w;
    accb += w * ((c ? Z[1] : Z[0]) - g.u[r]);
  }
  const int k0 = a.inc_rowptr[gi], k1 = a.inc_rowptr[gi + 1];
  // the injections of bus i itself (k = k0 - 1) and of every neighbour, and the flow measurement of every incident branch
  for (int k = k0 - 1; k < k1; ++k) {
    int lj = li;
    if (k >= k0) {
      int e, lo; bool is_from;
      if (!ws_slot(a, g, k, e, lo, is_from)) continue;
      lj = lo;
      if (!(lo == li && !is_from)) {     // (a branch from a bus to itself is listed twice: its flow is taken once)
        const int lf = is_from ? li : lo, lt = is_from ? lo : li;
        double Ze[2], Re[2];
        ws_meas(a.edge_attr + (int64_t)e * a.ldea, a.edge_mean, a.edge_std, Ze, Re, mask, ws_edge_id(a, e));
        if (Re[0] != 0.0 || Re[1] != 0.0) {
          const WsBranch f = ws_branch(g.u[2 * lf], g.u[2 * lf + 1], g.u[2 * lt], g.u[2 * lt + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
          double hp = 0.0, hq = 0.0;
          if (lf == li) { hp += c ? f.dp[1] : f.dp[0]; hq += c ? f.dq[1] : f.dq[0]; }
          if (lt == li) { hp += c ? f.dp[3] : f.dp[2]; hq += c ? f.dq[3] : f.dq[2]; }
          double wp = a.w_pf * Re[0], wq = a.w_pf * Re[1];
          const double rp = Ze[0] - f.p, rq = Ze[1] - f.q;
          if constexpr (Wt::robust) { wp *= wt.factor(wp, rp); wq *= wt.factor(wq, rq); }
          const double gp = wp * hp, gq = wq * hq;
          accb += gp * rp + gq * rq;
          ws_add(row, r, g.slk, 2 * lf, gp * f.dp[0] + gq * f.dq[0]);
          ws_add(row, r, g.slk, 2 * lf + 1, gp * f.dp[1] + gq * f.dq[1]);
          ws_add(row, r, g.slk, 2 * lt, gp * f.dp[2] + gq * f.dq[2]);
          ws_add(row, r, g.slk, 2 * lt + 1, gp * f.dp[3] + gq * f.dq[3]);
        }
      }
      if (lj == li) continue;            // (bus i's own injections were taken at k = k0 - 1)
      bool seen = false;                 // parallel branches list a neighbour more than once: its injections are taken at the first
      for (int q = k0; q < k; ++q) {
        int e2, lo2; bool f2;
        if (ws_slot(a, g, q, e2, lo2, f2) && lo2 == lj) seen = true;
      }
      if (seen) continue;
    }
    const int64_t gj = g.base + lj;
    double Z[4], R[4];
    ws_meas(a.x + gj * a.ldx, a.x_mean, a.x_std, Z, R, mask, ws_bus_id(gj));
    double wP = a.w_p * R[2], wQ = a.w_p * R[3];
    if (wP == 0.0 && wQ == 0.0) continue;
    const int j0 = a.inc_rowptr[gj], j1 = a.inc_rowptr[gj + 1];
    const double vj = g.u[2 * lj], tj = g.u[2 * lj + 1];
    // pass 1: P_j, Q_j, their derivatives at bus j's own state, and at state r
    double P = 0.0, Q = 0.0, sP[2] = {0.0, 0.0}, sQ[2] = {0.0, 0.0}, hP = 0.0, hQ = 0.0;
    for (int q = j0; q < j1; ++q) {
      int e, lo; bool is_from;
      if (!ws_slot(a, g, q, e, lo, is_from)) continue;
      const WsBranch f = ws_branch(vj, tj, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
      P -= f.p; Q -= f.q;
      sP[0] -= f.dp[0]; sP[1] -= f.dp[1]; sQ[0] -= f.dq[0]; sQ[1] -= f.dq[1];
      if (lo == li) { hP -= c ? f.dp[3] : f.dp[2]; hQ -= c ? f.dq[3] : f.dq[2]; }
    }
    if (lj == li) { hP += c ? sP[1] : sP[0]; hQ += c ? sQ[1] : sQ[0]; }
    const double rP = Z[2] - P, rQ = Z[3] - Q;
    if constexpr (Wt::robust) { wP *= wt.factor(wP, rP); wQ *= wt.factor(wQ, rQ); }
    const double gP = wP * hP, gQ = wQ * hQ;
    accb += gP * rP + gQ * rQ;
    // pass 2: the columns
    ws_add(row, r, g.slk, 2 * lj, gP * sP[0] + gQ * sQ[0]);
    ws_add(row, r, g.slk, 2 * lj + 1, gP * sP[1] + gQ * sQ[1]);
    for (int q = j0; q < j1; ++q) {
      int e, lo; bool is_from;
      if (!ws_slot(a, g, q, e, lo, is_from)) continue;
      if (2 * lo > r) continue;
      const WsBranch f = ws_branch(vj, tj, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
      ws_add(row, r, g.slk, 2 * lo, -(gP * f.dp[2] + gQ * f.dq[2]));
      ws_add(row, r, g.slk, 2 * lo + 1, -(gP * f.dp[3] + gQ * f.dq[3]));
    }
  }
  bvec[r] = accb;
}
// ... in the packed lower triangle with the b row (the LDS kernels' layout)
template <class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ void ws_accumulate_row(const dss2_wls_solve_args& a, const WsGraph& g, int r, double* __restrict__ Gp, int ns,
                                                  const Mask& mask, const Wt& wt = Wt()) {
  ws_accumulate_row_at(a, g, r, Gp + (size_t)r * (r + 1) / 2, Gp + (size_t)ns * (ns + 1) / 2, mask, wt);
}

// The two parts of J at the state in LDS for bus li: its own four measurements, and the flows of the branches it is the from-end of.
// With a weighting the sums are formed by the very same statements -- without any q < 1 they are the plain ones to the bit -- and a
// measurement with q < 1 then trades its term for rho's tail (`excess`); its q is written, and the number of q < 1 among the bus's own
// is returned.
template <class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ int ws_objective_bus(const dss2_wls_solve_args& a, const WsGraph& g, int li, double& jbus, double& jbranch,
                                                const Mask& mask, const Wt& wt = Wt()) {
  const int64_t gi = g.base + li;
  double Z[4], R[4];
  ws_meas(a.x + gi * a.ldx, a.x_mean, a.x_std, Z, R, mask, ws_bus_id(gi));
  const double vi = g.u[2 * li], ti = g.u[2 * li + 1];
  double P = 0.0, Q = 0.0;
  jbranch = 0.0;
  double corr_e = 0.0, corr_b = 0.0;     // (with a weighting only)
  int down = 0;
  const int k0 = a.inc_rowptr[gi], k1 = a.inc_rowptr[gi + 1];
  for (int k = k0; k < k1; ++k) {
    int e, lo; bool is_from;
    if (!ws_slot(a, g, k, e, lo, is_from)) continue;
    const WsBranch f = ws_branch(vi, ti, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
    P -= f.p; Q -= f.q;
    if (is_from) {
      double Ze[2], Re[2];
      ws_meas(a.edge_attr + (int64_t)e * a.ldea, a.edge_mean, a.edge_std, Ze, Re, mask, ws_edge_id(a, e));
      const double dp = Ze[0] - f.p, dq = Ze[1] - f.q;
      jbranch += a.w_pf * (Re[0] * dp * dp + Re[1] * dq * dq);
      if constexpr (Wt::robust) {
        const double rr[2] = {dp, dq};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double w = a.w_pf * Re[c], q = wt.factor(w, rr[c]);
          wt.edge_q[2 * (int64_t)e + c] = q;
          if (q < 1.0) { ++down; corr_e += wt.excess(w, rr[c]); }
        }
      }
    }
  }
  const double dv = Z[0] - vi, dt = Z[1] - ti, dP = Z[2] - P, dQ = Z[3] - Q;
  jbus = a.w_v * (R[0] * dv * dv + R[1] * dt * dt) + a.w_p * (R[2] * dP * dP + R[3] * dQ * dQ);
  if constexpr (Wt::robust) {
    const double rr[4] = {dv, dt, dP, dQ};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double w = (c < 2 ? a.w_v : a.w_p) * R[c], q = wt.factor(w, rr[c]);
      wt.bus_q[4 * gi + c] = q;
      if (q < 1.0) { ++down; corr_b += wt.excess(w, rr[c]); }
    }
    jbus += corr_b; jbranch += corr_e;
  }
  return down;
}

// max that keeps a NaN (either operand), so the result does not depend on the order of the reduction
__device__ __forceinline__ double ws_nanmax(double x, double y) { return (x != x) ? x : ((y != y) ? y : fmax(x, y)); }

// G, b <- 0, then every row by its owner.  Starts with a barrier (u, slk and whatever read the packed array before are done with).
template <int T, class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ void ws_form(const dss2_wls_solve_args& a, const WsGraph& g, double* __restrict__ Gp, int ns, int tid, const Mask& mask,
                                        const Wt& wt = Wt()) {
  const size_t tri = (size_t)ns * (ns + 1) / 2;
  __syncthreads();
  for (size_t p = tid; p < tri + ns; p += T) Gp[p] = 0.0;
  __syncthreads();
  for (int r = tid; r < ns; r += T) ws_accumulate_row(a, g, r, Gp, ns, mask, wt);
}

// Cholesky of the packed array WITH the b row (row ns), which leaves as y = L^-1 b.  False: a pivot was <= 0 or not finite (every
// thread reads the same LDS word: the answer is uniform); the loop runs on to its fixed end.
template <int T>
__device__ __forceinline__ bool ws_factor(double* __restrict__ Gp, int ns, int tid) {
  const int tx = tid % WS_TX, ty = tid / WS_TX;
  constexpr int TY = T / WS_TX;
  bool ok = true;
  for (int j = 0; j < ns; ++j) {
    __syncthreads();
    const size_t jj = (size_t)j * (j + 1) / 2 + j;
    const double d = Gp[jj];
    const bool good = d > 0.0 && d < INFINITY;
    ok = ok && good;
    const double s = good ? sqrt(d) : 1.0;
    for (int i = j + 1 + tid; i <= ns; i += T) Gp[(size_t)i * (i + 1) / 2 + j] /= s;
    __syncthreads();
    if (tid == 0) Gp[jj] = s;
    for (int i = j + 1 + ty; i <= ns; i += TY) {
      double* rowi = Gp + (size_t)i * (i + 1) / 2;
      const double lij = rowi[j];
      const int kmax = i < ns ? i : ns - 1;
      for (int k = j + 1 + tx; k <= kmax; k += WS_TX) rowi[k] -= lij * Gp[(size_t)k * (k + 1) / 2 + j];
    }
  }
  return ok;
}

// L^T du = y, one barrier per column; ends with a barrier
template <int T>
__device__ __forceinline__ void ws_back_substitute(const double* __restrict__ Gp, double* __restrict__ bvec, double* __restrict__ du, int ns, int tid) {
  for (int j = ns - 1; j >= 0; --j) {
    __syncthreads();
    const double* rowj = Gp + (size_t)j * (j + 1) / 2;
    const double xj = bvec[j] / rowj[j];
    for (int k = tid; k < j; k += T) bvec[k] -= rowj[k] * xj;
    if (tid == 0) du[j] = xj;
  }
  __syncthreads();
}

struct WsLds {                      // the carve of ws_bytes(n)
  double* Gp; double* bvec; double* u; double* du; int* ctl; unsigned char* slk;
};
__device__ __forceinline__ WsLds ws_carve(unsigned char* smem, int n) {
  const int ns = 2 * n;
  WsLds l;
  l.Gp = reinterpret_cast<double*>(smem);
  l.bvec = l.Gp + (size_t)ns * (ns + 1) / 2;      // row ns of the packed array
  l.u = l.bvec + ns;
  l.du = l.u + ns;
  l.ctl = reinterpret_cast<int*>(smem + ws_ctl_off(n));
  l.slk = smem + ws_slk_off(n);
  return l;
}

// slack flags and the start (init or flat; a slack angle is 0) of graph g into LDS
template <int T>
__device__ __forceinline__ void ws_load_start(const dss2_wls_solve_args& a, const WsGraph& g, const WsLds& l, int tid) {
  for (int k = tid; k < g.n; k += T) {
    const int64_t gi = g.base + k;
    const bool s = a.x[gi * a.ldx + 9] != 0.f;
    l.slk[k] = s ? 1 : 0;
    l.u[2 * k] = a.init ? (double)a.init[gi * a.ld_init] : 1.0;
    l.u[2 * k + 1] = (a.init && !s) ? (double)a.init[gi * a.ld_init + 1] : 0.0;
  }
}

struct WsTally { int iters, status; double last; };   // (thread 0's copies are the ones written out)

// The decision of an iteration from the step in du and `ok` (the factorisation's answer): wave 0 forms max |du|, thread 0 writes
// ctl = {stop, apply} and its tallies.  The caller's barrier comes next.
__device__ __forceinline__ void ws_decide(const dss2_wls_solve_args& a, const double* __restrict__ du, int* __restrict__ ctl, int ns, int tid,
                                          bool ok, WsTally& t) {
  if (tid < 64) {
    double m = 0.0;
    for (int k = tid; k < ns; k += 64) m = ws_nanmax(m, fabs(du[k]));
    for (int o = 32; o > 0; o >>= 1) m = ws_nanmax(m, __shfl_xor(m, o));
    if (tid == 0) {
      int stop = 0, apply = 0;
      if (!ok || !(m < INFINITY)) { t.status = 2; stop = 1; }
      else {
        apply = 1; ++t.iters; t.last = m;
        if (m < a.tol) { t.status = 0; stop = 1; }
      }
      ctl[0] = stop; ctl[1] = apply;
    }
  }
}

// Gauss-Newton from the state in LDS: at most a.max_iter iterations (the trip count is fixed; a graph that has stopped skips the body,
// uniformly over its workgroup).  Adds the updates applied to t.iters, sets t.status (1, then 0 or 2) and t.last.  Returns whether the
// factorisation failed (uniform).  Ends with a barrier.
// wt.at(it) is the weighting of iteration `it`.
template <int T, class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ bool ws_gauss_newton(const dss2_wls_solve_args& a, const WsGraph& g, const WsLds& l, int ns, int tid,
                                                const Mask& mask, WsTally& t, const Wt& wt = Wt()) {
  t.status = 1;
  bool active = true, failed = false;  // uniform over the workgroup
  for (int it = 0; it < a.max_iter; ++it) {
    if (active) {
      ws_form<T>(a, g, l.Gp, ns, tid, mask, wt.at(it));      // (its first barrier: u, slk of the start or of the previous iteration; the previous ctl has been read)
      const bool ok = ws_factor<T>(l.Gp, ns, tid);
      ws_back_substitute<T>(l.Gp, l.bvec, l.du, ns, tid);
      // ---- the decision: one thread writes it, all read it after the barrier
      ws_decide(a, l.du, l.ctl, ns, tid, ok, t);
      __syncthreads();
      if (l.ctl[1]) for (int r = tid; r < ns; r += T) l.u[r] += l.du[r];
      active = l.ctl[0] == 0;
      failed = l.ctl[0] != 0 && l.ctl[1] == 0;
    }
  }
  __syncthreads();
  return failed;
}

// J at the state in LDS: per-bus parts into the first 2 n words of the packed array, summed by thread 0 in bus order (jb, je are
// thread 0's).  The packed array is overwritten.  Ends with a barrier.  With a weighting the per-bus counts of q < 1 go through
// wt.cnt and thread 0 writes their sum to wt.n_down: no atomics.
template <int T, class Mask, class Wt = WsNoWeight>
__device__ __forceinline__ void ws_objective(const dss2_wls_solve_args& a, const WsGraph& g, double* __restrict__ Gp, int tid, const Mask& mask,
                                             double& jb, double& je, const Wt& wt = Wt()) {
  for (int k = tid; k < g.n; k += T) {
    double b, e;
    const int down = ws_objective_bus(a, g, k, b, e, mask, wt);
    Gp[k] = b; Gp[g.n + k] = e;
    if constexpr (Wt::robust) wt.cnt[k] = down;
  }
  __syncthreads();
  jb = 0.0; je = 0.0;
  if (tid == 0) {
    for (int k = 0; k < g.n; ++k) { jb += Gp[k]; je += Gp[g.n + k]; }
    if constexpr (Wt::robust) {
      int down = 0;
      for (int k = 0; k < g.n; ++k) down += wt.cnt[k];
      *wt.n_down = down;
    }
  }
  __syncthreads();
}

// The state in LDS, in fp32
template <int T>
__device__ __forceinline__ void ws_store_state(const dss2_wls_solve_args& a, const WsGraph& g, int ns, int tid) {
  for (int r = tid; r < ns; r += T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)g.u[r];
}
// The plain epilogue of graph gr: the state in fp32, J at the fp64 state (ws_objective through `scratch`: 2 n doubles that are idle
// by now), thread 0's tallies.  Ends with ws_objective's barrier: the next graph of this workgroup may reuse the LDS.
template <int T, class Wt>
__device__ __forceinline__ void ws_finish(const dss2_wls_solve_args& a, const WsGraph& g, int64_t gr, double* __restrict__ scratch, int ns,
                                          int tid, const WsTally& t, const Wt& wt) {
  ws_store_state<T>(a, g, ns, tid);
  double jb, je;
  ws_objective<T>(a, g, scratch, tid, WsNoMask(), jb, je, wt);
  if (tid == 0) {
    a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
    a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
  }
}

// The kernel with the gain matrix in LDS: one workgroup of T threads per graph, the workgroups stride over the graphs.  A graph's
// n (ws_range) sets its carve, its trip counts and its scratch; the LDS was allocated for the bound, and the carve of a smaller graph
// lies inside it.  Nothing is carried from one graph to the next: slk, u, ctl and the packed array are written before they are read,
// and a graph ends with a barrier.  Args is
// dss2_wls_solve_args (the plain estimator) or dss2_wls_robust_args (the Huber one: ws_weighting gives its WsHuber); the two differ
// in the weighting alone, and WsNoWeight's part of every statement compiles to nothing.
template <int T, class Args, class Range = WsAnyRange>
__global__ void __launch_bounds__(T) wls_lds_kernel(const Args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
  const dss2_wls_solve_args& a = ws_solve_block(b);
  const int tid = threadIdx.x;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  auto wt = ws_weighting(b);
  using Wt = decltype(wt);
  const int64_t n_graphs = Range::n_graphs(a);
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    const WsRange rg = Range::at(a, gr);
    if (!rg.ok) {                         // uniform over the workgroup
      if (tid == 0) {
        ws_refuse(a, gr);
        if constexpr (Wt::robust) b.n_downweighted[gr] = 0;
      }
      continue;
    }
    const int n = rg.n, ns = 2 * n;
    const WsLds l = ws_carve(ws_smem, n);
    if constexpr (Wt::robust) wt.cnt = reinterpret_cast<int*>(l.Gp + 2 * n);   // behind the objective's 2 n per-bus parts: n ints, inside the packed array
    const WsGraph g = ws_graph(rg.base, n, vlv, l.u, l.slk);
    ws_load_start<T>(a, g, l, tid);
    WsTally t = {0, 1, 0.0};
    ws_gauss_newton<T>(a, g, l, ns, tid, WsNoMask(), t, wt);
    if constexpr (Wt::robust) wt.n_down = b.n_downweighted + gr;
    ws_finish<T>(a, g, gr, l.Gp, ns, tid, t, wt);
  }
}

constexpr int WS_NARROW_STATES = 64;     // up to 64 states: one wave; above: four
constexpr int WS_GROUPS_NARROW = 2048, WS_GROUPS_WIDE = 512;

// The argument checks the entries share, in two parts around each entry's own size limit (`who` names the entry in the message); 0 or 2
inline int ws_check_batch(const dss2_wls_solve_args& a, const char* who) {
  const int n = a.nodes_per_graph;
  if (a.graph_ptr) {                     // n is a bound on a graph's bus count: the kernel checks every graph against it
    if (a.n_nodes <= 0 || a.n_edges < 0 || n <= 0 || a.n_graphs < 1) { set_error("%s: with a graph_ptr n_nodes, nodes_per_graph (the bound) and n_graphs must be positive", who); return 2; }
    return 0;
  }
  if (a.n_nodes <= 0 || a.n_edges < 0 || n <= 0 || a.n_nodes % n != 0) { set_error("%s: n_nodes must be a positive multiple of nodes_per_graph", who); return 2; }
  return 0;
}
inline int ws_check_rest(const dss2_wls_solve_args& a, const char* who) {
  if (a.max_iter < 1 || !(a.tol >= 0.0)) { set_error("%s: max_iter must be >= 1 and tol >= 0", who); return 2; }
  // (a batch without any branch -- one-bus graphs -- has no edge arrays: every incidence range is empty and nothing reads them)
  if (!a.x || !a.x_mean || !a.x_std || !a.edge_mean || !a.edge_std || !a.inc_rowptr ||
      (a.n_edges > 0 && (!a.edge_attr || !a.efrom || !a.eto || !a.inc_ent)) ||
      !a.state || !a.objective || !a.iterations || !a.status || !a.last_step || !a.vminmax) { set_error("%s: null argument", who); return 2; }
  if (a.ldx < 10 || a.ldea < 10 || (a.init && a.ld_init < 2) || a.max_groups < 0) { set_error("%s: bad leading dimension or max_groups", who); return 2; }
  return 0;
}
// ... for the kernels that keep the gain matrix in LDS (extra_lds is what the kernel needs beyond ws_bytes)
inline int ws_check_args(const dss2_wls_solve_args& a, const char* who, size_t extra_lds) {
  if (int rc = ws_check_batch(a, who)) return rc;
  const int n = a.nodes_per_graph;
  if (n > (1 << 20) || ws_bytes(n) + extra_lds > (size_t)kMaxLdsBytes) {
    set_error("%s: %d buses per graph need more than the %d bytes of LDS a workgroup has (the gain matrix lives in LDS)", who, n, kMaxLdsBytes);
    return 2;
  }
  return ws_check_rest(a, who);
}
inline int64_t ws_grid(const dss2_wls_solve_args& a) {
  const int64_t n_graphs = ws_n_graphs(a);
  int64_t grid = 2 * a.nodes_per_graph <= WS_NARROW_STATES ? WS_GROUPS_NARROW : WS_GROUPS_WIDE;
  if (a.max_groups > 0 && a.max_groups < grid) grid = a.max_groups;
  return n_graphs < grid ? n_graphs : grid;
}

// The launch of a kernel on the LDS carve, after the entry's checks: K64 for one wave (up to WS_NARROW_STATES states), K256 above;
// `lds` is the kernel's dynamic LDS.  K256 may need more than the 64 KiB a kernel gets unasked: the once-per-device flag of that
// request is a static of this template, so every kernel pair has its own.
template <auto K64, auto K256, class Args>
inline int ws_launch(const Args& b, size_t lds, const char* who, hipStream_t s) {
  const dss2_wls_solve_args& a = ws_solve_block(b);
  const int64_t grid = ws_grid(a);
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  if (2 * a.nodes_per_graph <= WS_NARROW_STATES) {
    hipLaunchKernelGGL(K64, dim3((unsigned)grid), dim3(64), lds, s, b);
  } else {
    static std::atomic<uint32_t> done{0};
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(K256), done, who)) return rc;
    hipLaunchKernelGGL(K256, dim3((unsigned)grid), dim3(256), lds, s, b);
  }
  return check_launch(who);
}

}  // namespace dss2
