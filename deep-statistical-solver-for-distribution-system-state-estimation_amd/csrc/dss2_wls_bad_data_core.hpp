// What a bad-data kernel needs beyond the solve and the inversion, apart from where the covariance lives: the measurement pass, the arg-max
// over the wave and the workgroup, the removal decision, the chi-square outputs and the entry's parameter checks.  The round body of
// csrc/dss2_wls_bad_data.hip (bd_round, which all three kernels run) calls them: how Sigma[p, q] is addressed is a template parameter --
// a callable Sg(p, q) that accepts the two indices in either order -- BdPacked here (Sigma in place of the packed gain matrix in LDS),
// BdBlockRows and BdBandRows there (Sigma on block rows and on band rows in global memory).
#pragma once
#include "dss2_wls_core.hpp"

namespace dss2 {

constexpr int BD_MAX_REMOVALS = 64;
constexpr int BD_WAVES = 4;
// the block after the solve's carve: red_v[4] doubles, red_i[4], red_c[4], rem[64] ints
constexpr size_t BD_EXTRA_BYTES = BD_WAVES * 8 + BD_WAVES * 4 + BD_WAVES * 4 + BD_MAX_REMOVALS * 4;

struct BdLds { double* red_v; int* red_i; int* red_c; int* rem; };
__device__ __forceinline__ BdLds bd_carve(unsigned char* block) {     // `block`: the BD_EXTRA_BYTES after the solve's carve (8-byte aligned)
  BdLds r;
  r.red_v = reinterpret_cast<double*>(block);
  r.red_i = reinterpret_cast<int*>(r.red_v + BD_WAVES);
  r.red_c = r.red_i + BD_WAVES;
  r.rem = r.red_c + BD_WAVES;
  return r;
}

struct BdPacked {                        // Sigma on the packed lower triangle (the LDS kernel)
  const double* Sg;
  __device__ __forceinline__ double operator()(int p, int q) const {
    const int hi = p > q ? p : q, lo = p > q ? q : p;
    return Sg[(size_t)hi * (hi + 1) / 2 + lo];
  }
};
// x^T Sigma[ca : ca + 2, cb : cb + 2] y
template <class Sigma>
__device__ __forceinline__ double bd_block(const Sigma& Sg, int ca, const double (&x)[2], int cb, const double (&y)[2]) {
  return x[0] * (Sg(ca, cb) * y[0] + Sg(ca, cb + 1) * y[1]) + x[1] * (Sg(ca + 1, cb) * y[0] + Sg(ca + 1, cb + 1) * y[1]);
}

struct BdBest { double rn; int id; };    // the arg-max so far: rn = -1 before any active measurement
// whether (r1, i1) beats (r2, i2): a NaN wins, then the larger value, then the smaller id
__device__ __forceinline__ bool bd_beats(double r1, int i1, double r2, int i2) {
  const bool n1 = r1 != r1, n2 = r2 != r2;
  if (n1 || n2) return n1 && (!n2 || i1 < i2);
  return r1 > r2 || (r1 == r2 && i1 < i2);
}

// One measurement: weight w, residual res, quadratic form q = h Sigma h^T -> S and rN (0, 0 where inactive or the graph failed)
__device__ __forceinline__ void bd_emit(double w, double res, double q, double s_min, bool failed, int id, double& rn, double& sens, BdBest& best, int& cnt) {
  rn = 0.0; sens = 0.0;
  if (!(w > 0.0)) return;
  ++cnt;
  if (failed) return;
  sens = 1.0 - w * q;
  rn = sens >= s_min ? fabs(res) * sqrt(w / sens) : 0.0;
  if (bd_beats(rn, id, best.rn, best.id)) { best.rn = rn; best.id = id; }
}

// Bus li's four measurements and the flows of the branches it is the from-end of, at the state in LDS and the covariance Sg(p, q).
template <class Mask, class Sigma>
__device__ __forceinline__ void bd_bus(const dss2_wls_bad_data_args& b, const WsGraph& g, const Sigma& Sg, int li, const Mask& mask,
                                       bool failed, BdBest& best, int& cnt) {
  const dss2_wls_solve_args& a = b.solve;
  const int64_t gi = g.base + li;
  double Z[4], R[4];
  ws_meas(a.x + gi * a.ldx, a.x_mean, a.x_std, Z, R, mask, ws_bus_id(gi));
  const double vi = g.u[2 * li], ti = g.u[2 * li + 1];
  const bool sl = g.slk[li] != 0;
  const int ci = 2 * li;
  const int k0 = a.inc_rowptr[gi], k1 = a.inc_rowptr[gi + 1];
  // pass 1: P_i, Q_i and their derivatives at the bus's own state; on the way the flow measurements of the branches leaving here
  double P = 0.0, Q = 0.0, sP[2] = {0.0, 0.0}, sQ[2] = {0.0, 0.0};
  for (int k = k0; k < k1; ++k) {
    int e, lo; bool is_from;
    if (!ws_slot(a, g, k, e, lo, is_from)) continue;
    const WsBranch f = ws_branch(vi, ti, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
    P -= f.p; Q -= f.q;
    sP[0] -= f.dp[0]; sP[1] -= f.dp[1]; sQ[0] -= f.dq[0]; sQ[1] -= f.dq[1];
    if (!is_from) continue;
    double Ze[2], Re[2];
    ws_meas(a.edge_attr + (int64_t)e * a.ldea, a.edge_mean, a.edge_std, Ze, Re, mask, ws_edge_id(a, e));
    const double wp = a.w_pf * Re[0], wq = a.w_pf * Re[1];
    double qp = 0.0, qq = 0.0;
    if (!failed && (wp > 0.0 || wq > 0.0)) {
      const bool so = g.slk[lo] != 0;
      const double hp0[2] = {f.dp[0], sl ? 0.0 : f.dp[1]}, hp1[2] = {f.dp[2], so ? 0.0 : f.dp[3]};
      const double hq0[2] = {f.dq[0], sl ? 0.0 : f.dq[1]}, hq1[2] = {f.dq[2], so ? 0.0 : f.dq[3]};
      const int co = 2 * lo;
      qp = bd_block(Sg, ci, hp0, ci, hp0) + 2.0 * bd_block(Sg, co, hp1, ci, hp0) + bd_block(Sg, co, hp1, co, hp1);
      qq = bd_block(Sg, ci, hq0, ci, hq0) + 2.0 * bd_block(Sg, co, hq1, ci, hq0) + bd_block(Sg, co, hq1, co, hq1);
    }
    double rn[2], sens[2];
    bd_emit(wp, Ze[0] - f.p, qp, b.s_min, failed, ws_edge_id(a, e), rn[0], sens[0], best, cnt);
    bd_emit(wq, Ze[1] - f.q, qq, b.s_min, failed, ws_edge_id(a, e) + 1, rn[1], sens[1], best, cnt);
    b.edge_rn[2 * (int64_t)e] = rn[0]; b.edge_rn[2 * (int64_t)e + 1] = rn[1];
    b.edge_sens[2 * (int64_t)e] = sens[0]; b.edge_sens[2 * (int64_t)e + 1] = sens[1];
  }
  const double w[4] = {a.w_v * R[0], a.w_v * R[1], a.w_p * R[2], a.w_p * R[3]};
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  if (!failed) {
    q[0] = Sg(ci, ci);
    q[1] = sl ? 0.0 : Sg(ci + 1, ci + 1);
    if (w[2] > 0.0 || w[3] > 0.0) {
      // the injections' rows: (sP, sQ) at the bus's own columns, minus the other end's derivatives at every incident branch's
      const double ownp[2] = {sP[0], sl ? 0.0 : sP[1]}, ownq[2] = {sQ[0], sl ? 0.0 : sQ[1]};
      double qp = bd_block(Sg, ci, ownp, ci, ownp), qq = bd_block(Sg, ci, ownq, ci, ownq);
      for (int k = k0; k < k1; ++k) {
        int e, lo; bool is_from;
        if (!ws_slot(a, g, k, e, lo, is_from)) continue;
        const WsBranch f = ws_branch(vi, ti, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
        const bool so = g.slk[lo] != 0;
        const double hp[2] = {-f.dp[2], so ? 0.0 : -f.dp[3]}, hq[2] = {-f.dq[2], so ? 0.0 : -f.dq[3]};
        const int co = 2 * lo;
        qp += bd_block(Sg, co, hp, co, hp) + 2.0 * bd_block(Sg, co, hp, ci, ownp);
        qq += bd_block(Sg, co, hq, co, hq) + 2.0 * bd_block(Sg, co, hq, ci, ownq);
        for (int k2 = k0; k2 < k; ++k2) {
          int e2, lo2; bool from2;
          if (!ws_slot(a, g, k2, e2, lo2, from2)) continue;
          const WsBranch f2 = ws_branch(vi, ti, g.u[2 * lo2], g.u[2 * lo2 + 1], a.edge_attr + (int64_t)e2 * a.ldea + 6, g.kk);
          const bool so2 = g.slk[lo2] != 0;
          const double hp2[2] = {-f2.dp[2], so2 ? 0.0 : -f2.dp[3]}, hq2[2] = {-f2.dq[2], so2 ? 0.0 : -f2.dq[3]};
          qp += 2.0 * bd_block(Sg, co, hp, 2 * lo2, hp2);
          qq += 2.0 * bd_block(Sg, co, hq, 2 * lo2, hq2);
        }
      }
      q[2] = qp; q[3] = qq;
    }
  }
  const double res[4] = {Z[0] - vi, Z[1] - ti, Z[2] - P, Z[3] - Q};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double rn, sens;
    bd_emit(w[c], res[c], q[c], b.s_min, failed, ws_bus_id(gi) + c, rn, sens, best, cnt);
    b.bus_rn[4 * gi + c] = rn;
    b.bus_sens[4 * gi + c] = sens;
  }
}

// The round's decision from every thread's arg-max and count of active measurements: per wave (shuffles), thread 0 over the waves;
// thread 0 records the removal (rem, removed, removed_rn) and writes ctl[2]; all read it after a barrier.  Returns whether the graph
// removes (uniform); n_active is thread 0's.  Two barriers.
template <int T>
__device__ __forceinline__ bool bd_decide(const dss2_wls_bad_data_args& b, const BdLds& r, int* __restrict__ ctl, int64_t gr, int slots, bool failed,
                                          int nrem, int tid, BdBest best, int cnt, int& n_active) {
  for (int o = 32; o > 0; o >>= 1) {
    const double orn = __shfl_xor(best.rn, o);
    const int oid = __shfl_xor(best.id, o);
    if (bd_beats(orn, oid, best.rn, best.id)) { best.rn = orn; best.id = oid; }
    cnt += __shfl_xor(cnt, o);
  }
  if ((tid & 63) == 0) { r.red_v[tid >> 6] = best.rn; r.red_i[tid >> 6] = best.id; r.red_c[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < T / 64; ++w) {
      if (bd_beats(r.red_v[w], r.red_i[w], best.rn, best.id)) { best.rn = r.red_v[w]; best.id = r.red_i[w]; }
      cnt += r.red_c[w];
    }
    n_active = cnt;
    int go = 0;
    if (!failed && best.rn > b.threshold && nrem < b.max_removals) {
      r.rem[nrem] = best.id;
      b.removed[gr * slots + nrem] = best.id;
      b.removed_rn[gr * slots + nrem] = best.rn;
      go = 1;
    }
    ctl[2] = go;
  }
  __syncthreads();
  return ctl[2] != 0;
}

// Thread 0's outputs of a graph: J, the tallies, dof, the chi-square limit (Wilson-Hilferty), suspect, the unused removal slots
__device__ __forceinline__ void bd_finish(const dss2_wls_bad_data_args& b, int64_t gr, const WsTally& t, double jb, double je, int n_active, int nrem,
                                          int slots, const unsigned char* __restrict__ slk, int n) {
  const dss2_wls_solve_args& a = b.solve;
  a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
  a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
  int nfree = 2 * n;
  for (int k = 0; k < n; ++k) nfree -= slk[k];
  const int dof = n_active - nfree;
  double lim = INFINITY;
  if (dof > 0) {
    const double d = (double)dof, c = 2.0 / (9.0 * d), w = 1.0 - c + b.z_p * sqrt(c);
    lim = d * (w * w * w);
  }
  b.dof[gr] = dof; b.chi2_limit[gr] = lim; b.suspect[gr] = (jb + je) > lim ? 1 : 0;
  b.n_removed[gr] = nrem;
  for (int q = nrem; q < slots; ++q) { b.removed[gr * slots + q] = -1; b.removed_rn[gr * slots + q] = 0.0; }
}

// Thread 0's outputs of a graph that ws_range refused: the solve's, and the test's at their "failed graph" values
__device__ __forceinline__ void bd_refuse(const dss2_wls_bad_data_args& b, int64_t gr, int slots) {
  ws_refuse(b.solve, gr);
  b.dof[gr] = 0; b.chi2_limit[gr] = INFINITY; b.suspect[gr] = 0; b.n_removed[gr] = 0;
  for (int q = 0; q < slots; ++q) { b.removed[gr * slots + q] = -1; b.removed_rn[gr * slots + q] = 0.0; }
}

// The parameter checks of a bad-data entry beyond the solve's (`who` names the entry in the message); 0 or 2
inline int bd_check_params(const dss2_wls_bad_data_args& b, const char* who) {
  const dss2_wls_solve_args& a = b.solve;
  if (4 * a.n_nodes + 2 * a.n_edges > (int64_t)INT32_MAX) {
    set_error("%s: measurement ids are int32: 4 N + 2 E = %lld does not fit", who, (long long)(4 * a.n_nodes + 2 * a.n_edges));
    return 2;
  }
  if (!(b.threshold > 0.0) || b.max_removals < 0 || b.max_removals > BD_MAX_REMOVALS || !(b.s_min > 0.0 && b.s_min < 1.0) || !(fabs(b.z_p) < INFINITY)) {
    set_error("%s: threshold must be > 0, max_removals in 0 .. %d, s_min in (0, 1) and z_p finite", who, BD_MAX_REMOVALS);
    return 2;
  }
  if (!b.dof || !b.chi2_limit || !b.suspect || !b.removed || !b.removed_rn || !b.n_removed || !b.bus_rn || !b.bus_sens || !b.state_std ||
      (a.n_edges > 0 && (!b.edge_rn || !b.edge_sens))) { set_error("%s: null argument", who); return 2; }
  return 0;
}

}  // namespace dss2
