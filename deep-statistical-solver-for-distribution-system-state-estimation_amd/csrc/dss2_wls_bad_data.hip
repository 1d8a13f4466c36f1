// Bad-data detection and removal on the batched WLS estimator, fp64, gfx950: the solve of dss2_wls_solve.hip, then the covariance,
// residual sensitivities, normalized residuals, the chi-square test and the removal of the largest normalized residual, repeated --
// all inside ONE launch, one workgroup per graph, the launch geometry of wls_solve.  The device functions of the solve are those of
// dss2_wls_core.hpp, with a mask that gives a removed measurement the weight 0 everywhere it enters.
//
//   LDS   the solve's carve (packed G with the b row, u, du, ctl, slack flags), then a fixed block:
//         red   per-wave partial results of the arg-max and of the count of active measurements (4 waves at most)
//         rem   the ids removed so far (at most 64)
//
//   per round (trip count = max_removals + 1; a graph that has stopped removing skips the body, uniformly over its workgroup)
//     1. Gauss-Newton from the state in LDS (ws_gauss_newton: the very loop of wls_solve).
//     2. G at the last iterate, formed and factorised once more; then IN PLACE on the packed lower triangle
//          L -> X = L^-1    column by column from the last: the column is copied to du, then row owner i forms -(X[i, j+1..i] . L[j+1..i, j]) / L[j, j]
//          X -> Sigma = X^T X   row by row from the first: thread j forms sum_{k >= i} X[k, i] X[k, j], a barrier, the row is written (rows
//                               above i are never read again, rows below are still X)
//        A slack angle's row and column of G are the identity, so Sigma has 1 on that diagonal and 0 beside it; its h entries are dropped.
//     3. thread l OWNS bus l's four measurements and the two flows of every branch bus l is the from-end of: h_i Sigma h_i^T as a double
//        sum over the (few) non-zeros of the Jacobian row, branch physics recomputed per visit as in the row accumulation.  An injection's
//        row has 2 (deg + 1) non-zeros: its quadratic form costs deg (deg + 1) / 2 + 2 deg branch evaluations.
//     4. arg-max of rN and the count of active measurements: per thread, per wave (shuffles), thread 0 over the waves; ties go to the
//        smallest id.  Thread 0 records the removal and writes the decision; all read it after a barrier.
//   afterwards: state, J with the final weights, dof, the chi-square limit, suspect, the tallies.
//
// Every __syncthreads() sits in control flow that is uniform over the workgroup (failed, the round's flag and ok are uniform: every
// thread derives them from the same LDS words).  The thread that owns a row of Sigma is its index: 2 n <= T is checked at the entry.
#include "dss2_wls_core.hpp"

namespace dss2 {

constexpr int BD_MAX_REMOVALS = 64;
constexpr int BD_WAVES = 4;
// the block after the solve's carve: red_v[4] doubles, red_i[4], red_c[4], rem[64] ints
constexpr size_t BD_EXTRA_BYTES = BD_WAVES * 8 + BD_WAVES * 4 + BD_WAVES * 4 + BD_MAX_REMOVALS * 4;
__host__ __device__ inline size_t bd_bytes(int n) { return ws_bytes(n) + BD_EXTRA_BYTES; }

// L (packed lower triangle, after ws_factor) -> Sigma = (L L^T)^-1 in place; tmp: ns doubles.  Starts and ends with a barrier.
template <int T>
__device__ __forceinline__ void bd_invert(double* __restrict__ Gp, double* __restrict__ tmp, int ns, int tid) {
  for (int j = ns - 1; j >= 0; --j) {
    __syncthreads();                     // the columns right of j are X; the previous tmp has been read
    const size_t jj = (size_t)j * (j + 1) / 2 + j;
    const double xjj = 1.0 / Gp[jj];
    for (int i = j + 1 + tid; i < ns; i += T) tmp[i] = Gp[(size_t)i * (i + 1) / 2 + j];
    __syncthreads();
    if (tid == 0) Gp[jj] = xjj;
    for (int i = j + 1 + tid; i < ns; i += T) {
      double* rowi = Gp + (size_t)i * (i + 1) / 2;
      double s = 0.0;
      for (int k = j + 1; k <= i; ++k) s += rowi[k] * tmp[k];
      rowi[j] = -s * xjj;
    }
  }
  __syncthreads();
  for (int i = 0; i < ns; ++i) {
    double s = 0.0;
    if (tid <= i)
      for (int k = i; k < ns; ++k) { const double* rowk = Gp + (size_t)k * (k + 1) / 2; s += rowk[i] * rowk[tid]; }
    __syncthreads();                     // row i has been read by everyone (rows below it are not written in this step)
    if (tid <= i) Gp[(size_t)i * (i + 1) / 2 + tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ double bd_sig(const double* __restrict__ Sg, int p, int q) {
  const int hi = p > q ? p : q, lo = p > q ? q : p;
  return Sg[(size_t)hi * (hi + 1) / 2 + lo];
}
// x^T Sigma[ca : ca + 2, cb : cb + 2] y
__device__ __forceinline__ double bd_block(const double* __restrict__ Sg, int ca, const double (&x)[2], int cb, const double (&y)[2]) {
  return x[0] * (bd_sig(Sg, ca, cb) * y[0] + bd_sig(Sg, ca, cb + 1) * y[1]) + x[1] * (bd_sig(Sg, ca + 1, cb) * y[0] + bd_sig(Sg, ca + 1, cb + 1) * y[1]);
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

// Bus li's four measurements and the flows of the branches it is the from-end of, at the state and the Sigma in LDS.
template <class Mask>
__device__ __forceinline__ void bd_bus(const dss2_wls_bad_data_args& b, const WsGraph& g, const double* __restrict__ Sg, int li, const Mask& mask,
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
    q[0] = bd_sig(Sg, ci, ci);
    q[1] = sl ? 0.0 : bd_sig(Sg, ci + 1, ci + 1);
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

template <int T>
__global__ void __launch_bounds__(T) wls_bad_data_kernel(const dss2_wls_bad_data_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bd_smem[];
  const dss2_wls_solve_args& a = b.solve;
  const int n = a.nodes_per_graph, ns = 2 * n;
  const WsLds l = ws_carve(bd_smem, n);
  double* red_v = reinterpret_cast<double*>(bd_smem + ws_bytes(n));
  int* red_i = reinterpret_cast<int*>(red_v + BD_WAVES);
  int* red_c = red_i + BD_WAVES;
  int* rem = red_c + BD_WAVES;
  const int tid = threadIdx.x;
  const int slots = b.max_removals > 1 ? b.max_removals : 1;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    WsGraph g;
    g.base = gr * n; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = l.u; g.slk = l.slk;
    ws_load_start<T>(a, g, l, tid);
    WsTally t = {0, 1, 0.0};
    int nrem = 0, n_active = 0;          // nrem is uniform; n_active is thread 0's
    bool removing = true;                // uniform
    for (int round = 0; round <= b.max_removals; ++round) {
      if (removing) {
        const WsRemoved mask = {rem, nrem};
        bool failed = ws_gauss_newton<T>(a, g, l, ns, tid, mask, t);
        if (!failed) {
          ws_form<T>(a, g, l.Gp, ns, tid, mask);
          if (!ws_factor<T>(l.Gp, ns, tid)) {
            failed = true;
            if (tid == 0) t.status = 2;
          }
        }
        if (!failed) bd_invert<T>(l.Gp, l.du, ns, tid);
        BdBest best = {-1.0, 0x7fffffff};
        int cnt = 0;
        for (int k = tid; k < n; k += T) bd_bus(b, g, l.Gp, k, mask, failed, best, cnt);
        for (int r = tid; r < ns; r += T)
          b.state_std[(g.base + (r >> 1)) * 2 + (r & 1)] = (failed || ((r & 1) && l.slk[r >> 1])) ? 0.0 : sqrt(l.Gp[(size_t)r * (r + 1) / 2 + r]);
        for (int o = 32; o > 0; o >>= 1) {
          const double orn = __shfl_xor(best.rn, o);
          const int oid = __shfl_xor(best.id, o);
          if (bd_beats(orn, oid, best.rn, best.id)) { best.rn = orn; best.id = oid; }
          cnt += __shfl_xor(cnt, o);
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = best.rn; red_i[tid >> 6] = best.id; red_c[tid >> 6] = cnt; }
        __syncthreads();
        if (tid == 0) {
          for (int w = 1; w < T / 64; ++w) {
            if (bd_beats(red_v[w], red_i[w], best.rn, best.id)) { best.rn = red_v[w]; best.id = red_i[w]; }
            cnt += red_c[w];
          }
          n_active = cnt;
          int go = 0;
          if (!failed && best.rn > b.threshold && nrem < b.max_removals) {
            rem[nrem] = best.id;
            b.removed[gr * slots + nrem] = best.id;
            b.removed_rn[gr * slots + nrem] = best.rn;
            go = 1;
          }
          l.ctl[2] = go;
        }
        __syncthreads();
        removing = l.ctl[2] != 0;
        if (removing) ++nrem;
      }
    }
    // ---- outputs: the state in fp32, J at the fp64 state with the final weights, the test, the tallies
    for (int r = tid; r < ns; r += T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)l.u[r];
    double jb, je;
    ws_objective<T>(a, g, l.Gp, tid, WsRemoved{rem, nrem}, jb, je);
    if (tid == 0) {
      a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
      a.iterations[gr] = t.iters; a.status[gr] = t.status; a.last_step[gr] = t.last;
      int nfree = ns;
      for (int k = 0; k < n; ++k) nfree -= l.slk[k];
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
    __syncthreads();                     // the next graph of this workgroup reuses the LDS (rem and slk included)
  }
}

}  // namespace dss2

using namespace dss2;

extern "C" size_t dss2_wls_bad_data_lds_bytes(int nodes_per_graph) {
  return nodes_per_graph > 0 ? bd_bytes(nodes_per_graph) : 0;
}

static int dss2_wls_bad_data_launch(const dss2_wls_bad_data_args* bp, void* stream);
extern "C" int dss2_wls_bad_data(const dss2_wls_bad_data_args* bp, void* stream) {
  if (!bp) { dss2::set_error("dss2_wls_bad_data: null argument"); return 2; }
  DSS2_RECORD([b = *bp](void* s_) { return dss2_wls_bad_data_launch(&b, s_); });
  return dss2_wls_bad_data_launch(bp, stream);
}
static int dss2_wls_bad_data_launch(const dss2_wls_bad_data_args* bp, void* stream) {
  const dss2_wls_bad_data_args& b = *bp;
  const dss2_wls_solve_args& a = b.solve;
  if (int rc = ws_check_args(a, "wls_bad_data", BD_EXTRA_BYTES)) return rc;
  const int n = a.nodes_per_graph;
  const bool narrow = 2 * n <= WS_NARROW_STATES;
  if (2 * n > 256) { set_error("wls_bad_data: %d states do not fit the workgroup that owns the covariance's rows", 2 * n); return 2; }
  if (4 * a.n_nodes + 2 * a.n_edges > (int64_t)INT32_MAX) {
    set_error("wls_bad_data: measurement ids are int32: 4 N + 2 E = %lld does not fit", (long long)(4 * a.n_nodes + 2 * a.n_edges));
    return 2;
  }
  if (!(b.threshold > 0.0) || b.max_removals < 0 || b.max_removals > BD_MAX_REMOVALS || !(b.s_min > 0.0 && b.s_min < 1.0) || !(fabs(b.z_p) < INFINITY)) {
    set_error("wls_bad_data: threshold must be > 0, max_removals in 0 .. %d, s_min in (0, 1) and z_p finite", BD_MAX_REMOVALS);
    return 2;
  }
  if (!b.dof || !b.chi2_limit || !b.suspect || !b.removed || !b.removed_rn || !b.n_removed || !b.bus_rn || !b.bus_sens || !b.state_std ||
      (a.n_edges > 0 && (!b.edge_rn || !b.edge_sens))) { set_error("wls_bad_data: null argument"); return 2; }
  hipStream_t s = as_stream(stream);
  const int64_t grid = ws_grid(a);
  const size_t lds = bd_bytes(n);
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  if (narrow) {
    hipLaunchKernelGGL(wls_bad_data_kernel<64>, dim3((unsigned)grid), dim3(64), lds, s, b);
  } else {
    static std::atomic<uint32_t> done{0};
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&wls_bad_data_kernel<256>), done, "wls_bad_data")) return rc;
    hipLaunchKernelGGL(wls_bad_data_kernel<256>, dim3((unsigned)grid), dim3(256), lds, s, b);
  }
  return check_launch("wls_bad_data");
}
