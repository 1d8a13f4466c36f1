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
#include "dss2_common.hpp"

namespace dss2 {

constexpr int WS_TX = 16;          // trailing update: 16 columns x (T / 16) rows of threads

// LDS carve (bytes from the 16-byte aligned dynamic base), shared by the kernel and dss2_wls_solve_lds_bytes
__host__ __device__ inline size_t ws_doubles(int n) { const size_t ns = 2 * (size_t)n; return ns * (ns + 1) / 2 + 3 * ns; }
__host__ __device__ inline size_t ws_ctl_off(int n) { return (ws_doubles(n) * 8 + 15) / 16 * 16; }
__host__ __device__ inline size_t ws_slk_off(int n) { return ws_ctl_off(n) + 16; }
__host__ __device__ inline size_t ws_bytes(int n) { return ws_slk_off(n) + ((size_t)n + 15) / 16 * 16; }

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

// double(z) * double(std) + double(mean) where the normalised entry is non-zero, else 0; a weight below 0 counts as 0
template <int PAIRS>
__device__ __forceinline__ void ws_meas(const float* __restrict__ in, const float* __restrict__ mean, const float* __restrict__ stdv,
                                        double (&Z)[PAIRS], double (&R)[PAIRS]) {
#pragma unroll
  for (int c = 0; c < PAIRS; ++c) {
    const float z = in[2 * c], r = in[2 * c + 1];
    Z[c] = (z != 0.f) ? (double)z * (double)stdv[2 * c] + (double)mean[2 * c] : 0.0;
    const double w = (r != 0.f) ? (double)r * (double)stdv[2 * c + 1] + (double)mean[2 * c + 1] : 0.0;
    R[c] = w < 0.0 ? 0.0 : w;
  }
}

struct WsGraph {                    // what the row owners need of the graph being solved
  int64_t base;                     // first bus
  int n;
  double kk;                        // V_lv^2
  const double* u;                  // LDS state
  const unsigned char* slk;         // LDS slack flags
};

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

// Row r of G and b[r]: every measurement with a non-zero Jacobian entry at state r, in a fixed order.
__device__ __forceinline__ void ws_accumulate_row(const dss2_wls_solve_args& a, const WsGraph& g, int r, double* __restrict__ Gp, int ns) {
  double* row = Gp + (size_t)r * (r + 1) / 2;
  double* bvec = Gp + (size_t)ns * (ns + 1) / 2;
  const int li = r >> 1, c = r & 1;
  if (c && g.slk[li]) { row[r] = 1.0; bvec[r] = 0.0; return; }     // a slack angle: identity row, held at 0
  const int64_t gi = g.base + li;
  double accb = 0.0;
  {   // the bus's own V (c = 0) or theta (c = 1)
    double Z[4], R[4];
    ws_meas(a.x + gi * a.ldx, a.x_mean, a.x_std, Z, R);
    const double w = a.w_v * (c ? R[1] : R[0]);
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
        ws_meas(a.edge_attr + (int64_t)e * a.ldea, a.edge_mean, a.edge_std, Ze, Re);
        if (Re[0] != 0.0 || Re[1] != 0.0) {
          const WsBranch f = ws_branch(g.u[2 * lf], g.u[2 * lf + 1], g.u[2 * lt], g.u[2 * lt + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
          double hp = 0.0, hq = 0.0;
          if (lf == li) { hp += c ? f.dp[1] : f.dp[0]; hq += c ? f.dq[1] : f.dq[0]; }
          if (lt == li) { hp += c ? f.dp[3] : f.dp[2]; hq += c ? f.dq[3] : f.dq[2]; }
          const double gp = a.w_pf * Re[0] * hp, gq = a.w_pf * Re[1] * hq;
          accb += gp * (Ze[0] - f.p) + gq * (Ze[1] - f.q);
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
    ws_meas(a.x + gj * a.ldx, a.x_mean, a.x_std, Z, R);
    const double wP = a.w_p * R[2], wQ = a.w_p * R[3];
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
    const double gP = wP * hP, gQ = wQ * hQ;
    accb += gP * (Z[2] - P) + gQ * (Z[3] - Q);
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

// The two parts of J at the state in LDS for bus li: its own four measurements, and the flows of the branches it is the from-end of.
__device__ __forceinline__ void ws_objective_bus(const dss2_wls_solve_args& a, const WsGraph& g, int li, double& jbus, double& jbranch) {
  const int64_t gi = g.base + li;
  double Z[4], R[4];
  ws_meas(a.x + gi * a.ldx, a.x_mean, a.x_std, Z, R);
  const double vi = g.u[2 * li], ti = g.u[2 * li + 1];
  double P = 0.0, Q = 0.0;
  jbranch = 0.0;
  const int k0 = a.inc_rowptr[gi], k1 = a.inc_rowptr[gi + 1];
  for (int k = k0; k < k1; ++k) {
    int e, lo; bool is_from;
    if (!ws_slot(a, g, k, e, lo, is_from)) continue;
    const WsBranch f = ws_branch(vi, ti, g.u[2 * lo], g.u[2 * lo + 1], a.edge_attr + (int64_t)e * a.ldea + 6, g.kk);
    P -= f.p; Q -= f.q;
    if (is_from) {
      double Ze[2], Re[2];
      ws_meas(a.edge_attr + (int64_t)e * a.ldea, a.edge_mean, a.edge_std, Ze, Re);
      const double dp = Ze[0] - f.p, dq = Ze[1] - f.q;
      jbranch += a.w_pf * (Re[0] * dp * dp + Re[1] * dq * dq);
    }
  }
  const double dv = Z[0] - vi, dt = Z[1] - ti, dP = Z[2] - P, dQ = Z[3] - Q;
  jbus = a.w_v * (R[0] * dv * dv + R[1] * dt * dt) + a.w_p * (R[2] * dP * dP + R[3] * dQ * dQ);
}

// max that keeps a NaN (either operand), so the result does not depend on the order of the reduction
__device__ __forceinline__ double ws_nanmax(double x, double y) { return (x != x) ? x : ((y != y) ? y : fmax(x, y)); }

template <int T>
__global__ void __launch_bounds__(T) wls_solve_kernel(const dss2_wls_solve_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
  const int n = a.nodes_per_graph, ns = 2 * n;
  const size_t tri = (size_t)ns * (ns + 1) / 2;
  double* Gp = reinterpret_cast<double*>(ws_smem);
  double* bvec = Gp + tri;             // row ns of the packed array
  double* u = bvec + ns;
  double* du = u + ns;
  int* ctl = reinterpret_cast<int*>(ws_smem + ws_ctl_off(n));
  unsigned char* slk = ws_smem + ws_slk_off(n);
  const int tid = threadIdx.x, tx = tid % WS_TX, ty = tid / WS_TX;
  constexpr int TY = T / WS_TX;
  float vlv, vhv;
  vminmax_fold(a.vminmax, vlv, vhv);
  const int64_t n_graphs = a.n_nodes / n;
  for (int64_t gr = blockIdx.x; gr < n_graphs; gr += gridDim.x) {
    WsGraph g;
    g.base = gr * n; g.n = n; g.kk = (double)vlv * (double)vlv; g.u = u; g.slk = slk;
    for (int l = tid; l < n; l += T) {
      const int64_t gi = g.base + l;
      const bool s = a.x[gi * a.ldx + 9] != 0.f;
      slk[l] = s ? 1 : 0;
      u[2 * l] = a.init ? (double)a.init[gi * a.ld_init] : 1.0;
      u[2 * l + 1] = (a.init && !s) ? (double)a.init[gi * a.ld_init + 1] : 0.0;
    }
    int iters = 0, status = 1;           // (thread 0's copies are the ones written out)
    double last = 0.0;
    bool active = true;                  // uniform over the workgroup
    for (int it = 0; it < a.max_iter; ++it) {
      if (active) {
        __syncthreads();                 // u, slk of the start or of the previous iteration; the previous ctl has been read
        for (size_t p = tid; p < tri + ns; p += T) Gp[p] = 0.0;
        __syncthreads();
        for (int r = tid; r < ns; r += T) ws_accumulate_row(a, g, r, Gp, ns);
        // ---- Cholesky of G with b as row ns; afterwards row ns holds y = L^-1 b
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
        // ---- L^T du = y
        for (int j = ns - 1; j >= 0; --j) {
          __syncthreads();
          const double* rowj = Gp + (size_t)j * (j + 1) / 2;
          const double xj = bvec[j] / rowj[j];
          for (int k = tid; k < j; k += T) bvec[k] -= rowj[k] * xj;
          if (tid == 0) du[j] = xj;
        }
        __syncthreads();
        // ---- the decision: one thread writes it, all read it after the barrier
        if (tid < 64) {
          double m = 0.0;
          for (int k = tid; k < ns; k += 64) m = ws_nanmax(m, fabs(du[k]));
          for (int o = 32; o > 0; o >>= 1) m = ws_nanmax(m, __shfl_xor(m, o));
          if (tid == 0) {
            int stop = 0, apply = 0;
            if (!ok || !(m < INFINITY)) { status = 2; stop = 1; }
            else {
              apply = 1; ++iters; last = m;
              if (m < a.tol) { status = 0; stop = 1; }
            }
            ctl[0] = stop; ctl[1] = apply;
          }
        }
        __syncthreads();
        if (ctl[1]) for (int r = tid; r < ns; r += T) u[r] += du[r];
        active = ctl[0] == 0;
      }
    }
    __syncthreads();
    // ---- outputs: the state in fp32, J at the fp64 state (per-bus parts summed by one thread in bus order)
    for (int r = tid; r < ns; r += T) a.state[(g.base + (r >> 1)) * 2 + (r & 1)] = (float)u[r];
    for (int l = tid; l < n; l += T) {
      double jb, je;
      ws_objective_bus(a, g, l, jb, je);
      Gp[l] = jb; Gp[n + l] = je;
    }
    __syncthreads();
    if (tid == 0) {
      double jb = 0.0, je = 0.0;
      for (int l = 0; l < n; ++l) { jb += Gp[l]; je += Gp[n + l]; }
      a.objective[2 * gr] = jb; a.objective[2 * gr + 1] = je;
      a.iterations[gr] = iters; a.status[gr] = status; a.last_step[gr] = last;
    }
    __syncthreads();                     // the next graph of this workgroup reuses the LDS
  }
}

constexpr int WS_NARROW_STATES = 64;     // up to 64 states: one wave; above: four
constexpr int WS_GROUPS_NARROW = 2048, WS_GROUPS_WIDE = 512;

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
  const int n = a.nodes_per_graph;
  if (a.n_nodes <= 0 || a.n_edges < 0 || n <= 0 || a.n_nodes % n != 0) { set_error("wls_solve: n_nodes must be a positive multiple of nodes_per_graph"); return 2; }
  if (n > (1 << 20) || ws_bytes(n) > (size_t)kMaxLdsBytes) {
    set_error("wls_solve: %d buses per graph need more than the %d bytes of LDS a workgroup has (the gain matrix lives in LDS)", n, kMaxLdsBytes);
    return 2;
  }
  if (a.max_iter < 1 || !(a.tol >= 0.0)) { set_error("wls_solve: max_iter must be >= 1 and tol >= 0"); return 2; }
  if (!a.x || !a.edge_attr || !a.x_mean || !a.x_std || !a.edge_mean || !a.edge_std || !a.efrom || !a.eto || !a.inc_rowptr || !a.inc_ent ||
      !a.state || !a.objective || !a.iterations || !a.status || !a.last_step || !a.vminmax) { set_error("wls_solve: null argument"); return 2; }
  if (a.ldx < 10 || a.ldea < 10 || (a.init && a.ld_init < 2) || a.max_groups < 0) { set_error("wls_solve: bad leading dimension or max_groups"); return 2; }
  hipStream_t s = as_stream(stream);
  const int64_t n_graphs = a.n_nodes / n;
  const bool narrow = 2 * n <= WS_NARROW_STATES;
  int64_t grid = narrow ? WS_GROUPS_NARROW : WS_GROUPS_WIDE;
  if (a.max_groups > 0 && a.max_groups < grid) grid = a.max_groups;
  if (n_graphs < grid) grid = n_graphs;
  const size_t lds = ws_bytes(n);
  launch_vminmax(a.x + 8, a.ldx, a.n_nodes, a.vminmax, s);
  if (narrow) {
    hipLaunchKernelGGL(wls_solve_kernel<64>, dim3((unsigned)grid), dim3(64), lds, s, a);
  } else {
    static std::atomic<uint32_t> done{0};
    if (int rc = ensure_max_lds(reinterpret_cast<const void*>(&wls_solve_kernel<256>), done, "wls_solve")) return rc;
    hipLaunchKernelGGL(wls_solve_kernel<256>, dim3((unsigned)grid), dim3(256), lds, s, a);
  }
  return check_launch("wls_solve");
}
