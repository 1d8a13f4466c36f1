// The reference's gnn_dsse convs (PyG GCN2Conv, FAConv, TAGConv) on gfx950: forward and backward.
//
// Lane mapping, the head Linears and the nonlinearity: dss2_lanegroup.hpp.  The head's weight gradient is dss2_lanegroup_wgrad.
// Every conv maps C channels to C channels (C <= lane group).
//
// Propagation P, j = edge_index[0] the source and i = edge_index[1] the target, with gcn_norm's weights read from dis[N]:
//     (P h)_i = sum_{e: j->i} dis_j dis_i h_j  [+ dis_i^2 h_i]
// loops = 1 (add_remaining_self_loops): edges with j == i are skipped and every node with dis_i != 0 gets one loop (dis_i == 0
// only on nodes a cached structure does not cover: they have no loop, as in PyG).  loops = 0: every edge counts, no loop.
// normalize = False is dis = 1 with loops = 0.  dss2_gnn_dis builds dis once per structure and mode.
//
//   GCN2   a = (1 - alpha) P h;  shared: u = a + alpha x0, out = u W1;  not shared: u = a, out = u W1 + (alpha x0) W2
//   FA     out_i = sum_{e: j->i} (tanh(att_l.h_j + att_r.h_i) w_e) h_j  (+ the loop)  + eps x0_i  (eps term only when eps != 0)
//   TAG    out = sum_{k=0..K} (P^k h) W_k^T + b: forward hops 1..K-1 write P^k h, hop K forms the sum
// then y = phi(out), and in the last conv's last launch the head.
//
// Backward, per conv l with dv = dy * phi'(y) (the "local step" of the target node):
//   GCN2   du = dv W1^T (stored), dW1 += u^T dv (dW2 += (alpha x0)^T dv), dx0 += alpha du (alpha dv W2^T); source pass:
//          dh_j = (1 - alpha) (P^T du)_j
//   FA     per incoming edge s_e = (1 - t_e^2) w_e (dv_i . h_j) (stored per edge; the loop's per node), S_i = sum s_e;
//          part_i = S_i att_r + t_ii w_ii dv_i (stored); d att_r += S_i h_i; dx0 += eps dv.  Source pass:
//          dh_j = part_j + sum_{e: j->i} t_e w_e dv_i + (sum_{e: j->} s_e + s_jj) att_l;  d att_l += (...) h_j
//   TAG    g_k = dv W_k (stored, k = 0..K), dW_k += dv^T P^k h, db += dv; K adjoint hops r <- g_k + P^T r, the last is dh
// Every logit, tanh and weight in the backward comes from the forward's own functions, so both passes see the same bits.  The
// local step of conv l - 1 runs in the launch of conv l's source pass (the last hop for TAG).  Weight gradients go to the
// workgroup's slab row; no float atomics.
#include "dss2_lanegroup.hpp"

using namespace dss2;

namespace {

constexpr int KMAX = DSS2_GNN_MAX_K;

struct ConvSm {
  float A[KMAX + 1][GMAX][GMAX + 1];   // lane r reads row r: GCN2 A[m][c][k] = W_m[k][c]; TAG A[k][o][c] = W_k[o][c]
};

__device__ void stage_conv(ConvSm& s, const dss2_gnn_conv& p) {
  const int nm = p.kind == DSS2_GNN_TAG ? p.K + 1 : (p.kind == DSS2_GNN_GCN2 ? (p.W[1] ? 2 : 1) : 0);
  for (int t = threadIdx.x; t < nm * GMAX * GMAX; t += NT) {
    const int m = t / (GMAX * GMAX), r = t / GMAX % GMAX, k = t % GMAX;
    float v = 0.f;
    if (r < p.c && k < p.c) v = p.kind == DSS2_GNN_TAG ? p.W[m][r * p.c + k] : p.W[m][k * p.c + r];
    s.A[m][r][k] = v;
  }
}

// the sum over the lane group by xor butterfly: every lane ends with the same bits (each step adds a pair in either order)
template <int G>
__device__ __forceinline__ float allsum(float v) {
#pragma unroll
  for (int m = G / 2; m >= 1; m /= 2) v += __shfl_xor(v, m, G);
  return v;
}

__device__ __forceinline__ float edge_w(const float* dis, int64_t j, int64_t i) { return dis[j] * dis[i]; }

// FA's attention coefficient t_e w_e for source logit al (att_l . h_j) and target logit ar (att_r . h_i)
__device__ __forceinline__ float fa_t(float al, float ar) { return tanhf(al + ar); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void gnn_fwd_kernel(const dss2_gnn_args a) {
  __shared__ ConvSm cs;
  __shared__ HeadSm hs;
  const dss2_gnn_conv& p = a.lo;
  const int kind = a.has_lo ? p.kind : 0;
  const bool combine = a.has_lo && (kind != DSS2_GNN_TAG || a.hop == p.K);   // this launch forms the conv's output
  if (combine) stage_conv(cs, p);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const bool in = a.has_lo && c < p.c;
  const float* dis = a.g.dis;
  const int loops = a.g.loops;
  const float attl = (kind == DSS2_GNN_FA && in) ? p.W[0][c] : 0.f, attr = (kind == DSS2_GNN_FA && in) ? p.W[1][c] : 0.f;
  const int64_t NC = n * p.c;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float y = 0.f;
    if (a.has_lo) {
      const float hi = in ? p.h[i * p.ldh + c] : 0.f;
      const float di = dis[i];
      const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
      float out = 0.f;
      if (kind == DSS2_GNN_GCN2) {
        float agg = 0.f;
        for (int q = r0; q < r1; ++q) {
          const int64_t j = a.g.col[q];
          if (loops && j == i) continue;
          agg = fmaf(edge_w(dis, j, i), in ? p.h[j * p.ldh + c] : 0.f, agg);
        }
        if (loops && di != 0.f) agg = fmaf(di * di, hi, agg);
        const float ua = (1.f - p.param) * agg;
        const float ax = in ? p.param * p.x0[i * p.ldx0 + c] : 0.f;
        const bool shared = p.W[1] == nullptr;
        const float u = shared ? ua + ax : ua;
        if (in) p.u[i * p.c + c] = u;
#pragma unroll
        for (int k = 0; k < G; ++k) out = fmaf(cs.A[0][c][k], __shfl(u, k, G), out);
        if (!shared) {
          float o2 = 0.f;
#pragma unroll
          for (int k = 0; k < G; ++k) o2 = fmaf(cs.A[1][c][k], __shfl(ax, k, G), o2);
          out += o2;
        }
      } else if (kind == DSS2_GNN_FA) {
        const float ar = allsum<G>(attr * hi);
        float agg = 0.f;
        for (int q = r0; q < r1; ++q) {
          const int64_t j = a.g.col[q];
          if (loops && j == i) continue;
          const float hj = in ? p.h[j * p.ldh + c] : 0.f;
          const float al = allsum<G>(attl * hj);
          agg = fmaf(fa_t(al, ar) * edge_w(dis, j, i), hj, agg);
        }
        if (loops && di != 0.f) agg = fmaf(fa_t(allsum<G>(attl * hi), ar) * (di * di), hi, agg);
        out = agg;
        if (p.param != 0.f) out = fmaf(p.param, in ? p.x0[i * p.ldx0 + c] : 0.f, out);
      } else {   // TAG hop a.hop (1..K) of P^{hop-1} h; hop 0 (K = 0) only combines
        float agg = 0.f;
        if (a.hop > 0) {
          const float* src = a.hop == 1 ? p.h : p.u + (a.hop - 2) * NC;
          const int64_t lds = a.hop == 1 ? p.ldh : p.c;
          for (int q = r0; q < r1; ++q) {
            const int64_t j = a.g.col[q];
            agg = fmaf(edge_w(dis, j, i), in ? src[j * lds + c] : 0.f, agg);
          }
          if (!combine) {
            if (in) p.u[(a.hop - 1) * NC + i * p.c + c] = agg;
            continue;
          }
        }
        out = (in && p.bias) ? p.bias[c] : 0.f;
#pragma unroll
        for (int m = 0; m <= KMAX; ++m) {
          if (m > p.K) break;
          const float pm = m == 0 ? hi : (m == p.K ? agg : (in ? p.u[(m - 1) * NC + i * p.c + c] : 0.f));
          if (m == p.K && m > 0 && in) p.u[(m - 1) * NC + i * p.c + c] = agg;
          float o = 0.f;
#pragma unroll
          for (int k = 0; k < G; ++k) o = fmaf(cs.A[m][c][k], __shfl(pm, k, G), o);
          out += o;
        }
      }
      y = act(out, a.g.nonlin);
      if (in) p.y[i * p.c + c] = y;
    } else if (a.has_head) {
      y = c < a.head.c ? a.head.hin[i * a.head.ldhin + c] : 0.f;
    }
    if (a.has_head) head_forward<G>(hs, a.head, i, c, y);
  }
}

// ---- backward: [head backward | source pass / adjoint hop of conv `up` | gy], then [local step of conv `lo`] or dh ---------------
template <int G>
__global__ __launch_bounds__(NT) void gnn_bwd_kernel(const dss2_gnn_args a) {
  __shared__ ConvSm ls;
  __shared__ HeadSm hs;
  __shared__ float red[NT][GMAX + 1];
  if (a.has_lo) stage_conv(ls, a.lo);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const float* dis = a.g.dis;
  const int loops = a.g.loops, nl = a.g.nonlin;
  const dss2_gnn_conv& up = a.up;
  const dss2_gnn_conv& lo = a.lo;
  const int ukind = a.has_up ? up.kind : 0, lkind = a.has_lo ? lo.kind : 0;
  const int C = a.has_lo ? lo.c : (a.has_up ? up.c : 0);
  const bool in = c < C;
  const int64_t NC = n * C;
  const float u_attl = (ukind == DSS2_GNN_FA && in) ? up.W[0][c] : 0.f, u_attr = (ukind == DSS2_GNN_FA && in) ? up.W[1][c] : 0.f;
  const float l_attl = (lkind == DSS2_GNN_FA && in) ? lo.W[0][c] : 0.f, l_attr = (lkind == DSS2_GNN_FA && in) ? lo.W[1][c] : 0.f;
  float gw[KMAX + 1][G];   // lo: the weight partials of lane c (GCN2: dW_m[k][c]; TAG: dW_k[c][k'])
  float gb = 0.f;          // lo: TAG d bias[c]; FA d att_r[c]
  float gu = 0.f;          // up: FA d att_l[c]
#pragma unroll
  for (int m = 0; m <= KMAX; ++m)
#pragma unroll
    for (int k = 0; k < G; ++k) gw[m][k] = 0.f;
  const bool last_hop = !(ukind == DSS2_GNN_TAG) || a.hop == 0;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float gy = 0.f;   // gradient of lo's output (or of the model input) at channel c
    if (a.has_head) {
      gy = head_backward<G>(hs, a.head, i, c);
    } else if (a.has_up) {
      const int r0 = a.g.rowptrT[i], r1 = a.g.rowptrT[i + 1];
      const float di = dis[i];
      if (ukind == DSS2_GNN_GCN2) {
        float acc = 0.f;
        for (int q = r0; q < r1; ++q) {
          const int64_t t = a.g.colT[q];
          if (loops && t == i) continue;
          acc = fmaf(edge_w(dis, i, t), in ? up.d[t * C + c] : 0.f, acc);
        }
        if (loops && di != 0.f) acc = fmaf(di * di, in ? up.d[i * C + c] : 0.f, acc);
        gy = (1.f - up.param) * acc;
      } else if (ukind == DSS2_GNN_FA) {
        const float hi = in ? up.h[i * up.ldh + c] : 0.f;
        const float al = allsum<G>(u_attl * hi);
        float acc = in ? up.part[i * C + c] : 0.f, sl = up.sn[i];
        for (int q = r0; q < r1; ++q) {
          const int64_t t = a.g.colT[q], e = a.g.entT[q] & 0x7fffffff;
          if (loops && t == i) continue;
          const float ar = allsum<G>(u_attr * (in ? up.h[t * up.ldh + c] : 0.f));
          acc = fmaf(fa_t(al, ar) * edge_w(dis, i, t), in ? up.d[t * C + c] : 0.f, acc);
          sl += up.se[e];
        }
        gy = fmaf(sl, u_attl, acc);
        gu = fmaf(sl, hi, gu);
      } else {   // TAG adjoint hop: r_hop = g_hop + P^T r_{hop+1}
        float acc = 0.f;
        if (a.rin)
          for (int q = r0; q < r1; ++q) {
            const int64_t t = a.g.colT[q];
            acc = fmaf(edge_w(dis, i, t), in ? a.rin[t * C + c] : 0.f, acc);
          }
        gy = (in ? up.d[a.hop * NC + i * C + c] : 0.f) + acc;
        if (!last_hop) {
          if (in) a.rout[i * C + c] = gy;
          continue;
        }
      }
    } else {
      gy = in ? a.gy[i * a.ldgy + c] : 0.f;
    }
    if (!a.has_lo) {
      if (a.dh && c < a.dh_cols) a.dh[i * a.dh_cols + c] = a.dx0 ? gy + a.dx0[i * C + c] : gy;
      continue;
    }
    // local step of conv lo for node i
    const float dv = in ? gy * act_grad(lo.y[i * C + c], nl) : 0.f;
    float gx0 = 0.f;   // this conv's x0-path gradient
    if (lkind == DSS2_GNN_GCN2) {
      const float u = in ? lo.u[i * C + c] : 0.f;
      float du = 0.f;
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const float dk = __shfl(dv, k, G);
        du = fmaf(ls.A[0][k][c], dk, du);
        gw[0][k] = fmaf(__shfl(u, k, G), dv, gw[0][k]);
      }
      if (in) lo.d[i * C + c] = du;
      if (lo.W[1]) {
        const float ax = in ? lo.param * lo.x0[i * lo.ldx0 + c] : 0.f;
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) {
          d2 = fmaf(ls.A[1][k][c], __shfl(dv, k, G), d2);
          gw[1][k] = fmaf(__shfl(ax, k, G), dv, gw[1][k]);
        }
        gx0 = lo.param * d2;
      } else {
        gx0 = lo.param * du;
      }
    } else if (lkind == DSS2_GNN_FA) {
      if (in) lo.d[i * C + c] = dv;
      const float hi = in ? lo.h[i * lo.ldh + c] : 0.f, di = dis[i];
      const float ar = allsum<G>(l_attr * hi);
      const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
      float S = 0.f;
      for (int q = r0; q < r1; ++q) {
        const int64_t j = a.g.col[q], e = a.g.ent[q] & 0x7fffffff;
        if (loops && j == i) continue;
        const float hj = in ? lo.h[j * lo.ldh + c] : 0.f;
        const float t = fa_t(allsum<G>(l_attl * hj), ar);
        const float s = (1.f - t * t) * (edge_w(dis, j, i) * allsum<G>(dv * hj));
        if (c == 0) lo.se[e] = s;
        S += s;
      }
      float part = 0.f, sll = 0.f;
      if (loops && di != 0.f) {
        const float t = fa_t(allsum<G>(l_attl * hi), ar), w = di * di;
        sll = (1.f - t * t) * (w * allsum<G>(dv * hi));
        S += sll;
        part = (t * w) * dv;
      }
      if (c == 0) lo.sn[i] = sll;
      if (in) lo.part[i * C + c] = fmaf(S, l_attr, part);
      gb = fmaf(S, hi, gb);
      gx0 = lo.param != 0.f ? lo.param * dv : 0.f;
    } else {   // TAG: g_k = dv W_k, dW_k[c][k'] += dv_c (P^k h)_k', db += dv
      const float hi = in ? lo.h[i * lo.ldh + c] : 0.f;
#pragma unroll
      for (int m = 0; m <= KMAX; ++m) {
        if (m > lo.K) break;
        const float pm = m == 0 ? hi : (in ? lo.u[(m - 1) * NC + i * C + c] : 0.f);
        float g = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) {
          g = fmaf(ls.A[m][k][c], __shfl(dv, k, G), g);
          gw[m][k] = fmaf(dv, __shfl(pm, k, G), gw[m][k]);
        }
        if (in) lo.d[m * NC + i * C + c] = g;
      }
      gb += dv;
    }
    if (a.dx0 && lkind != DSS2_GNN_TAG && in) a.dx0[i * C + c] = a.dx0_first ? gx0 : a.dx0[i * C + c] + gx0;
  }
  // this workgroup's partials -> its slab row (fixed order over the lane groups)
  float* row = a.g.slab + (int64_t)blockIdx.x * a.g.slab_len;
  if (ukind == DSS2_GNN_FA) {   // columns at slab_off: att_l[C], att_r[C]; the source pass owns att_l
    red[threadIdx.x][0] = gu;
    __syncthreads();
    for (int t = threadIdx.x; t < C; t += NT) row[up.slab_off + t] = group_sum<G>(red, t, 0);
    __syncthreads();
  }
  if (lkind == DSS2_GNN_FA) {
    red[threadIdx.x][0] = gb;
    __syncthreads();
    for (int t = threadIdx.x; t < C; t += NT) row[lo.slab_off + C + t] = group_sum<G>(red, t, 0);
    __syncthreads();
  }
  if (lkind == DSS2_GNN_GCN2 || lkind == DSS2_GNN_TAG) {
    // GCN2 at slab_off: weight1[C][C] (, weight2[C][C]), element [k][c] from lane c's gw[m][k].
    // TAG at slab_off: bias[C], lins.m.weight[C][C] (m = 0..K), element [c][k] from lane c's gw[m][k].
    const bool tag = lkind == DSS2_GNN_TAG;
    const int nm = tag ? lo.K + 1 : (lo.W[1] ? 2 : 1), base = lo.slab_off + (tag ? C : 0);
#pragma unroll
    for (int m = 0; m <= KMAX; ++m) {
      if (m >= nm) break;
#pragma unroll
      for (int k = 0; k < G; ++k) red[threadIdx.x][k] = gw[m][k];
      red[threadIdx.x][G] = gb;
      __syncthreads();
      for (int t = threadIdx.x; t < C * C; t += NT) {
        const int r = t / C, s = t % C;   // element [r][s]
        row[base + m * C * C + t] = tag ? group_sum<G>(red, r, s) : group_sum<G>(red, s, r);
      }
      if (tag && m == 0)
        for (int t = threadIdx.x; t < C; t += NT) row[lo.slab_off + t] = group_sum<G>(red, t, G);
      __syncthreads();
    }
  }
}

__global__ void gnn_dis_kernel(const int32_t* rowptr, const int32_t* col, int64_t n, int mode, float* dis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode == 0) { dis[i] = 1.f; return; }
  int deg = 0;
  for (int q = rowptr[i]; q < rowptr[i + 1]; ++q) deg += (mode == 2 && col[q] == i) ? 0 : 1;
  deg += mode == 2;
  dis[i] = deg > 0 ? 1.f / sqrtf((float)deg) : 0.f;
}

int check_conv(const dss2_gnn_conv& p, const dss2_gnn_args& a, const char* what) {
  if (p.kind != DSS2_GNN_GCN2 && p.kind != DSS2_GNN_FA && p.kind != DSS2_GNN_TAG) { set_error("%s: conv kind %d", what, p.kind); return 2; }
  if (p.c < 1 || p.c > a.group) { set_error("%s: %d channels exceed the lane group %d (limit %d)", what, p.c, a.group, GMAX); return 2; }
  if (p.K < 0 || p.K > KMAX) { set_error("%s: K = %d outside [0, %d]", what, p.K, KMAX); return 2; }
  const int nw = p.kind == DSS2_GNN_TAG ? p.K + 1 : (p.kind == DSS2_GNN_FA ? 2 : 1);
  for (int m = 0; m < nw; ++m)
    if (!p.W[m]) { set_error("%s: weight %d is missing", what, m); return 2; }
  if (!p.h || !p.y || (p.kind != DSS2_GNN_TAG && !p.x0)) { set_error("%s: a conv pointer is missing", what); return 2; }
  if ((p.kind == DSS2_GNN_GCN2 || (p.kind == DSS2_GNN_TAG && p.K > 0)) && !p.u) { set_error("%s: no u / hop buffer", what); return 2; }
  return 0;
}

int check_args(const dss2_gnn_args& a, bool forward, const char* what) {
  if (int rc = check_lanegroup_args(a, what)) return rc;
  if ((a.has_lo || a.has_up) && (!a.g.dis || !a.g.rowptr || !a.g.rowptrT)) { set_error("%s: graph pointer missing", what); return 2; }
  if (a.has_up)
    if (int rc = check_conv(a.up, a, what)) return rc;
  if (a.has_lo)
    if (int rc = check_conv(a.lo, a, what)) return rc;
  if (a.has_up && a.has_lo && a.up.c != a.lo.c) { set_error("%s: convs of different widths", what); return 2; }
  return check_pass_args(a, forward, what);
}

}  // namespace

static int dss2_gnn_forward_launch(const dss2_gnn_args* ap, void* stream) {
  const dss2_gnn_args& a = *ap;
  if (int rc = check_args(a, true, "dss2_gnn_forward")) return rc;
  if (a.has_lo) {
    const bool tag = a.lo.kind == DSS2_GNN_TAG;
    if (tag ? (a.hop < (a.lo.K ? 1 : 0) || a.hop > a.lo.K) : a.hop != 0) { set_error("dss2_gnn_forward: hop %d", a.hop); return 2; }
    if (a.has_head && tag && a.hop != a.lo.K) { set_error("dss2_gnn_forward: the head goes with the last hop"); return 2; }
  }
  return launch_group(gnn_fwd_kernel<8>, gnn_fwd_kernel<16>, gnn_fwd_kernel<32>, a, stream, "dss2_gnn_forward");
}

static int dss2_gnn_backward_launch(const dss2_gnn_args* ap, void* stream) {
  const dss2_gnn_args& a = *ap;
  if (int rc = check_args(a, false, "dss2_gnn_backward")) return rc;
  if (a.has_up) {
    const dss2_gnn_conv& u = a.up;
    if (!u.d) { set_error("dss2_gnn_backward: the source pass has no gradient buffer"); return 2; }
    if (u.kind == DSS2_GNN_FA && (!u.se || !u.sn || !u.part)) { set_error("dss2_gnn_backward: FA buffers missing"); return 2; }
    if (u.kind == DSS2_GNN_TAG) {
      if (a.hop < 0 || a.hop >= (u.K ? u.K : 1)) { set_error("dss2_gnn_backward: hop %d", a.hop); return 2; }
      if ((u.K > 0) != (a.rin != nullptr) || (a.hop > 0 && !a.rout)) { set_error("dss2_gnn_backward: adjoint hop buffers"); return 2; }
      if (a.hop > 0 && a.has_lo) { set_error("dss2_gnn_backward: only the last adjoint hop takes a local step"); return 2; }
    } else if (a.hop != 0) {
      set_error("dss2_gnn_backward: hop %d", a.hop); return 2;
    }
  }
  if (a.has_lo) {
    const dss2_gnn_conv& l = a.lo;
    if (!l.d || (l.kind == DSS2_GNN_FA && (!l.se || !l.sn || !l.part))) { set_error("dss2_gnn_backward: local step buffers missing"); return 2; }
  }
  return launch_group(gnn_bwd_kernel<8>, gnn_bwd_kernel<16>, gnn_bwd_kernel<32>, a, stream, "dss2_gnn_backward");
}

static int dss2_gnn_dis_launch(const int32_t* rowptr, const int32_t* col, int64_t n, int mode, float* dis, void* stream) {
  if (!rowptr || !dis || n <= 0 || mode < 0 || mode > 2) { set_error("dss2_gnn_dis: bad arguments"); return 2; }
  hipLaunchKernelGGL(gnn_dis_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), rowptr, col, n, mode, dis);
  return check_launch("dss2_gnn_dis");
}

extern "C" int dss2_gnn_forward(const dss2_gnn_args* ap, void* stream) {
  return dss2::entry(dss2_gnn_forward_launch, stream, dss2::copied(ap, "dss2_gnn_forward"));
}

extern "C" int dss2_gnn_backward(const dss2_gnn_args* ap, void* stream) {
  return dss2::entry(dss2_gnn_backward_launch, stream, dss2::copied(ap, "dss2_gnn_backward"));
}

extern "C" int dss2_gnn_dis(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int mode, float* dis, void* stream) {
  return dss2::entry(dss2_gnn_dis_launch, stream, rowptr, col, n_nodes, mode, dis);
}
