// The reference's MultiConvNet (networks.py:737-835) on gfx950: parallel PyG ChebConv (normalization=None), one per edge feature,
// whose edge weights come out of a small MLP -- so the loss is differentiated with respect to an edge weight.  The semantics, the
// adjoint and the launches: include/dss2_hip.h (dss2_cheb_*).
//
// Lane mapping and launch geometry: dss2_lanegroup.hpp (one node per lane group, lane c owns channel c, one slab row per workgroup).
// The lins' weight gradients are outer products of dv and the saved T_k, and the edge MLP's of dz1 / dw and ea / a1:
// dss2_lanegroup_wgrad, into the one slab that dss2_reduce_slabs_multi sums.  fp32 VALU; no float atomics: every dwh / ddn entry has
// one owning lane group per launch (the SOURCE node's, in the pass over the CSR by source), and the launches are ordered on the stream.
//
// The edge kernels run one thread per node (over its outgoing edges) or per stored edge; their maximum and their sum are reduced per
// workgroup and then over the workgroups, both in index order.
#include "dss2_lanegroup.hpp"

using namespace dss2;

namespace {

constexpr int KMAX = DSS2_CHEB_MAX_K, FMAX = DSS2_CHEB_MAX_CONVS, HIDMAX = 64, WGMAX = 256;

struct MatSm {
  float A[GMAX][GMAX + 1];   // [o][c] = W[o][c]: the forward's lane o reads row o, the backward's lane c column c
};

__device__ void stage_mat(MatSm& s, const float* W, int cout, int cin) {
  for (int t = threadIdx.x; t < GMAX * GMAX; t += NT) {
    const int o = t / GMAX, c = t % GMAX;
    s.A[o][c] = (W && o < cout && c < cin) ? W[o * cin + c] : 0.f;
  }
}

// the sum over the lane group by xor butterfly: every lane ends with the same bits
template <int G>
__device__ __forceinline__ float allsum(float v) {
#pragma unroll
  for (int m = G / 2; m >= 1; m /= 2) v += __shfl_xor(v, m, G);
  return v;
}

// lane c's element of W^T v (v: lane o holds element o)
template <int G>
__device__ __forceinline__ float matT_vec(const MatSm& s, int c, float v) {
  float g = 0.f;
#pragma unroll
  for (int o = 0; o < G; ++o) g = fmaf(s.A[o][c], __shfl(v, o, G), g);
  return g;
}

// lane o's element of W v (v: lane c holds element c)
template <int G>
__device__ __forceinline__ float mat_vec(const MatSm& s, int o, float v) {
  float g = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) g = fmaf(s.A[o][k], __shfl(v, k, G), g);
  return g;
}

__device__ __forceinline__ float drop_mult(const dss2_cheb_args& a, uint64_t seed, uint64_t off, int id, int64_t i, int c) {
  return dropout_mult4(seed, off, (uint32_t)id, (uint32_t)i, (uint32_t)(c >> 2), a.drop_thr, a.drop_scale)[c & 3];
}

// ---- forward hop -----------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void cheb_fwd_kernel(const dss2_cheb_args a) {
  __shared__ MatSm ws[FMAX + 1];   // ws[f] = lins[hop] of conv f; ws[FMAX] = the sum over f of lins[0] (T_0 = x for every conv)
  __shared__ float bs[GMAX];       // the sum of the biases
  const dss2_cheb_layer& p = a.lo;
  const int F = a.g.n_convs, K = p.K, hop = a.hop;
  const bool first = hop <= 1, last = hop == K - 1;
  if (hop >= 1)
    for (int f = 0; f < F; ++f) stage_mat(ws[f], p.W[f][hop], p.cout, p.cin);
  if (first) {
    for (int t = threadIdx.x; t < GMAX * GMAX; t += NT) {
      const int o = t / GMAX, c = t % GMAX;
      float v = 0.f;
      if (o < p.cout && c < p.cin)
        for (int f = 0; f < F; ++f) v += p.W[f][0][o * p.cin + c];
      ws[FMAX].A[o][c] = v;
    }
    for (int t = threadIdx.x; t < GMAX; t += NT) {
      float v = 0.f;
      if (t < p.cout)
        for (int f = 0; f < F; ++f) v += p.bias[f] ? p.bias[f][t] : 0.f;
      bs[t] = v;
    }
  }
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, R = a.g.n_rows, stride = (int64_t)gridDim.x * (NT / G);
  const bool in = c < p.cin, oc = c < p.cout;
  const int64_t NC = n * p.cin;
  uint64_t seed = 0, off = 0;
  const bool drop = last && p.drop_id > 0 && a.drop_state;
  if (drop) { seed = a.drop_state[0]; off = a.drop_state[1]; }
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    const float xi = in ? p.h[i * p.ldh + c] : 0.f;
    float out = first ? bs[c] + mat_vec<G>(ws[FMAX], c, xi) : (oc ? p.y[i * p.cout + c] : 0.f);
    if (hop >= 1) {
      const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
      for (int f = 0; f < F; ++f) {
        const float* Tf = p.T + (int64_t)f * (K - 1) * NC;           // T_k of conv f at Tf + (k - 1) NC
        const float* prev = hop == 1 ? p.h : Tf + (hop - 2) * NC;     // T_{hop-1}
        const int64_t ldp = hop == 1 ? p.ldh : p.cin;
        const float tp = hop == 1 ? xi : (in ? prev[i * ldp + c] : 0.f);
        const float* wh = a.g.what + f * R;
        float acc = (a.g.dn[f * n + i] - 1.f) * tp;
        for (int q = r0; q < r1; ++q) {
          const int64_t j = a.g.col[q];
          if (j == i) continue;
          acc = fmaf(wh[a.g.ent[q] & 0x7fffffff], in ? prev[j * ldp + c] : 0.f, acc);
        }
        float tn = acc;
        if (hop >= 2) tn = 2.f * acc - (hop == 2 ? xi : (in ? Tf[(hop - 3) * NC + i * p.cin + c] : 0.f));
        if (in) p.T[(int64_t)f * (K - 1) * NC + (hop - 1) * NC + i * p.cin + c] = tn;
        out += mat_vec<G>(ws[f], c, tn);
      }
    }
    if (last) {
      if (drop) out *= drop_mult(a, seed, off, p.drop_id, i, c);
      if (p.relu) out = relu_nan(out);
    }
    if (oc) p.y[i * p.cout + c] = out;
  }
}

// ---- backward: [adjoint hop of `up` | gy], then [local step of `lo`] or dh ---------------------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void cheb_bwd_kernel(const dss2_cheb_args a) {
  __shared__ MatSm us[FMAX];   // up: lins[hop - 1] of conv f (lins[0] when K = 1)
  __shared__ MatSm ls[FMAX];   // lo: lins[K - 1] of conv f (K >= 2)
  const dss2_cheb_layer& up = a.up;
  const dss2_cheb_layer& lo = a.lo;
  const int F = a.g.n_convs, hop = a.hop;
  if (a.has_up)
    for (int f = 0; f < F; ++f) stage_mat(us[f], up.W[f][up.K == 1 ? 0 : hop - 1], up.cout, up.cin);
  if (a.has_lo && lo.K >= 2)
    for (int f = 0; f < F; ++f) stage_mat(ls[f], lo.W[f][lo.K - 1], lo.cout, lo.cin);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, R = a.g.n_rows, E2 = a.g.n_edges, stride = (int64_t)gridDim.x * (NT / G);
  const bool pass_on = !a.has_up || up.K == 1 || hop == 1;   // this launch ends the layer `up`: its r_0 goes to lo or to dh
  uint64_t seed = 0, off = 0;
  const bool drop = a.has_lo && lo.drop_id > 0 && a.drop_state;
  if (drop) { seed = a.drop_state[0]; off = a.drop_state[1]; }
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float gy = 0.f;   // gradient of lo's output (or of the model input) at channel c
    if (a.has_up) {
      const int K = up.K, ci = up.cin;
      const bool in = c < ci;
      const int64_t NC = n * ci;
      const float dvo = c < up.cout ? up.dv[i * up.cout + c] : 0.f;
      const int r0 = a.g.rowptrT[i], r1 = a.g.rowptrT[i + 1];
      for (int f = 0; f < F; ++f) {
        const float g = matT_vec<G>(us[f], c, dvo);   // lins[hop - 1]^T dv
        if (K == 1) { gy += g; continue; }
        const float tl = !in ? 0.f : (hop == 1 ? up.h[i * up.ldh + c] : up.T[((int64_t)f * (K - 1) + hop - 2) * NC + i * ci + c]);   // T_{hop-1}(i)
        const float* rk = up.r[hop % 2] + f * NC;
        const float* wh = a.g.what + f * R;
        const float ck = hop == 1 ? 1.f : 2.f;
        const float ri = in ? rk[i * ci + c] : 0.f;
        float acc = (a.g.dn[f * n + i] - 1.f) * ri;
        const float sd = ck * allsum<G>(ri * tl);
        if (c == 0) a.ddn[f * n + i] = a.acc_first ? sd : a.ddn[f * n + i] + sd;
        for (int q = r0; q < r1; ++q) {
          const int64_t t = a.g.colT[q];
          if (t == i) continue;
          const float rt = in ? rk[t * ci + c] : 0.f;
          acc = fmaf(wh[a.g.entT[q] & 0x7fffffff], rt, acc);
          const float se = ck * allsum<G>(rt * tl);
          const int64_t d = f * E2 + a.g.permT[q];
          if (c == 0) a.dwh[d] = a.acc_first ? se : a.dwh[d] + se;
        }
        float rn = fmaf(ck, acc, g);
        if (hop + 1 <= K - 1 && in) rn -= up.r[(hop + 1) % 2][f * NC + i * ci + c];
        if (hop > 1) {
          if (in) up.r[(hop - 1) % 2][f * NC + i * ci + c] = rn;   // (over r_{hop+1}(i), which only this lane read)
        } else {
          gy += rn;
        }
      }
    } else {
      gy = (a.has_lo && c < lo.cout) ? a.gy[i * a.ldgy + c] : 0.f;
    }
    if (!pass_on) continue;
    if (!a.has_lo) {
      if (a.dh && c < a.dh_cols) a.dh[i * a.dh_cols + c] = gy;
      continue;
    }
    // local step of the layer lo for node i
    const bool oc = c < lo.cout;
    float dv = oc ? gy : 0.f;
    if (drop) dv *= drop_mult(a, seed, off, lo.drop_id, i, c);
    if (lo.relu && oc) dv = relu_open(lo.y[i * lo.cout + c]) ? dv : 0.f;
    if (oc) lo.dv[i * lo.cout + c] = dv;
    if (lo.K >= 2) {
      const int64_t NC = n * lo.cin;
      for (int f = 0; f < F; ++f) {
        const float g = matT_vec<G>(ls[f], c, dv);
        if (c < lo.cin) lo.r[(lo.K - 1) % 2][f * NC + i * lo.cin + c] = g;
      }
    }
  }
}

// ---- the edge weights ----------------------------------------------------------------------------------------------------------------
struct MlpSm { float W1[HIDMAX][2], b1[HIDMAX], W2[2][HIDMAX], b2[2]; };

__device__ void stage_mlp(MlpSm& s, const dss2_cheb_edge_args& a) {
  for (int t = threadIdx.x; t < a.hid; t += blockDim.x) {
    s.W1[t][0] = a.W1[2 * t]; s.W1[t][1] = a.W1[2 * t + 1]; s.b1[t] = a.b1[t];
    s.W2[0][t] = a.W2[t]; s.W2[1][t] = a.W2[a.hid + t];
  }
  if (threadIdx.x < 2) s.b2[threadIdx.x] = a.b2[threadIdx.x];
}

__device__ __forceinline__ float mlp_hidden(const MlpSm& s, int h, float e0, float e1) {
  return relu_nan(fmaf(s.W1[h][1], e1, fmaf(s.W1[h][0], e0, s.b1[h])));
}

// the weights of stored edge r for every conv
__device__ __forceinline__ void edge_weights(const MlpSm& s, const dss2_cheb_edge_args& a, int64_t r, float (&w)[FMAX]) {
#pragma unroll
  for (int f = 0; f < FMAX; ++f) w[f] = 0.f;
  if (a.has_mlp) {
    const float e0 = a.ea[r * a.ldea], e1 = a.ea[r * a.ldea + 1];
    float o0 = s.b2[0], o1 = s.b2[1];
    for (int h = 0; h < a.hid; ++h) {
      const float z = mlp_hidden(s, h, e0, e1);
      o0 = fmaf(s.W2[0][h], z, o0);
      o1 = fmaf(s.W2[1][h], z, o1);
    }
    w[0] = e0 + o0;
    w[1] = e1 + o1;
  } else {
#pragma unroll
    for (int f = 0; f < FMAX; ++f)
      if (f < a.g.n_convs) w[f] = a.w_in[r * a.ldw + f];
  }
}

// one candidate of torch's max: a NaN wins; on a tie the lower index (torch splits the gradient evenly there)
// (the index is d < n_edges or n_edges + i: below 2^32 - 8 by the Topology's limits, so 32 bits and NONE hold it)
constexpr uint32_t NONE = 0xffffffffu;
struct Best {
  float v;
  uint32_t i;   // NONE: no candidate yet
  __device__ __forceinline__ void take(float cv, uint32_t ci) {
    bool b;
    if (i == NONE) b = true;
    else if (cv != cv) b = v == v || ci < i;
    else if (v != v) b = false;
    else b = cv > v || (cv == v && ci < i);
    v = b ? cv : v;
    i = b ? ci : i;
  }
};

// w of every stored edge (written by the thread of its source node), deg into dn, the workgroup's maximum of -w_d and deg_i
__global__ __launch_bounds__(WGMAX) void cheb_edge_fwd_kernel(const dss2_cheb_edge_args a) {
  __shared__ MlpSm ms;
  __shared__ float rv[FMAX][WGMAX];
  __shared__ uint32_t ri[FMAX][WGMAX];
  if (a.has_mlp) stage_mlp(ms, a);
  __syncthreads();
  const int F = a.g.n_convs;
  const int64_t n = a.g.n_nodes, R = a.g.n_rows, E2 = a.g.n_edges;
  Best b0{0.f, NONE}, b1{0.f, NONE}, b2{0.f, NONE}, b3{0.f, NONE};   // conv f's candidate (FMAX = 4)
  static_assert(FMAX == 4, "one Best per conv");
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    for (int q = a.g.rowptrT[j]; q < a.g.rowptrT[j + 1]; ++q) {
      const int64_t t = a.g.colT[q], r = a.g.entT[q] & 0x7fffffff, d = a.g.permT[q];
      float w[FMAX];
      edge_weights(ms, a, r, w);
      if (d < R) {      // the stored direction (d == r) writes the weights
        a.g.w[r] = w[0];
        if (F > 1) a.g.w[R + r] = w[1];
        if (F > 2) a.g.w[2 * R + r] = w[2];
        if (F > 3) a.g.w[3 * R + r] = w[3];
      }
      if (t != j) {
        d0 += w[0]; d1 += w[1]; d2 += w[2]; d3 += w[3];
        const uint32_t di = (uint32_t)d;
        b0.take(-w[0], di); b1.take(-w[1], di); b2.take(-w[2], di); b3.take(-w[3], di);
      }
    }
    a.g.dn[j] = d0;
    if (F > 1) a.g.dn[n + j] = d1;
    if (F > 2) a.g.dn[2 * n + j] = d2;
    if (F > 3) a.g.dn[3 * n + j] = d3;
    const uint32_t ni = (uint32_t)(E2 + j);
    b0.take(d0, ni); b1.take(d1, ni); b2.take(d2, ni); b3.take(d3, ni);
  }
  rv[0][threadIdx.x] = b0.v; ri[0][threadIdx.x] = b0.i;
  rv[1][threadIdx.x] = b1.v; ri[1][threadIdx.x] = b1.i;
  rv[2][threadIdx.x] = b2.v; ri[2][threadIdx.x] = b2.i;
  rv[3][threadIdx.x] = b3.v; ri[3][threadIdx.x] = b3.i;
  __syncthreads();
  if ((int)threadIdx.x < F) {
    const int f = threadIdx.x;
    Best m{0.f, NONE};
    for (int t = 0; t < (int)blockDim.x; ++t)
      if (ri[f][t] != NONE) m.take(rv[f][t], ri[f][t]);
    a.pmax[f * a.n_wg + blockIdx.x] = m.v;
    a.parg[f * a.n_wg + blockIdx.x] = m.i == NONE ? -1 : (int64_t)m.i;
  }
}

__device__ __forceinline__ float no_inf(float v) { return v == INFINITY ? 0.f : v; }

__global__ __launch_bounds__(WGMAX) void cheb_edge_norm_kernel(const dss2_cheb_edge_args a) {
  __shared__ float lam[FMAX];
  const int F = a.g.n_convs;
  if ((int)threadIdx.x < F) {
    const int f = threadIdx.x;
    Best m{0.f, NONE};
    if (a.lambda_given) {
      m.v = a.lambda;
    } else {
      for (int t = 0; t < a.n_wg; ++t)
        if (a.parg[f * a.n_wg + t] >= 0) m.take(a.pmax[f * a.n_wg + t], (uint32_t)a.parg[f * a.n_wg + t]);
      m.v = 2.f * m.v;
    }
    lam[f] = m.v;
    if (blockIdx.x == 0) { a.g.lam[f] = m.v; a.g.arg[f] = m.i == NONE ? -1 : (int64_t)m.i; }
  }
  __syncthreads();
  const int64_t n = a.g.n_nodes, R = a.g.n_rows;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (n > R ? n : R); t += (int64_t)gridDim.x * blockDim.x)
    for (int f = 0; f < F; ++f) {
      if (t < R) a.g.what[f * R + t] = no_inf((2.f * -a.g.w[f * R + t]) / lam[f]);
      if (t < n) a.g.dn[f * n + t] = no_inf((2.f * a.g.dn[f * n + t]) / lam[f]);
    }
}

// psum[f][wg] = this workgroup's part of sum_d what_d dwh_d + sum_i dn_i ddn_i
__global__ __launch_bounds__(WGMAX) void cheb_edge_bwd_sum_kernel(const dss2_cheb_edge_args a) {
  __shared__ float red[FMAX][WGMAX];
  const int F = a.g.n_convs;
  const int64_t n = a.g.n_nodes, R = a.g.n_rows, E2 = a.g.n_edges;
  float s[FMAX];
#pragma unroll
  for (int f = 0; f < FMAX; ++f) s[f] = 0.f;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int f = 0; f < FMAX; ++f) {
      if (f >= F) break;
      for (int q = a.g.rowptrT[j]; q < a.g.rowptrT[j + 1]; ++q) {
        if (a.g.colT[q] == j) continue;
        s[f] = fmaf(a.g.what[f * R + (a.g.entT[q] & 0x7fffffff)], a.dwh[f * E2 + a.g.permT[q]], s[f]);
      }
      s[f] = fmaf(a.g.dn[f * n + j], a.ddn[f * n + j], s[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < FMAX; ++f) red[f][threadIdx.x] = s[f];
  __syncthreads();
  if ((int)threadIdx.x < F) {
    float v = 0.f;
    for (int t = 0; t < (int)blockDim.x; ++t) v += red[threadIdx.x][t];
    a.psum[threadIdx.x * a.n_wg + blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(WGMAX) void cheb_edge_bwd_kernel(const dss2_cheb_edge_args a) {
  __shared__ MlpSm ms;
  __shared__ float dlam2[FMAX], lam[FMAX];   // 2 d lambda; lambda
  const int F = a.g.n_convs;
  if (a.has_mlp) stage_mlp(ms, a);
  if ((int)threadIdx.x < F) {
    const int f = threadIdx.x;
    float v = 0.f;
    if (!a.zero_in && !a.lambda_given)
      for (int t = 0; t < a.n_wg; ++t) v += a.psum[f * a.n_wg + t];
    lam[f] = a.g.lam[f];
    dlam2[f] = (a.zero_in || a.lambda_given) ? 0.f : 2.f * (-v / lam[f]);
  }
  __syncthreads();
  const int64_t n = a.g.n_nodes, R = a.g.n_rows, E2 = a.g.n_edges;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    float gw[FMAX];
#pragma unroll
    for (int f = 0; f < FMAX; ++f) {
      gw[f] = 0.f;
      if (f >= F || a.zero_in) continue;
      const int64_t arg = a.g.arg[f];
      for (int64_t d = r; d < E2; d += R) {      // the stored direction and, in a doubled graph, its reverse
        const int64_t s = d < R ? a.g.efrom[r] : a.g.eto[r], t = d < R ? a.g.eto[r] : a.g.efrom[r];
        if (s == t) continue;
        gw[f] += (2.f / lam[f]) * (a.ddn[f * n + s] - a.dwh[f * E2 + d]);
        if (arg == d) gw[f] -= dlam2[f];
        if (arg == E2 + s) gw[f] += dlam2[f];
      }
    }
#pragma unroll
    for (int f = 0; f < FMAX; ++f)
      if (f < F) a.dw[r * F + f] = gw[f];
    if (a.has_mlp) {
      const float e0 = a.ea[r * a.ldea], e1 = a.ea[r * a.ldea + 1];
      for (int h = 0; h < a.hid; ++h) {
        const float z = mlp_hidden(ms, h, e0, e1);
        const float da = fmaf(ms.W2[1][h], gw[1], ms.W2[0][h] * gw[0]);
        a.a1[r * a.hid + h] = z;
        a.dz1[r * a.hid + h] = relu_open(z) ? da : 0.f;
      }
    }
  }
}

// ---- argument checks ---------------------------------------------------------------------------------------------------------------
int check_graph(const dss2_cheb_graph& g, const char* what) {
  if (g.n_nodes <= 0 || g.n_edges < 0 || g.n_rows < 0 || (g.n_edges != g.n_rows && g.n_edges != 2 * g.n_rows)) {
    set_error("%s: %lld nodes, %lld directed edges of %lld stored ones", what, (long long)g.n_nodes, (long long)g.n_edges, (long long)g.n_rows);
    return 2;
  }
  if (g.n_edges + g.n_nodes >= (int64_t)NONE) { set_error("%s: %lld edges + %lld nodes do not fit the 32-bit arg-max index", what, (long long)g.n_edges, (long long)g.n_nodes); return 2; }
  if (g.n_convs < 1 || g.n_convs > FMAX) { set_error("%s: %d parallel convs outside [1, %d]", what, g.n_convs, FMAX); return 2; }
  if (!g.rowptr || !g.rowptrT || !g.dn || !g.lam || !g.arg) { set_error("%s: graph pointer missing", what); return 2; }
  if (g.n_edges > 0 && (!g.col || !g.ent || !g.colT || !g.entT || !g.permT || !g.efrom || !g.eto || !g.w || !g.what)) {
    set_error("%s: edge pointer missing", what);
    return 2;
  }
  return 0;
}

int check_layer(const dss2_cheb_layer& p, const dss2_cheb_args& a, bool backward, const char* what) {
  if (p.cin < 1 || p.cin > a.group || p.cout < 1 || p.cout > a.group) {
    set_error("%s: %d -> %d channels exceed the lane group %d (limit %d)", what, p.cin, p.cout, a.group, GMAX);
    return 2;
  }
  if (p.K < 1 || p.K > KMAX) { set_error("%s: K = %d outside [1, %d]", what, p.K, KMAX); return 2; }
  for (int f = 0; f < a.g.n_convs; ++f)
    for (int k = 0; k < p.K; ++k)
      if (!p.W[f][k]) { set_error("%s: lins.%d.weight of conv %d is missing", what, k, f); return 2; }
  if (!p.h || !p.y || (p.K > 1 && !p.T)) { set_error("%s: a layer pointer is missing", what); return 2; }
  if (backward && (!p.dv || (p.K > 1 && (!p.r[0] || !p.r[1])))) { set_error("%s: a backward buffer of the layer is missing", what); return 2; }
  if (p.drop_id < 0 || (p.drop_id > 0 && !a.drop_state)) { set_error("%s: dropout id %d without a state", what, p.drop_id); return 2; }
  return 0;
}

int check_args(const dss2_cheb_args& a, bool forward, const char* what) {
  if (int rc = check_lanegroup_args(a, what)) return rc;
  if (a.has_head) { set_error("%s: these models have no head", what); return 2; }
  if (int rc = check_graph(a.g, what)) return rc;
  if (a.has_up)
    if (int rc = check_layer(a.up, a, true, what)) return rc;
  if (a.has_lo)
    if (int rc = check_layer(a.lo, a, !forward, what)) return rc;
  return check_pass_args(a, forward, what);
}

int check_edge_args(const dss2_cheb_edge_args& a, bool forward, const char* what) {
  if (int rc = check_graph(a.g, what)) return rc;
  if (a.n_wg < 1 || a.n_wg > WGMAX || !a.pmax || !a.parg || !a.psum) { set_error("%s: %d workgroups (1..%d) / no partials", what, a.n_wg, WGMAX); return 2; }
  if (a.has_mlp) {
    if (a.g.n_convs != 2 || a.hid < 1 || a.hid > HIDMAX) { set_error("%s: the edge MLP feeds 2 convs through 1..%d hidden units (got %d, %d)", what, HIDMAX, a.g.n_convs, a.hid); return 2; }
    if (!a.W1 || !a.b1 || !a.W2 || !a.b2 || (a.g.n_rows > 0 && (!a.ea || a.ldea < 2))) { set_error("%s: an edge MLP pointer is missing", what); return 2; }
    if (!forward && a.g.n_rows > 0 && (!a.dz1 || !a.a1)) { set_error("%s: no dz1 / a1", what); return 2; }
  } else if (a.g.n_rows > 0 && (!a.w_in || a.ldw < a.g.n_convs)) {
    set_error("%s: no edge weights", what);
    return 2;
  }
  if (!forward && a.g.n_rows > 0 && (!a.dw || (!a.zero_in && (!a.dwh || !a.ddn)))) { set_error("%s: a gradient buffer is missing", what); return 2; }
  return 0;
}

}  // namespace

static int dss2_cheb_forward_launch(const dss2_cheb_args* ap, void* stream) {
  const dss2_cheb_args& a = *ap;
  if (int rc = check_args(a, true, "dss2_cheb_forward")) return rc;
  if (!a.has_lo || a.hop < (a.lo.K > 1 ? 1 : 0) || a.hop > a.lo.K - 1) { set_error("dss2_cheb_forward: hop %d", a.hop); return 2; }
  return launch_group(cheb_fwd_kernel<8>, cheb_fwd_kernel<16>, cheb_fwd_kernel<32>, a, stream, "dss2_cheb_forward");
}

static int dss2_cheb_backward_launch(const dss2_cheb_args* ap, void* stream) {
  const dss2_cheb_args& a = *ap;
  if (int rc = check_args(a, false, "dss2_cheb_backward")) return rc;
  if (a.has_up) {
    const dss2_cheb_layer& u = a.up;
    if (a.hop < (u.K > 1 ? 1 : 0) || a.hop > u.K - 1) { set_error("dss2_cheb_backward: hop %d", a.hop); return 2; }
    if (u.K > 1 && (!a.dwh || !a.ddn)) { set_error("dss2_cheb_backward: no dwh / ddn"); return 2; }
    if (a.hop > 1 && a.has_lo) { set_error("dss2_cheb_backward: only the last adjoint hop takes a local step"); return 2; }
    if (a.has_lo && a.lo.cout != u.cin) { set_error("dss2_cheb_backward: layer widths %d -> %d do not chain", a.lo.cout, u.cin); return 2; }
    if (!a.has_lo && a.dh && a.dh_cols != u.cin) { set_error("dss2_cheb_backward: dh has %d columns, the layer %d", a.dh_cols, u.cin); return 2; }
  }
  return launch_group(cheb_bwd_kernel<8>, cheb_bwd_kernel<16>, cheb_bwd_kernel<32>, a, stream, "dss2_cheb_backward");
}

static int dss2_cheb_edge_forward_launch(const dss2_cheb_edge_args* ap, void* stream) {
  const dss2_cheb_edge_args& a = *ap;
  if (int rc = check_edge_args(a, true, "dss2_cheb_edge_forward")) return rc;
  hipLaunchKernelGGL(cheb_edge_fwd_kernel, dim3((unsigned)a.n_wg), dim3(WGMAX), 0, as_stream(stream), a);
  hipLaunchKernelGGL(cheb_edge_norm_kernel, dim3((unsigned)a.n_wg), dim3(WGMAX), 0, as_stream(stream), a);
  return check_launch("dss2_cheb_edge_forward");
}

static int dss2_cheb_edge_backward_launch(const dss2_cheb_edge_args* ap, void* stream) {
  const dss2_cheb_edge_args& a = *ap;
  if (int rc = check_edge_args(a, false, "dss2_cheb_edge_backward")) return rc;
  if (a.g.n_rows == 0) return 0;
  if (!a.zero_in && !a.lambda_given)
    hipLaunchKernelGGL(cheb_edge_bwd_sum_kernel, dim3((unsigned)a.n_wg), dim3(WGMAX), 0, as_stream(stream), a);
  hipLaunchKernelGGL(cheb_edge_bwd_kernel, dim3((unsigned)a.n_wg), dim3(WGMAX), 0, as_stream(stream), a);
  return check_launch("dss2_cheb_edge_backward");
}

extern "C" int dss2_cheb_forward(const dss2_cheb_args* ap, void* stream) {
  return dss2::entry(dss2_cheb_forward_launch, stream, dss2::copied(ap, "dss2_cheb_forward"));
}

extern "C" int dss2_cheb_backward(const dss2_cheb_args* ap, void* stream) {
  return dss2::entry(dss2_cheb_backward_launch, stream, dss2::copied(ap, "dss2_cheb_backward"));
}

extern "C" int dss2_cheb_edge_forward(const dss2_cheb_edge_args* ap, void* stream) {
  return dss2::entry(dss2_cheb_edge_forward_launch, stream, dss2::copied(ap, "dss2_cheb_edge_forward"));
}

extern "C" int dss2_cheb_edge_backward(const dss2_cheb_edge_args* ap, void* stream) {
  return dss2::entry(dss2_cheb_edge_backward_launch, stream, dss2::copied(ap, "dss2_cheb_edge_backward"));
}
