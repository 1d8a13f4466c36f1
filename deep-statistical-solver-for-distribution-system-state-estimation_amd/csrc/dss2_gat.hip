// GATv2 (PyG GATv2Conv, one or several heads) and the GAT_DSSE model on gfx950: forward and backward.
//
// Lane mapping, the head Linears and the nonlinearity: dss2_lanegroup.hpp.  The weights of the one or two layers a launch touches
// are staged in LDS.  With H > 1 heads of C channels a lane is (head h, channel c) at h * Cp + c, Cp = C rounded up to a power of
// two and H * Cp <= the lane group; lanes with c >= C are inert.  Everything below holds per head: the logit is the xor butterfly
// over the head's Cp lanes, so the softmax max, sum and alpha live per head in the lanes' own registers, and the saved max / sum are
// [N][H].  concat = 0 takes the mean over the heads (lane shuffles across the H sub-groups) before the bias and the nonlinearity.
// One head runs the kernels instantiated without any of this (MH = false): the arithmetic of a lane-per-channel group.
//
// Per target i (CSR by target of the edge list as given; with add_self_loops the input's self loops are skipped and one self
// loop whose edge term is the MEAN of the non-loop incoming edges' terms -- lin_edge is linear, so that is lin_edge of the mean
// attribute, PyG's fill_value = 'mean' -- is appended):
//     e_j = att . leaky_relu(x_r[i] + x_l[j] + W_e ea_j)         x_l, x_r recomputed from h (C_in FMAs per lane and edge)
//     out_i = sum_j softmax(e)_j x_l[j] + bias                    softmax as PyG: exp(e - max) / (sum + 1e-16), online
// The backward is two node-parallel passes per layer: a per-target pass (softmax backward, d att, d bias, d W_e, d x_r and the
// per-edge d x_l contributions) and a per-source pass over the CSR by source that sums those into d x_l and forms
// d h = W_l^T d x_l + W_r^T d x_r.  The source pass of layer l and the target pass of layer l - 1 run in ONE launch.  The
// outer-product weight gradients (lin_l, lin_r, the head) are one batched dss2_lanegroup_wgrad launch over all layers at the end.
// Every weight-gradient partial goes to the workgroup's slab row; dss2_reduce_slabs_multi sums them in a fixed order: no float
// atomics.
#include "dss2_lanegroup.hpp"

using namespace dss2;

namespace {

struct ConvSm {
  float Wl[GMAX][GMAX + 1], Wr[GMAX][GMAX + 1], We[GMAX][EDMAX + 1];
  float bl[GMAX], br[GMAX], att[GMAX], bias[GMAX];
};

__host__ __device__ inline int heads_of(const dss2_gat_conv& p) { return p.heads > 1 ? p.heads : 1; }
__host__ __device__ inline int pow2_from(int c) {
  int v = 1;
  while (v < c) v <<= 1;
  return v;
}
// head mean instead of concatenation (one head: the same thing, taken as concatenation)
__host__ __device__ inline bool mean_of(const dss2_gat_conv& p) { return p.heads > 1 && !p.concat; }

// Where a lane of the group stands in a conv.  One head (MH = false): lane c is channel c, as ever.  Several heads: lane
// hd * cp + ch is channel ch of head hd (cp = cout rounded up to a power of two), parameter row r = hd * cout + ch of the w = H * cout
// rows; lanes with ch >= cout or hd >= H are inert (on = false; their staged weights are zero).  oc: the output's columns.
struct LaneMap {
  int H, cp, hd, ch, r, w, oc;
  bool on;
};
template <bool MH>
__device__ __forceinline__ LaneMap lane_map(const dss2_gat_conv& p, int lane, int G) {
  LaneMap L;
  if constexpr (MH) {
    L.H = heads_of(p);
    L.cp = pow2_from(p.cout);
    const int lg = __ffs(L.cp) - 1;
    L.hd = lane >> lg;
    L.ch = lane & (L.cp - 1);
    L.on = L.hd < L.H && L.ch < p.cout;
    L.r = L.hd * p.cout + L.ch;
    L.w = L.H * p.cout;
    L.oc = mean_of(p) ? p.cout : L.w;
  } else {
    L.H = 1; L.cp = G; L.hd = 0; L.ch = lane; L.r = lane; L.w = p.cout; L.oc = p.cout;
    L.on = lane < p.cout;
  }
  return L;
}

// Staged by padded lane row: row t of the LDS arrays is the parameter row of lane t (zero for an inert lane), so the kernels index
// LDS by lane whatever the head count.  The bias of a head mean has cout entries and sits in the lanes of head 0.  One head
// (MH = false): lane row = parameter row, the staging without any index arithmetic (at B = 64 the staging is a visible part of these
// latency-bound launches: the head-aware form cost the one-head driver line 3 % of its replayed step).
template <bool MH>
__device__ void stage_conv(ConvSm& s, const dss2_gat_conv& p, int ed) {
  if constexpr (MH) {
    const int H = heads_of(p), cp = pow2_from(p.cout), lg = __ffs(cp) - 1;
    const bool mean = mean_of(p);
    auto prow = [&](int t) {
      const int hd = t >> lg, ch = t & (cp - 1);
      return (hd < H && ch < p.cout) ? hd * p.cout + ch : -1;
    };
    for (int t = threadIdx.x; t < GMAX * GMAX; t += NT) {
      const int r = t / GMAX, k = t % GMAX, pr = prow(r);
      const bool in = pr >= 0 && k < p.cin;
      s.Wl[r][k] = in ? p.Wl[pr * p.cin + k] : 0.f;
      s.Wr[r][k] = in ? p.Wr[pr * p.cin + k] : 0.f;
    }
    for (int t = threadIdx.x; t < GMAX * EDMAX; t += NT) {
      const int r = t / EDMAX, k = t % EDMAX, pr = prow(r);
      s.We[r][k] = (pr >= 0 && k < ed && p.We) ? p.We[pr * ed + k] : 0.f;
    }
    for (int t = threadIdx.x; t < GMAX; t += NT) {
      const int pr = prow(t);
      const bool in = pr >= 0;
      s.bl[t] = (in && p.bl) ? p.bl[pr] : 0.f;
      s.br[t] = (in && p.br) ? p.br[pr] : 0.f;
      s.att[t] = in ? p.att[pr] : 0.f;
      const int pb = mean ? (t < p.cout ? t : -1) : pr;
      s.bias[t] = (pb >= 0 && p.bias) ? p.bias[pb] : 0.f;
    }
  } else {
    for (int t = threadIdx.x; t < GMAX * GMAX; t += NT) {
      const int r = t / GMAX, k = t % GMAX;
      const bool in = r < p.cout && k < p.cin;
      s.Wl[r][k] = in ? p.Wl[r * p.cin + k] : 0.f;
      s.Wr[r][k] = in ? p.Wr[r * p.cin + k] : 0.f;
    }
    for (int t = threadIdx.x; t < GMAX * EDMAX; t += NT) {
      const int r = t / EDMAX, k = t % EDMAX;
      s.We[r][k] = (r < p.cout && k < ed && p.We) ? p.We[r * ed + k] : 0.f;
    }
    for (int t = threadIdx.x; t < GMAX; t += NT) {
      const bool in = t < p.cout;
      s.bl[t] = (in && p.bl) ? p.bl[t] : 0.f;
      s.br[t] = (in && p.br) ? p.br[t] : 0.f;
      s.att[t] = in ? p.att[t] : 0.f;
      s.bias[t] = (in && p.bias) ? p.bias[t] : 0.f;
    }
  }
}

template <int G>
__device__ __forceinline__ float gsum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}
// the same xor butterfly over the cp lanes of the lane's head (cp a power of two, uniform); every lane of a head gets the same bits
template <int G>
__device__ __forceinline__ float hsum(float v, int cp) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1)
    if (o < cp) v += __shfl_xor(v, o, G);
  return v;
}
// the logit-sized sums: over the group (one head) or over the lane's head
template <int G, bool MH>
__device__ __forceinline__ float lsum(float v, int cp) {
  if constexpr (MH) return hsum<G>(v, cp);
  else return gsum<G>(v);
}

// x_l[j][c] (or x_r) of lane c: b[c] + sum_k W[c][k] h[j][k]
__device__ __forceinline__ float proj(const float (*W)[GMAX + 1], float b, int c, const float* hrow, int cin) {
  float v = b;
  for (int k = 0; k < cin; ++k) v = fmaf(W[c][k], hrow[k], v);
  return v;
}
__device__ __forceinline__ float eproj(const ConvSm& s, int c, const float* earow, int ed) {
  float v = 0.f;
  for (int k = 0; k < ed; ++k) v = fmaf(s.We[c][k], earow[k], v);
  return v;
}

// ---- forward: one GATv2 layer (target pass, fused nonlinearity) and / or the two head Linears --------------------------------
// c is the LANE of the group everywhere below: the channel with one head, (head, channel) through LaneMap with several.
template <int G, bool MH>
__global__ __launch_bounds__(NT) void gat_fwd_kernel(const dss2_gat_args a) {
  __shared__ ConvSm cs;
  __shared__ HeadSm hs;
  if (a.has_lo) stage_conv<MH>(cs, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const int ed = a.g.ed, loops = a.g.add_self_loops;
  const float slope = a.g.slope;
  const LaneMap L = lane_map<MH>(a.lo, c, G);
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float y = 0.f;
    if (a.has_lo) {
      const dss2_gat_conv& p = a.lo;
      const float* hi = p.h + i * p.ldh;
      const float xr = proj(cs.Wr, cs.br[c], c, hi, p.cin), at = cs.att[c];
      float m = -INFINITY, s = 0.f, acc = 0.f, eesum = 0.f;
      int cnt = 0;
      const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
      for (int q = r0; q <= r1; ++q) {
        int64_t j;
        float ee;
        if (q < r1) {
          j = a.g.col[q];
          if (loops && j == i) continue;
          ee = ed ? eproj(cs, c, a.g.ea + (int64_t)(a.g.ent[q] & 0x7fffffff) * a.g.ldea, ed) : 0.f;
          eesum += ee;
          ++cnt;
        } else {
          if (!loops) break;
          j = i;
          ee = cnt ? eesum / (float)cnt : 0.f;
        }
        const float xl = proj(cs.Wl, cs.bl[c], c, p.h + j * p.ldh, p.cin);
        const float z = xr + xl + ee;
        const float l = lsum<G, MH>(at * (z > 0.f ? z : slope * z), L.cp);
        if (l > m) {
          const float sc = expf(m - l);
          s = s * sc + 1.f;
          acc = acc * sc + xl;
          m = l;
        } else {
          const float pe = expf(l - m);
          s += pe;
          acc = fmaf(pe, xl, acc);
        }
      }
      if constexpr (MH) {
        const float v = acc / (s + 1e-16f);
        if (mean_of(p)) {      // the mean over the heads in a fixed order, the bias after it; head 0's lanes carry the output
          float t = 0.f;
          for (int hd = 0; hd < L.H; ++hd) t += __shfl(v, hd * L.cp + L.ch, G);
          y = L.hd == 0 ? act(t / (float)L.H + cs.bias[c], a.g.nonlin) : 0.f;
          if (L.hd == 0 && L.ch < p.cout) p.y[i * p.cout + L.ch] = y;
        } else {
          y = act(v + cs.bias[c], a.g.nonlin);
          if (L.on) p.y[i * L.w + L.r] = y;
        }
        if (L.ch == 0 && L.hd < L.H) { p.m[i * L.H + L.hd] = m; p.s[i * L.H + L.hd] = s; }
      } else {
        y = act(acc / (s + 1e-16f) + cs.bias[c], a.g.nonlin);
        if (c < p.cout) p.y[i * p.cout + c] = y;
        if (c == 0) { p.m[i] = m; p.s[i] = s; }
      }
    } else if (a.has_head) {
      y = c < a.head.c ? a.head.hin[i * a.head.ldhin + c] : 0.f;
    }
    if (a.has_head) head_forward<G>(hs, a.head, i, c, y);
  }
}

// ---- backward: [head backward] or [source pass of layer `up`], then [target pass of layer `lo`] ------------------------------
// gy arrives by output COLUMN: lane k holds the gradient of column k of lo's output (from the head, from up's source pass, whose
// lane k is its input channel k, or from a.gy).  With several heads the target pass hands it to the (head, channel) lanes.
template <int G, bool MH>
__global__ __launch_bounds__(NT) void gat_bwd_kernel(const dss2_gat_args a) {
  __shared__ ConvSm us, ls;
  __shared__ HeadSm hs;
  __shared__ float red[NT][2 + EDMAX];
  if (a.has_up) stage_conv<MH>(us, a.up, a.g.ed);
  if (a.has_lo) stage_conv<MH>(ls, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const int ed = a.g.ed, loops = a.g.add_self_loops, nl = a.g.nonlin;
  const float slope = a.g.slope;
  const LaneMap U = lane_map<MH>(a.up, c, G), L = lane_map<MH>(a.lo, c, G);
  float g_att = 0.f, g_bias = 0.f, g_we[EDMAX];      // g_bias by output column, g_att and g_we by lane
#pragma unroll
  for (int k = 0; k < EDMAX; ++k) g_we[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float gy = 0.f;   // gradient of the output of layer lo (or of the model input) at column c
    if (a.has_head) {
      gy = head_backward<G>(hs, a.head, i, c);
    } else if (a.has_up) {
      const dss2_gat_conv& p = a.up;
      float dxl = (loops && U.on) ? p.dself[i * U.w + U.r] : 0.f;
      const int r0 = a.g.rowptrT[i], r1 = a.g.rowptrT[i + 1];
      for (int q = r0; q < r1; ++q) {
        if (loops && a.g.colT[q] == i) continue;
        const int64_t e = a.g.entT[q] & 0x7fffffff;
        dxl += U.on ? p.dedge[e * U.w + U.r] : 0.f;
      }
      const float dxr = U.on ? p.dxr[i * U.w + U.r] : 0.f;
      if (U.on) p.dxl[i * U.w + U.r] = dxl;
#pragma unroll
      for (int k = 0; k < G; ++k) {      // over the lane rows: d h[c] = sum_r W_l[r][c] d x_l[r] + W_r[r][c] d x_r[r]
        const float gl = __shfl(dxl, k, G), gr = __shfl(dxr, k, G);
        gy = fmaf(us.Wl[k][c], gl, fmaf(us.Wr[k][c], gr, gy));
      }
    } else {
      gy = c < L.oc ? a.gy[i * a.ldgy + c] : 0.f;
    }
    if (!a.has_lo) {
      if (a.dh && c < a.dh_cols) a.dh[i * a.dh_cols + c] = gy;
      continue;
    }
    // target pass of layer lo for node i
    const dss2_gat_conv& p = a.lo;
    const bool on = L.on;
    float go, m, inv;
    if constexpr (MH) {
      // the activation's gradient on the output column, d bias per column; then to the lanes: column hd * cout + ch, or with a head
      // mean column ch over H for every head
      const float gc = c < L.oc ? gy * (nl ? act_grad(p.y[i * L.oc + c], nl) : 1.f) : 0.f;
      g_bias += gc;
      go = mean_of(p) ? __shfl(gc, L.ch, G) / (float)L.H : __shfl(gc, on ? L.r : 0, G);
      if (!on) go = 0.f;
      const bool live = L.hd < L.H;      // (the lanes of a head past the last one: alpha = 0)
      m = live ? p.m[i * L.H + L.hd] : 0.f;
      inv = live ? 1.f / (p.s[i * L.H + L.hd] + 1e-16f) : 0.f;
    } else {
      go = on ? gy * (nl ? act_grad(p.y[i * p.cout + c], nl) : 1.f) : 0.f;
      g_bias += go;
      m = p.m[i];
      inv = 1.f / (p.s[i] + 1e-16f);
    }
    const float* hi = p.h + i * p.ldh;
    const float xr = proj(ls.Wr, ls.br[c], c, hi, p.cin), at = ls.att[c];
    const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
    // pass A: sum_f alpha_f dalpha_f (and the self loop's mean edge term)
    float eesum = 0.f, T = 0.f;
    int cnt = 0;
    for (int q = r0; q < r1; ++q) {
      const int64_t j = a.g.col[q];
      if (loops && j == i) continue;
      const float ee = ed ? eproj(ls, c, a.g.ea + (int64_t)(a.g.ent[q] & 0x7fffffff) * a.g.ldea, ed) : 0.f;
      eesum += ee;
      ++cnt;
      const float xl = proj(ls.Wl, ls.bl[c], c, p.h + j * p.ldh, p.cin);
      const float z = xr + xl + ee;
      const float al = expf(lsum<G, MH>(at * (z > 0.f ? z : slope * z), L.cp) - m) * inv;
      T = fmaf(al, lsum<G, MH>(go * xl, L.cp), T);
    }
    const float ee_self = cnt ? eesum / (float)cnt : 0.f;
    float dxr = 0.f, dz_share = 0.f;
    if (loops) {   // the self loop: its share of d W_e is spread over the edges its attribute is the mean of
      const float xl = proj(ls.Wl, ls.bl[c], c, hi, p.cin);
      const float z = xr + xl + ee_self, lr = z > 0.f ? z : slope * z;
      const float al = expf(lsum<G, MH>(at * lr, L.cp) - m) * inv;
      const float da = lsum<G, MH>(go * xl, L.cp);
      T = fmaf(al, da, T);
      // T is complete only now: the self loop's own dl needs it
      const float dl = al * (da - T);
      const float dz = dl * at * (z > 0.f ? 1.f : slope);
      g_att = fmaf(dl, lr, g_att);
      dxr += dz;
      if (on) p.dself[i * L.w + L.r] = fmaf(al, go, dz);
      dz_share = cnt ? dz / (float)cnt : 0.f;
    }
    // pass B: per-edge softmax backward
    for (int q = r0; q < r1; ++q) {
      const int64_t j = a.g.col[q];
      if (loops && j == i) continue;
      const int64_t e = a.g.ent[q] & 0x7fffffff;
      const float* er = a.g.ea + e * a.g.ldea;
      const float ee = ed ? eproj(ls, c, er, ed) : 0.f;
      const float xl = proj(ls.Wl, ls.bl[c], c, p.h + j * p.ldh, p.cin);
      const float z = xr + xl + ee, lr = z > 0.f ? z : slope * z;
      const float al = expf(lsum<G, MH>(at * lr, L.cp) - m) * inv;
      const float dl = al * (lsum<G, MH>(go * xl, L.cp) - T);
      const float dz = dl * at * (z > 0.f ? 1.f : slope);
      g_att = fmaf(dl, lr, g_att);
      dxr += dz;
      if (on) p.dedge[e * L.w + L.r] = fmaf(al, go, dz);
      const float dw = dz + dz_share;
#pragma unroll
      for (int k = 0; k < EDMAX; ++k)
        if (k < ed) g_we[k] = fmaf(dw, er[k], g_we[k]);
    }
    if (on) p.dxr[i * L.w + L.r] = dxr;
  }
  if (!a.has_lo) return;
  // this workgroup's partials of d att, d bias, d W_e -> its slab row (fixed order over the lane groups)
  red[threadIdx.x][0] = g_att;
  red[threadIdx.x][1] = g_bias;
#pragma unroll
  for (int k = 0; k < EDMAX; ++k) red[threadIdx.x][2 + k] = g_we[k];
  __syncthreads();
  const dss2_gat_conv& p = a.lo;
  float* row = a.g.slab + (int64_t)blockIdx.x * a.g.slab_len + p.slab_off;
  if constexpr (MH) {
    // columns att[w], bias[oc], (lin_l, lin_r: dss2_lanegroup_wgrad), W_e[w][ed]; parameter row r sits in lane (r / cout) * cp + r % cout
    const int w = L.w, oc = L.oc, cols = w + oc + w * ed;
    for (int t = threadIdx.x; t < cols; t += NT) {
      int ln, k;
      float* dst;
      if (t < w) { k = 0; ln = (t / p.cout) * L.cp + t % p.cout; dst = row + t; }
      else if (t < w + oc) { k = 1; ln = t - w; dst = row + t; }
      else { const int u = t - w - oc, r = u / ed; k = 2 + u % ed; ln = (r / p.cout) * L.cp + r % p.cout; dst = row + 3 * w + oc + 2 * w * p.cin + u; }
      *dst = group_sum<G>(red, ln, k);
    }
  } else {
    const int cols = p.cout * (2 + ed);
    for (int t = threadIdx.x; t < cols; t += NT) {
      int ch, k;
      float* dst;
      if (t < 2 * p.cout) { k = t / p.cout; ch = t % p.cout; dst = row + t; }
      else { const int u = t - 2 * p.cout; ch = u / ed; k = 2 + u % ed; dst = row + 4 * p.cout + 2 * p.cout * p.cin + u; }
      *dst = group_sum<G>(red, ch, k);
    }
  }
}

// several heads anywhere in the launch: the head-aware kernels
bool multi_head(const dss2_gat_args& a) { return (a.has_up && a.up.heads > 1) || (a.has_lo && a.lo.heads > 1); }

int check_args(const dss2_gat_args& a, bool forward, const char* what) {
  if (int rc = check_lanegroup_args(a, what)) return rc;
  const dss2_gat_conv* cv[2] = {a.has_up ? &a.up : nullptr, a.has_lo ? &a.lo : nullptr};
  const bool multi = multi_head(a);
  for (const dss2_gat_conv* p : cv) {
    if (!p) continue;
    if (p->cin < 1 || p->cout < 1 || p->cin > a.group || p->cout > a.group) {
      set_error("%s: channels %d -> %d exceed the lane group %d (limit %d)", what, p->cin, p->cout, a.group, GMAX); return 2;
    }
    if (p->heads < 0) { set_error("%s: heads %d", what, p->heads); return 2; }
    if (multi && heads_of(*p) * pow2_from(p->cout) > a.group) {
      set_error("%s: %d heads of %d channels take %d lanes, the lane group has %d (limit %d)", what, heads_of(*p), p->cout,
                heads_of(*p) * pow2_from(p->cout), a.group, GMAX);
      return 2;
    }
  }
  if (a.has_head && a.has_lo && a.lo.heads > 1 && a.lo.concat) {
    set_error("%s: the head Linears after %d concatenated heads (the head reads a head mean: concat = 0)", what, a.lo.heads); return 2;
  }
  return check_pass_args(a, forward, what);
}

}  // namespace

static int dss2_gat_forward_launch(const dss2_gat_args* ap, void* stream) {
  if (int rc = check_args(*ap, true, "dss2_gat_forward")) return rc;
  if (multi_head(*ap))
    return launch_group(gat_fwd_kernel<8, true>, gat_fwd_kernel<16, true>, gat_fwd_kernel<32, true>, *ap, stream, "dss2_gat_forward");
  return launch_group(gat_fwd_kernel<8, false>, gat_fwd_kernel<16, false>, gat_fwd_kernel<32, false>, *ap, stream, "dss2_gat_forward");
}

static int dss2_gat_backward_launch(const dss2_gat_args* ap, void* stream) {
  if (int rc = check_args(*ap, false, "dss2_gat_backward")) return rc;
  if (multi_head(*ap))
    return launch_group(gat_bwd_kernel<8, true>, gat_bwd_kernel<16, true>, gat_bwd_kernel<32, true>, *ap, stream, "dss2_gat_backward");
  return launch_group(gat_bwd_kernel<8, false>, gat_bwd_kernel<16, false>, gat_bwd_kernel<32, false>, *ap, stream, "dss2_gat_backward");
}

extern "C" int dss2_gat_forward(const dss2_gat_args* ap, void* stream) {
  return dss2::entry(dss2_gat_forward_launch, stream, dss2::copied(ap, "dss2_gat_forward"));
}

extern "C" int dss2_gat_backward(const dss2_gat_args* ap, void* stream) {
  return dss2::entry(dss2_gat_backward_launch, stream, dss2::copied(ap, "dss2_gat_backward"));
}
