// GATv2 (PyG GATv2Conv, heads = 1) and the GAT_DSSE model on gfx950: forward and backward.
//
// Lane mapping, the head Linears and the nonlinearity: dss2_lanegroup.hpp.  The weights of the one or two layers a launch touches
// are staged in LDS.
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

__device__ void stage_conv(ConvSm& s, const dss2_gat_conv& p, int ed) {
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

template <int G>
__device__ __forceinline__ float gsum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
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
template <int G>
__global__ __launch_bounds__(NT) void gat_fwd_kernel(const dss2_gat_args a) {
  __shared__ ConvSm cs;
  __shared__ HeadSm hs;
  if (a.has_lo) stage_conv(cs, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const int ed = a.g.ed, loops = a.g.add_self_loops;
  const float slope = a.g.slope;
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
        const float l = gsum<G>(at * (z > 0.f ? z : slope * z));
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
      y = act(acc / (s + 1e-16f) + cs.bias[c], a.g.nonlin);
      if (c < p.cout) p.y[i * p.cout + c] = y;
      if (c == 0) { p.m[i] = m; p.s[i] = s; }
    } else if (a.has_head) {
      y = c < a.head.c ? a.head.hin[i * a.head.ldhin + c] : 0.f;
    }
    if (a.has_head) head_forward<G>(hs, a.head, i, c, y);
  }
}

// ---- backward: [head backward] or [source pass of layer `up`], then [target pass of layer `lo`] ------------------------------
template <int G>
__global__ __launch_bounds__(NT) void gat_bwd_kernel(const dss2_gat_args a) {
  __shared__ ConvSm us, ls;
  __shared__ HeadSm hs;
  __shared__ float red[NT][2 + EDMAX];
  if (a.has_up) stage_conv(us, a.up, a.g.ed);
  if (a.has_lo) stage_conv(ls, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const int ed = a.g.ed, loops = a.g.add_self_loops, nl = a.g.nonlin;
  const float slope = a.g.slope;
  float g_att = 0.f, g_bias = 0.f, g_we[EDMAX];
#pragma unroll
  for (int k = 0; k < EDMAX; ++k) g_we[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float gy = 0.f;   // gradient of the output of layer lo (or of the model input) at channel c
    if (a.has_head) {
      gy = head_backward<G>(hs, a.head, i, c);
    } else if (a.has_up) {
      const dss2_gat_conv& p = a.up;
      float dxl = (loops && c < p.cout) ? p.dself[i * p.cout + c] : 0.f;
      const int r0 = a.g.rowptrT[i], r1 = a.g.rowptrT[i + 1];
      for (int q = r0; q < r1; ++q) {
        if (loops && a.g.colT[q] == i) continue;
        const int64_t e = a.g.entT[q] & 0x7fffffff;
        dxl += c < p.cout ? p.dedge[e * p.cout + c] : 0.f;
      }
      const float dxr = c < p.cout ? p.dxr[i * p.cout + c] : 0.f;
      if (c < p.cout) p.dxl[i * p.cout + c] = dxl;
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const float gl = __shfl(dxl, k, G), gr = __shfl(dxr, k, G);
        gy = fmaf(us.Wl[k][c], gl, fmaf(us.Wr[k][c], gr, gy));
      }
    } else {
      gy = c < a.lo.cout ? a.gy[i * a.ldgy + c] : 0.f;
    }
    if (!a.has_lo) {
      if (a.dh && c < a.dh_cols) a.dh[i * a.dh_cols + c] = gy;
      continue;
    }
    // target pass of layer lo for node i
    const dss2_gat_conv& p = a.lo;
    const bool on = c < p.cout;
    const float go = on ? gy * (nl ? act_grad(p.y[i * p.cout + c], nl) : 1.f) : 0.f;
    g_bias += go;
    const float* hi = p.h + i * p.ldh;
    const float xr = proj(ls.Wr, ls.br[c], c, hi, p.cin), at = ls.att[c];
    const float m = p.m[i], inv = 1.f / (p.s[i] + 1e-16f);
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
      const float al = expf(gsum<G>(at * (z > 0.f ? z : slope * z)) - m) * inv;
      T = fmaf(al, gsum<G>(go * xl), T);
    }
    const float ee_self = cnt ? eesum / (float)cnt : 0.f;
    float dxr = 0.f, dz_share = 0.f;
    if (loops) {   // the self loop: its share of d W_e is spread over the edges its attribute is the mean of
      const float xl = proj(ls.Wl, ls.bl[c], c, hi, p.cin);
      const float z = xr + xl + ee_self, lr = z > 0.f ? z : slope * z;
      const float al = expf(gsum<G>(at * lr) - m) * inv;
      const float da = gsum<G>(go * xl);
      T = fmaf(al, da, T);
      // T is complete only now: the self loop's own dl needs it
      const float dl = al * (da - T);
      const float dz = dl * at * (z > 0.f ? 1.f : slope);
      g_att = fmaf(dl, lr, g_att);
      dxr += dz;
      if (on) p.dself[i * p.cout + c] = fmaf(al, go, dz);
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
      const float al = expf(gsum<G>(at * lr) - m) * inv;
      const float dl = al * (gsum<G>(go * xl) - T);
      const float dz = dl * at * (z > 0.f ? 1.f : slope);
      g_att = fmaf(dl, lr, g_att);
      dxr += dz;
      if (on) p.dedge[e * p.cout + c] = fmaf(al, go, dz);
      const float dw = dz + dz_share;
#pragma unroll
      for (int k = 0; k < EDMAX; ++k)
        if (k < ed) g_we[k] = fmaf(dw, er[k], g_we[k]);
    }
    if (on) p.dxr[i * p.cout + c] = dxr;
  }
  if (!a.has_lo) return;
  // this workgroup's partials of d att, d bias, d W_e -> its slab row (fixed order over the lane groups)
  red[threadIdx.x][0] = g_att;
  red[threadIdx.x][1] = g_bias;
#pragma unroll
  for (int k = 0; k < EDMAX; ++k) red[threadIdx.x][2 + k] = g_we[k];
  __syncthreads();
  const dss2_gat_conv& p = a.lo;
  const int cols = p.cout * (2 + ed);
  float* row = a.g.slab + (int64_t)blockIdx.x * a.g.slab_len + p.slab_off;
  for (int t = threadIdx.x; t < cols; t += NT) {
    int ch, k;
    float* dst;
    if (t < 2 * p.cout) { k = t / p.cout; ch = t % p.cout; dst = row + t; }
    else { const int u = t - 2 * p.cout; ch = u / ed; k = 2 + u % ed; dst = row + 4 * p.cout + 2 * p.cout * p.cin + u; }
    *dst = group_sum<G>(red, ch, k);
  }
}

int check_args(const dss2_gat_args& a, bool forward, const char* what) {
  if (int rc = check_lanegroup_args(a, what)) return rc;
  const dss2_gat_conv* cv[2] = {a.has_up ? &a.up : nullptr, a.has_lo ? &a.lo : nullptr};
  for (const dss2_gat_conv* p : cv)
    if (p && (p->cin < 1 || p->cout < 1 || p->cin > a.group || p->cout > a.group)) {
      set_error("%s: channels %d -> %d exceed the lane group %d (limit %d)", what, p->cin, p->cout, a.group, GMAX); return 2;
    }
  return check_pass_args(a, forward, what);
}

}  // namespace

static int dss2_gat_forward_launch(const dss2_gat_args* ap, void* stream) {
  if (int rc = check_args(*ap, true, "dss2_gat_forward")) return rc;
  return launch_group(gat_fwd_kernel<8>, gat_fwd_kernel<16>, gat_fwd_kernel<32>, *ap, stream, "dss2_gat_forward");
}

static int dss2_gat_backward_launch(const dss2_gat_args* ap, void* stream) {
  if (int rc = check_args(*ap, false, "dss2_gat_backward")) return rc;
  return launch_group(gat_bwd_kernel<8>, gat_bwd_kernel<16>, gat_bwd_kernel<32>, *ap, stream, "dss2_gat_backward");
}

extern "C" int dss2_gat_forward(const dss2_gat_args* ap, void* stream) {
  return run_entry(dss2_gat_forward_launch, ap, stream, "dss2_gat_forward");
}

extern "C" int dss2_gat_backward(const dss2_gat_args* ap, void* stream) {
  return run_entry(dss2_gat_backward_launch, ap, stream, "dss2_gat_backward");
}
