// GINE (PyG GINEConv with nn = one Linear) and the GINE_DSSE model on gfx950: forward and backward.
//
// Lane mapping, the head Linears and the nonlinearity: dss2_lanegroup.hpp.  The head's weight gradient is dss2_lanegroup_wgrad.
//
// One layer, j = edge_index[0] the source and i = edge_index[1] the target, edges as given (no doubling, no self loops added):
//     m_e   = h_j + W_e ea_e + b_e                 (without lin: h_j + ea_e)
//     z_i   = sum_{e: j->i} relu(m_e) + (1 + eps) h_i
//     y_i   = phi(W_nn z_i + b_nn)                  eps read from device memory, so replays follow a trained eps
// Backward, per conv l, with dh the gradient of its output:
//     dv = dh * phi'(y)     dz = W_nn^T dv           (node-local: the "local step")
//     dh_in[j] = (1 + eps) dz_j + sum_{e: j->i} [relu open at m_e] dz_i      (the "source pass", CSR by source)
// The source pass of conv l recomputes m_e with the forward's own function, so every ReLU gate is the forward's bit for bit; it
// also forms d W_e / d b_e (each edge has one source, so each edge is visited once).  The local step of conv l - 1 (or dx) runs
// in the same launch.  The local step forms d eps and the shared nn's partial d W_nn = dv z^T, d b_nn = dv; those go to the
// workgroup's row of a second slab, [n_slabs][n_convs][nn_len], which dss2_reduce_slabs_multi sums as n_slabs * n_convs rows in
// a fixed order.  No float atomics.
#include "dss2_lanegroup.hpp"

using namespace dss2;

namespace {

struct ConvSm {
  float Wn[GMAX][GMAX + 1], We[GMAX][EDMAX + 1];
  float bn[GMAX], be[GMAX];
};

__device__ void stage_conv(ConvSm& s, const dss2_gine_conv& p, int ed) {
  for (int t = threadIdx.x; t < GMAX * GMAX; t += NT) {
    const int r = t / GMAX, k = t % GMAX;
    s.Wn[r][k] = (r < p.cout && k < p.cin) ? p.Wn[r * p.cin + k] : 0.f;
  }
  for (int t = threadIdx.x; t < GMAX * EDMAX; t += NT) {
    const int r = t / EDMAX, k = t % EDMAX;
    s.We[r][k] = (r < p.cin && k < ed && p.We) ? p.We[r * ed + k] : 0.f;
  }
  for (int t = threadIdx.x; t < GMAX; t += NT) {
    s.bn[t] = t < p.cout ? p.bn[t] : 0.f;
    s.be[t] = (t < p.cin && p.be) ? p.be[t] : 0.f;
  }
}

// the message m_e of lane c before the ReLU.  The forward and the source pass both call this, so the gates agree bit for bit.
__device__ __forceinline__ float message(const ConvSm& s, const dss2_gine_graph& g, int c, float hj, int64_t e, int cin) {
  const float* er = g.ea + e * g.ldea;
  float v;
  if (g.ed) {
    v = s.be[c];
    for (int k = 0; k < g.ed; ++k) v = fmaf(s.We[c][k], er[k], v);
  } else {
    v = c < cin ? er[c] : 0.f;
  }
  return hj + v;
}

// ---- forward: one GINE layer (nonlinearity fused) and / or the two head Linears -------------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void gine_fwd_kernel(const dss2_gine_args a) {
  __shared__ ConvSm cs;
  __shared__ HeadSm hs;
  if (a.has_lo) stage_conv(cs, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const float ope = a.has_lo ? 1.f + a.lo.eps[0] : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float y = 0.f;
    if (a.has_lo) {
      const dss2_gine_conv& p = a.lo;
      const bool in = c < p.cin;
      float agg = 0.f;
      const int r0 = a.g.rowptr[i], r1 = a.g.rowptr[i + 1];
      for (int q = r0; q < r1; ++q) {
        const int64_t j = a.g.col[q], e = a.g.ent[q] & 0x7fffffff;
        const float hj = in ? p.h[j * p.ldh + c] : 0.f;
        agg += relu_nan(message(cs, a.g, c, hj, e, p.cin));
      }
      const float hi = in ? p.h[i * p.ldh + c] : 0.f;
      const float z = in ? agg + ope * hi : 0.f;
      if (in) p.z[i * p.cin + c] = z;
      float v = cs.bn[c];
#pragma unroll
      for (int k = 0; k < G; ++k) v = fmaf(cs.Wn[c][k], __shfl(z, k, G), v);
      y = act(v, a.g.nonlin);
      if (c < p.cout) p.y[i * p.cout + c] = y;
    } else if (a.has_head) {
      y = c < a.head.c ? a.head.hin[i * a.head.ldhin + c] : 0.f;
    }
    if (a.has_head) head_forward<G>(hs, a.head, i, c, y);
  }
}

// ---- backward: [head backward | source pass of conv `up` | gy], then [local step of conv `lo`] or the input gradient ---------------
template <int G>
__global__ __launch_bounds__(NT) void gine_bwd_kernel(const dss2_gine_args a) {
  __shared__ ConvSm us, ls;
  __shared__ HeadSm hs;
  __shared__ float red[NT][GMAX + 1];
  if (a.has_up) stage_conv(us, a.up, a.g.ed);
  if (a.has_lo) stage_conv(ls, a.lo, a.g.ed);
  if (a.has_head) stage_head(hs, a.head);
  __syncthreads();
  const int c = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t n = a.g.n_nodes, stride = (int64_t)gridDim.x * (NT / G);
  const int ed = a.g.ed, nl = a.g.nonlin;
  const float ope_up = a.has_up ? 1.f + a.up.eps[0] : 0.f;
  float g_we[EDMAX], g_be = 0.f;     // up: d W_e row c, d b_e[c]
  float g_wn[G], g_bn = 0.f, g_eps = 0.f;   // lo: d W_nn row c, d b_nn[c], lane c's share of d eps
#pragma unroll
  for (int k = 0; k < EDMAX; ++k) g_we[k] = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) g_wn[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * (NT / G) + grp; i < n; i += stride) {
    float gy = 0.f;   // gradient of lo's output (or of the model input) at channel c
    if (a.has_head) {
      gy = head_backward<G>(hs, a.head, i, c);
    } else if (a.has_up) {
      const dss2_gine_conv& p = a.up;
      const bool in = c < p.cin;
      const float hj = in ? p.h[i * p.ldh + c] : 0.f;
      const float dzj = in ? p.dz[i * p.cin + c] : 0.f;
      float acc = 0.f;
      const int r0 = a.g.rowptrT[i], r1 = a.g.rowptrT[i + 1];
      for (int q = r0; q < r1; ++q) {
        const int64_t t = a.g.colT[q], e = a.g.entT[q] & 0x7fffffff;
        const float m = message(us, a.g, c, hj, e, p.cin);
        const float d = (in && relu_open(m)) ? p.dz[t * p.cin + c] : 0.f;
        acc += d;
        if (ed) {
          const float* er = a.g.ea + e * a.g.ldea;
          g_be += d;
#pragma unroll
          for (int k = 0; k < EDMAX; ++k)
            if (k < ed) g_we[k] = fmaf(d, er[k], g_we[k]);
        }
      }
      gy = fmaf(ope_up, dzj, acc);
    } else {
      gy = c < a.lo.cout ? a.gy[i * a.ldgy + c] : 0.f;
    }
    if (!a.has_lo) {
      if (a.dh && c < a.dh_cols) a.dh[i * a.dh_cols + c] = gy;
      continue;
    }
    // local step of conv lo for node i
    const dss2_gine_conv& p = a.lo;
    const float dv = c < p.cout ? gy * act_grad(p.y[i * p.cout + c], nl) : 0.f;
    const float zc = c < p.cin ? p.z[i * p.cin + c] : 0.f;
    float dz = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      dz = fmaf(ls.Wn[k][c], __shfl(dv, k, G), dz);
      g_wn[k] = fmaf(dv, __shfl(zc, k, G), g_wn[k]);
    }
    g_bn += dv;
    if (c < p.cin) {
      p.dz[i * p.cin + c] = dz;
      g_eps = fmaf(dz, p.h[i * p.ldh + c], g_eps);
    }
  }
  // this workgroup's partials -> its slab rows (fixed order over the lane groups)
  float* row = a.g.slab + (int64_t)blockIdx.x * a.g.slab_len;
  if (a.has_up && ed) {
    const dss2_gine_conv& p = a.up;
#pragma unroll
    for (int k = 0; k < EDMAX; ++k) red[threadIdx.x][k] = g_we[k];
    red[threadIdx.x][EDMAX] = g_be;
    __syncthreads();
    // columns at slab_off: eps[1], lin.weight[cin][ed], lin.bias[cin]; this launch owns the lin part
    for (int t = threadIdx.x; t < p.cin * (ed + 1); t += NT) {
      const int ch = t < p.cin * ed ? t / ed : t - p.cin * ed, k = t < p.cin * ed ? t % ed : EDMAX;
      row[p.slab_off + 1 + t] = group_sum<G>(red, ch, k);
    }
    __syncthreads();
  }
  if (a.has_lo) {
    const dss2_gine_conv& p = a.lo;
#pragma unroll
    for (int k = 0; k < G; ++k) red[threadIdx.x][k] = g_wn[k];
    red[threadIdx.x][G] = g_bn;
    __syncthreads();
    float* nrow = a.g.nslab + (int64_t)blockIdx.x * a.g.nslab_len + p.nn_off;
    for (int t = threadIdx.x; t < p.cout * (p.cin + 1); t += NT) {
      const int ch = t < p.cout * p.cin ? t / p.cin : t - p.cout * p.cin, k = t < p.cout * p.cin ? t % p.cin : G;
      nrow[t] = group_sum<G>(red, ch, k);
    }
    __syncthreads();
    red[threadIdx.x][0] = g_eps;
    __syncthreads();
    if (threadIdx.x == 0) {
      float v = 0.f;
      for (int g = 0; g < NT / G; ++g)
        for (int ch = 0; ch < G; ++ch) v += red[g * G + ch][0];
      row[p.slab_off] = v;
    }
  }
}

int check_conv(const dss2_gine_conv& p, const dss2_gine_args& a, const char* what) {
  if (p.cin < 1 || p.cout < 1 || p.cin > a.group || p.cout > a.group) {
    set_error("%s: channels %d -> %d exceed the lane group %d (limit %d)", what, p.cin, p.cout, a.group, GMAX); return 2;
  }
  if (!p.eps || !p.Wn || !p.bn || !p.h || (a.g.ed && (!p.We || !p.be))) { set_error("%s: a conv pointer is missing", what); return 2; }
  return 0;
}

int check_args(const dss2_gine_args& a, bool forward, const char* what) {
  if (int rc = check_lanegroup_args(a, what)) return rc;
  if (a.has_up)
    if (int rc = check_conv(a.up, a, what)) return rc;
  if (a.has_lo)
    if (int rc = check_conv(a.lo, a, what)) return rc;
  return check_pass_args(a, forward, what);
}

}  // namespace

static int dss2_gine_forward_launch(const dss2_gine_args* ap, void* stream) {
  if (int rc = check_args(*ap, true, "dss2_gine_forward")) return rc;
  return launch_group(gine_fwd_kernel<8>, gine_fwd_kernel<16>, gine_fwd_kernel<32>, *ap, stream, "dss2_gine_forward");
}

static int dss2_gine_backward_launch(const dss2_gine_args* ap, void* stream) {
  const dss2_gine_args& a = *ap;
  if (int rc = check_args(a, false, "dss2_gine_backward")) return rc;
  if (a.has_lo && !a.g.nslab) { set_error("dss2_gine_backward: no slab"); return 2; }
  return launch_group(gine_bwd_kernel<8>, gine_bwd_kernel<16>, gine_bwd_kernel<32>, a, stream, "dss2_gine_backward");
}

extern "C" int dss2_gine_forward(const dss2_gine_args* ap, void* stream) {
  return dss2::entry(dss2_gine_forward_launch, stream, dss2::copied(ap, "dss2_gine_forward"));
}

extern "C" int dss2_gine_backward(const dss2_gine_args* ap, void* stream) {
  return dss2::entry(dss2_gine_backward_launch, stream, dss2::copied(ap, "dss2_gine_backward"));
}
