// The lane-group core shared by the GAT (dss2_gat.hip), GINE (dss2_gine.hip) and gnn_dsse (dss2_gnn.hip) kernels.
//
// Lane mapping: one lane group of G (8 / 16 / 32) lanes per node, lane c owns channel c; a 256-thread workgroup holds 256 / G
// nodes at a time and walks the nodes with a grid stride (the grid is the slab count, so every workgroup writes exactly one slab
// row).  fp32 VALU throughout: at C = 8 there is no matrix work worth the MFMA.  Weights are staged in LDS with rows padded to
// 33 / 17 floats (lane c reading row c hits bank c).
//
// Here: the two head Linears (LDS staging, the fused forward and backward of one node), the model nonlinearity and its gradient,
// the fixed-order lane-group sum of a workgroup's partials, the argument checks the models share, the group dispatch and the
// body of an extern "C" entry point.  The head's outer-product weight gradient is dss2_lanegroup_wgrad (dss2_lanegroup.hip).
// Nothing here knows which model calls it; the conv staging, the message, the softmax and the slab columns stay in the model files.
#pragma once

#include "dss2_common.hpp"

#include <math.h>

namespace dss2 {

constexpr int GMAX = 32, EDMAX = 16, DMAX = 32, NT = 256;

struct HeadSm {
  float W1[DMAX][GMAX + 1], W2[DMAX][DMAX + 1], b1[DMAX], b2[DMAX];
};

__device__ inline void stage_head(HeadSm& s, const dss2_lanegroup_head& p) {
  for (int t = threadIdx.x; t < DMAX * GMAX; t += NT) {
    const int d = t / GMAX, c = t % GMAX;
    s.W1[d][c] = (d < p.dense && c < p.c) ? p.W1[d * p.c + c] : 0.f;
  }
  for (int t = threadIdx.x; t < DMAX * DMAX; t += NT) {
    const int o = t / DMAX, d = t % DMAX;
    s.W2[o][d] = (o < p.nout && d < p.dense) ? p.W2[o * p.dense + d] : 0.f;
  }
  for (int t = threadIdx.x; t < DMAX; t += NT) {
    s.b1[t] = t < p.dense ? p.b1[t] : 0.f;
    s.b2[t] = t < p.nout ? p.b2[t] : 0.f;
  }
}

// the model's nonlinearity: 0 none (a standalone conv), 1 LeakyReLU(0.01), 2 ReLU, 3 Tanh
__device__ __forceinline__ float act(float v, int mode) {
  if (mode == 1) return v > 0.f ? v : 0.01f * v;
  if (mode == 2) return relu_nan(v);
  if (mode == 3) return tanhf(v);
  return v;
}
// its derivative from the saved OUTPUT, with torch's gates: leaky_relu_backward (input > 0; y > 0 <=> v > 0, NaN takes the
// slope), threshold_backward on the ReLU's result (y <= 0 closes, NaN passes), tanh_backward (1 - y^2)
__device__ __forceinline__ float act_grad(float y, int mode) {
  if (mode == 1) return y > 0.f ? 1.f : 0.01f;
  if (mode == 2) return relu_open(y) ? 1.f : 0.f;
  if (mode == 3) return 1.f - y * y;
  return 1.f;
}

// head forward of node i: y is lane c's channel of the head input; writes z1 = W1 y + b1 and out = W2 z1 + b2
template <int G>
__device__ __forceinline__ void head_forward(const HeadSm& hs, const dss2_lanegroup_head& hp, int64_t i, int c, float y) {
  float z1[DMAX / G];
#pragma unroll
  for (int u = 0; u < DMAX / G; ++u) z1[u] = hs.b1[u * G + c];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const float yk = __shfl(y, k, G);
#pragma unroll
    for (int u = 0; u < DMAX / G; ++u) z1[u] = fmaf(hs.W1[u * G + c][k], yk, z1[u]);
  }
  float o[DMAX / G];
#pragma unroll
  for (int u = 0; u < DMAX / G; ++u) {
    o[u] = hs.b2[u * G + c];
    if (u * G + c < hp.dense) hp.z1[i * hp.dense + u * G + c] = z1[u];
  }
#pragma unroll
  for (int v = 0; v < DMAX / G; ++v)
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const float zd = __shfl(z1[v], k, G);
#pragma unroll
      for (int u = 0; u < DMAX / G; ++u) o[u] = fmaf(hs.W2[u * G + c][v * G + k], zd, o[u]);
    }
#pragma unroll
  for (int u = 0; u < DMAX / G; ++u)
    if (u * G + c < hp.nout) hp.out[i * hp.ldo + u * G + c] = o[u];
}

// head backward of node i: writes dz1 = W2^T gout and returns lane c's channel of the head input's gradient, W1^T dz1
template <int G>
__device__ __forceinline__ float head_backward(const HeadSm& hs, const dss2_lanegroup_head& hp, int64_t i, int c) {
  float dz[DMAX / G], gy = 0.f;
#pragma unroll
  for (int u = 0; u < DMAX / G; ++u) dz[u] = 0.f;
  for (int o = 0; o < hp.nout; ++o) {
    const float go = hp.gout[i * hp.ldgo + o];
#pragma unroll
    for (int u = 0; u < DMAX / G; ++u) dz[u] = fmaf(hs.W2[o][u * G + c], go, dz[u]);
  }
#pragma unroll
  for (int u = 0; u < DMAX / G; ++u) {
    if (u * G + c < hp.dense) hp.dz1[i * hp.dense + u * G + c] = dz[u];
#pragma unroll
    for (int k = 0; k < G; ++k) gy = fmaf(hs.W1[u * G + k][c], __shfl(dz[u], k, G), gy);
  }
  return gy;
}

// lane-group fixed-order sum of red[g * G + ch][k] over the NT / G groups (rows of any width W)
template <int G, int W>
__device__ __forceinline__ float group_sum(const float (*red)[W], int ch, int k) {
  float v = 0.f;
  for (int g = 0; g < NT / G; ++g) v += red[g * G + ch][k];
  return v;
}

// the checks of a lane-group model's args (dss2_gat_args / _gine_args / _gnn_args) that do not depend on the model: graph sizes, edge
// width, lane group, head widths, and no head next to a source pass.  The model checks its convs.
template <class Args>
inline int check_lanegroup_args(const Args& a, const char* what) {
  if (a.g.n_nodes <= 0 || a.g.n_slabs <= 0) { set_error("%s: empty batch / no slabs", what); return 2; }
  if (a.g.ed < 0 || a.g.ed > EDMAX) { set_error("%s: edge_dim %d outside [0, %d]", what, a.g.ed, EDMAX); return 2; }
  if (a.group != 8 && a.group != 16 && a.group != 32) { set_error("%s: lane group %d (8, 16 or 32)", what, a.group); return 2; }
  if (a.has_head && (a.head.c < 1 || a.head.c > a.group || a.head.dense < 1 || a.head.dense > DMAX || a.head.nout < 1 || a.head.nout > DMAX)) {
    set_error("%s: head %d -> %d -> %d outside the limits (C <= lane group, dense, out <= %d)", what, a.head.c, a.head.dense, a.head.nout, DMAX);
    return 2;
  }
  if (a.has_head && a.has_up) { set_error("%s: head and source pass in one launch", what); return 2; }
  return 0;
}

// what a forward (something to run, no source pass) and a backward launch (an output gradient, a slab) need in every model;
// what is the entry point's name
template <class Args>
inline int check_pass_args(const Args& a, bool forward, const char* what) {
  if (forward && !a.has_lo && !a.has_head) { set_error("%s: nothing to do", what); return 2; }
  if (forward && a.has_up) { set_error("%s: no source pass in the forward", what); return 2; }
  if (!forward && !a.has_head && !a.has_up && (!a.has_lo || !a.gy)) { set_error("%s: no output gradient", what); return 2; }
  if (!forward && !a.g.slab) { set_error("%s: no slab", what); return 2; }
  return 0;
}

// launches the model's kernel for G = a.group (8, 16 or 32, checked) on a.g.n_slabs workgroups of NT threads
template <class Args>
inline int launch_group(void (*k8)(Args), void (*k16)(Args), void (*k32)(Args), const Args& a, void* stream, const char* what) {
  void (*k)(Args) = a.group == 8 ? k8 : (a.group == 16 ? k16 : k32);
  hipLaunchKernelGGL(k, dim3((unsigned)a.g.n_slabs), dim3(NT), 0, as_stream(stream), a);
  return check_launch(what);
}

}  // namespace dss2
