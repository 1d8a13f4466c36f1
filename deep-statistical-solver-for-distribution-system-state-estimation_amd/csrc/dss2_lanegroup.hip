// Outer-product weight gradients of the lane-group models (GAT: lin_l, lin_r and the head; GINE: the head), one batched launch.
// Node chunk s of ceil(N / n_slabs) rows goes to slab row s; dss2_reduce_slabs_multi sums the rows in a fixed order.
#include "dss2_lanegroup.hpp"

using namespace dss2;

namespace {

// slab[s][col + o * xw + k] = sum_{n in chunk s} Gm[n][o] X[n][k], then the column sums of Gm
__global__ __launch_bounds__(NT) void lanegroup_wgrad_kernel(const dss2_lanegroup_wgrad_args a) {
  const dss2_lanegroup_wgrad_job& jb = a.jobs[blockIdx.y];
  const int64_t chunk = (a.n_nodes + gridDim.x - 1) / gridDim.x;
  const int64_t n0 = (int64_t)blockIdx.x * chunk, n1 = n0 + chunk < a.n_nodes ? n0 + chunk : a.n_nodes;
  const int nw = jb.gw * jb.xw;
  float* row = a.slab + (int64_t)blockIdx.x * a.slab_len + jb.col;
  for (int t = threadIdx.x; t < nw + jb.gw; t += NT) {
    float v = 0.f;
    if (t < nw) {
      const int o = t / jb.xw, k = t % jb.xw;
      for (int64_t n = n0; n < n1; ++n) v = fmaf(jb.G[n * jb.ldg + o], jb.X[n * jb.ldx + k], v);
    } else {
      const int o = t - nw;
      for (int64_t n = n0; n < n1; ++n) v += jb.G[n * jb.ldg + o];
    }
    row[t] = v;
  }
}

}  // namespace

static int dss2_lanegroup_wgrad_launch(const dss2_lanegroup_wgrad_args* ap, void* stream) {
  const dss2_lanegroup_wgrad_args& a = *ap;
  if (a.n_jobs < 1 || a.n_jobs > DSS2_LANEGROUP_WGRAD_MAX_JOBS || a.n_slabs < 1 || a.n_nodes < 1) {
    set_error("dss2_lanegroup_wgrad: %d jobs (1..%d), %d slabs", a.n_jobs, DSS2_LANEGROUP_WGRAD_MAX_JOBS, a.n_slabs);
    return 2;
  }
  hipLaunchKernelGGL(lanegroup_wgrad_kernel, dim3((unsigned)a.n_slabs, (unsigned)a.n_jobs), dim3(NT), 0, as_stream(stream), a);
  return check_launch("dss2_lanegroup_wgrad");
}

extern "C" int dss2_lanegroup_wgrad(const dss2_lanegroup_wgrad_args* ap, void* stream) {
  return dss2::entry(dss2_lanegroup_wgrad_launch, stream, dss2::copied(ap, "dss2_lanegroup_wgrad"));
}
