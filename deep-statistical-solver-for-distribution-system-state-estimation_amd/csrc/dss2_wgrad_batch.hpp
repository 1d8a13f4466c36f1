#pragma once
// Shared by the weight-gradient translation units: dss2_wgrad.hip (fp32 MFMA, and the selection of every launch's kernel),
// dss2_wgrad16.hip (bf16x6), dss2_wgrad16h.hip / dss2_wgrad16th.hip (f16x3).
#include "dss2_common.hpp"

namespace dss2 {

// Several layers of identical shape in ONE launch (blockIdx.z = layer): the layers of a block are
// independent once all output gradients exist, and at small H one layer alone cannot fill the chip.
constexpr int WGRAD_MAX_BATCH = 8;
struct WgradBatch {
  const float* G[WGRAD_MAX_BATCH]; const float* X[WGRAD_MAX_BATCH]; float* slab[WGRAD_MAX_BATCH];
  const float* rowscale2[WGRAD_MAX_BATCH];   // per layer (NULL: plain layer)
  int n; long long slab_stride;
};

// The environment switches of the weight gradient (all default on; DSS2_WGRAD_NB: the widest NB tried, default 4), read once.
struct WgradSwitches { int tall_f16, tall_pair, tall16, tall_db, nb_max, narrow_stream, ksplit; };
const WgradSwitches& wgrad_switches();

// dss2_wgrad.hip: the kernel of a launch and its geometry (dss2_wgrad_plan_t, include/dss2_hip.h).  n_layers = 0: dss2_wgrad;
// >= 1: dss2_wgrad_batched.  The dispatch launches from this record, the exported queries read it.  Each family below states
// only ITS shape conditions and LDS formula; the operand conditions the 16-bit families share are written once, in wgrad_select.
dss2_wgrad_plan_t wgrad_select(const dss2_wgrad_args& a, int n_layers);

// All 16-bit kernels but the 64-row one: a workgroup owns 64 output x 128 input columns (the 64-row kernel: 128 x 128)
inline int wgrad16_grid_y(int nrb, int hout, int hin) {
  return nrb != 2 ? ((hout + 63) / 64) * ((hin + 127) / 128) : ((hout + 127) / 128) * ((hin + 127) / 128);
}

// One launch of a 16-bit kernel (all take 128 input columns per workgroup) from the plan: the LDS opt-in once per kernel, the plan's grid and LDS
template <class K, class... Extra>
inline int launch_wgrad16_kernel(K kern, std::atomic<uint32_t>& lds_done, const char* what, int nt, const dss2_wgrad_args& a, hipStream_t stream,
                                 const WgradBatch& wb, const dss2_wgrad_plan_t& p, Extra... extra) {
  if (ensure_max_lds(reinterpret_cast<const void*>(kern), lds_done, what)) return 1;
  hipLaunchKernelGGL(kern, dim3(a.n_split, p.grid_y, p.z_groups), dim3(nt), p.launch_lds, stream, a, (a.hin + 127) / 128, wb, extra...);
  return check_launch(what);
}

// dss2_wgrad16.hip: the bf16x6 kernels (64-row, 32-row, tall).  rs2: some layer of the launch carries rowscale2.
bool wgrad16_shape(const dss2_wgrad_args& a);
size_t wgrad16_lds_bytes(int nrb, int nmat, int ell_width);
int launch_wgrad16(const dss2_wgrad_args& a, hipStream_t stream, const WgradBatch& wb, const dss2_wgrad_plan_t& p, bool rs2);

// dss2_wgrad16h.hip: the f16x3 kernel (32-row tiles; args.mfma_bf16 = 2 | headroom bits << 8 | gathered hops << 16)
bool wgrad16h_shape(const dss2_wgrad_args& a);
size_t wgrad16h_lds_bytes(int nmat, bool hops_mfma);
int launch_wgrad16h(const dss2_wgrad_args& a, hipStream_t stream, const WgradBatch& wb, const dss2_wgrad_plan_t& p, bool rs2);

// dss2_wgrad16th.hip: the f16x3 kernel of 96- .. 192-row tiles (same args.mfma_bf16 convention); pair: two layers per workgroup
bool wgrad16th_shape(const dss2_wgrad_args& a);
bool wgrad16th_pair_shape(const dss2_wgrad_args& a, int n_layers);
size_t wgrad16th_lds_bytes(int nrb, int nmat, int ell_width);
int launch_wgrad16th(const dss2_wgrad_args& a, hipStream_t stream, const WgradBatch& wb, const dss2_wgrad_plan_t& p, bool rs2);

}  // namespace dss2
