// Fused multi-tensor optimizers: one launch updates every parameter tensor of the model.  The reference driver's is Adamax
// (torch.optim.Adamax semantics, /root/reference/dss2_run.py:91-92,143):
//   exp_avg = b1*exp_avg + (1-b1)*g ;  exp_inf = max(b2*exp_inf, |g| + eps) ;
//   p -= lr / (1 - b1^t) * exp_avg / exp_inf           (weight_decay: g += wd * p first)
#include <type_traits>
#include "dss2_weightspace.hpp"

namespace dss2 {

// advances the device-side step count in front of the by-value launches of a capturable optimizer (dss2_optim_step_dev)
__global__ void step_tick_kernel(float* __restrict__ step_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step_dev[0] += 1.f;
}

// (small_gemm_body / small_gemm_tile: dss2_weightspace.hpp)
__global__ void __launch_bounds__(256) small_gemm_kernel(const dss2_sgemm_desc* __restrict__ descs, float* base_out) {
  __shared__ __attribute__((aligned(16))) float As[SG_T][SG_LDA];   // As[i][k]
  __shared__ float Bs[SG_KC][SG_T + 1];                             // Bs[k][j]
  small_gemm_tile(descs + blockIdx.y, base_out, As, Bs, (int)blockIdx.x);
}

}  // namespace dss2

static int dss2_small_gemm_launch(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream) {
  if (n_desc <= 0) return 0;
  if (max_tiles <= 0) { dss2::set_error("small_gemm: max_tiles must be positive"); return 2; }
  hipLaunchKernelGGL(dss2::small_gemm_kernel, dim3(max_tiles, n_desc), dim3(256), 0, dss2::as_stream(stream),
                     descs, base_out);
  return dss2::check_launch("small_gemm");
}
extern "C" int dss2_small_gemm(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream) {
  return dss2::entry(dss2_small_gemm_launch, stream, descs, n_desc, max_tiles, base_out);      // (descs: a DEVICE table)
}

// ---- Adamax, Adam / AdamW, RMSprop, SGD (see dss2_hip.h): one multi-tensor kernel templated on the rule.  The arithmetic is torch's
//      single-tensor path in fp32, fmaf where torch has lerp / addcmul.
namespace dss2 {

constexpr int OPTIM_CHUNK = 80;       // descriptors per launch, by value in the kernel arguments (80 x 48 B + hyper < 4 KB)
struct OptimTable { dss2_optim_desc d[OPTIM_CHUNK]; };

// t: this step's 1-based count; bc1 / bc2: 1 - beta^t (from the host, or from the device-side count).  first / stride: this thread's
// grid-stride walk, formed in the KERNEL bodies: read in here, blockDim.x is not folded to a kernel-argument load and comes from the
// dispatch packet by a vector load in front of the loop (+0.2 us on the 12 us flat launch of the C2 model).
template <int RULE>
__device__ __forceinline__ void optim_walk(float* __restrict__ param, const float* __restrict__ grad, float* s0, float* s1, float* s2,
                                           int64_t n, const dss2_optim_hyper& h, float t, float bc1, float bc2, int64_t first,
                                           int64_t stride) {
  const float lr = h.lr_dev ? h.lr_dev[0] : h.lr;
  const float wd = h.weight_decay;
  const int flags = h.flags;
  const float clr = lr / bc1;                     // ADAM / ADAMAX step size
  const float bc2s = sqrtf(bc2);
  for (int64_t i = first; i < n; i += stride) {
    float g = grad[i];
    float p = param[i];
    if constexpr (RULE == DSS2_OPT_ADAMAX) {
      if (wd != 0.f) g = fmaf(wd, p, g);
      const float m = fmaf(h.beta1, s0[i], (1.f - h.beta1) * g);       // lerp(exp_avg, g, 1-b1)
      const float u = fmaxf(h.beta2 * s1[i], fabsf(g) + h.eps);
      s0[i] = m;
      s1[i] = u;
      param[i] = p - clr * (m / u);
    } else if constexpr (RULE == DSS2_OPT_ADAM) {
      if (wd != 0.f) {
        if (flags & DSS2_OPT_DECOUPLED_WD) p *= 1.f - lr * wd;
        else g = fmaf(wd, p, g);
      }
      const float m = fmaf(h.beta1, s0[i], h.omb1 * g);                // lerp(exp_avg, g, 1-b1)
      float v = fmaf(h.omb2 * g, g, h.beta2 * s1[i]);                  // mul_(b2).addcmul_(g, g, 1-b2)
      s0[i] = m;
      s1[i] = v;
      if (flags & DSS2_OPT_AMSGRAD) {
        v = fmaxf(s2[i], v);
        s2[i] = v;
      }
      const float denom = sqrtf(v) / bc2s + h.eps;
      param[i] = p - clr * (m / denom);
    } else if constexpr (RULE == DSS2_OPT_RMSPROP) {
      if (wd != 0.f) g = fmaf(wd, p, g);
      const float sq = fmaf(h.omb2 * g, g, h.beta2 * s0[i]);           // mul_(alpha).addcmul_(g, g, 1-alpha)
      s0[i] = sq;
      float avg;
      if (flags & DSS2_OPT_CENTERED) {
        const float ga = fmaf(h.beta2, s2[i], h.omb2 * g);             // lerp(grad_avg, g, 1-alpha)
        s2[i] = ga;
        avg = sqrtf(fmaf(-ga, ga, sq));
      } else {
        avg = sqrtf(sq);
      }
      avg += h.eps;
      if (flags & DSS2_OPT_MOMENTUM) {
        const float buf = fmaf(h.momentum, s1[i], g / avg);
        s1[i] = buf;
        param[i] = p - lr * buf;
      } else {
        param[i] = p - lr * (g / avg);
      }
    } else {                                                           // DSS2_OPT_SGD
      if (wd != 0.f) g = fmaf(wd, p, g);
      if (flags & DSS2_OPT_MOMENTUM) {
        const float buf = t == 1.f ? g : fmaf(h.momentum, s0[i], h.omdamp * g);      // torch clones the gradient at the first step
        s0[i] = buf;
        g = (flags & DSS2_OPT_NESTEROV) ? fmaf(h.momentum, buf, g) : buf;
      }
      param[i] = p - lr * g;
    }
  }
}

template <int RULE>
__global__ void __launch_bounds__(256) optim_kernel(const OptimTable tab, const dss2_optim_hyper h, float t, float bc1, float bc2,
                                                    const float* __restrict__ step_dev) {
  const dss2_optim_desc& d = tab.d[blockIdx.y];
  if (step_dev) {                                  // (already advanced by step_tick_kernel)
    t = step_dev[0];
    bc1 = 1.f - powf(h.beta1, t);
    bc2 = 1.f - powf(h.beta2, t);
  }
  optim_walk<RULE>(d.param, d.grad, d.s0, d.s1, d.s2, d.n, h, t, bc1, bc2,
                   (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// Descriptor i of a flat-bucket table (in device memory) in either layout: dss2_optim_flat_desc, or the 40-byte dss2_adamax_flat_desc of
// dss2_adamax_step_flat, which has no third slot.  Workgroup-uniform.
__device__ __forceinline__ dss2_optim_flat_desc load_flat_desc(const void* __restrict__ descs, int adamax_layout, int i) {
  if (!adamax_layout) return static_cast<const dss2_optim_flat_desc*>(descs)[i];
  const dss2_adamax_flat_desc a = static_cast<const dss2_adamax_flat_desc*>(descs)[i];
  return {a.param, a.grad_off, a.exp_avg, a.exp_inf, nullptr, a.n};
}

// The last workgroup to arrive advances the device-side count.  Every workgroup has READ the count before it arrives: the
// barrier drains its loads (s_waitcnt vmcnt(0)), and only then is the arrival posted.  Nothing is published through memory, so
// a relaxed device-scope atomic is enough -- a release fence here would be an L2 write-back per workgroup on MI355X.
__device__ __forceinline__ void last_arrival_advances(float* step_dev, unsigned* counter) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x * gridDim.y - 1) {
      step_dev[0] += 1.f;
      *counter = 0u;
    }
  }
}

// One launch for every tensor of a flat gradient bucket (descriptor table in device memory, see dss2_hip.h).
template <int RULE>
__global__ void __launch_bounds__(256) optim_flat_kernel(const void* __restrict__ descs, int adamax_layout, const float* __restrict__ grad_base,
                                                         const dss2_optim_hyper h, float t, float bc1, float bc2, float* step_dev,
                                                         unsigned* counter) {
  const dss2_optim_flat_desc d = load_flat_desc(descs, adamax_layout, blockIdx.y);
  if (step_dev) {
    t = step_dev[0] + 1.f;                         // this step's (1-based) count
    bc1 = 1.f - powf(h.beta1, t);
    bc2 = 1.f - powf(h.beta2, t);
  }
  optim_walk<RULE>(d.param, grad_base + d.grad_off, d.s0, d.s1, d.s2, d.n, h, t, bc1, bc2,
                   (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  if (step_dev) last_arrival_advances(step_dev, counter);
}

// ---- global-norm gradient clipping: fp64 partial per workgroup, re-added in index order by every workgroup of the second launch
constexpr int GRAD_CHUNK = DSS2_OPTIM_GRAD_CHUNK;       // {pointer, n} descriptors per launch, by value (192 x 16 B = 3 KB)
constexpr int GRAD_MAX_PARTIALS = DSS2_OPTIM_MAX_PARTIALS;
struct GradTable { dss2_grad_desc d[GRAD_CHUNK]; };

__global__ void __launch_bounds__(256) grad_sqsum_kernel(const GradTable tab, const dss2_grad_flat_desc* __restrict__ flat,
                                                         const float* __restrict__ grad_base, int n_desc, double* __restrict__ partials) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int j = 0; j < n_desc; ++j) {
    const float* __restrict__ g = flat ? grad_base + flat[j].grad_off : tab.d[j].grad;
    const int64_t n = flat ? flat[j].n : tab.d[j].n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      const double v = (double)g[i];
      acc = fma(v, v, acc);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {              // fixed tree: the same bits every run
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) grad_clip_scale_kernel(const GradTable tab, const dss2_grad_flat_desc* __restrict__ flat,
                                                              float* __restrict__ grad_base, int n_desc, const double* __restrict__ partials,
                                                              int n_partials, float max_norm, float* __restrict__ norm_out) {
  double sum = 0.0;
  for (int k = 0; k < n_partials; ++k) sum += partials[k];
  const float total = (float)sqrt(sum);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = total;
  const float c = max_norm / (total + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;            // (a NaN stays a NaN: torch.clamp(max=1.0))
  if (coef == 1.f) return;                         // g * 1 = g
  for (int j = 0; j < n_desc; ++j) {
    float* __restrict__ g = flat ? grad_base + flat[j].grad_off : tab.d[j].grad;
    const int64_t n = flat ? flat[j].n : tab.d[j].n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] *= coef;
  }
}

}  // namespace dss2

static int optim_hyper_check(const dss2_optim_hyper* h, const char* who) {
  if (!h) { dss2::set_error("%s: null hyper-parameters", who); return 2; }
  if (h->rule < DSS2_OPT_ADAM || h->rule > DSS2_OPT_ADAMAX) { dss2::set_error("%s: unknown rule %d", who, h->rule); return 2; }
  return 0;
}

// which of the three state slots the rule reads and writes
static int optim_slot_mask(const dss2_optim_hyper& h) {
  switch (h.rule) {
    case DSS2_OPT_ADAM: return 3 | ((h.flags & DSS2_OPT_AMSGRAD) ? 4 : 0);
    case DSS2_OPT_RMSPROP: return 1 | ((h.flags & DSS2_OPT_MOMENTUM) ? 2 : 0) | ((h.flags & DSS2_OPT_CENTERED) ? 4 : 0);
    case DSS2_OPT_SGD: return (h.flags & DSS2_OPT_MOMENTUM) ? 1 : 0;
    default: return 3;
  }
}

// h.rule -> the kernel instantiation: f gets the rule as a std::integral_constant, for both the by-value and the flat launch
template <class F>
static void optim_for_rule(int rule, F&& f) {
  switch (rule) {
    case DSS2_OPT_ADAM: f(std::integral_constant<int, DSS2_OPT_ADAM>{}); break;
    case DSS2_OPT_RMSPROP: f(std::integral_constant<int, DSS2_OPT_RMSPROP>{}); break;
    case DSS2_OPT_SGD: f(std::integral_constant<int, DSS2_OPT_SGD>{}); break;
    default: f(std::integral_constant<int, DSS2_OPT_ADAMAX>{}); break;
  }
}

// workgroups per tensor: one per `per_wg` elements of the largest tensor, 1 .. 64
static unsigned optim_grid_x(int64_t max_n, int per_wg) {
  const int64_t bx = (max_n + per_wg - 1) / per_wg;
  return bx > 64 ? 64u : bx < 1 ? 1u : (unsigned)bx;
}

// A host table travels to the kernels by value, one TABLE of descriptors per launch: launch(tab, c0, n) gets descriptors c0 .. c0 + n - 1
// and may refuse them with a nonzero return, which ends the walk.
template <class TABLE, class DESC, class LAUNCH>
static int for_each_chunk(const DESC* descs_host, int n_desc, LAUNCH&& launch) {
  constexpr int CHUNK = (int)std::extent<decltype(TABLE::d)>::value;
  for (int c0 = 0; c0 < n_desc; c0 += CHUNK) {
    const int n = n_desc - c0 < CHUNK ? n_desc - c0 : CHUNK;
    TABLE tab = {};
    for (int i = 0; i < n; ++i) tab.d[i] = descs_host[c0 + i];
    if (int rc = launch(tab, c0, n)) return rc;
  }
  return 0;
}

// The launch bodies below serve dss2_optim_step* and their Adamax adapters; `who` is the entry point the caller used, for error texts.
static int optim_launch(const char* who, const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper& h, float t, float bc1,
                        float bc2, const float* step_dev, hipStream_t s) {
  const int mask = optim_slot_mask(h);
  const int rc = for_each_chunk<dss2::OptimTable>(descs_host, n_desc, [&](const dss2::OptimTable& tab, int c0, int n) {
    int64_t max_n = 0;
    for (int i = 0; i < n; ++i) {
      const dss2_optim_desc& d = tab.d[i];
      if (!d.param || !d.grad || ((mask & 1) && !d.s0) || ((mask & 2) && !d.s1) || ((mask & 4) && !d.s2) || d.n < 0) {
        dss2::set_error("%s: descriptor %d is incomplete", who, c0 + i);
        return 2;
      }
      if (d.n > max_n) max_n = d.n;
    }
    const dim3 grid(optim_grid_x(max_n, 256), n);
    optim_for_rule(h.rule, [&](auto rule) {
      hipLaunchKernelGGL(dss2::optim_kernel<decltype(rule)::value>, grid, dim3(256), 0, s, tab, h, t, bc1, bc2, step_dev);
    });
    return 0;
  });
  return rc ? rc : dss2::check_launch(who);
}

static int optim_step_launch(const char* who, const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper& h, int step, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host) { dss2::set_error("%s: null descriptor table", who); return 2; }
  if (step < 1) { dss2::set_error("%s: step must be >= 1", who); return 2; }
  return optim_launch(who, descs_host, n_desc, h, (float)step, 1.f - powf(h.beta1, (float)step), 1.f - powf(h.beta2, (float)step), nullptr,
                      dss2::as_stream(stream));
}

static int optim_step_dev_launch(const char* who, const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper& h, float* step_dev, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host || !step_dev) { dss2::set_error("%s: null argument", who); return 2; }
  hipLaunchKernelGGL(dss2::step_tick_kernel, dim3(1), dim3(64), 0, dss2::as_stream(stream), step_dev);
  return optim_launch(who, descs_host, n_desc, h, 1.f, 1.f, 1.f, step_dev, dss2::as_stream(stream));
}

// descs_dev: a device table of dss2_optim_flat_desc, or (adamax_layout) of dss2_adamax_flat_desc
static int optim_step_flat_launch(const char* who, const void* descs_dev, int adamax_layout, int n_desc, int64_t max_n, const float* grad_base,
                                  const dss2_optim_hyper& h, int step, float* step_dev, uint32_t* counter, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_dev || !grad_base || n_desc > 65535) { dss2::set_error("%s: bad arguments", who); return 2; }
  if (step < 0 || (step == 0 && (!step_dev || !counter))) { dss2::set_error("%s: step >= 1, or step == 0 with step_dev and counter", who); return 2; }
  // a workgroup walks up to 16 elements per thread: few, fat workgroups (and few arrivals at the step counter's word)
  const dim3 grid(optim_grid_x(max_n, 4096), n_desc);
  const float t = step > 0 ? (float)step : 1.f;
  const float bc1 = step > 0 ? 1.f - powf(h.beta1, t) : 1.f, bc2 = step > 0 ? 1.f - powf(h.beta2, t) : 1.f;
  float* sd = step > 0 ? nullptr : step_dev;
  optim_for_rule(h.rule, [&](auto rule) {
    hipLaunchKernelGGL(dss2::optim_flat_kernel<decltype(rule)::value>, grid, dim3(256), 0, dss2::as_stream(stream), descs_dev, adamax_layout,
                       grad_base, h, t, bc1, bc2, sd, counter);
  });
  return dss2::check_launch(who);
}

extern "C" int dss2_optim_step(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, int step, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step")) return rc;
  return dss2::entry(optim_step_launch, stream, "optim_step", dss2::kept(descs_host, n_desc), n_desc, *hyper, step);
}

extern "C" int dss2_optim_step_dev(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, float* step_dev, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step_dev")) return rc;
  return dss2::entry(optim_step_dev_launch, stream, "optim_step_dev", dss2::kept(descs_host, n_desc), n_desc, *hyper, step_dev);
}

extern "C" int dss2_optim_step_flat(const dss2_optim_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base,
                                    const dss2_optim_hyper* hyper, int step, float* step_dev, uint32_t* counter, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step_flat")) return rc;
  return dss2::entry(optim_step_flat_launch, stream, "optim_step_flat", descs_dev, 0, n_desc, max_n, grad_base, *hyper, step, step_dev, counter);
}

// ---- the Adamax entry points of the header: adapters onto the launch bodies above (rule ADAMAX, learning rate from the host)
static dss2_optim_hyper adamax_hyper(float lr, float beta1, float beta2, float eps, float weight_decay) {
  dss2_optim_hyper h = {};
  h.rule = DSS2_OPT_ADAMAX;
  h.lr = lr; h.beta1 = beta1; h.beta2 = beta2; h.eps = eps; h.weight_decay = weight_decay;
  return h;
}

// (one allocation per call: the converted table is what the launch walks and, when a plan records, what its closure copies)
static std::vector<dss2_optim_desc> adamax_descs(const dss2_adamax_desc* descs_host, int n_desc) {
  std::vector<dss2_optim_desc> d(descs_host && n_desc > 0 ? (size_t)n_desc : 0);
  for (size_t i = 0; i < d.size(); ++i) {
    const dss2_adamax_desc& a = descs_host[i];
    d[i] = {a.param, a.grad, a.exp_avg, a.exp_inf, nullptr, a.n};
  }
  return d;
}

extern "C" int dss2_adamax_step(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream) {
  const dss2_optim_hyper h = adamax_hyper(lr, beta1, beta2, eps, weight_decay);
  const std::vector<dss2_optim_desc> d = adamax_descs(descs_host, n_desc);
  return dss2::entry(optim_step_launch, stream, "adamax_step", dss2::kept(d.data(), d.size()), n_desc, h, step);
}

extern "C" int dss2_adamax_step_dev(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, float* step_dev, void* stream) {
  const dss2_optim_hyper h = adamax_hyper(lr, beta1, beta2, eps, weight_decay);
  const std::vector<dss2_optim_desc> d = adamax_descs(descs_host, n_desc);
  return dss2::entry(optim_step_dev_launch, stream, "adamax_step_dev", dss2::kept(d.data(), d.size()), n_desc, h, step_dev);
}

// (the table is in device memory in the 40-byte layout: the kernel reads it as it is)
extern "C" int dss2_adamax_step_flat(const dss2_adamax_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* step_dev, uint32_t* counter, void* stream) {
  const dss2_optim_hyper h = adamax_hyper(lr, beta1, beta2, eps, weight_decay);
  return dss2::entry(optim_step_flat_launch, stream, "adamax_step_flat", descs_dev, 1, n_desc, max_n, grad_base, h, step, step_dev, counter);
}

// ---- gradient clipping: by-value chunks of a host table, or the whole device table of a flat bucket, for both launches
static int grad_args_check(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base, int n_desc,
                           int n_wg, const void* partials, const char* who) {
  if ((!descs_host) == (!descs_dev) || (descs_dev && !grad_base) || !partials) { dss2::set_error("%s: a host table, or a device table with its bucket", who); return 2; }
  const int chunks = descs_dev ? 1 : (n_desc + dss2::GRAD_CHUNK - 1) / dss2::GRAD_CHUNK;
  if (n_wg < 1 || (int64_t)chunks * n_wg > dss2::GRAD_MAX_PARTIALS) { dss2::set_error("%s: %d launches x %d workgroups exceed %d partials", who, chunks, n_wg, dss2::GRAD_MAX_PARTIALS); return 2; }
  if (descs_host)
    for (int i = 0; i < n_desc; ++i)
      if (!descs_host[i].grad || descs_host[i].n < 0) { dss2::set_error("%s: descriptor %d is incomplete", who, i); return 2; }
  return 0;
}

// (both bodies refuse n_desc <= 0 before they choose between the tables, so kept()'s null for an empty host table decides nothing)
static int dss2_grad_sqsum_partials_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base, int n_desc, int n_wg, double* partials, void* stream) {
  if (n_desc <= 0) { dss2::set_error("grad_sqsum_partials: no gradients"); return 2; }
  if (int rc = grad_args_check(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, "grad_sqsum_partials")) return rc;
  hipStream_t s = dss2::as_stream(stream);
  if (descs_dev) {
    hipLaunchKernelGGL(dss2::grad_sqsum_kernel, dim3(n_wg), dim3(256), 0, s, dss2::GradTable{}, descs_dev, grad_base, n_desc, partials);
  } else {
    int c = 0;                                     // chunk c writes partials[c * n_wg ..]
    if (int rc = for_each_chunk<dss2::GradTable>(descs_host, n_desc, [&](const dss2::GradTable& tab, int, int n) {
          hipLaunchKernelGGL(dss2::grad_sqsum_kernel, dim3(n_wg), dim3(256), 0, s, tab, nullptr, nullptr, n, partials + (int64_t)c++ * n_wg);
          return 0;
        })) return rc;
  }
  return dss2::check_launch("grad_sqsum_partials");
}
extern "C" int dss2_grad_sqsum_partials(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base,
                                        int n_desc, int n_wg, double* partials, void* stream) {
  return dss2::entry(dss2_grad_sqsum_partials_launch, stream, dss2::kept(descs_host, n_desc), descs_dev, grad_base, n_desc, n_wg, partials);
}

static int dss2_grad_clip_scale_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc, int n_wg, const double* partials, float max_norm, float* norm_out, void* stream) {
  if (n_desc <= 0) { dss2::set_error("grad_clip_scale: no gradients"); return 2; }
  if (int rc = grad_args_check(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, "grad_clip_scale")) return rc;
  if (!norm_out) { dss2::set_error("grad_clip_scale: null norm_out"); return 2; }
  hipStream_t s = dss2::as_stream(stream);
  if (descs_dev) {
    hipLaunchKernelGGL(dss2::grad_clip_scale_kernel, dim3(n_wg), dim3(256), 0, s, dss2::GradTable{}, descs_dev, grad_base, n_desc, partials, n_wg, max_norm, norm_out);
  } else {
    const int chunks = (n_desc + dss2::GRAD_CHUNK - 1) / dss2::GRAD_CHUNK;
    if (int rc = for_each_chunk<dss2::GradTable>(descs_host, n_desc, [&](const dss2::GradTable& tab, int, int n) {
          hipLaunchKernelGGL(dss2::grad_clip_scale_kernel, dim3(n_wg), dim3(256), 0, s, tab, nullptr, nullptr, n, partials, chunks * n_wg, max_norm, norm_out);
          return 0;
        })) return rc;
  }
  return dss2::check_launch("grad_clip_scale");
}
extern "C" int dss2_grad_clip_scale(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc,
                                    int n_wg, const double* partials, float max_norm, float* norm_out, void* stream) {
  return dss2::entry(dss2_grad_clip_scale_launch, stream, dss2::kept(descs_host, n_desc), descs_dev, grad_base, n_desc, n_wg, partials, max_norm, norm_out);
}


// ---- dropout random state (see dss2_hip.h) -------------------------------------------------------------------------------
namespace dss2 {
__global__ void rng_next_kernel(unsigned long long* __restrict__ state, unsigned long long* __restrict__ snap,
                                unsigned long long host_seed, int use_host_seed) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (use_host_seed) { snap[0] = host_seed; snap[1] = 0; }
  else { snap[0] = state[0]; snap[1] = state[1]; state[1] = state[1] + 1; }
}

__global__ void __launch_bounds__(256) dropout_mask_kernel(const uint64_t* __restrict__ snap, uint32_t id, uint32_t thr, float scale,
                                                           int64_t n_rows, int h, float* __restrict__ out, int64_t ldo) {
  const uint64_t seed = snap[0], off = snap[1];
  const int groups = (h + 3) >> 2;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_rows * groups; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / groups;
    const int g = (int)(t - row * groups);
    const f32x4 m = dropout_mult4(seed, off, id, (uint32_t)row, (uint32_t)g, thr, scale);
    for (int q = 0; q < 4; ++q)
      if (4 * g + q < h) out[row * ldo + 4 * g + q] = m[q];
  }
}
}  // namespace dss2

static int dss2_rng_next_launch(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream) {
  if (!snapshot || (!use_host_seed && !state)) { dss2::set_error("rng_next: null argument"); return 2; }
  hipLaunchKernelGGL(dss2::rng_next_kernel, dim3(1), dim3(64), 0, dss2::as_stream(stream),
                     reinterpret_cast<unsigned long long*>(state), reinterpret_cast<unsigned long long*>(snapshot),
                     (unsigned long long)host_seed, use_host_seed);
  return dss2::check_launch("rng_next");
}
extern "C" int dss2_rng_next(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream) {
  return dss2::entry(dss2_rng_next_launch, stream, state, snapshot, host_seed, use_host_seed);
}

// p -> (threshold, scale) exactly as the Python side computes them for the kernels (one definition: this one)
extern "C" void dss2_dropout_params(float p, uint32_t* thr, float* scale) {
  if (p <= 0.f) { *thr = 0u; *scale = 1.f; }
  else if (p >= 1.f) { *thr = 0u; *scale = 0.f; }
  else {
    const double t = (double)p * 4294967296.0;
    *thr = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
    *scale = 1.f / (1.f - p);
  }
}

static int dss2_dropout_mask_launch(const uint64_t* snapshot, int32_t drop_id, float p, int64_t n_rows, int h, float* out, int64_t ldo, void* stream) {
  if (!snapshot || !out || drop_id <= 0 || h <= 0) { dss2::set_error("dropout_mask: bad arguments"); return 2; }
  if (n_rows <= 0) return 0;
  uint32_t thr; float scale;
  dss2_dropout_params(p, &thr, &scale);
  int64_t blocks = (n_rows * ((h + 3) / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dss2::dropout_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, dss2::as_stream(stream), snapshot,
                     (uint32_t)drop_id, thr, scale, n_rows, h, out, ldo);
  return dss2::check_launch("dropout_mask");
}
extern "C" int dss2_dropout_mask(const uint64_t* snapshot, int32_t drop_id, float p, int64_t n_rows, int h, float* out,
                                 int64_t ldo, void* stream) {
  return dss2::entry(dss2_dropout_mask_launch, stream, snapshot, drop_id, p, n_rows, h, out, ldo);
}


// ---- gradient through "dropout, then ReLU" of a layer output (networks.py:268-269 between the layers of the Multi* variants):
//      gpre = g * mask * (y > 0), y = the layer's post-activation output, mask regenerated from the layer's dropout spec.
namespace dss2 {
__global__ void __launch_bounds__(256) gate_grad_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out,
                                                        int64_t n_rows, int h, const uint64_t* __restrict__ snap, uint32_t id,
                                                        uint32_t thr, float scale, int relu) {
  const uint64_t seed = snap ? snap[0] : 0, off = snap ? snap[1] : 0;
  const int groups = (h + 3) >> 2;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_rows * groups; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / groups;
    const int gq = (int)(t - row * groups);
    f32x4 m = {1.f, 1.f, 1.f, 1.f};
    if (snap) m = dropout_mult4(seed, off, id, (uint32_t)row, (uint32_t)gq, thr, scale);
    for (int q = 0; q < 4; ++q) {
      const int c = 4 * gq + q;
      if (c < h) {
        const int64_t i = row * h + c;
        out[i] = (!relu || relu_open(y[i])) ? g[i] * m[q] : 0.f;
      }
    }
  }
}
}  // namespace dss2

static int dss2_gate_grad_launch(const float* g, const float* y, float* out, int64_t n_rows, int h, const uint64_t* snapshot, int32_t drop_id, float p, int relu, void* stream) {
  if (!g || !out || (relu && !y) || h <= 0) { dss2::set_error("gate_grad: bad arguments"); return 2; }
  if (n_rows <= 0) return 0;
  uint32_t thr = 0; float scale = 1.f;
  if (snapshot) dss2_dropout_params(p, &thr, &scale);
  int64_t blocks = (n_rows * ((h + 3) / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dss2::gate_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, dss2::as_stream(stream), g, y, out, n_rows, h,
                     snapshot, (uint32_t)drop_id, thr, scale, relu);
  return dss2::check_launch("gate_grad");
}
extern "C" int dss2_gate_grad(const float* g, const float* y, float* out, int64_t n_rows, int h, const uint64_t* snapshot, int32_t drop_id, float p, int relu, void* stream) {
  return dss2::entry(dss2_gate_grad_launch, stream, g, y, out, n_rows, h, snapshot, drop_id, p, relu);
}
