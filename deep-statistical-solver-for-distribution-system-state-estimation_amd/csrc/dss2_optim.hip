// Fused multi-tensor Adamax (torch.optim.Adamax semantics, the optimizer of the reference driver,
// /root/reference/dss2_run.py:91-92,143): one launch updates every parameter tensor of the model.
//   exp_avg = b1*exp_avg + (1-b1)*g ;  exp_inf = max(b2*exp_inf, |g| + eps) ;
//   p -= lr / (1 - b1^t) * exp_avg / exp_inf           (weight_decay: g += wd * p first)
#include "dss2_weightspace.hpp"

namespace dss2 {

__global__ void adamax_tick_kernel(float* __restrict__ step_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step_dev[0] += 1.f;
}

// step_dev != NULL: the 1-based step count lives on the device (already advanced by adamax_tick_kernel), so the launch can
// sit inside a hipGraph and every replay uses the next count; NULL: bias_corr1 was computed by the host.
constexpr int ADAMAX_CHUNK = 96;      // descriptors per launch, by value in the kernel arguments (96 x 40 B < 4 KB)
struct AdamaxTable { dss2_adamax_desc d[ADAMAX_CHUNK]; };

__global__ void __launch_bounds__(256) adamax_kernel(const AdamaxTable tab, float lr, float beta1,
                                                     float beta2, float eps, float weight_decay, float bias_corr1,
                                                     const float* __restrict__ step_dev) {
  const dss2_adamax_desc& d = tab.d[blockIdx.y];
  if (step_dev) bias_corr1 = 1.f - powf(beta1, step_dev[0]);
  const float clr = lr / bias_corr1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) {
    float g = d.grad[i];
    const float p = d.param[i];
    if (weight_decay != 0.f) g = fmaf(weight_decay, p, g);
    const float m = fmaf(beta1, d.exp_avg[i], (1.f - beta1) * g);        // lerp(exp_avg, g, 1-b1)
    const float u = fmaxf(beta2 * d.exp_inf[i], fabsf(g) + eps);
    d.exp_avg[i] = m;
    d.exp_inf[i] = u;
    d.param[i] = p - clr * (m / u);
  }
}

// One launch for every tensor of a flat gradient bucket (descriptor table in device memory, see dss2_hip.h).
__global__ void __launch_bounds__(256) adamax_flat_kernel(const dss2_adamax_flat_desc* __restrict__ descs,
                                                          const float* __restrict__ grad_base, float lr, float beta1, float beta2,
                                                          float eps, float weight_decay, float bias_corr1, float* step_dev,
                                                          unsigned* counter) {
  const dss2_adamax_flat_desc d = descs[blockIdx.y];
  if (step_dev) bias_corr1 = 1.f - powf(beta1, step_dev[0] + 1.f);      // this step's (1-based) count
  const float clr = lr / bias_corr1;
  const float* __restrict__ grad = grad_base + d.grad_off;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) {
    float g = grad[i];
    const float p = d.param[i];
    if (weight_decay != 0.f) g = fmaf(weight_decay, p, g);
    const float m = fmaf(beta1, d.exp_avg[i], (1.f - beta1) * g);
    const float u = fmaxf(beta2 * d.exp_inf[i], fabsf(g) + eps);
    d.exp_avg[i] = m;
    d.exp_inf[i] = u;
    d.param[i] = p - clr * (m / u);
  }
  if (!step_dev) return;
  // The last workgroup to arrive advances the device-side count.  Every workgroup has READ the count before it arrives: the
  // barrier drains its loads (s_waitcnt vmcnt(0)), and only then is the arrival posted.  Nothing is published through memory, so
  // a relaxed device-scope atomic is enough -- a release fence here would be an L2 write-back per workgroup on MI355X.
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x * gridDim.y - 1) {
      step_dev[0] += 1.f;
      *counter = 0u;
    }
  }
}

// (small_gemm_body / small_gemm_tile: dss2_weightspace.hpp)
__global__ void __launch_bounds__(256) small_gemm_kernel(const dss2_sgemm_desc* __restrict__ descs, float* base_out) {
  __shared__ __attribute__((aligned(16))) float As[SG_T][SG_LDA];   // As[i][k]
  __shared__ float Bs[SG_KC][SG_T + 1];                             // Bs[k][j]
  small_gemm_tile(descs + blockIdx.y, base_out, As, Bs, (int)blockIdx.x);
}

}  // namespace dss2

static int dss2_small_gemm_launch(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream);
extern "C" int dss2_small_gemm(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream) {
  DSS2_RECORD([descs, n_desc, max_tiles, base_out](void* s_) { return dss2_small_gemm_launch(descs, n_desc, max_tiles, base_out, s_); });
  return dss2_small_gemm_launch(descs, n_desc, max_tiles, base_out, stream);
}
static int dss2_small_gemm_launch(const dss2_sgemm_desc* descs, int n_desc, int max_tiles, float* base_out, void* stream) {
  if (n_desc <= 0) return 0;
  if (max_tiles <= 0) { dss2::set_error("small_gemm: max_tiles must be positive"); return 2; }
  hipLaunchKernelGGL(dss2::small_gemm_kernel, dim3(max_tiles, n_desc), dim3(256), 0, dss2::as_stream(stream),
                     descs, base_out);
  return dss2::check_launch("small_gemm");
}

static int adamax_launch(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float bc1, const float* step_dev, hipStream_t s) {
  for (int c0 = 0; c0 < n_desc; c0 += dss2::ADAMAX_CHUNK) {
    const int n = n_desc - c0 < dss2::ADAMAX_CHUNK ? n_desc - c0 : dss2::ADAMAX_CHUNK;
    dss2::AdamaxTable tab = {};
    int64_t max_n = 0;
    for (int i = 0; i < n; ++i) {
      tab.d[i] = descs_host[c0 + i];
      if (!tab.d[i].param || !tab.d[i].grad || !tab.d[i].exp_avg || !tab.d[i].exp_inf) { dss2::set_error("adamax_step: descriptor %d is incomplete", c0 + i); return 2; }
      if (tab.d[i].n > max_n) max_n = tab.d[i].n;
    }
    int64_t bx = (max_n + 255) / 256;
    if (bx > 64) bx = 64;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(dss2::adamax_kernel, dim3((unsigned)bx, n), dim3(256), 0, s, tab, lr, beta1, beta2, eps, weight_decay, bc1, step_dev);
  }
  return dss2::check_launch("adamax_step");
}

static int dss2_adamax_step_launch(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
extern "C" int dss2_adamax_step(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream) {
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), n_desc, lr, beta1, beta2, eps, weight_decay, step](void* s_) { return dss2_adamax_step_launch(dss2::plan_ptr(d), n_desc, lr, beta1, beta2, eps, weight_decay, step, s_); });
  return dss2_adamax_step_launch(descs_host, n_desc, lr, beta1, beta2, eps, weight_decay, step, stream);
}
static int dss2_adamax_step_launch(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host) { dss2::set_error("adamax_step: null descriptor table"); return 2; }
  if (step < 1) { dss2::set_error("adamax_step: step must be >= 1"); return 2; }
  return adamax_launch(descs_host, n_desc, lr, beta1, beta2, eps, weight_decay, 1.f - powf(beta1, (float)step), nullptr, dss2::as_stream(stream));
}

static int dss2_adamax_step_flat_launch(const dss2_adamax_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* step_dev, uint32_t* counter, void* stream);
extern "C" int dss2_adamax_step_flat(const dss2_adamax_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* step_dev, uint32_t* counter, void* stream) {
  DSS2_RECORD([descs_dev, n_desc, max_n, grad_base, lr, beta1, beta2, eps, weight_decay, step, step_dev, counter](void* s_) { return dss2_adamax_step_flat_launch(descs_dev, n_desc, max_n, grad_base, lr, beta1, beta2, eps, weight_decay, step, step_dev, counter, s_); });
  return dss2_adamax_step_flat_launch(descs_dev, n_desc, max_n, grad_base, lr, beta1, beta2, eps, weight_decay, step, step_dev, counter, stream);
}
static int dss2_adamax_step_flat_launch(const dss2_adamax_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* step_dev, uint32_t* counter, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_dev || !grad_base || n_desc > 65535) { dss2::set_error("adamax_step_flat: bad arguments"); return 2; }
  if (step < 0 || (step == 0 && (!step_dev || !counter))) { dss2::set_error("adamax_step_flat: step >= 1, or step == 0 with step_dev and counter"); return 2; }
  int64_t bx = (max_n + 4095) / 4096;      // a workgroup walks up to 16 elements per thread: few, fat workgroups (and few
  if (bx > 64) bx = 64;                    // arrivals at the step counter's word)
  if (bx < 1) bx = 1;
  const float bc1 = step > 0 ? 1.f - powf(beta1, (float)step) : 1.f;
  hipLaunchKernelGGL(dss2::adamax_flat_kernel, dim3((unsigned)bx, n_desc), dim3(256), 0, dss2::as_stream(stream), descs_dev, grad_base,
                     lr, beta1, beta2, eps, weight_decay, bc1, step > 0 ? nullptr : step_dev, counter);
  return dss2::check_launch("adamax_step_flat");
}

static int dss2_adamax_step_dev_launch(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, float* step_dev, void* stream);
extern "C" int dss2_adamax_step_dev(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, float* step_dev, void* stream) {
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), n_desc, lr, beta1, beta2, eps, weight_decay, step_dev](void* s_) { return dss2_adamax_step_dev_launch(dss2::plan_ptr(d), n_desc, lr, beta1, beta2, eps, weight_decay, step_dev, s_); });
  return dss2_adamax_step_dev_launch(descs_host, n_desc, lr, beta1, beta2, eps, weight_decay, step_dev, stream);
}
static int dss2_adamax_step_dev_launch(const dss2_adamax_desc* descs_host, int n_desc, float lr, float beta1, float beta2, float eps, float weight_decay, float* step_dev, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host || !step_dev) { dss2::set_error("adamax_step_dev: null argument"); return 2; }
  hipLaunchKernelGGL(dss2::adamax_tick_kernel, dim3(1), dim3(64), 0, dss2::as_stream(stream), step_dev);
  return adamax_launch(descs_host, n_desc, lr, beta1, beta2, eps, weight_decay, 1.f, step_dev, dss2::as_stream(stream));
}

// ---- Adam / AdamW, RMSprop, SGD, and Adamax with a device-side learning rate (see dss2_hip.h): one multi-tensor kernel templated on
//      the rule.  The arithmetic is torch's single-tensor path in fp32, fmaf where torch has lerp / addcmul (as adamax_kernel).
namespace dss2 {

constexpr int OPTIM_CHUNK = 80;       // descriptors per launch, by value in the kernel arguments (80 x 48 B + hyper < 4 KB)
struct OptimTable { dss2_optim_desc d[OPTIM_CHUNK]; };

// t: this step's 1-based count; bc1 / bc2: 1 - beta^t (from the host, or from the device-side count)
template <int RULE>
__device__ __forceinline__ void optim_walk(float* __restrict__ param, const float* __restrict__ grad, float* s0, float* s1, float* s2,
                                           int64_t n, const dss2_optim_hyper& h, float t, float bc1, float bc2) {
  const float lr = h.lr_dev ? h.lr_dev[0] : h.lr;
  const float wd = h.weight_decay;
  const int flags = h.flags;
  const float clr = lr / bc1;                     // ADAM / ADAMAX step size
  const float bc2s = sqrtf(bc2);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float g = grad[i];
    float p = param[i];
    if constexpr (RULE == DSS2_OPT_ADAMAX) {      // the operations of adamax_kernel, in its order
      if (wd != 0.f) g = fmaf(wd, p, g);
      const float m = fmaf(h.beta1, s0[i], (1.f - h.beta1) * g);
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
  if (step_dev) {                                  // (already advanced by adamax_tick_kernel)
    t = step_dev[0];
    bc1 = 1.f - powf(h.beta1, t);
    bc2 = 1.f - powf(h.beta2, t);
  }
  optim_walk<RULE>(d.param, d.grad, d.s0, d.s1, d.s2, d.n, h, t, bc1, bc2);
}

template <int RULE>
__global__ void __launch_bounds__(256) optim_flat_kernel(const dss2_optim_flat_desc* __restrict__ descs, const float* __restrict__ grad_base,
                                                         const dss2_optim_hyper h, float t, float bc1, float bc2, float* step_dev,
                                                         unsigned* counter) {
  const dss2_optim_flat_desc d = descs[blockIdx.y];
  if (step_dev) {
    t = step_dev[0] + 1.f;                         // this step's (1-based) count
    bc1 = 1.f - powf(h.beta1, t);
    bc2 = 1.f - powf(h.beta2, t);
  }
  optim_walk<RULE>(d.param, grad_base + d.grad_off, d.s0, d.s1, d.s2, d.n, h, t, bc1, bc2);
  if (!step_dev) return;
  // the last workgroup to arrive advances the count: the pattern of adamax_flat_kernel (every workgroup has read the count before the
  // barrier; nothing is published through memory, so the arrival is a relaxed device-scope atomic without a fence)
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x * gridDim.y - 1) {
      step_dev[0] += 1.f;
      *counter = 0u;
    }
  }
}

// ---- global-norm gradient clipping: fp64 partial per workgroup, re-added in index order by every workgroup of the second launch
constexpr int GRAD_CHUNK = 192;       // {pointer, n} descriptors per launch, by value (192 x 16 B = 3 KB)
constexpr int GRAD_MAX_PARTIALS = 256;
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

template <int RULE>
static void optim_launch_rule(const dss2::OptimTable& tab, dim3 grid, const dss2_optim_hyper& h, float t, float bc1, float bc2,
                              const float* step_dev, hipStream_t s) {
  hipLaunchKernelGGL(dss2::optim_kernel<RULE>, grid, dim3(256), 0, s, tab, h, t, bc1, bc2, step_dev);
}

static int optim_launch(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper& h, float t, float bc1, float bc2,
                        const float* step_dev, hipStream_t s) {
  const int mask = optim_slot_mask(h);
  for (int c0 = 0; c0 < n_desc; c0 += dss2::OPTIM_CHUNK) {
    const int n = n_desc - c0 < dss2::OPTIM_CHUNK ? n_desc - c0 : dss2::OPTIM_CHUNK;
    dss2::OptimTable tab = {};
    int64_t max_n = 0;
    for (int i = 0; i < n; ++i) {
      const dss2_optim_desc& d = tab.d[i] = descs_host[c0 + i];
      if (!d.param || !d.grad || ((mask & 1) && !d.s0) || ((mask & 2) && !d.s1) || ((mask & 4) && !d.s2) || d.n < 0) {
        dss2::set_error("optim_step: descriptor %d is incomplete", c0 + i);
        return 2;
      }
      if (d.n > max_n) max_n = d.n;
    }
    int64_t bx = (max_n + 255) / 256;
    if (bx > 64) bx = 64;
    if (bx < 1) bx = 1;
    const dim3 grid((unsigned)bx, n);
    switch (h.rule) {
      case DSS2_OPT_ADAM: optim_launch_rule<DSS2_OPT_ADAM>(tab, grid, h, t, bc1, bc2, step_dev, s); break;
      case DSS2_OPT_RMSPROP: optim_launch_rule<DSS2_OPT_RMSPROP>(tab, grid, h, t, bc1, bc2, step_dev, s); break;
      case DSS2_OPT_SGD: optim_launch_rule<DSS2_OPT_SGD>(tab, grid, h, t, bc1, bc2, step_dev, s); break;
      default: optim_launch_rule<DSS2_OPT_ADAMAX>(tab, grid, h, t, bc1, bc2, step_dev, s); break;
    }
  }
  return dss2::check_launch("optim_step");
}

static int dss2_optim_step_launch(const dss2_optim_desc* descs_host, int n_desc, dss2_optim_hyper h, int step, void* stream);
extern "C" int dss2_optim_step(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, int step, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step")) return rc;
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), n_desc, h = *hyper, step](void* s_) { return dss2_optim_step_launch(dss2::plan_ptr(d), n_desc, h, step, s_); });
  return dss2_optim_step_launch(descs_host, n_desc, *hyper, step, stream);
}
static int dss2_optim_step_launch(const dss2_optim_desc* descs_host, int n_desc, dss2_optim_hyper h, int step, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host) { dss2::set_error("optim_step: null descriptor table"); return 2; }
  if (step < 1) { dss2::set_error("optim_step: step must be >= 1"); return 2; }
  return optim_launch(descs_host, n_desc, h, (float)step, 1.f - powf(h.beta1, (float)step), 1.f - powf(h.beta2, (float)step), nullptr,
                      dss2::as_stream(stream));
}

static int dss2_optim_step_dev_launch(const dss2_optim_desc* descs_host, int n_desc, dss2_optim_hyper h, float* step_dev, void* stream);
extern "C" int dss2_optim_step_dev(const dss2_optim_desc* descs_host, int n_desc, const dss2_optim_hyper* hyper, float* step_dev, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step_dev")) return rc;
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), n_desc, h = *hyper, step_dev](void* s_) { return dss2_optim_step_dev_launch(dss2::plan_ptr(d), n_desc, h, step_dev, s_); });
  return dss2_optim_step_dev_launch(descs_host, n_desc, *hyper, step_dev, stream);
}
static int dss2_optim_step_dev_launch(const dss2_optim_desc* descs_host, int n_desc, dss2_optim_hyper h, float* step_dev, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_host || !step_dev) { dss2::set_error("optim_step_dev: null argument"); return 2; }
  hipLaunchKernelGGL(dss2::adamax_tick_kernel, dim3(1), dim3(64), 0, dss2::as_stream(stream), step_dev);
  return optim_launch(descs_host, n_desc, h, 1.f, 1.f, 1.f, step_dev, dss2::as_stream(stream));
}

template <int RULE>
static void optim_flat_launch_rule(dim3 grid, const dss2_optim_flat_desc* descs_dev, const float* grad_base, const dss2_optim_hyper& h,
                                   float t, float bc1, float bc2, float* step_dev, uint32_t* counter, hipStream_t s) {
  hipLaunchKernelGGL(dss2::optim_flat_kernel<RULE>, grid, dim3(256), 0, s, descs_dev, grad_base, h, t, bc1, bc2, step_dev, counter);
}

static int dss2_optim_step_flat_launch(const dss2_optim_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, dss2_optim_hyper h, int step, float* step_dev, uint32_t* counter, void* stream);
extern "C" int dss2_optim_step_flat(const dss2_optim_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base,
                                    const dss2_optim_hyper* hyper, int step, float* step_dev, uint32_t* counter, void* stream) {
  if (int rc = optim_hyper_check(hyper, "optim_step_flat")) return rc;
  DSS2_RECORD([descs_dev, n_desc, max_n, grad_base, h = *hyper, step, step_dev, counter](void* s_) { return dss2_optim_step_flat_launch(descs_dev, n_desc, max_n, grad_base, h, step, step_dev, counter, s_); });
  return dss2_optim_step_flat_launch(descs_dev, n_desc, max_n, grad_base, *hyper, step, step_dev, counter, stream);
}
static int dss2_optim_step_flat_launch(const dss2_optim_flat_desc* descs_dev, int n_desc, int64_t max_n, const float* grad_base, dss2_optim_hyper h, int step, float* step_dev, uint32_t* counter, void* stream) {
  if (n_desc <= 0) return 0;
  if (!descs_dev || !grad_base || n_desc > 65535) { dss2::set_error("optim_step_flat: bad arguments"); return 2; }
  if (step < 0 || (step == 0 && (!step_dev || !counter))) { dss2::set_error("optim_step_flat: step >= 1, or step == 0 with step_dev and counter"); return 2; }
  int64_t bx = (max_n + 4095) / 4096;      // few, fat workgroups, as adamax_step_flat
  if (bx > 64) bx = 64;
  if (bx < 1) bx = 1;
  const dim3 grid((unsigned)bx, n_desc);
  const float t = step > 0 ? (float)step : 1.f;
  const float bc1 = step > 0 ? 1.f - powf(h.beta1, t) : 1.f, bc2 = step > 0 ? 1.f - powf(h.beta2, t) : 1.f;
  float* sd = step > 0 ? nullptr : step_dev;
  hipStream_t s = dss2::as_stream(stream);
  switch (h.rule) {
    case DSS2_OPT_ADAM: optim_flat_launch_rule<DSS2_OPT_ADAM>(grid, descs_dev, grad_base, h, t, bc1, bc2, sd, counter, s); break;
    case DSS2_OPT_RMSPROP: optim_flat_launch_rule<DSS2_OPT_RMSPROP>(grid, descs_dev, grad_base, h, t, bc1, bc2, sd, counter, s); break;
    case DSS2_OPT_SGD: optim_flat_launch_rule<DSS2_OPT_SGD>(grid, descs_dev, grad_base, h, t, bc1, bc2, sd, counter, s); break;
    default: optim_flat_launch_rule<DSS2_OPT_ADAMAX>(grid, descs_dev, grad_base, h, t, bc1, bc2, sd, counter, s); break;
  }
  return dss2::check_launch("optim_step_flat");
}

// by-value chunks of a host table, or the whole device table of a flat bucket, for both clipping launches
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

static int dss2_grad_sqsum_partials_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base, int n_desc, int n_wg, double* partials, void* stream);
extern "C" int dss2_grad_sqsum_partials(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base,
                                        int n_desc, int n_wg, double* partials, void* stream) {
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), host = descs_host != nullptr, descs_dev, grad_base, n_desc, n_wg, partials](void* s_) { return dss2_grad_sqsum_partials_launch(host ? d.data() : nullptr, descs_dev, grad_base, n_desc, n_wg, partials, s_); });
  return dss2_grad_sqsum_partials_launch(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, stream);
}
static int dss2_grad_sqsum_partials_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, const float* grad_base, int n_desc, int n_wg, double* partials, void* stream) {
  if (n_desc <= 0) { dss2::set_error("grad_sqsum_partials: no gradients"); return 2; }
  if (int rc = grad_args_check(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, "grad_sqsum_partials")) return rc;
  hipStream_t s = dss2::as_stream(stream);
  dss2::GradTable tab = {};
  if (descs_dev) {
    hipLaunchKernelGGL(dss2::grad_sqsum_kernel, dim3(n_wg), dim3(256), 0, s, tab, descs_dev, grad_base, n_desc, partials);
  } else {
    for (int c0 = 0, c = 0; c0 < n_desc; c0 += dss2::GRAD_CHUNK, ++c) {
      const int n = n_desc - c0 < dss2::GRAD_CHUNK ? n_desc - c0 : dss2::GRAD_CHUNK;
      for (int i = 0; i < n; ++i) tab.d[i] = descs_host[c0 + i];
      hipLaunchKernelGGL(dss2::grad_sqsum_kernel, dim3(n_wg), dim3(256), 0, s, tab, nullptr, nullptr, n, partials + (int64_t)c * n_wg);
    }
  }
  return dss2::check_launch("grad_sqsum_partials");
}

static int dss2_grad_clip_scale_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc, int n_wg, const double* partials, float max_norm, float* norm_out, void* stream);
extern "C" int dss2_grad_clip_scale(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc,
                                    int n_wg, const double* partials, float max_norm, float* norm_out, void* stream) {
  DSS2_RECORD([d = dss2::plan_keep(descs_host, (size_t)(n_desc > 0 ? n_desc : 0)), host = descs_host != nullptr, descs_dev, grad_base, n_desc, n_wg, partials, max_norm, norm_out](void* s_) { return dss2_grad_clip_scale_launch(host ? d.data() : nullptr, descs_dev, grad_base, n_desc, n_wg, partials, max_norm, norm_out, s_); });
  return dss2_grad_clip_scale_launch(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, max_norm, norm_out, stream);
}
static int dss2_grad_clip_scale_launch(const dss2_grad_desc* descs_host, const dss2_grad_flat_desc* descs_dev, float* grad_base, int n_desc, int n_wg, const double* partials, float max_norm, float* norm_out, void* stream) {
  if (n_desc <= 0) { dss2::set_error("grad_clip_scale: no gradients"); return 2; }
  if (int rc = grad_args_check(descs_host, descs_dev, grad_base, n_desc, n_wg, partials, "grad_clip_scale")) return rc;
  if (!norm_out) { dss2::set_error("grad_clip_scale: null norm_out"); return 2; }
  hipStream_t s = dss2::as_stream(stream);
  dss2::GradTable tab = {};
  if (descs_dev) {
    hipLaunchKernelGGL(dss2::grad_clip_scale_kernel, dim3(n_wg), dim3(256), 0, s, tab, descs_dev, grad_base, n_desc, partials, n_wg, max_norm, norm_out);
  } else {
    const int chunks = (n_desc + dss2::GRAD_CHUNK - 1) / dss2::GRAD_CHUNK;
    for (int c0 = 0; c0 < n_desc; c0 += dss2::GRAD_CHUNK) {
      const int n = n_desc - c0 < dss2::GRAD_CHUNK ? n_desc - c0 : dss2::GRAD_CHUNK;
      for (int i = 0; i < n; ++i) tab.d[i] = descs_host[c0 + i];
      hipLaunchKernelGGL(dss2::grad_clip_scale_kernel, dim3(n_wg), dim3(256), 0, s, tab, nullptr, nullptr, n, partials, chunks * n_wg, max_norm, norm_out);
    }
  }
  return dss2::check_launch("grad_clip_scale");
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

static int dss2_rng_next_launch(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream);
extern "C" int dss2_rng_next(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream) {
  DSS2_RECORD([state, snapshot, host_seed, use_host_seed](void* s_) { return dss2_rng_next_launch(state, snapshot, host_seed, use_host_seed, s_); });
  return dss2_rng_next_launch(state, snapshot, host_seed, use_host_seed, stream);
}
static int dss2_rng_next_launch(uint64_t* state, uint64_t* snapshot, uint64_t host_seed, int use_host_seed, void* stream) {
  if (!snapshot || (!use_host_seed && !state)) { dss2::set_error("rng_next: null argument"); return 2; }
  hipLaunchKernelGGL(dss2::rng_next_kernel, dim3(1), dim3(64), 0, dss2::as_stream(stream),
                     reinterpret_cast<unsigned long long*>(state), reinterpret_cast<unsigned long long*>(snapshot),
                     (unsigned long long)host_seed, use_host_seed);
  return dss2::check_launch("rng_next");
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

static int dss2_dropout_mask_launch(const uint64_t* snapshot, int32_t drop_id, float p, int64_t n_rows, int h, float* out, int64_t ldo, void* stream);
extern "C" int dss2_dropout_mask(const uint64_t* snapshot, int32_t drop_id, float p, int64_t n_rows, int h, float* out,
                                 int64_t ldo, void* stream) {
  DSS2_RECORD([=](void* s_) { return dss2_dropout_mask_launch(snapshot, drop_id, p, n_rows, h, out, ldo, s_); });
  return dss2_dropout_mask_launch(snapshot, drop_id, p, n_rows, h, out, ldo, stream);
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

static int dss2_gate_grad_launch(const float* g, const float* y, float* out, int64_t n_rows, int h, const uint64_t* snapshot, int32_t drop_id, float p, int relu, void* stream);
extern "C" int dss2_gate_grad(const float* g, const float* y, float* out, int64_t n_rows, int h, const uint64_t* snapshot, int32_t drop_id, float p, int relu, void* stream) {
  DSS2_RECORD([g, y, out, n_rows, h, snapshot, drop_id, p, relu](void* s_) { return dss2_gate_grad_launch(g, y, out, n_rows, h, snapshot, drop_id, p, relu, s_); });
  return dss2_gate_grad_launch(g, y, out, n_rows, h, snapshot, drop_id, p, relu, stream);
}
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
