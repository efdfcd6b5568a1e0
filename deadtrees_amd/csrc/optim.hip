// Fused global-norm clip + Adam over ONE flat parameter buffer, plus library plumbing.
// Replaces torch.nn.utils.clip_grad_norm_(0.5) (reference configs/trainer/default.yaml:18, applied by
// Lightning) and torch.optim.Adam.step (deadtrees/network/segmodel.py:420-425) — ~47x4 small ATen
// launches per step in the reference — with two HBM-bound passes: read g (norm), then
// read g,m,v,p / write m,v,p.  The clip coefficient and the non-finite-loss skip flag stay on the
// device: no host synchronisation in the step.
#include "conv_host.h"

#include <math.h>
#include <string.h>

static thread_local char g_err[512] = "";

void dt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* dt_last_error(void) { return g_err; }
extern "C" int dt_version(void) { return 100; }
extern "C" int dt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

#define SUMSQ_PER_WG (256 * 4 * 16)

extern "C" int dt_sumsq_rows(int64_t n) { return dt_cdiv(n, SUMSQ_PER_WG); }

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                    double* __restrict__ partial) {
  const int64_t base = (int64_t)blockIdx.x * SUMSQ_PER_WG;
  float s = 0.f;
  for (int it = 0; it < 16; ++it) {
    const int64_t i = base + ((int64_t)it * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    } else {
      for (int64_t j = i; j < n && j < i + 4; ++j) s += g[j] * g[j];
    }
  }
  __shared__ double sh[4];
  const double w = wave_sum_d((double)s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int dt_sumsq(const float* g, int64_t n, double* partial, void* stream) {
  DT_REQUIRE(g && partial && n > 0, "sumsq: bad args");
  DT_REQUIRE((((uintptr_t)g) & 15) == 0, "sumsq: g must be 16-byte aligned");
  hipLaunchKernelGGL(sumsq_kernel, dim3(dt_sumsq_rows(n)), dim3(256), 0, (hipStream_t)stream, g, n, partial);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ partial, int rows,
                                                        float max_norm, float gscale, float* norm,
                                                        float* clipcoef, int32_t* skip) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // gradients in the buffer are gscale * true gradient (e.g. sum over replicas -> gscale = 1/N)
    const float nrm = (float)sqrt(sh[0]) * fabsf(gscale);
    norm[0] = nrm;
    float c = max_norm > 0.f ? max_norm / (nrm + 1e-6f) : 1.f;
    if (c > 1.f) c = 1.f;
    clipcoef[0] = c * gscale;
    // a NaN/Inf anywhere in the gradient (e.g. through BatchNorm statistics of a channel that overflowed while the loss
    // stayed finite) would reach every parameter through the clip coefficient: drop the update instead
    if (skip && !(nrm == nrm && fabsf(nrm) != INFINITY)) skip[0] = 1;
  }
}

extern "C" int dt_clip_coef(const double* partial, int rows, float max_norm, float gscale, float* norm,
                            float* clipcoef, int32_t* skip_flag, void* stream) {
  DT_REQUIRE(partial && norm && clipcoef && rows > 0, "clip_coef: bad args");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, rows, max_norm, gscale,
                     norm, clipcoef, skip_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   float lr, float b1, float b2, float omb1, float omb2, float eps,
                                                   float bc1, float bc2,
                                                   const float* __restrict__ clipcoef,
                                                   const int32_t* __restrict__ skip,
                                                   const float* __restrict__ hyper) {
  if (skip && skip[0] != 0) return;
  if (hyper) {   // per-step scalars read from the device: a captured HIP graph replays with fresh values
    lr = hyper[0];
    bc1 = hyper[1];
    bc2 = hyper[2];
  }
  const float cc = clipcoef ? clipcoef[0] : 1.f;
  const float step = lr / bc1;
  const float rs2 = 1.f / sqrtf(bc2);
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * cc;
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // torch.optim.Adam (single-tensor path): exp_avg.lerp_(grad, 1-b1); exp_avg_sq = b2*v + (1-b2) g^2
      // omb = 1 - beta computed in double on the host like torch's Python scalars (1.f - 0.999f is off by 1.3e-5)
      mm[k] = mm[k] + (gg[k] - mm[k]) * omb1;
      vv[k] = vv[k] * b2 + omb2 * gg[k] * gg[k];
      const float denom = sqrtf(vv[k]) * rs2 + eps;
      pp[k] = pp[k] - step * (mm[k] / denom);
    }
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(p)[i] = pp;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t i = n4 << 2; i < n; ++i) {
      const float gk = g[i] * cc;
      const float mk = m[i] + (gk - m[i]) * omb1;
      const float vk = v[i] * b2 + omb2 * gk * gk;
      m[i] = mk;
      v[i] = vk;
      p[i] = p[i] - step * (mk / (sqrtf(vk) * rs2 + eps));
    }
  }
}

extern "C" int dt_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1,
                            double beta2, float eps, float bias_c1, float bias_c2, const float* clipcoef,
                            const int32_t* skip_flag, void* stream) {
  DT_REQUIRE(p && g && m && v && n > 0 && bias_c1 > 0.f && bias_c2 > 0.f, "adam: bad args");
  DT_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0,
             "adam: buffers must be 16-byte aligned");
  const int grid = dt_ew_grid(n >> 2, 256 * 16);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_c1, bias_c2, clipcoef,
                     skip_flag, (const float*)nullptr);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---- per-step scalars of the optimiser on the device (no ATen algebra, no host sync, HIP-graph capturable)
__global__ void skip_from_loss_kernel(const float* __restrict__ loss, int32_t* __restrict__ skip) {
  const float l = loss[0];
  skip[0] = (l == l && fabsf(l) != INFINITY) ? 0 : 1;
}

extern "C" int dt_skip_from_loss(const float* loss, int32_t* skip_flag, void* stream) {
  DT_REQUIRE(loss && skip_flag, "skip_from_loss: bad args");
  hipLaunchKernelGGL(skip_from_loss_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, skip_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

__global__ void adam_advance_kernel(double* __restrict__ t, const int32_t* __restrict__ skip,
                                    const double* __restrict__ lr, double b1, double b2, float* __restrict__ hyper) {
  double tt = t[0];
  if (!(skip && skip[0] != 0)) tt += 1.0;    // a skipped step leaves the step count alone (torch: no optimizer.step)
  t[0] = tt;
  const double te = tt < 1.0 ? 1.0 : tt;
  hyper[0] = (float)lr[0];
  hyper[1] = (float)(1.0 - pow(b1, te));
  hyper[2] = (float)(1.0 - pow(b2, te));
}

extern "C" int dt_adam_advance(double* t_dev, const int32_t* skip_flag, const double* lr_dev, double beta1, double beta2,
                               float* hyper, void* stream) {
  DT_REQUIRE(t_dev && lr_dev && hyper, "adam_advance: bad args");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t_dev, skip_flag, lr_dev,
                     beta1, beta2, hyper);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                                double beta1, double beta2, float eps, const float* clipcoef, const int32_t* skip_flag,
                                void* stream) {
  DT_REQUIRE(p && g && m && v && hyper && n > 0, "adam_dev: bad args");
  DT_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0,
             "adam_dev: buffers must be 16-byte aligned");
  const int grid = dt_ew_grid(n >> 2, 256 * 16);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, 0.f,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, 1.f, 1.f, clipcoef, skip_flag,
                     hyper);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---- clip + Adam over the TRAINABLE ranges of the flat buffer (frozen encoder: torch.optim.Adam skips a parameter
// whose .grad is None — its m, v and step count do not move — and clip_grad_norm_ sees only parameters with a gradient).
// Range table (device, int64 [4 * nranges]): (lo, hi, first partial row, segment).  lo / hi are multiples of 4 (the
// flat layout aligns every tensor to 4 floats); `segment` indexes the per-segment step counts t_seg[] and the bias
// corrections hyper_seg[3 * segment ..]: every range carries its own count, so a range that was frozen for k steps
// starts its first update with the step-1 bias correction.  Frozen ranges are neither read nor written.

__device__ __forceinline__ int rg_find(const int64_t* __restrict__ table, int nranges, int64_t row) {
  int r = 0;
  while (r + 1 < nranges && table[4 * (r + 1) + 2] <= row) ++r;
  return r;
}

__global__ __launch_bounds__(256) void sumsq_ranges_kernel(const float* __restrict__ g, const int64_t* __restrict__ table,
                                                           int nranges, double* __restrict__ partial) {
  const int r = rg_find(table, nranges, blockIdx.x);
  const int64_t lo = table[4 * r], hi = table[4 * r + 1];
  const int64_t base = lo + ((int64_t)blockIdx.x - table[4 * r + 2]) * SUMSQ_PER_WG;
  float s = 0.f;
  for (int it = 0; it < 16; ++it) {
    const int64_t i = base + ((int64_t)it * 256 + threadIdx.x) * 4;
    if (i + 3 < hi) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
      s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    } else {
      for (int64_t j = i; j < hi && j < i + 4; ++j) s += g[j] * g[j];
    }
  }
  __shared__ double sh[4];
  const double w = wave_sum_d((double)s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int dt_sumsq_ranges(const float* g, const int64_t* table, int nranges, int rows, double* partial,
                               void* stream) {
  DT_REQUIRE(g && table && partial && nranges > 0 && rows > 0, "sumsq_ranges: bad args");
  DT_REQUIRE((((uintptr_t)g) & 15) == 0, "sumsq_ranges: g must be 16-byte aligned");
  hipLaunchKernelGGL(sumsq_ranges_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, g, table, nranges,
                     partial);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

__global__ void adam_advance_ranges_kernel(double* __restrict__ t_seg, const int64_t* __restrict__ table, int nranges,
                                           const int32_t* __restrict__ skip, const double* __restrict__ lr, double b1,
                                           double b2, float* __restrict__ hyper_seg) {
  const int r = threadIdx.x;
  if (r >= nranges) return;
  const int s = (int)table[4 * r + 3];
  double tt = t_seg[s];
  if (!(skip && skip[0] != 0)) tt += 1.0;
  t_seg[s] = tt;
  const double te = tt < 1.0 ? 1.0 : tt;
  hyper_seg[3 * s + 0] = (float)lr[0];
  hyper_seg[3 * s + 1] = (float)(1.0 - pow(b1, te));
  hyper_seg[3 * s + 2] = (float)(1.0 - pow(b2, te));
}

extern "C" int dt_adam_advance_ranges(double* t_seg, const int64_t* table, int nranges, const int32_t* skip_flag,
                                      const double* lr_dev, double beta1, double beta2, float* hyper_seg, void* stream) {
  DT_REQUIRE(t_seg && table && lr_dev && hyper_seg && nranges > 0 && nranges <= 64, "adam_advance_ranges: bad args");
  hipLaunchKernelGGL(adam_advance_ranges_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t_seg, table, nranges,
                     skip_flag, lr_dev, beta1, beta2, hyper_seg);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// grid (x: element blocks of the longest range, y: range); the body is adam_kernel's arithmetic
__global__ __launch_bounds__(256) void adam_ranges_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          const int64_t* __restrict__ table, float b2, float omb1,
                                                          float omb2, float eps, const float* __restrict__ clipcoef,
                                                          const int32_t* __restrict__ skip,
                                                          const float* __restrict__ hyper_seg) {
  if (skip && skip[0] != 0) return;
  const int r = blockIdx.y;
  const int64_t lo = table[4 * r], hi = table[4 * r + 1];
  const int s = (int)table[4 * r + 3];
  const float cc = clipcoef ? clipcoef[0] : 1.f;
  const float step = hyper_seg[3 * s] / hyper_seg[3 * s + 1];
  const float rs2 = 1.f / sqrtf(hyper_seg[3 * s + 2]);
  const int64_t n4 = (hi - lo) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + lo);
  f32x4* m4 = reinterpret_cast<f32x4*>(m + lo);
  f32x4* v4 = reinterpret_cast<f32x4*>(v + lo);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + lo);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 gg = g4[i] * cc;
    f32x4 mm = m4[i];
    f32x4 vv = v4[i];
    f32x4 pp = p4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mm[k] = mm[k] + (gg[k] - mm[k]) * omb1;
      vv[k] = vv[k] * b2 + omb2 * gg[k] * gg[k];
      const float denom = sqrtf(vv[k]) * rs2 + eps;
      pp[k] = pp[k] - step * (mm[k] / denom);
    }
    m4[i] = mm;
    v4[i] = vv;
    p4[i] = pp;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t i = lo + (n4 << 2); i < hi; ++i) {
      const float gk = g[i] * cc;
      const float mk = m[i] + (gk - m[i]) * omb1;
      const float vk = v[i] * b2 + omb2 * gk * gk;
      m[i] = mk;
      v[i] = vk;
      p[i] = p[i] - step * (mk / (sqrtf(vk) * rs2 + eps));
    }
  }
}

extern "C" int dt_adam_step_ranges(float* p, const float* g, float* m, float* v, const int64_t* table, int nranges,
                                   int64_t max_len, const float* hyper_seg, double beta1, double beta2, float eps,
                                   const float* clipcoef, const int32_t* skip_flag, void* stream) {
  DT_REQUIRE(p && g && m && v && table && hyper_seg && nranges > 0 && nranges <= 65535 && max_len > 0,
             "adam_ranges: bad args");
  DT_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0,
             "adam_ranges: buffers must be 16-byte aligned");
  int64_t grid = ((max_len >> 2) + 255) / 256;
  if (grid > 256 * 16 / nranges) grid = 256 * 16 / nranges;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adam_ranges_kernel, dim3((unsigned)grid, (unsigned)nranges), dim3(256), 0, (hipStream_t)stream, p, g,
                     m, v, table, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, clipcoef, skip_flag,
                     hyper_seg);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---- averaged copy of the flat parameter buffer (torch.optim.swa_utils.AveragedModel: get_swa_multi_avg_fn /
// get_ema_multi_avg_fn).  The number of averaged models lives on the device and is advanced there, like t_dev of
// dt_adam_advance: one thread bumps it (unless the step is skipped), then the streaming pass reads the NEW count, so
// every workgroup sees the same value whatever order they run in.  Same launches for every update: capturable.
__global__ void weight_average_advance_kernel(int64_t* __restrict__ count, const int32_t* __restrict__ skip) {
  if (!(skip && skip[0] != 0)) count[0] = count[0] + 1;
}

__device__ __forceinline__ float wavg_one(float a, float p, int mode, float div, float omd) {
  // SWA: avg + (p - avg) / (n + 1); EMA: avg.lerp(p, 1 - decay) (weight < 0.5 form: avg + w * (p - avg))
  return mode == DT_AVG_SWA ? a + (p - a) / div : a + (p - a) * omd;
}

__global__ __launch_bounds__(256) void weight_average_kernel(float* __restrict__ avg, const float* __restrict__ p,
                                                             int64_t n, const int64_t* __restrict__ count,
                                                             const int32_t* __restrict__ skip, int mode, float omd) {
  if (skip && skip[0] != 0) return;
  const int64_t cnt = count[0];            // already advanced: this is model number cnt
  const bool first = cnt <= 1;
  const float div = (float)cnt;
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
    f32x4 aa = pp;
    if (!first) {
      aa = reinterpret_cast<const f32x4*>(avg)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) aa[k] = wavg_one(aa[k], pp[k], mode, div, omd);
    }
    reinterpret_cast<f32x4*>(avg)[i] = aa;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t i = n4 << 2; i < n; ++i) avg[i] = first ? p[i] : wavg_one(avg[i], p[i], mode, div, omd);
  }
}

extern "C" int dt_weight_average(float* avg, const float* p, int64_t n, int64_t* count_dev, const int32_t* skip_flag,
                                 int mode, double decay, void* stream) {
  DT_REQUIRE(avg && p && count_dev && n > 0, "weight_average: bad args");
  DT_REQUIRE(mode == DT_AVG_SWA || mode == DT_AVG_EMA, "weight_average: mode %d (DT_AVG_SWA or DT_AVG_EMA)", mode);
  DT_REQUIRE(mode != DT_AVG_EMA || (decay >= 0.0 && decay <= 1.0), "weight_average: decay %g outside [0, 1]", decay);
  DT_REQUIRE(((((uintptr_t)avg) | ((uintptr_t)p)) & 15) == 0, "weight_average: buffers must be 16-byte aligned");
  const int grid = dt_ew_grid(n >> 2, 256 * 16);
  hipLaunchKernelGGL(weight_average_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, count_dev, skip_flag);
  DT_LAUNCH_CHECK();
  hipLaunchKernelGGL(weight_average_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, avg, p, n,
                     (const int64_t*)count_dev, skip_flag, mode, (float)(1.0 - decay));
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// cumulative moving average of BatchNorm statistics (momentum=None in torch: factor 1 / num_batches_tracked): the batch
// count and the momentum dt_bn_finalize_dev reads stay on the device, so a captured recalibration pass replays
__global__ void cma_advance_kernel(int64_t* __restrict__ n, float* __restrict__ momentum) {
  const int64_t k = n[0] + 1;
  n[0] = k;
  momentum[0] = (float)(1.0 / (double)k);
}

extern "C" int dt_cma_advance(int64_t* n_dev, float* momentum_dev, void* stream) {
  DT_REQUIRE(n_dev && momentum_dev, "cma_advance: bad args");
  hipLaunchKernelGGL(cma_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, n_dev, momentum_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
