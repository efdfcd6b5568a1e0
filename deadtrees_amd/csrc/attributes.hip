// Patch attributes (deployment/attributes.py holds the contract): per patch of a label plane the sums, sums of squares,
// minima and maxima of the bands of a planar uint8 raster, the sums of the quantised normalised differences of up to four
// band pairs and, with probabilities, the sum and the minimum of the quantised probability of the pixel's own class.
// Integers only; a sum, a minimum and a maximum do not depend on the order of their terms, so the tables are a pure
// function of the inputs.
//
// One init launch presets the table rows, one pass walks the pixels.  A wave owns AT_SPAN consecutive 64-pixel chunks of
// the row-major plane (the walk of patch_areas_kernel): the runs of equal label in a chunk are found with pt_runs — a run
// may wrap a row end, nothing here is geometry —, every quantity is reduced per run by a segmented scan across the wave
// (32-bit partials: 64 terms of at most 255^2 or 65535), the run still open at the end of a chunk is carried into the next
// one in 64 bits, and a finished run issues ONE atomic per quantity into its table row.  All quantities scan in step and
// only labelled lanes take partners, so the steps end with the longest labelled run of the chunk; a chunk of background
// loads no band and scans nothing.  No workgroup waits for another, no scalar leaves the device.
#include <limits.h>

#include "conv_host.h"
#include "patch_runs.h"

#define AT_SPAN 16                       // 64-pixel chunks per wave
#define AT_MAXC 8                        // bands
#define AT_MAXI 4                        // band pairs
#define AT_MAXK 8                        // classes
#define AT_MAX_SIDE 16384
#define AT_MAX_PIXELS 2147483646ll       // labels are int32 and 1-based
#define AT_T_ZERO 32767u                 // the quantised normalised difference of a pixel with v_a + v_b == 0

struct at_add {
  __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a + b; }
};
struct at_min {
  __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return min(a, b); }
};
struct at_max {
  __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); }
};

// one step of a segmented scan: after the steps with distances 1, 2, .. d a lane that takes part holds its quantity over its
// next min(2d, reach) lanes.  take == d < reach, and reach never leaves the wave, so lane + d is a lane of it
template <int N, class Op>
__device__ __forceinline__ void at_step(unsigned (&v)[N], int d, bool take, Op op) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const unsigned other = __shfl_down(v[q], d, 64);
    if (take) v[q] = op(v[q], other);
  }
}

// what a lane does with the quantities of its run in this chunk.  merge: lane 0 continues the carried run; carry_row >= 0:
// lane 0 writes the carried run out (it ended with the previous chunk); run_row >= 0: a head lane writes its finished run
struct at_plan {
  int last_head;
  bool merge;
  int carry_row, run_row;
};

// v: the quantity over the lane's run in this chunk (valid in head lanes)
__device__ __forceinline__ void at_sum(const at_plan& p, unsigned v, unsigned long long& carry,
                                       unsigned long long* __restrict__ sums, int Q, int q) {
  unsigned long long s = v;
  if (p.merge) s += carry;
  if (p.carry_row >= 0) atomicAdd(&sums[(int64_t)p.carry_row * Q + q], carry);
  if (p.run_row >= 0) atomicAdd(&sums[(int64_t)p.run_row * Q + q], s);
  carry = __shfl(s, p.last_head, 64);
}
__device__ __forceinline__ void at_low(const at_plan& p, unsigned v, int& carry, int32_t* __restrict__ ext, int M, int m) {
  int s = (int)v;
  if (p.merge) s = min(s, carry);
  if (p.carry_row >= 0) atomicMin(&ext[(int64_t)p.carry_row * M + m], carry);
  if (p.run_row >= 0) atomicMin(&ext[(int64_t)p.run_row * M + m], s);
  carry = __shfl(s, p.last_head, 64);
}
__device__ __forceinline__ void at_high(const at_plan& p, unsigned v, int& carry, int32_t* __restrict__ ext, int M, int m) {
  int s = (int)v;
  if (p.merge) s = max(s, carry);
  if (p.carry_row >= 0) atomicMax(&ext[(int64_t)p.carry_row * M + m], carry);
  if (p.run_row >= 0) atomicMax(&ext[(int64_t)p.run_row * M + m], s);
  carry = __shfl(s, p.last_head, 64);
}

// the table row of a label, -1 for a root the dense plane does not know
__device__ __forceinline__ int at_row(const int32_t* __restrict__ dense, int label, int rows) {
  const int row = dense[label - 1];
  return (unsigned)row < (unsigned)rows ? row : -1;
}

// columns of a sums row: band sums [0, C), sums of squares [C, 2C), pair sums [2C, 2C + I), the confidence sum 2C + I;
// of an extremes row: band minima [0, C), maxima [C, 2C), the confidence minimum 2C
__global__ __launch_bounds__(256) void attribute_init_kernel(int rows, int C, int Q, int M, int64_t* __restrict__ sums,
                                                             int32_t* __restrict__ ext) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t W = Q + M;
  if (t >= rows * W) return;
  const int64_t r = t / W;
  const int k = (int)(t % W);
  if (k < Q) {
    sums[r * Q + k] = 0;
  } else {
    const int m = k - Q;
    ext[r * M + m] = m < C ? 255 : m < 2 * C ? 0 : 65535;
  }
}

// pair k reads the bands (pa >> 4k) & 15 and (pb >> 4k) & 15
template <int C, bool CONF>
__global__ __launch_bounds__(256) void patch_attributes_kernel(const int32_t* __restrict__ labels,
                                                               const uint8_t* __restrict__ raster, int64_t n,
                                                               const int32_t* __restrict__ dense, int rows,
                                                               const uint8_t* __restrict__ classes,
                                                               const float* __restrict__ probs, int K, int I, unsigned pa,
                                                               unsigned pb, unsigned long long* __restrict__ sums,
                                                               int32_t* __restrict__ ext) {
  const int Q = 2 * C + I + (CONF ? 1 : 0), M = 2 * C + (CONF ? 1 : 0);
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (AT_SPAN * 64);
  int carry_label = 0;                                    // wave-uniform: the run left open by the previous chunk
  unsigned long long c_sum[C], c_sq[C], c_pair[AT_MAXI], c_conf = 0;
  int c_min[C], c_max[C], c_cmin = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) c_sum[c] = c_sq[c] = 0, c_min[c] = c_max[c] = 0;
#pragma unroll
  for (int k = 0; k < AT_MAXI; ++k) c_pair[k] = 0;
  // lane 0 writes the carried run out: behind a wave's last chunk, and in front of a chunk without a labelled pixel
  auto flush_carry = [&]() {
    const int row = at_row(dense, carry_label, rows);
    if (row < 0) return;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      atomicAdd(&sums[(int64_t)row * Q + c], c_sum[c]);
      atomicAdd(&sums[(int64_t)row * Q + C + c], c_sq[c]);
      atomicMin(&ext[(int64_t)row * M + c], c_min[c]);
      atomicMax(&ext[(int64_t)row * M + C + c], c_max[c]);
    }
#pragma unroll
    for (int k = 0; k < AT_MAXI; ++k)
      if (k < I) atomicAdd(&sums[(int64_t)row * Q + 2 * C + k], c_pair[k]);
    if (CONF) {
      atomicAdd(&sums[(int64_t)row * Q + 2 * C + I], c_conf);
      atomicMin(&ext[(int64_t)row * M + 2 * C], c_cmin);
    }
  };
  for (int j = 0; j < AT_SPAN; ++j) {
    const int64_t i = base + j * 64 + lane;
    if (i - lane >= n) break;
    const int label = pt_label_at(labels, i, n);
    if (__ballot(label != 0) == 0) {                      // background only, most chunks of a real map: no band is loaded
      if (lane == 0 && carry_label) flush_carry();
      carry_label = 0;
      continue;
    }
    // this lane's terms: band values twice (sum, minimum, maximum start from them), their squares, the pairs' t, and q
    unsigned add[2 * C], low[C], high[C], pair[AT_MAXI], conf[1] = {0u}, conf_low[1];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      add[c] = low[c] = high[c] = i < n ? raster[(int64_t)c * n + i] : 0u;
      add[C + c] = add[c] * add[c];
    }
#pragma unroll
    for (int k = 0; k < AT_MAXI; ++k) {
      pair[k] = 0;
      if (k >= I) continue;
      const unsigned a = (pa >> (4 * k)) & 15u, b = (pb >> (4 * k)) & 15u;
      unsigned va = 0, vb = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        va = a == (unsigned)c ? add[c] : va;
        vb = b == (unsigned)c ? add[c] : vb;
      }
      const unsigned s = va + vb;
      pair[k] = s ? (va * 65534u + (s >> 1)) / s : AT_T_ZERO;
    }
    if (CONF && label) {
      const int cls = classes[i];
      const float p = cls < K ? probs[(int64_t)cls * n + i] : 0.f;
      const float clipped = fminf(p > 0.f ? p : 0.f, 1.f);                          // NaN -> 0
      conf[0] = (unsigned)floorf(__fadd_rn(__fmul_rn(clipped, 65535.f), 0.5f));      // two roundings, never fused
    }
    conf_low[0] = conf[0];
    bool head;
    int len;
    at_plan plan;
    uint64_t heads;
    pt_runs(label, false, lane, head, len, heads);       // len: the distance to the next head, in every lane
    // every quantity over the lanes lane .. lane + len - 1, all in step; background is never written out, so its lanes take
    // no partner and the steps end with the longest labelled run of the chunk
    const int reach = label ? len : 1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = d < reach;
      if (__ballot(take) == 0) break;
      at_step(add, d, take, at_add());
      at_step(low, d, take, at_min());
      at_step(high, d, take, at_max());
#pragma unroll
      for (int k = 0; k < AT_MAXI; ++k)
        if (k < I) {
          const unsigned other = __shfl_down(pair[k], d, 64);
          if (take) pair[k] += other;
        }
      if (CONF) {
        at_step(conf, d, take, at_add());
        at_step(conf_low, d, take, at_min());
      }
    }
    const int first = __shfl(label, 0, 64);
    plan.last_head = 63 - __clzll((long long)heads);
    plan.merge = lane == 0 && carry_label == first;
    plan.carry_row = lane == 0 && carry_label && carry_label != first ? at_row(dense, carry_label, rows) : -1;
    plan.run_row = head && lane != plan.last_head && label ? at_row(dense, label, rows) : -1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      at_sum(plan, add[c], c_sum[c], sums, Q, c);
      at_sum(plan, add[C + c], c_sq[c], sums, Q, C + c);
      at_low(plan, low[c], c_min[c], ext, M, c);
      at_high(plan, high[c], c_max[c], ext, M, C + c);
    }
#pragma unroll
    for (int k = 0; k < AT_MAXI; ++k)
      if (k < I) at_sum(plan, pair[k], c_pair[k], sums, Q, 2 * C + k);
    if (CONF) {
      at_sum(plan, conf[0], c_conf, sums, Q, 2 * C + I);
      at_low(plan, conf_low[0], c_cmin, ext, M, 2 * C);
    }
    carry_label = __shfl(label, plan.last_head, 64);
  }
  if (lane == 0 && carry_label) flush_carry();
}

// ---------------------------------------------------------------- entry points
extern "C" int dt_attribute_span(int* chunks) {
  DT_REQUIRE(chunks, "attribute_span: null pointer");
  *chunks = AT_SPAN;
  return DT_OK;
}

template <int C>
static void at_launch(bool conf, dim3 grid, hipStream_t st, const int32_t* labels, const uint8_t* raster, int64_t pixels,
                      const int32_t* dense, int n, const uint8_t* classes, const float* probs, int K, int I, unsigned pa,
                      unsigned pb, int64_t* sums, int32_t* ext) {
  if (conf)
    hipLaunchKernelGGL((patch_attributes_kernel<C, true>), grid, dim3(256), 0, st, labels, raster, pixels, dense, n, classes,
                       probs, K, I, pa, pb, (unsigned long long*)sums, ext);
  else
    hipLaunchKernelGGL((patch_attributes_kernel<C, false>), grid, dim3(256), 0, st, labels, raster, pixels, dense, n, classes,
                       probs, K, I, pa, pb, (unsigned long long*)sums, ext);
}

extern "C" int dt_patch_attributes_u8(const int32_t* labels, const uint8_t* raster, int C, int h, int w,
                                      const int32_t* dense_plane, int n, const uint8_t* classes, const float* probs, int K,
                                      const int* pairs, int n_pairs, int64_t* sums, int32_t* extremes, void* stream) {
  DT_REQUIRE(labels && raster && dense_plane, "patch_attributes_u8: null pointer");
  DT_REQUIRE(h >= 1 && w >= 1 && h <= AT_MAX_SIDE && w <= AT_MAX_SIDE && (int64_t)h * w <= AT_MAX_PIXELS,
             "patch_attributes_u8: raster %dx%d: sides must be in 1..%d and h * w <= 2^31 - 2", h, w, AT_MAX_SIDE);
  DT_REQUIRE(C >= 1 && C <= AT_MAXC, "patch_attributes_u8: C=%d bands unsupported (1..%d)", C, AT_MAXC);
  DT_REQUIRE(n_pairs >= 0 && n_pairs <= AT_MAXI && (n_pairs == 0 || pairs), "patch_attributes_u8: %d band pairs (0..%d)",
             n_pairs, AT_MAXI);
  DT_REQUIRE((classes == nullptr) == (probs == nullptr), "patch_attributes_u8: probabilities come with their class map");
  DT_REQUIRE(probs == nullptr || (K >= 2 && K <= AT_MAXK), "patch_attributes_u8: K=%d unsupported (2..%d)", K, AT_MAXK);
  const int64_t pixels = (int64_t)h * w;
  DT_REQUIRE(n >= 0 && n <= pixels, "patch_attributes_u8: n=%d rows for %lld pixels", n, (long long)pixels);
  unsigned pa = 0, pb = 0;
  for (int k = 0; k < n_pairs; ++k) {
    DT_REQUIRE(pairs[2 * k] >= 0 && pairs[2 * k] < C && pairs[2 * k + 1] >= 0 && pairs[2 * k + 1] < C,
               "patch_attributes_u8: pair %d names the bands (%d, %d) of a %d-band raster", k, pairs[2 * k], pairs[2 * k + 1], C);
    pa |= (unsigned)pairs[2 * k] << (4 * k);
    pb |= (unsigned)pairs[2 * k + 1] << (4 * k);
  }
  if (n == 0) return DT_OK;
  DT_REQUIRE(sums && extremes, "patch_attributes_u8: null table");
  const bool conf = probs != nullptr;
  const int Q = 2 * C + n_pairs + (conf ? 1 : 0), M = 2 * C + (conf ? 1 : 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attribute_init_kernel, dim3((unsigned)(((int64_t)n * (Q + M) + 255) / 256)), dim3(256), 0, st, n, C, Q, M,
                     sums, extremes);
  const dim3 grid((unsigned)((pixels + 4 * AT_SPAN * 64 - 1) / (4 * AT_SPAN * 64)));
#define AT_CASE(c) \
  case c: at_launch<c>(conf, grid, st, labels, raster, pixels, dense_plane, n, classes, probs, K, n_pairs, pa, pb, sums, extremes); break
  switch (C) {
    AT_CASE(1);
    AT_CASE(2);
    AT_CASE(3);
    AT_CASE(4);
    AT_CASE(5);
    AT_CASE(6);
    AT_CASE(7);
    AT_CASE(8);
  }
#undef AT_CASE
  DT_LAUNCH_CHECK();
  return DT_OK;
}
