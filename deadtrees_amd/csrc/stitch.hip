// Overlap-stitched tiled inference (BASELINE configs[5] "overlap-stitch"; the reference has none): the windowed
// input gather and the blend of the overlapping windows' predictions into the raster, all on the device.
//
// Geometry (one definition: stitch_windows below, deployment/tiler.py::window_grid restates it in numpy and
// tests/test_overlap_stitch_host.py compares the two).  d = window edge, o = overlap (even, 0 <= o <= d/2), s = d - o the
// stride; an axis of length L carries n(L) = max(1, ceil((L - o) / s)) windows, window k = i * nx + j has its origin at
// (i * s, j * s) (row-major), pixels beyond the raster are the tiler's zero byte.  o <= d/2 means d <= 2s: a raster pixel
// lies in at most 2 windows per axis, 4 in all.  At o = 0 this is the d x d block grid of dt_split_normalize_u8.
//
// All four kernels stream: one thread per pixel in a grid-stride loop, coalesced along x, no atomics, no LDS.
#include "conv_host.h"

#define ST_CAP (256 * 16)   // grid cap, as EW_CAP of elementwise.hip: 16 workgroups per CU, grid-stride beyond

static inline int stitch_windows(int L, int d, int o) {
  const int s = d - o;
  const int n = (L - o + s - 1) / s;
  return n > 1 ? n : 1;
}
static inline bool stitch_geometry_ok(int d, int o) { return d > 0 && o >= 0 && (o & 1) == 0 && 2 * o <= d; }

extern "C" int dt_stitch_window_count(int L, int d, int overlap) {
  DT_REQUIRE(L > 0 && d > 0, "stitch_window_count: bad sizes");
  DT_REQUIRE(overlap >= 0 && (overlap & 1) == 0, "stitch_window_count: overlap must be even and >= 0");
  DT_REQUIRE(2 * overlap <= d, "stitch_window_count: overlap must be <= d/2");
  return stitch_windows(L, d, overlap);
}

// ------------------------------------------------------------------ input gather
// deployment/tiler.py:121-134 + utils/data_handling.py:9-20 (zero-pad the raster, cut it into d x d windows in row-major
// order) + scripts/inference.py:94-96 (albumentations Normalize per sub-tile) as ONE gather: raster uint8 [Cs][h][w]
// (band-major, what rioxarray hands over) -> fp32 NHWC windows [count][d][d][Cd], windows first .. first + count - 1 of the
// nwx-wide grid with origins `stride` apart.  stride == d is the non-overlapping block split (dt_split_normalize_u8 calls
// this with it).  One thread per output pixel: Cd byte loads (coalesced along x per band), Cd dword stores.
__global__ __launch_bounds__(256) void window_normalize_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                                  int h, int w, int d, int wstride, int nwx, int first,
                                                                  int64_t n_pix, int Cd, f32x4 mean, f32x4 stdv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t plane = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const int x = (int)(i % d), y = (int)((i / d) % d), blk = first + (int)(i / ((int64_t)d * d));
    const int gy = (blk / nwx) * wstride + y, gx = (blk % nwx) * wstride + x;
    const bool in = gy < h && gx < w;
    for (int c = 0; c < Cd; ++c) {
      const float v = in ? (float)src[c * plane + (int64_t)gy * w + gx] : 0.f;
      dst[i * Cd + c] = (v - mean[c] * 255.f) * (1.f / (stdv[c] * 255.f));   // the arithmetic of normalize_u8_kernel
    }
  }
}

extern "C" int dt_window_normalize_u8(const uint8_t* raster_chw, float* dst_nhwc, int Csrc, int h, int w, int d, int stride,
                                      int nwx, int first, int count, int Cdst, const float* mean, const float* stdv,
                                      void* stream) {
  DT_REQUIRE(raster_chw && dst_nhwc && mean && stdv && h > 0 && w > 0 && d > 0 && nwx > 0 && first >= 0 && count > 0 &&
                 Cdst > 0 && Cdst <= 4 && Cdst <= Csrc,
             "window_normalize_u8: bad args");
  DT_REQUIRE(stride > 0 && stride <= d, "window_normalize_u8: stride must be in (0, d]");
  const int o = d - stride;
  DT_REQUIRE((o & 1) == 0, "window_normalize_u8: overlap d - stride must be even");
  DT_REQUIRE(2 * o <= d, "window_normalize_u8: overlap d - stride must be <= d/2");
  DT_REQUIRE(nwx == stitch_windows(w, d, o), "window_normalize_u8: nwx is not the window count of the raster width");
  DT_REQUIRE((int64_t)first + count <= (int64_t)stitch_windows(h, d, o) * nwx,
             "window_normalize_u8: window range outside the grid");
  f32x4 m = {0, 0, 0, 0}, s = {1, 1, 1, 1};
  for (int c = 0; c < Cdst; ++c) {
    m[c] = mean[c];
    s[c] = stdv[c];
  }
  const int64_t n_pix = (int64_t)count * d * d;
  hipLaunchKernelGGL(window_normalize_u8_kernel, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0, (hipStream_t)stream,
                     raster_chw, dst_nhwc, h, w, d, stride, nwx, first, n_pix, Cdst, m, s);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ------------------------------------------------------------------ average mode: blend of the windows' class probabilities
// Blend weight of window pixel (y, x): r(y) * r(x), r(t) = min(1, (t + 1) / (o + 1), (d - t) / (o + 1)) — a linear ramp over
// the o pixels a window shares with its neighbour; the two ramps of an overlap sum to 1.
__device__ __forceinline__ float stitch_ramp(int t, int d, int o) {
  const float q = (float)(o + 1);
  return fminf(1.f, fminf((float)(t + 1) / q, (float)(d - t) / q));
}

// Gather form: one thread owns one raster pixel of the rows [row0, row0 + n_pix / w) and visits the (at most 2 x 2) windows
// that cover it, in ascending window index; the windows outside first .. first + count - 1 are not in this call's logits and
// are skipped.  Per visited window: softmax over K (accurate expf, max subtracted), acc[k] += weight * p_k.  Every pixel's
// sum is thus built in ONE order, one fp32 add per window, whatever the batch size and however the windows are split into
// calls (calls in ascending window order): the accumulator is bit-identical across batchings.
// logits fp32 NCHW [count][K][d][d]; acc fp32 planar [K][h][w], zeroed before the first call.
template <int K>
__global__ __launch_bounds__(256) void stitch_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ acc,
                                                                int h, int w, int d, int o, int ny, int nx, int first,
                                                                int count, int row0, int64_t n_pix) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t plane = (int64_t)h * w, wplane = (int64_t)d * d;
  const int s = d - o;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const int gx = (int)(i % w), gy = row0 + (int)(i / w);
    const int iy1 = min(gy / s, ny - 1), ix1 = min(gx / s, nx - 1);
    const int iy0 = (iy1 > 0 && gy < (iy1 - 1) * s + d) ? iy1 - 1 : iy1;
    const int ix0 = (ix1 > 0 && gx < (ix1 - 1) * s + d) ? ix1 - 1 : ix1;
    const int64_t pix = (int64_t)gy * w + gx;
    float a[K];
    bool touched = false;
    for (int iy = iy0; iy <= iy1; ++iy) {
      for (int ix = ix0; ix <= ix1; ++ix) {
        const int k = iy * nx + ix - first;
        if (k < 0 || k >= count) continue;
        if (!touched) {
#pragma unroll
          for (int c = 0; c < K; ++c) a[c] = acc[c * plane + pix];
          touched = true;
        }
        const int y = gy - iy * s, x = gx - ix * s;
        const float* p = logits + (int64_t)k * K * wplane + (int64_t)y * d + x;
        float l[K];
#pragma unroll
        for (int c = 0; c < K; ++c) l[c] = p[c * wplane];
        float mx = l[0];
#pragma unroll
        for (int c = 1; c < K; ++c) mx = fmaxf(mx, l[c]);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
          l[c] = expf(l[c] - mx);
          sum += l[c];
        }
        const float wgt = stitch_ramp(y, d, o) * stitch_ramp(x, d, o);
#pragma unroll
        for (int c = 0; c < K; ++c) a[c] += wgt * (l[c] / sum);
      }
    }
    if (touched) {
#pragma unroll
      for (int c = 0; c < K; ++c) acc[c * plane + pix] = a[c];
    }
  }
}

extern "C" int dt_stitch_accumulate(const float* logits, float* acc, int K, int h, int w, int d, int overlap, int first,
                                    int count, void* stream) {
  DT_REQUIRE(logits && acc && h > 0 && w > 0 && d > 0 && first >= 0 && count > 0, "stitch_accumulate: bad args");
  DT_REQUIRE(K >= 1 && K <= 4, "stitch_accumulate: K must be in 1..4");
  DT_REQUIRE(overlap >= 0 && (overlap & 1) == 0, "stitch_accumulate: overlap must be even and >= 0");
  DT_REQUIRE(2 * overlap <= d, "stitch_accumulate: overlap must be <= d/2");
  const int ny = stitch_windows(h, d, overlap), nx = stitch_windows(w, d, overlap), s = d - overlap;
  DT_REQUIRE((int64_t)first + count <= (int64_t)ny * nx, "stitch_accumulate: window range outside the grid");
  // only the raster rows under this batch's window rows
  const int row0 = (first / nx) * s;
  const int64_t row1_full = (int64_t)((first + count - 1) / nx) * s + d;
  const int row1 = row1_full < h ? (int)row1_full : h;
  const int64_t n_pix = (int64_t)(row1 - row0) * w;
  const dim3 grid(dt_ew_grid(n_pix, ST_CAP)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define ST_ACC(KK)                                                                                                      \
  hipLaunchKernelGGL(stitch_accumulate_kernel<KK>, grid, block, 0, st, logits, acc, h, w, d, overlap, ny, nx, first, count, \
                     row0, n_pix)
  switch (K) {
    case 1: ST_ACC(1); break;
    case 2: ST_ACC(2); break;
    case 3: ST_ACC(3); break;
    default: ST_ACC(4); break;
  }
#undef ST_ACC
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// Class map of the accumulator: argmax over k, ties -> lowest index (strict >, the head kernel's rule); probs (optional,
// fp32 [K][h][w]) = acc_k / sum_k acc.  Every raster pixel lies in a window with weight >= 1 / (o + 1)^2, so the sum of a
// completed accumulator is > 0.
template <int K>
__global__ __launch_bounds__(256) void stitch_finalize_kernel(const float* __restrict__ acc, uint8_t* __restrict__ classes,
                                                              float* __restrict__ probs, int64_t n_pix) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    float a[K];
#pragma unroll
    for (int c = 0; c < K; ++c) a[c] = acc[c * n_pix + i];
    int best = 0;
    float bv = a[0], sum = a[0];
#pragma unroll
    for (int c = 1; c < K; ++c) {
      sum += a[c];
      if (a[c] > bv) {
        bv = a[c];
        best = c;
      }
    }
    classes[i] = (uint8_t)best;
    if (probs) {
#pragma unroll
      for (int c = 0; c < K; ++c) probs[c * n_pix + i] = a[c] / sum;
    }
  }
}

extern "C" int dt_stitch_finalize(const float* acc, uint8_t* classes, float* probs, int K, int h, int w, void* stream) {
  DT_REQUIRE(acc && classes && h > 0 && w > 0, "stitch_finalize: bad args");
  DT_REQUIRE(K >= 1 && K <= 4, "stitch_finalize: K must be in 1..4");
  const int64_t n_pix = (int64_t)h * w;
  const dim3 grid(dt_ew_grid(n_pix, ST_CAP)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define ST_FIN(KK) hipLaunchKernelGGL(stitch_finalize_kernel<KK>, grid, block, 0, st, acc, classes, probs, n_pix)
  switch (K) {
    case 1: ST_FIN(1); break;
    case 2: ST_FIN(2); break;
    case 3: ST_FIN(3); break;
    default: ST_FIN(4); break;
  }
#undef ST_FIN
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ------------------------------------------------------------------ crop mode: each window keeps its centre
// Window i of n keeps the rows (columns alike) [i * s + (i > 0) * o/2, i * s + d - (i < n - 1) * o/2): interior windows give
// up o/2 pixels on each shared edge.  The kept regions tile the padded raster exactly once, so every raster pixel has ONE
// owner window: i = clamp((g - o/2) / s, 0, n - 1) per axis.  One thread per raster pixel of the rows the batch's window rows
// keep; it copies the owner's byte when the owner is one of the windows first .. first + count - 1 (maps uint8
// [count][d][d], the head kernel's fused argmax) and leaves the pixel alone otherwise: disjoint writes, deterministic.
__global__ __launch_bounds__(256) void stitch_classes_u8_kernel(const uint8_t* __restrict__ maps, uint8_t* __restrict__ classes,
                                                                int w, int d, int o, int ny, int nx, int first, int count,
                                                                int row0, int64_t n_pix) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int s = d - o, half = o / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const int gx = (int)(i % w), gy = row0 + (int)(i / w);
    const int iy = gy < half ? 0 : min((gy - half) / s, ny - 1);
    const int ix = gx < half ? 0 : min((gx - half) / s, nx - 1);
    const int k = iy * nx + ix - first;
    if (k < 0 || k >= count) continue;
    classes[(int64_t)gy * w + gx] = maps[((int64_t)k * d + (gy - iy * s)) * d + (gx - ix * s)];
  }
}

extern "C" int dt_stitch_classes_u8(const uint8_t* maps, uint8_t* classes, int h, int w, int d, int overlap, int first,
                                    int count, void* stream) {
  DT_REQUIRE(maps && classes && h > 0 && w > 0 && d > 0 && first >= 0 && count > 0, "stitch_classes_u8: bad args");
  DT_REQUIRE(overlap >= 0 && (overlap & 1) == 0, "stitch_classes_u8: overlap must be even and >= 0");
  DT_REQUIRE(2 * overlap <= d, "stitch_classes_u8: overlap must be <= d/2");
  const int ny = stitch_windows(h, d, overlap), nx = stitch_windows(w, d, overlap), s = d - overlap;
  DT_REQUIRE((int64_t)first + count <= (int64_t)ny * nx, "stitch_classes_u8: window range outside the grid");
  const int i0 = first / nx, i1 = (first + count - 1) / nx;
  const int row0 = i0 * s + (i0 > 0 ? overlap / 2 : 0);
  const int64_t row1_full = (int64_t)i1 * s + d - (i1 < ny - 1 ? overlap / 2 : 0);
  const int row1 = row1_full < h ? (int)row1_full : h;
  const int64_t n_pix = (int64_t)(row1 - row0) * w;
  hipLaunchKernelGGL(stitch_classes_u8_kernel, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0, (hipStream_t)stream, maps,
                     classes, w, d, overlap, ny, nx, first, count, row0, n_pix);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
