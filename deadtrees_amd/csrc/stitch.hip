// Overlap-stitched tiled inference (BASELINE configs[5] "overlap-stitch"; the reference has none): the windowed
// input gather and the blend of the overlapping windows' predictions into the raster, all on the device.
//
// Geometry (one definition: stitch_windows below, deployment/tiler.py::window_grid restates it in numpy and
// tests/test_overlap_stitch_host.py compares the two).  d = window edge, o = overlap (even, 0 <= o <= d/2), s = d - o the
// stride; an axis of length L carries n(L) = max(1, ceil((L - o) / s)) windows, window k = i * nx + j has its origin at
// (i * s, j * s) (row-major), pixels beyond the raster are the tiler's zero byte.  o <= d/2 means d <= 2s: a raster pixel
// lies in at most 2 windows per axis, 4 in all.  At o = 0 this is the d x d block grid of dt_split_normalize_u8.
//
// Test-time augmentation: the gather cuts T <= 8 dihedral views (views.h) of every window and the accumulate averages the
// views' softmax probabilities before the blend; several models accumulate into one raster (soft vote).  A plain window is
// the identity view: the gather and the accumulate are ONE kernel body each, in two instantiations — VIEWS = false, the
// lean form of the caller without views (and with ramp weights), and VIEWS = true, the general one.
//
// All kernels stream: one thread per pixel in a grid-stride loop, coalesced along x, no atomics, no LDS.
#include "conv_host.h"
#include "views.h"

#define ST_CAP (256 * 16)   // grid cap, as EW_CAP (conv_host.h): 16 workgroups per CU, grid-stride beyond

static inline int stitch_windows(int L, int d, int o) {
  const int s = d - o;
  const int n = (L - o + s - 1) / s;
  return n > 1 ? n : 1;
}
// the geometry rules of every entry point, in the one place that words them
static inline int stitch_geometry_check(int d, int o, const char* tag) {
  DT_REQUIRE(d > 0, "%s: bad sizes", tag);
  DT_REQUIRE(o >= 0 && (o & 1) == 0, "%s: overlap must be even and >= 0", tag);
  DT_REQUIRE(2 * o <= d, "%s: overlap must be <= d/2", tag);
  return DT_OK;
}
// ... and the window grid of an h x w raster with the range first .. first + count - 1 inside it
static inline int stitch_grid_check(int h, int w, int d, int o, int first, int count, const char* tag, int* ny, int* nx) {
  DT_TRY(stitch_geometry_check(d, o, tag));
  *ny = stitch_windows(h, d, o);
  *nx = stitch_windows(w, d, o);
  DT_REQUIRE((int64_t)first + count <= (int64_t)*ny * *nx, "%s: window range outside the grid", tag);
  return DT_OK;
}

// f(std::integral_constant<int, K>) for the class count K in 1..4 (checked by the caller): the kernels take K as a
// template argument
template <class F>
static inline void stitch_for_classes(int K, F&& f) {
  switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// T <= 8 views travel by value in the kernel arguments, 4 bits each: view v = (flip, rot) sits at bits 4v .. 4v + 3 as
// flip | rot << 2.  `views` is the host array (flip_0, rot_0, flip_1, rot_1, ...).  inverse: pack the view that undoes
// each one instead: rot90^k is undone by rot90^(4-k); a view with a flip is its own inverse (flip . rot90^-k = rot90^k . flip).
// views == NULL (n_views must be 0 then) is the one identity view: T = 1, packed 0.
#define ST_MAX_VIEWS 8
static inline int stitch_pack_views(const int* views, int n_views, bool inverse, const char* tag, int* T, uint32_t* packed) {
  *T = 1;
  *packed = 0;
  if (views == nullptr) {
    DT_REQUIRE(n_views == 0, "%s: null views need n_views == 0 (the identity view)", tag);
    return DT_OK;
  }
  DT_REQUIRE(n_views >= 1 && n_views <= ST_MAX_VIEWS, "%s: the number of views must be in 1..8", tag);
  for (int v = 0; v < n_views; ++v) {
    const int flip = views[2 * v], rot = views[2 * v + 1];
    DT_REQUIRE(flip >= 0 && flip <= 2, "%s: flip of view %d must be in 0..2", tag, v);
    DT_REQUIRE(rot >= 0 && rot <= 3, "%s: rot of view %d must be in 0..3", tag, v);
    const int r = (inverse && flip == 0) ? (4 - rot) & 3 : rot;
    *packed |= (uint32_t)(flip | (r << 2)) << (4 * v);
  }
  *T = n_views;
  return DT_OK;
}
__device__ __forceinline__ int stitch_view_flip(uint32_t packed, int v) { return (int)(packed >> (4 * v)) & 3; }
__device__ __forceinline__ int stitch_view_rot(uint32_t packed, int v) { return (int)(packed >> (4 * v + 2)) & 3; }

extern "C" int dt_stitch_window_count(int L, int d, int overlap) {
  DT_REQUIRE(L > 0, "stitch_window_count: bad sizes");
  DT_TRY(stitch_geometry_check(d, overlap, "stitch_window_count"));
  return stitch_windows(L, d, overlap);
}

// ------------------------------------------------------------------ input gather
// deployment/tiler.py:121-134 + utils/data_handling.py:9-20 (zero-pad the raster, cut it into d x d windows in row-major
// order) + scripts/inference.py:94-96 (albumentations Normalize per sub-tile) as ONE gather: raster uint8 [Cs][h][w]
// (band-major, what rioxarray hands over) -> fp32 NHWC windows [count][d][d][Cd], windows first .. first + count - 1 of the
// nwx-wide grid with origins `stride` apart.  stride == d is the non-overlapping block split (dt_split_normalize_u8 calls
// this with it).  One thread per output pixel: Cd byte loads (coalesced along x per band), Cd dword stores.
// window pixel (y, x) of window blk: Cd byte loads, Cd dword stores at dp
__device__ __forceinline__ void window_pixel_normalize(const uint8_t* __restrict__ src, float* __restrict__ dp, int h, int w,
                                                       int64_t plane, int wstride, int nwx, int blk, int y, int x, int Cd,
                                                       f32x4 mean, f32x4 stdv) {
  const int gy = (blk / nwx) * wstride + y, gx = (blk % nwx) * wstride + x;
  const bool in = gy < h && gx < w;
  for (int c = 0; c < Cd; ++c) {
    const float v = in ? (float)src[c * plane + (int64_t)gy * w + gx] : 0.f;
    dp[c] = (v - mean[c] * 255.f) * (1.f / (stdv[c] * 255.f));   // the arithmetic of normalize_u8_kernel
  }
}

// VIEWS = false: output tile k is window first + k (T and views are not read).  VIEWS = true: T views per window, output
// tile k * T + v is view v of window first + k, [count][T][d][d][Cd].  The output pixel (y, x) of a view is the window pixel
// aug_source_pixel names, through the arithmetic above: every view is a bit-exact permutation of the plain window (zero
// padding beyond the raster included: it applies to the window pixel).  Stores stay coalesced; the byte loads of a
// transposing view (rot odd) walk a raster column.
template <bool VIEWS>
__global__ __launch_bounds__(256) void window_normalize_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                                  int h, int w, int d, int wstride, int nwx, int first,
                                                                  int64_t n_pix, int Cd, f32x4 mean, f32x4 stdv, int T,
                                                                  uint32_t views) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t plane = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const int x = (int)(i % d), y = (int)((i / d) % d);
    const int64_t tile = i / ((int64_t)d * d);
    if constexpr (VIEWS) {
      const int v = (int)(tile % T), blk = first + (int)(tile / T);
      int sy, sx;
      aug_source_pixel(stitch_view_flip(views, v), stitch_view_rot(views, v), y, x, d, d, &sy, &sx);
      window_pixel_normalize(src, dst + i * Cd, h, w, plane, wstride, nwx, blk, sy, sx, Cd, mean, stdv);
    } else {
      window_pixel_normalize(src, dst + i * Cd, h, w, plane, wstride, nwx, first + (int)tile, y, x, Cd, mean, stdv);
    }
  }
}

extern "C" int dt_window_normalize_u8(const uint8_t* raster_chw, float* dst_nhwc, int Csrc, int h, int w, int d, int stride,
                                      int nwx, int first, int count, int Cdst, const float* mean, const float* stdv,
                                      const int* views, int n_views, void* stream) {
  const char* tag = "window_normalize_u8";
  DT_REQUIRE(raster_chw && dst_nhwc && mean && stdv && h > 0 && w > 0 && d > 0 && nwx > 0 && first >= 0 && count > 0 &&
                 Cdst > 0 && Cdst <= 4 && Cdst <= Csrc,
             "%s: bad args", tag);
  DT_REQUIRE(stride > 0 && stride <= d, "%s: stride must be in (0, d]", tag);
  DT_TRY(stitch_geometry_check(d, d - stride, tag));
  DT_REQUIRE(nwx == stitch_windows(w, d, d - stride), "%s: nwx is not the window count of the raster width", tag);
  int ny, nx, T;
  DT_TRY(stitch_grid_check(h, w, d, d - stride, first, count, tag, &ny, &nx));
  uint32_t packed;
  DT_TRY(stitch_pack_views(views, n_views, false, tag, &T, &packed));
  f32x4 m{0, 0, 0, 0}, s{1, 1, 1, 1};
  for (int c = 0; c < Cdst; ++c) {
    m[c] = mean[c];
    s[c] = stdv[c];
  }
  const int64_t n_pix = (int64_t)count * T * d * d;
  const auto kernel = views ? window_normalize_u8_kernel<true> : window_normalize_u8_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0, (hipStream_t)stream, raster_chw, dst_nhwc, h, w,
                     d, stride, nwx, first, n_pix, Cdst, m, s, T, packed);
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

// Softmax over the K logits p[c * wplane]: accurate expf, max subtracted.  l[c] = exp(logit_c - max), returns their sum; the
// probability is l[c] / sum.
template <int K>
__device__ __forceinline__ float stitch_softmax_terms(const float* __restrict__ p, int64_t wplane, float* l) {
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
  return sum;
}

// Gather form: one thread owns one raster pixel of the rows [row0, row0 + n_pix / w) and visits the (at most 2 x 2) windows
// that cover it, in ascending window index; the windows outside first .. first + count - 1 are not in this call's logits and
// are skipped.  Per visited window: softmax over K (accurate expf, max subtracted), acc[k] += weight * p_k.  Every pixel's
// sum is thus built in ONE order, one fp32 add per window, whatever the batch size and however the windows are split into
// calls (calls in ascending window order): the accumulator is bit-identical across batchings.
// acc fp32 planar [K][h][w], zeroed before the first call.
//
// VIEWS = false: logits fp32 NCHW [count][K][d][d], ramp weights; T, inv_views and keep are not read.
// VIEWS = true: logits fp32 [count][T][K][d][d], tile k * T + v is the network's answer to view v of window first + k.
// Window pixel (y, x) sits in view v at aug_source_pixel of the INVERSE view (inv_views, packed by the host).  Per covering
// window: the T softmax vectors are summed in ascending v, times 1.0f / T, then acc += weight * mean.  One order per pixel
// (windows ascending, views ascending within a window): bit-identical across batchings as above, and at T = 1 with the
// identity view the sum is 0 + p, the factor 1.0f: the bits of the VIEWS = false instantiation.
// keep = 0: ramp weights.  keep = 1: weight 1 inside the window's kept region of crop mode (stitch_classes_u8_kernel), 0
// outside, so exactly one window contributes per pixel; a window of weight 0 is not read.
// Lanes adjacent in raster x read a transposing view (rot odd) d floats apart.
template <int K, bool VIEWS>
__global__ __launch_bounds__(256) void stitch_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ acc,
                                                                int h, int w, int d, int o, int ny, int nx, int first,
                                                                int count, int row0, int64_t n_pix, int T,
                                                                uint32_t inv_views, int keep) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t plane = (int64_t)h * w, wplane = (int64_t)d * d;
  const int s = d - o, half = o / 2;
  const float inv_t = 1.f / (float)T;
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
        const int y = gy - iy * s, x = gx - ix * s;
        float wgt;
        if (VIEWS && keep) {
          const bool in = y >= (iy > 0 ? half : 0) && y < d - (iy < ny - 1 ? half : 0) && x >= (ix > 0 ? half : 0) &&
                          x < d - (ix < nx - 1 ? half : 0);
          wgt = in ? 1.f : 0.f;
        } else {
          wgt = stitch_ramp(y, d, o) * stitch_ramp(x, d, o);
        }
        if (VIEWS && wgt == 0.f) continue;
        if (!touched) {
#pragma unroll
          for (int c = 0; c < K; ++c) a[c] = acc[c * plane + pix];
          touched = true;
        }
        float m[K], l[K];
        if constexpr (VIEWS) {
#pragma unroll
          for (int c = 0; c < K; ++c) m[c] = 0.f;
          for (int v = 0; v < T; ++v) {
            int vy, vx;
            aug_source_pixel(stitch_view_flip(inv_views, v), stitch_view_rot(inv_views, v), y, x, d, d, &vy, &vx);
            const float sum =
                stitch_softmax_terms<K>(logits + ((int64_t)k * T + v) * K * wplane + (int64_t)vy * d + vx, wplane, l);
#pragma unroll
            for (int c = 0; c < K; ++c) m[c] += l[c] / sum;
          }
#pragma unroll
          for (int c = 0; c < K; ++c) a[c] += wgt * (m[c] * inv_t);
        } else {
          const float sum = stitch_softmax_terms<K>(logits + (int64_t)k * K * wplane + (int64_t)y * d + x, wplane, l);
#pragma unroll
          for (int c = 0; c < K; ++c) a[c] += wgt * (l[c] / sum);
        }
      }
    }
    if (touched) {
#pragma unroll
      for (int c = 0; c < K; ++c) acc[c * plane + pix] = a[c];
    }
  }
}

extern "C" int dt_stitch_accumulate(const float* logits, float* acc, int K, int h, int w, int d, int overlap, int first,
                                    int count, const int* views, int n_views, int weight_mode, void* stream) {
  const char* tag = "stitch_accumulate";
  DT_REQUIRE(logits && acc && h > 0 && w > 0 && d > 0 && first >= 0 && count > 0, "%s: bad args", tag);
  DT_REQUIRE(K >= 1 && K <= 4, "%s: K must be in 1..4", tag);
  int ny, nx, T;
  DT_TRY(stitch_grid_check(h, w, d, overlap, first, count, tag, &ny, &nx));
  uint32_t inv;
  DT_TRY(stitch_pack_views(views, n_views, true, tag, &T, &inv));
  DT_REQUIRE(weight_mode == DT_STITCH_WEIGHT_RAMP || weight_mode == DT_STITCH_WEIGHT_KEEP,
             "%s: weight_mode must be DT_STITCH_WEIGHT_RAMP or DT_STITCH_WEIGHT_KEEP", tag);
  const int keep = weight_mode == DT_STITCH_WEIGHT_KEEP;
  // the raster rows [row0, row1) under the batch's window rows
  const int s = d - overlap, row0 = (first / nx) * s;
  const int64_t row1_full = (int64_t)((first + count - 1) / nx) * s + d;
  const int row1 = row1_full < h ? (int)row1_full : h;
  const int64_t n_pix = (int64_t)(row1 - row0) * w;
  const bool lean = views == nullptr && !keep;   // no views, ramp weights: nothing of the general form is needed
  stitch_for_classes(K, [&](auto kk) {
    constexpr int KK = decltype(kk)::value;
    const auto kernel = lean ? stitch_accumulate_kernel<KK, false> : stitch_accumulate_kernel<KK, true>;
    hipLaunchKernelGGL(kernel, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0, (hipStream_t)stream, logits, acc, h, w, d,
                       overlap, ny, nx, first, count, row0, n_pix, T, inv, keep);
  });
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
  stitch_for_classes(K, [&](auto kk) {
    hipLaunchKernelGGL(stitch_finalize_kernel<decltype(kk)::value>, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0,
                       (hipStream_t)stream, acc, classes, probs, n_pix);
  });
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
  int ny, nx;
  DT_TRY(stitch_grid_check(h, w, d, overlap, first, count, "stitch_classes_u8", &ny, &nx));
  const int s = d - overlap, i0 = first / nx, i1 = (first + count - 1) / nx;
  const int row0 = i0 * s + (i0 > 0 ? overlap / 2 : 0);
  const int64_t row1_full = (int64_t)i1 * s + d - (i1 < ny - 1 ? overlap / 2 : 0);
  const int row1 = row1_full < h ? (int)row1_full : h;
  const int64_t n_pix = (int64_t)(row1 - row0) * w;
  hipLaunchKernelGGL(stitch_classes_u8_kernel, dim3(dt_ew_grid(n_pix, ST_CAP)), dim3(256), 0, (hipStream_t)stream, maps,
                     classes, w, d, overlap, ny, nx, first, count, row0, n_pix);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
