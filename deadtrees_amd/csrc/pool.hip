// Batch gather from the device-resident sample pool (data/pool.py): the whole input side of a training step in ONE launch.
//
// The pool holds every decoded sample of a split as uint8 in HBM: images [N][H][W][4] (RGBA words), masks [N][H][W],
// land-use maps [N][H][W] and the exact byte sum of every image (the mean RandomBrightnessContrast needs; it does not change
// under flips and turns, so it is computed once at decode time instead of once per batch).  A batch is B pool indices plus
// the per-sample draws of the reference's train_transform (data/deadtreedata.py:128-146); the kernel applies
// flip / rot90 / brightness-contrast / Normalize with the arithmetic of augment_normalize_u8_kernel (elementwise.hip), writes
// the image PLANAR (NCHW fp32, what HipTrainer.step takes) and widens the label maps to int64 through the same pixel map
// (aug_source_pixel of views.h).  It replaces index_select x3 + dt_augment_normalize_u8 (2 launches) + 2 casts +
// dt_augment_labels x2 and writes straight into the buffers a captured training step reads.
//
// A memory kernel: per lane 4 consecutive x of one output row -> 4 source words (one 4-byte load per pixel, all channels),
// one 16-byte store per channel plane, 2 x 16-byte stores per label map.  Rows whose length is no multiple of 4 (or output
// buffers that are not 16-byte aligned) take the same lanes with scalar stores.  Every pool offset is 64-bit: a pool of
// 256 x 256 tiles passes 2^31 bytes at 5,461 samples.
//
// The kernel never reads outside the pool: a sample whose index is outside [0, N), or that asks for an odd turn of a
// non-square tile, is written as zeros and raises a bit of err_flag.
//
// dt_pool_gather_combined makes the same batch out of several pools (the reference's main + extra shard sets): slot b
// takes sample idx[b] of pool src[b].  There is ONE kernel and one host path: the pools are the rows of a table that
// travels as a kernel argument, and the single pool of dt_pool_gather_batch is a table of one row read without src.
#include "common.h"
#include "views.h"

typedef long long i64x2 __attribute__((ext_vector_type(2)));

#define POOL_ERR_INDEX 1   // err_flag bits (include/deadtrees_hip.h: DT_POOL_ERR_*)
#define POOL_ERR_TURN 2
#define POOL_ERR_SOURCE 4

// One slot of a batch: sample s of the pool (images, masks, lu, sums) into slot blockIdx.y of the outputs.  bad: the
// error bits the caller found for s (the index, or the source, is out of range); everything here is uniform per workgroup
template <bool VEC>
__device__ __forceinline__ void pool_gather_slot(
    const uint32_t* __restrict__ images, const uint8_t* __restrict__ masks, const uint8_t* __restrict__ lu,
    const unsigned long long* __restrict__ sums, const int64_t s, const int bad, const int32_t* __restrict__ geo,
    const float* __restrict__ bc, float* __restrict__ img_out, int64_t* __restrict__ mask_out, int64_t* __restrict__ lu_out,
    int32_t* __restrict__ err_flag, int H, int W, int Cd, int merge_above, f32x4 mean, f32x4 stdv) {
  const int b = blockIdx.y;
  const int flip = geo[2 * b], rot = geo[2 * b + 1];
  const int err = bad | (((rot & 1) && H != W) ? POOL_ERR_TURN : 0);
  if (err && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err_flag, err);
  const bool live = err == 0;      // uniform per workgroup; a dead sample reads nothing and writes zeros
  const float alpha = bc[2 * b], beta = bc[2 * b + 1];
  // RandomBrightnessContrast on uint8 (brightness_by_max=False), as augment_normalize_u8_kernel: the image mean over all
  // four stored bands
  const float add = (!live || beta == 0.f) ? 0.f : (float)((double)beta * ((double)sums[s] / ((double)H * W * 4)));
  const bool lut = alpha != 1.f || beta != 0.f;
  const int W4 = (W + 3) >> 2;
  const int64_t n_pix = (int64_t)H * W, n_quads = (int64_t)H * W4;
  const int64_t src0 = live ? s * n_pix : 0;           // pixel offset of the sample in the pool
  float* ib = img_out + (int64_t)b * Cd * n_pix;
  int64_t* mb = mask_out + (int64_t)b * n_pix;
  int64_t* lb = lu_out ? lu_out + (int64_t)b * n_pix : nullptr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * 256) {
    const int y = (int)(q / W4), x0 = (int)(q - (int64_t)y * W4) * 4;
    const int n = W - x0 < 4 ? W - x0 : 4;             // < 4 only in the last quad of a row with W % 4 != 0
    uint32_t px[4] = {0, 0, 0, 0};
    int64_t mv[4] = {0, 0, 0, 0}, lv[4] = {0, 0, 0, 0};
    if (live) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          int sy, sx;
          aug_source_pixel(flip, rot, y, x0 + j, H, W, &sy, &sx);
          const int64_t o = src0 + (int64_t)sy * W + sx;
          px[j] = images[o];
          const int64_t m = masks[o];
          mv[j] = (merge_above && m > 1) ? 1 : m;     // classes == 2: every class above 1 is "dead tree" (:179-180)
          if (lb) lv[j] = lu[o];
        }
      }
    }
    const int64_t o = (int64_t)y * W + x0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < Cd) {
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = (float)((px[j] >> (8 * c)) & 255u);
          if (lut) {
            v = v * alpha + add;
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
            v = floorf(v);
          }
          r[j] = live ? (v - mean[c] * 255.f) * (1.f / (stdv[c] * 255.f)) : 0.f;
        }
        float* dp = ib + (int64_t)c * n_pix + o;
        if (VEC) {
          *(f32x4*)dp = r;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < n) dp[j] = r[j];
        }
      }
    }
    if (VEC) {
      *(i64x2*)(mb + o) = i64x2{mv[0], mv[1]};
      *(i64x2*)(mb + o + 2) = i64x2{mv[2], mv[3]};
      if (lb) {
        *(i64x2*)(lb + o) = i64x2{lv[0], lv[1]};
        *(i64x2*)(lb + o + 2) = i64x2{lv[2], lv[3]};
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          mb[o + j] = mv[j];
          if (lb) lb[o + j] = lv[j];
        }
      }
    }
  }
}

// Slot b out of row src[b] of the table (row 0 without src: the single pool), which is a kernel argument — the row index
// is a scalar (blockIdx.y -> one scalar load of src), so the row's four pointers and its n arrive by scalar loads from the
// kernarg segment: no vector work, no private copy of the table.
struct pool_table {
  dt_pool_source s[DT_POOL_MAX_SOURCES];
};

template <bool VEC>
__global__ __launch_bounds__(256) void pool_gather_kernel(
    const pool_table tab, const int n_sources, const int32_t* __restrict__ src, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ geo, const float* __restrict__ bc, float* __restrict__ img_out,
    int64_t* __restrict__ mask_out, int64_t* __restrict__ lu_out, int32_t* __restrict__ err_flag, int H, int W, int Cd,
    int merge_above, f32x4 mean, f32x4 stdv) {
  const int j = src ? src[blockIdx.y] : 0;
  const int64_t s = idx[blockIdx.y];
  const bool known = j >= 0 && j < n_sources;
  const dt_pool_source& p = tab.s[known ? j : 0];        // (row 0 always exists; a slot with an unknown source reads nothing)
  const int bad = !known ? POOL_ERR_SOURCE : ((s < 0 || s >= p.n) ? POOL_ERR_INDEX : 0);
  pool_gather_slot<VEC>((const uint32_t*)p.images, p.masks, p.lu, (const unsigned long long*)p.sums, s, bad, geo, bc,
                        img_out, mask_out, lu_out, err_flag, H, W, Cd, merge_above, mean, stdv);
}

// Everything both entries do; who: the entry's name, for the messages.  src may be NULL with one source.
static int pool_gather_launch(const char* who, const dt_pool_source* sources, int n_sources, const int32_t* src,
                              const int32_t* idx, const int32_t* geo, const float* bc, float* img_out, int64_t* mask_out,
                              int64_t* lu_out, int32_t* err_flag, int B, int H, int W, int Cdst, int merge_above,
                              const float* mean, const float* stdv, void* stream) {
  DT_REQUIRE(sources && idx && geo && bc && img_out && mask_out && err_flag && mean && stdv, "%s: null argument", who);
  DT_REQUIRE(n_sources >= 1 && n_sources <= DT_POOL_MAX_SOURCES, "%s: 1 .. %d sources", who, DT_POOL_MAX_SOURCES);
  DT_REQUIRE(src || n_sources == 1, "%s: null argument (src may be NULL with one source only)", who);
  DT_REQUIRE(B > 0 && H > 0 && W > 0 && Cdst > 0 && Cdst <= 4, "%s: bad sizes", who);
  DT_REQUIRE(B <= 65535, "%s: B must be <= 65535", who);
  pool_table tab = {};
  for (int j = 0; j < n_sources; ++j) {
    const dt_pool_source& p = sources[j];
    DT_REQUIRE(p.images && p.masks && p.sums && p.n > 0, "%s: source %d: null array or no samples", who, j);
    DT_REQUIRE(!lu_out || p.lu, "%s: lu_out needs lu in every source (source %d has none)", who, j);
    DT_REQUIRE(((uintptr_t)p.images & 3) == 0, "%s: the image pool must be 4-byte aligned (source %d)", who, j);
    tab.s[j] = p;
    if (!lu_out) tab.s[j].lu = nullptr;
  }
  f32x4 m = {0, 0, 0, 0}, s = {1, 1, 1, 1};
  for (int c = 0; c < Cdst; ++c) {
    m[c] = mean[c];
    s[c] = stdv[c];
  }
  const bool vec = (W & 3) == 0 && (((uintptr_t)img_out | (uintptr_t)mask_out | (uintptr_t)lu_out) & 15) == 0;
  int gx = dt_cdiv((int64_t)H * ((W + 3) / 4), 256);
  if (gx > 1024) gx = 1024;
  const dim3 grid(gx, B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(pool_gather_kernel<true>, grid, block, 0, st, tab, n_sources, src, idx, geo, bc, img_out, mask_out,
                       lu_out, err_flag, H, W, Cdst, merge_above, m, s);
  else
    hipLaunchKernelGGL(pool_gather_kernel<false>, grid, block, 0, st, tab, n_sources, src, idx, geo, bc, img_out, mask_out,
                       lu_out, err_flag, H, W, Cdst, merge_above, m, s);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_pool_gather_batch(const uint8_t* images, const uint8_t* masks, const uint8_t* lu, const uint64_t* sums,
                                    const int32_t* idx, const int32_t* geo, const float* bc, float* img_out,
                                    int64_t* mask_out, int64_t* lu_out, int32_t* err_flag, int64_t N, int B, int H, int W,
                                    int Cdst, int merge_above, const float* mean, const float* stdv, void* stream) {
  DT_REQUIRE((lu == nullptr) == (lu_out == nullptr), "pool_gather_batch: lu and lu_out go together");
  DT_REQUIRE(N > 0, "pool_gather_batch: bad sizes");
  const dt_pool_source one = {images, masks, lu, sums, N};
  return pool_gather_launch("pool_gather_batch", &one, 1, nullptr, idx, geo, bc, img_out, mask_out, lu_out, err_flag, B, H,
                            W, Cdst, merge_above, mean, stdv, stream);
}

extern "C" int dt_pool_gather_combined(const dt_pool_source* sources, int n_sources, const int32_t* src, const int32_t* idx,
                                       const int32_t* geo, const float* bc, float* img_out, int64_t* mask_out,
                                       int64_t* lu_out, int32_t* err_flag, int B, int H, int W, int Cdst, int merge_above,
                                       const float* mean, const float* stdv, void* stream) {
  return pool_gather_launch("pool_gather_combined", sources, n_sources, src, idx, geo, bc, img_out, mask_out, lu_out,
                            err_flag, B, H, W, Cdst, merge_above, mean, stdv, stream);
}
