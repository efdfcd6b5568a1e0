// Cover grids (deployment/cover.py states the contract): area-weighted class counts per zone and per cell of a coarser
// grid, from a uint8 class map that already sits in HBM.  A grid is two strictly increasing edge tables in 1/256 pixel,
// yq[gy + 1] and xq[gx + 1], every cell at least one pixel (256) wide, so a pixel meets at most two cells per axis.
//   sums[g][x][z][c] += sum over pixels (i, j) with zones == z and classes == c of wy(g, i) * wx(x, j)
//   wy(g, i) = max(0, min(yq[g + 1], 256 (i + 1)) - max(yq[g], 256 i)), wx likewise: units of 1/65536 pixel.
// Integers only: exact and independent of the order, so the device equals the numpy definition bit for bit.
//
// Parallel over the SOURCE: one 256-lane workgroup per CV_TH x CV_TW pixel tile (the tile of patches.hip), the grid is
// the number of tiles, every pixel is read once whatever the cell size.  Lane t owns 8 consecutive pixels of tile row
// t / 8 (one 8-byte load where the address allows it, bytes otherwise: maps are crops and members of stacked tensors).
// The cells a tile meets are found by a uniform binary search in the edge tables; a lane searches only inside that range.
//
// A real map is > 95 % one class and all pixels of a tile that fall in one cell share their bins, so nothing is added
// pixel by pixel: a lane first combines its runs of equal (x cell, bin) — usually ONE run of 8 pixels —, the runs a
// wave's lanes end with are combined across the wave per distinct (cell, bin) (up to CV_WAVE_KEYS of them, butterfly
// sums, one LDS atomic each), the four waves meet in LDS (a tile holds 2048 pixels of weight <= 65536: uint32 is enough),
// and the workgroup issues at most one 64-bit global atomic per non-empty (cell, bin).  When the cells a tile meets times
// Z * K exceed CV_LDS_WORDS (cells of about one pixel) the lanes add their runs to `sums` directly: each cell then has
// few pixels and contention is low.
#include "conv_host.h"

#define CV_TH 32                 // tile rows
#define CV_TW 64                 // tile columns: 8 lanes of 8 pixels
#define CV_LDS_WORDS 8192        // 32 KB of uint32 bins per workgroup: four workgroups fit a CU beside their registers
#define CV_WAVE_KEYS 4           // distinct (cell, bin) keys combined across a wave before the lanes add on their own
#define CV_MAX_SIDE 16384
#define CV_MAX_Q (1 << 23)

static_assert(CV_TH * CV_TW == 256 * 8, "8 pixels per lane");

// first k in [lo, hi) with q[k + 1] > v (the first cell that ends behind v); hi without one.  q holds hi + 1 entries or more
__device__ __forceinline__ int cv_first_ending_behind(const int32_t* __restrict__ q, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid + 1] > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// first k in [lo, hi) with q[k] >= v (the first cell that starts at or behind v); hi without one
__device__ __forceinline__ int cv_first_starting_at(const int32_t* __restrict__ q, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] >= v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// the overlap of the cell [e0, e1) with pixel p = [256 p, 256 (p + 1)), in 1/256 pixel
__device__ __forceinline__ uint32_t cv_weight(int e0, int e1, int p) {
  const int lo = max(e0, 256 * p), hi = min(e1, 256 * p + 256);
  return (uint32_t)max(0, hi - lo);
}

__device__ __forceinline__ uint32_t cv_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// 8 pixels at p (n < 8 of them at the raster's right edge) as one little-endian word
__device__ __forceinline__ uint64_t cv_load8(const uint8_t* __restrict__ p, int n) {
  if (n == 8 && ((uintptr_t)p & 7u) == 0) return *(const uint64_t*)p;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < n) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

// where a workgroup adds: its LDS bins over the ncx cells from (g_lo, c_lo) on, or `sums` itself
struct cv_target {
  uint32_t* acc;
  unsigned long long* sums;
  int g_lo, c_lo, ncx, gx, B;
  bool direct;
};

__device__ __forceinline__ void cv_add(const cv_target& t, int g, int c, int bin, uint32_t v) {
  if (v == 0) return;
  if (t.direct) atomicAdd(&t.sums[((int64_t)g * t.gx + c) * t.B + bin], (unsigned long long)v);
  else atomicAdd(&t.acc[((g - t.g_lo) * t.ncx + (c - t.c_lo)) * t.B + bin], v);
}

// a run: x weights s0 / s1 of the cells c / c + 1, in the rows' cells g / g + 1 with y weights wy0 / wy1.  A zero weight
// stands for a cell that is not there
__device__ __forceinline__ void cv_add_run(const cv_target& t, int g, int c, int bin, uint32_t s0, uint32_t s1, uint32_t wy0,
                                           uint32_t wy1) {
  cv_add(t, g, c, bin, s0 * wy0);
  cv_add(t, g + 1, c, bin, s0 * wy1);
  cv_add(t, g, c + 1, bin, s1 * wy0);
  cv_add(t, g + 1, c + 1, bin, s1 * wy1);
}

__global__ __launch_bounds__(256) void cover_grid_kernel(const uint8_t* __restrict__ classes,
                                                         const uint8_t* __restrict__ zones, int h, int w, int K, int Z,
                                                         const int32_t* __restrict__ yq, int gy,
                                                         const int32_t* __restrict__ xq, int gx, int ntx,
                                                         unsigned long long* __restrict__ sums, int32_t* __restrict__ err) {
  __shared__ uint32_t acc[CV_LDS_WORDS];
  const int ty0 = (int)(blockIdx.x / (unsigned)ntx) * CV_TH, tx0 = (int)(blockIdx.x % (unsigned)ntx) * CV_TW;
  const int ty1 = min(ty0 + CV_TH, h), tx1 = min(tx0 + CV_TW, w);
  // the cells the tile meets, [g_lo, g_end) x [c_lo, c_end): uniform over the workgroup
  const int g_lo = cv_first_ending_behind(yq, 0, gy, 256 * ty0);
  const int g_end = cv_first_starting_at(yq, g_lo, gy, 256 * ty1);
  const int c_lo = cv_first_ending_behind(xq, 0, gx, 256 * tx0);
  const int c_end = cv_first_starting_at(xq, c_lo, gx, 256 * tx1);
  cv_target tg;
  tg.acc = acc;
  tg.sums = sums;
  tg.g_lo = g_lo;
  tg.c_lo = c_lo;
  tg.ncx = c_end - c_lo;
  tg.gx = gx;
  tg.B = Z * K;
  const int64_t nwords = (int64_t)(g_end - g_lo) * tg.ncx * tg.B;
  tg.direct = nwords > CV_LDS_WORDS;
  if (!tg.direct) {
    for (int k = threadIdx.x; k < (int)nwords; k += 256) acc[k] = 0;
    __syncthreads();
  }

  const int lane = threadIdx.x & 63;
  const int i = ty0 + (int)(threadIdx.x >> 3), xa = tx0 + 8 * (int)(threadIdx.x & 7u);
  uint32_t flag = 0, wy0 = 0, wy1 = 0, s0 = 0, s1 = 0;
  int g = g_lo, run_c = 0, run_bin = -1;               // run_bin < 0: no run is open
  if (i < h && xa < w) {
    g = cv_first_ending_behind(yq, g_lo, g_end, 256 * i);
    if (g < g_end) wy0 = cv_weight(yq[g], yq[g + 1], i);
    if (g + 1 < g_end) wy1 = cv_weight(yq[g + 1], yq[g + 2], i);
    const int n = min(8, w - xa);
    const int64_t at = (int64_t)i * w + xa;
    const uint64_t cw = cv_load8(classes + at, n), zw = zones ? cv_load8(zones + at, n) : 0;
    // the cell c of the current pixel and its successor: edges e0 < e1 < e2 (read only where the cells are there)
    int c = cv_first_ending_behind(xq, c_lo, c_end, 256 * xa);
    int e0 = c < c_end ? xq[c] : 0, e1 = c < c_end ? xq[c + 1] : 0, e2 = c + 1 < c_end ? xq[c + 2] : 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      if (p < n) {
        const int j = xa + p;
        if (c < c_end && e1 <= 256 * j) {             // cells are >= one pixel wide: at most one step per pixel
          ++c;
          e0 = e1;
          e1 = e2;
          e2 = c + 1 < c_end ? xq[c + 2] : 0;
        }
        const uint32_t w0 = c < c_end ? cv_weight(e0, e1, j) : 0u, w1 = c + 1 < c_end ? cv_weight(e1, e2, j) : 0u;
        const int cv = (int)((cw >> (8 * p)) & 0xffu), zv = (int)((zw >> (8 * p)) & 0xffu);
        if (cv >= K) flag |= 1u;
        if (zv >= Z) flag |= 2u;
        const int bin = (cv >= K || zv >= Z || (w0 | w1) == 0) ? -1 : zv * K + cv;
        if (bin != run_bin || c != run_c) {
          if (run_bin >= 0) cv_add_run(tg, g, run_c, run_bin, s0, s1, wy0, wy1);
          run_bin = bin;
          run_c = c;
          s0 = s1 = 0;
        }
        s0 += w0;
        s1 += w1;
      }
    }
  }
  // the run every lane ends with
  if (tg.direct) {
    if (run_bin >= 0) cv_add_run(tg, g, run_c, run_bin, s0, s1, wy0, wy1);
  } else {
    // (g, c, bin) relative to the tile's cells: a tile meets at most 33 x 65 cells of a pixel or more, and bins are < 64
    const int key = run_bin < 0 ? -1 : ((g - g_lo) << 19) | ((run_c - c_lo) << 6) | run_bin;
    bool pending = run_bin >= 0;
    for (int it = 0; it < CV_WAVE_KEYS; ++it) {
      const unsigned long long waiting = __ballot(pending);
      if (!waiting) break;                                  // uniform over the wave
      const int leader = __ffsll(waiting) - 1;
      const int k = __shfl(key, leader, 64);
      const bool mine = pending && key == k;
      const uint32_t a00 = cv_wave_sum(mine ? s0 * wy0 : 0u), a10 = cv_wave_sum(mine ? s0 * wy1 : 0u);
      const uint32_t a01 = cv_wave_sum(mine ? s1 * wy0 : 0u), a11 = cv_wave_sum(mine ? s1 * wy1 : 0u);
      if (lane == leader) {
        cv_add(tg, g, run_c, run_bin, a00);
        cv_add(tg, g + 1, run_c, run_bin, a10);
        cv_add(tg, g, run_c + 1, run_bin, a01);
        cv_add(tg, g + 1, run_c + 1, run_bin, a11);
      }
      if (mine) pending = false;
    }
    if (pending) cv_add_run(tg, g, run_c, run_bin, s0, s1, wy0, wy1);
  }
  const uint32_t wave_flag = (__ballot(flag & 1u) ? 1u : 0u) | (__ballot(flag & 2u) ? 2u : 0u);
  if (lane == 0 && wave_flag) atomicOr(err, (int)wave_flag);

  if (!tg.direct) {
    __syncthreads();
    const int per_row = tg.ncx * tg.B;
    for (int k = threadIdx.x; k < (int)nwords; k += 256) {
      const uint32_t v = acc[k];
      if (v) atomicAdd(&sums[((int64_t)(g_lo + k / per_row) * gx + c_lo) * tg.B + k % per_row], (unsigned long long)v);
    }
  }
}

extern "C" int dt_cover_grid_u8(const uint8_t* classes, const uint8_t* zones, int h, int w, int K, int Z, const int32_t* yq,
                                int gy, const int32_t* xq, int gx, int64_t* sums, int32_t* err_flag, void* stream) {
  DT_REQUIRE(classes && yq && xq && sums && err_flag, "cover_grid_u8: null pointer");
  DT_REQUIRE(h >= 1 && w >= 1 && h <= CV_MAX_SIDE && w <= CV_MAX_SIDE, "cover_grid_u8: raster %d x %d unsupported (1..%d)", h, w,
             CV_MAX_SIDE);
  DT_REQUIRE(K >= 2 && K <= 8, "cover_grid_u8: K=%d unsupported (2..8)", K);
  DT_REQUIRE(Z >= 1 && Z <= 8, "cover_grid_u8: Z=%d unsupported (1..8)", Z);
  DT_REQUIRE(zones != nullptr || Z == 1, "cover_grid_u8: Z=%d needs a zones map (without one every pixel is zone 0)", Z);
  DT_REQUIRE(gy >= 1 && gx >= 1 && (int64_t)gy * gx * Z * K <= ((int64_t)1 << 26),
             "cover_grid_u8: %d x %d cells of %d bins unsupported (gy * gx * Z * K <= 2^26)", gy, gx, Z * K);
  const int nty = dt_cdiv(h, CV_TH), ntx = dt_cdiv(w, CV_TW);
  hipLaunchKernelGGL(cover_grid_kernel, dim3((unsigned)(nty * ntx)), dim3(256), 0, (hipStream_t)stream, classes, zones, h, w, K,
                     Z, yq, gy, xq, gx, ntx, (unsigned long long*)sums, err_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
