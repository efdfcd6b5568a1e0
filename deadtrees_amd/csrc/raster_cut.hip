// Training samples straight from an ortho raster (the array arithmetic of the reference's scripts/createdataset.py:53-194 and
// scripts/computestats.py:111-161; deadtrees_amd/data/rasters.py states the contract in numpy).  A raster rgbn uint8 [4][h][w]
// with h, w <= S stands in the top-left corner of a zero [4][S][S] array, its mask and land-use map likewise; the array is cut
// into n = (S / t)^2 sub-tiles of t x t in make_blocks_vectorized's order.  One pass over the bytes gives, per sub-tile, the
// census row (dead pixels, min / max, the bytes not in {0, 255}, the per-band sums and sums of squares: what the blank filter,
// the dead percentage, the status flag and the band statistics are functions of) and, for the sub-tiles that `slot` names, the
// sample in DevicePool's layout: the four bands interleaved, mask, land-use map and the byte sum of the image.
//
// Work split: a workgroup owns RC_QUADS * 256 quads (a quad is 4 pixels side by side in one row) of ONE sub-tile, so a 256 x 256
// sub-tile is shared by 16 workgroups and a 2048^2 raster is 1024 workgroups.  A lane sums its 16 pixels in registers, a wave
// combines its lanes with a butterfly, the four waves meet once in LDS, and the workgroup issues one 64-bit integer atomic per
// census column (14) and one for sums[]: 15 * 16 atomics per 384 KiB sample.  Integers only: exact, and independent of the
// split and of the order.  The rows are preset (zeros; 255 for the minima) by a small launch of its own on the same stream.
//
// 32-bit partials: a lane holds 16 pixels, a workgroup 4096.  Per band sum <= 4096 * 255 < 2^21 and sumsq <= 4096 * 65025 =
// 266 342 400 < 2^32, the counts <= 16384: every partial up to and including the workgroup's fits uint32; the global columns
// are 64-bit (sumsq of one band of a 256^2 sub-tile reaches 65536 * 65025 = 4 261 478 400: past 2^31 and 0.8 % short of
// 2^32; a 512^2 sub-tile reaches four times that).
//
// Source rows start at any byte: w is arbitrary and the three maps may be views into one upload.  A quad is fetched as the one
// or two ALIGNED dwords that hold its valid bytes, shifted together in registers; the second dword is read only when one of the
// quad's valid bytes lies in it, so no load touches a dword that lies wholly outside the array.  Bytes right of w or below h
// are not read at all: they are the zero padding (land use without a map: ones).  Pool rows are 4-byte aligned: the image quad
// is one 16-byte store when the pool's base allows it and four dword stores otherwise.
#include "conv_host.h"

#define RC_THREADS 256
#define RC_QUADS 4                                   // quads per lane
#define RC_WG_QUADS (RC_THREADS * RC_QUADS)          // quads per workgroup: 4096 pixels
#define RC_COLS 14                                   // census columns in use; DT_CENSUS_COLS = 16 with the padding
#define RC_HI 0x80808080u
#define RC_LO 0x7f7f7f7fu

// bytes p[0 .. nv) in the low bytes of a dword, zeros above; 0 <= nv <= 4
__device__ __forceinline__ uint32_t rc_load_quad(const uint8_t* __restrict__ p, int nv) {
  if (nv <= 0) return 0u;
  const unsigned s = (unsigned)((uintptr_t)p & 3u);
  const uint32_t* __restrict__ w = (const uint32_t*)(p - s);       // holds p[0]: a byte of the array
  const uint32_t lo = w[0];
  const uint32_t hi = (s + (unsigned)nv > 4u) ? w[1] : 0u;          // holds p[nv - 1] when it is read
  const uint32_t v = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * s));
  return nv >= 4 ? v : (v & ((1u << (8 * nv)) - 1u));
}

// bit 7 of every non-zero byte
__device__ __forceinline__ uint32_t rc_nonzero(uint32_t x) { return (((x & RC_LO) + RC_LO) | x) & RC_HI; }

__device__ __forceinline__ uint32_t rc_byte(uint32_t x, int p) { return (x >> (8 * p)) & 0xffu; }

__device__ __forceinline__ uint32_t rc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t rc_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t rc_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// census rows to their neutral values; sums[] of the rows that slot names to zero
__global__ __launch_bounds__(RC_THREADS) void raster_cut_init_kernel(int n, const int32_t* __restrict__ slot,
                                                                     int64_t pool_rows, unsigned long long* __restrict__ sums,
                                                                     unsigned long long* __restrict__ census) {
  const int64_t j = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (j >= (int64_t)n * DT_CENSUS_COLS) return;
  if (census) {
    const int col = (int)(j % DT_CENSUS_COLS);
    census[j] = (col == DT_CENSUS_VMIN || col == DT_CENSUS_B0MIN) ? 255ull : 0ull;
  }
  if (slot && j < n) {
    const int64_t row = slot[j];
    if (row >= 0 && row < pool_rows) sums[row] = 0ull;
  }
}

__global__ __launch_bounds__(RC_THREADS) void raster_cut_kernel(
    const uint8_t* __restrict__ rgbn, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ lu, int h, int w, int S,
    int t, int chunks, const int32_t* __restrict__ slot, int64_t pool_rows, int wide, uint8_t* __restrict__ images,
    uint8_t* __restrict__ masks, uint8_t* __restrict__ lu_out, unsigned long long* __restrict__ sums,
    unsigned long long* __restrict__ census) {
  __shared__ uint32_t part[RC_THREADS / 64][RC_COLS];
  const int tile = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
  const int nb = S / t, qpr = t >> 2, Q = qpr * t;          // sub-tiles per side; quads per row and per sub-tile
  const int y0 = (tile / nb) * t, x0 = (tile % nb) * t;
  int64_t row = slot ? (int64_t)slot[tile] : -1;
  if (row >= pool_rows) row = -1;
  const int64_t plane = (int64_t)h * w, tt = (int64_t)t * t;

  uint32_t dead = 0, mid = 0, vmin = 255u, vmax = 0u, b0min = 255u, b0max = 0u;
  uint32_t sum[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < RC_QUADS; ++k) {
    const int q = chunk * RC_WG_QUADS + k * RC_THREADS + (int)threadIdx.x;
    if (q >= Q) continue;
    const int ly = q / qpr, lx = (q - ly * qpr) * 4;
    const int y = y0 + ly, x = x0 + lx;
    const int nv = y < h ? min(max(w - x, 0), 4) : 0;
    const int64_t at = (int64_t)y * w + x;                          // (used only when nv > 0)
    uint32_t b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = rc_load_quad(rgbn + c * plane + at, nv);
    const uint32_t m = mask ? rc_load_quad(mask + at, nv) : 0u;
    const uint32_t l = lu ? rc_load_quad(lu + at, nv) : 0x01010101u;

    dead += (uint32_t)__popc(rc_nonzero(m));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mid += (uint32_t)__popc(rc_nonzero(b[c]) & rc_nonzero(~b[c]));
      uint32_t lo = 255u, hi = 0u;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t v = rc_byte(b[c], p);
        sum[c] += v;
        sq[c] += v * v;
        lo = min(lo, v);
        hi = max(hi, v);
      }
      vmin = min(vmin, lo);
      vmax = max(vmax, hi);
      if (c == 0) {
        b0min = min(b0min, lo);
        b0max = max(b0max, hi);
      }
    }

    if (row >= 0) {
      uint32_t px[4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
        px[p] = rc_byte(b[0], p) | (rc_byte(b[1], p) << 8) | (rc_byte(b[2], p) << 16) | (rc_byte(b[3], p) << 24);
      const int64_t o = row * tt + (int64_t)ly * t + lx;            // pixel of the pool; o % 4 == 0
      uint32_t* __restrict__ ip = (uint32_t*)(images + 4 * o);
      if (wide) {
        u32x4 v4;
        v4[0] = px[0]; v4[1] = px[1]; v4[2] = px[2]; v4[3] = px[3];
        *(u32x4*)ip = v4;
      } else {
        ip[0] = px[0]; ip[1] = px[1]; ip[2] = px[2]; ip[3] = px[3];
      }
      *(uint32_t*)(masks + o) = m;
      *(uint32_t*)(lu_out + o) = l;
    }
  }

  uint32_t red[RC_COLS];
  red[DT_CENSUS_DEAD] = rc_wave_sum(dead);
  red[DT_CENSUS_VMIN] = rc_wave_min(vmin);
  red[DT_CENSUS_VMAX] = rc_wave_max(vmax);
  red[DT_CENSUS_B0MIN] = rc_wave_min(b0min);
  red[DT_CENSUS_B0MAX] = rc_wave_max(b0max);
  red[DT_CENSUS_MID] = rc_wave_sum(mid);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    red[DT_CENSUS_SUM + c] = rc_wave_sum(sum[c]);
    red[DT_CENSUS_SUMSQ + c] = rc_wave_sum(sq[c]);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < RC_COLS; ++i) part[wave][i] = red[i];
  }
  __syncthreads();
  if (threadIdx.x < RC_COLS) {
    const int i = threadIdx.x;
    const uint32_t a = part[0][i], b1 = part[1][i], c2 = part[2][i], d3 = part[3][i];
    const bool is_min = i == DT_CENSUS_VMIN || i == DT_CENSUS_B0MIN, is_max = i == DT_CENSUS_VMAX || i == DT_CENSUS_B0MAX;
    const uint32_t v = is_min ? min(min(a, b1), min(c2, d3)) : is_max ? max(max(a, b1), max(c2, d3)) : a + b1 + c2 + d3;
    if (census) {
      unsigned long long* dst = census + (int64_t)tile * DT_CENSUS_COLS + i;
      if (is_min) atomicMin(dst, (unsigned long long)v);
      else if (is_max) atomicMax(dst, (unsigned long long)v);
      else if (v) atomicAdd(dst, (unsigned long long)v);
    }
  }
  if (threadIdx.x == 0 && row >= 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      total += (unsigned long long)part[0][DT_CENSUS_SUM + c] + part[1][DT_CENSUS_SUM + c] + part[2][DT_CENSUS_SUM + c] +
               part[3][DT_CENSUS_SUM + c];
    if (total) atomicAdd(sums + row, total);
  }
}

extern "C" int dt_raster_cut_u8(const uint8_t* rgbn_chw, const uint8_t* mask, const uint8_t* lu, int h, int w, int S, int t,
                                const int32_t* slot, int64_t pool_rows, uint8_t* images, uint8_t* masks, uint8_t* lu_out,
                                uint64_t* sums, int64_t* census, void* stream) {
  DT_REQUIRE(rgbn_chw != nullptr, "raster_cut_u8: null rgbn");
  DT_REQUIRE(t >= 32 && t % 32 == 0, "raster_cut_u8: tile size t=%d must be a positive multiple of 32", t);
  DT_REQUIRE(S >= t && S % t == 0, "raster_cut_u8: source_dim S=%d must be a multiple of the tile size t=%d", S, t);
  DT_REQUIRE(S <= 32768, "raster_cut_u8: source_dim S=%d unsupported (<= 32768)", S);
  DT_REQUIRE(h >= 1 && h <= S && w >= 1 && w <= S, "raster_cut_u8: raster %dx%d must be 1..S=%d in height and width", h, w, S);
  DT_REQUIRE(slot != nullptr || census != nullptr, "raster_cut_u8: slot and census are both null: nothing to do");
  if (slot) {
    DT_REQUIRE(images && masks && lu_out && sums, "raster_cut_u8: slot given but an output pointer is null");
    DT_REQUIRE(pool_rows >= 1, "raster_cut_u8: pool_rows=%lld must be >= 1 with a slot table", (long long)pool_rows);
    DT_REQUIRE(((uintptr_t)images & 3) == 0 && ((uintptr_t)masks & 3) == 0 && ((uintptr_t)lu_out & 3) == 0,
               "raster_cut_u8: images, masks and lu_out must be 4-byte aligned");
    DT_REQUIRE(((uintptr_t)sums & 7) == 0, "raster_cut_u8: sums must be 8-byte aligned");
  }
  DT_REQUIRE(((uintptr_t)census & 7) == 0, "raster_cut_u8: census must be 8-byte aligned");
  const int nb = S / t, n = nb * nb;
  const int chunks = dt_cdiv((int64_t)t * t / 4, RC_WG_QUADS);
  const int64_t wgs = (int64_t)n * chunks;
  DT_REQUIRE(wgs <= 0x7fffffffLL, "raster_cut_u8: %lld workgroups exceed the grid", (long long)wgs);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(raster_cut_init_kernel, dim3(dt_cdiv((int64_t)n * DT_CENSUS_COLS, RC_THREADS)), dim3(RC_THREADS), 0, st,
                     n, slot, pool_rows, (unsigned long long*)sums, (unsigned long long*)census);
  DT_LAUNCH_CHECK();
  const int wide = slot && ((uintptr_t)images & 15) == 0;
  hipLaunchKernelGGL(raster_cut_kernel, dim3((unsigned)wgs), dim3(RC_THREADS), 0, st, rgbn_chw, mask, lu, h, w, S, t, chunks,
                     slot, pool_rows, wide, images, masks, lu_out, (unsigned long long*)sums, (unsigned long long*)census);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
