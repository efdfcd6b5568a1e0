// Raster statistics (scripts/computestats_inference.py, scripts/aggregate_results.py, deployment/server.py:112 of the
// reference): class counts per zone of a uint8 class map that already sits in HBM, so that the numbers are taken before the
// map is downloaded.  counts[z][c] += #{i < n : zones[i] == z, classes[i] == c}; integers only: exact, order independent.
//
// A real map is > 95 % one class: a per-pixel LDS atomic (confusion_kernel's scheme) would send all 64 lanes of a wave to
// one LDS word.  Here every lane counts privately in registers, a wave combines its lanes once with a butterfly, the four
// waves of a workgroup meet once in LDS, and a workgroup issues at most one 64-bit global atomic per non-empty bin.
//
// Bytes, not words: the maps handed in are crops and slices (member m of a stacked [M, h, w] tensor with odd h * w), so
// neither pointer is aligned and the two may be misaligned differently.  The pixels before the first 16-byte boundary of
// `classes` (the head, < 16) and those after the last full 16 bytes (the tail, < 16) are read byte by byte by two lanes of
// workgroup 0; the body is one aligned 16-byte load per lane of `classes` and, for `zones`, the one or two ALIGNED 16-byte
// words that hold the same 16 pixels, shifted together in registers.  Both words contain at least one byte of the zones
// array (shown at the load), so no load touches a 16-byte granule that lies wholly outside the array.
//
// Counting is byte-parallel inside a dword.  A pixel becomes the code z * 8 + c < 64; a pixel that enters no count (class
// >= K, zone >= Z, or a padding byte of the head / tail vector) becomes 0x7f.  All codes are < 0x80, so for a bin b the sum
// (code ^ b) + 0x7f has bit 7 set exactly in the bytes that differ from b, without a carry between bytes.
#include "conv_host.h"

#define RS_MAXK 8
#define RS_MAXZ 8
#define RS_CAP 512          // grid cap: two workgroups per CU; each workgroup ends with <= Z * K global atomics
#define RS_HI 0x80808080u
#define RS_LO 0x7f7f7f7fu

// bit 7 of every byte of x that is >= L; lim = (0x80 - L) * 0x01010101 with 1 <= L <= 8.  (x & 0x7f) + (0x80 - L) <= 0xfd:
// no carry; it reaches 0x80 exactly when the low seven bits are >= L, and `| x` covers the bytes >= 0x80
__device__ __forceinline__ uint32_t rs_ge(uint32_t x, uint32_t lim) { return (((x & RS_LO) + lim) | x) & RS_HI; }

__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// 16 pixels: cw / zw hold their class / zone bytes, skip has bit 7 set in the bytes that are not pixels
template <int KC, int ZC>
__device__ __forceinline__ void rs_count16(const uint32_t (&cw)[4], const uint32_t (&zw)[4], const uint32_t (&skip)[4],
                                           uint32_t klim, uint32_t zlim, uint32_t (&cnt)[KC * ZC], uint32_t& flag) {
  uint32_t code[4], badc = 0, badz = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t gc = rs_ge(cw[j], klim) & ~skip[j], gz = rs_ge(zw[j], zlim) & ~skip[j];
    badc |= gc;
    badz |= gz;
    const uint32_t dead = ((gc | gz | skip[j]) >> 7) * 0x7fu;          // 0x7f in every byte that enters no count
    code[j] = (cw[j] & 0x07070707u) | ((zw[j] & 0x07070707u) << 3) | dead;
  }
  flag |= (badc ? 1u : 0u) | (badz ? 2u : 0u);
#pragma unroll
  for (int z = 0; z < ZC; ++z) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const uint32_t b = (uint32_t)(z * 8 + c) * 0x01010101u;
      uint32_t differ = 0;                                             // bit 7 - j of byte p: pixel 4 j + p is not in bin b
#pragma unroll
      for (int j = 0; j < 4; ++j) differ |= (((code[j] ^ b) + RS_LO) & RS_HI) >> j;
      cnt[z * KC + c] += 16u - (uint32_t)__popc(differ);
    }
  }
}

// up to 15 pixels p[0 .. len) read byte by byte into a 16-pixel vector; the remaining bytes are marked in skip
__device__ __forceinline__ void rs_load_edge(const uint8_t* __restrict__ c, const uint8_t* __restrict__ z, int len,
                                             uint32_t (&cw)[4], uint32_t (&zw)[4], uint32_t (&skip)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cw[j] = zw[j] = skip[j] = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (4 * j + p < len) {
        cw[j] |= (uint32_t)c[4 * j + p] << (8 * p);
        if (z) zw[j] |= (uint32_t)z[4 * j + p] << (8 * p);
      } else {
        skip[j] |= 0x80u << (8 * p);
      }
    }
  }
}

// bytes [s, s + 16) of the 32 bytes a || b, 0 < s < 16 (uniform): a dword shift of s / 4 and a byte shift of s % 4
__device__ __forceinline__ void rs_shift16(const u32x4 a, const u32x4 b, unsigned s, uint32_t (&out)[4]) {
  const uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  const unsigned q = s >> 2, r8 = (s & 3u) * 8u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t lo = w[j], hi = w[j + 1];
    if (q == 1) { lo = w[j + 1]; hi = w[j + 2]; }
    if (q == 2) { lo = w[j + 2]; hi = w[j + 3]; }
    if (q == 3) { lo = w[j + 3]; hi = w[j + 4]; }
    out[j] = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> r8);
  }
}

// classes + head is 16-byte aligned; nvec full 16-byte vectors follow it, then tail < 16 pixels.  KC >= K and ZC >= Z are the
// compiled bin counts (the values K .. KC - 1 / Z .. ZC - 1 are out of range like any other and their bins stay zero).
template <int KC, int ZC>
__global__ __launch_bounds__(256) void zonal_counts_kernel(const uint8_t* __restrict__ classes,
                                                           const uint8_t* __restrict__ zones, int head, int64_t nvec,
                                                           int tail, int K, int Z,
                                                           unsigned long long* __restrict__ counts,
                                                           int32_t* __restrict__ err) {
  __shared__ uint32_t part[4][KC * ZC];
  const uint32_t klim = (uint32_t)(0x80 - K) * 0x01010101u, zlim = (uint32_t)(0x80 - Z) * 0x01010101u;
  uint32_t cnt[KC * ZC];
#pragma unroll
  for (int i = 0; i < KC * ZC; ++i) cnt[i] = 0;
  uint32_t flag = 0;
  uint32_t cw[4], zw[4] = {0, 0, 0, 0}, skip[4] = {0, 0, 0, 0};

  const u32x4* __restrict__ cvec = (const u32x4*)(classes + head);
  // zones + head = zal + zs with zal 16-byte aligned, 0 <= zs < 16: pixel vector i is bytes [zs, zs + 16) of zal[i] || zal[i + 1].
  // zal[i] holds zones[head + 16 i] (zs <= 15) and, when zs > 0, zal[i + 1] holds zones[head + 16 i + 15]: pixels of vector i
  const unsigned zs = zones ? (unsigned)((uintptr_t)(zones + head) & 15u) : 0u;
  const u32x4* __restrict__ zal = zones ? (const u32x4*)(zones + head - zs) : nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const u32x4 cv = cvec[i];
    cw[0] = cv[0]; cw[1] = cv[1]; cw[2] = cv[2]; cw[3] = cv[3];
    if (zal) {
      const u32x4 za = zal[i];
      if (zs) {
        rs_shift16(za, zal[i + 1], zs, zw);
      } else {
        zw[0] = za[0]; zw[1] = za[1]; zw[2] = za[2]; zw[3] = za[3];
      }
    }
    rs_count16<KC, ZC>(cw, zw, skip, klim, zlim, cnt, flag);
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {      // lane 0: the head, lane 1: the tail
    const int len = threadIdx.x == 0 ? head : tail;
    const int64_t at = threadIdx.x == 0 ? 0 : head + 16 * nvec;
    if (len > 0) {
      rs_load_edge(classes + at, zones ? zones + at : nullptr, len, cw, zw, skip);
      rs_count16<KC, ZC>(cw, zw, skip, klim, zlim, cnt, flag);
    }
  }
  if (flag) atomicOr(err, (int)flag);

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < KC * ZC; ++i) {
    const uint32_t s = rs_wave_sum(cnt[i]);
    if (lane == 0) part[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < KC * ZC) {
    const int z = threadIdx.x / KC, c = threadIdx.x % KC;
    const unsigned long long s = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                 part[3][threadIdx.x];
    if (z < Z && c < K && s) atomicAdd(&counts[z * K + c], s);
  }
}

extern "C" int dt_zonal_counts_u8(const uint8_t* classes, const uint8_t* zones, int64_t n, int K, int Z, int64_t* counts,
                                  int32_t* err_flag, void* stream) {
  DT_REQUIRE(classes && counts && err_flag, "zonal_counts_u8: null pointer");
  DT_REQUIRE(n >= 1, "zonal_counts_u8: n must be >= 1 (n=%lld)", (long long)n);
  DT_REQUIRE(K >= 2 && K <= RS_MAXK, "zonal_counts_u8: K=%d unsupported (2..%d)", K, RS_MAXK);
  DT_REQUIRE(Z >= 1 && Z <= RS_MAXZ, "zonal_counts_u8: Z=%d unsupported (1..%d)", Z, RS_MAXZ);
  DT_REQUIRE(zones != nullptr || Z == 1, "zonal_counts_u8: Z=%d needs a zones map (without one every pixel is zone 0)", Z);
  const int64_t to_boundary = (int64_t)((16 - ((uintptr_t)classes & 15)) & 15);
  const int head = (int)(to_boundary < n ? to_boundary : n);
  const int64_t nvec = (n - head) / 16;
  const int tail = (int)(n - head - 16 * nvec);
  const dim3 grid(dt_ew_grid(nvec, RS_CAP)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define RS_LAUNCH(KC, ZC)                                                                                              \
  hipLaunchKernelGGL((zonal_counts_kernel<KC, ZC>), grid, block, 0, st, classes, zones, head, nvec, tail, K, Z,         \
                     (unsigned long long*)counts, err_flag)
#define RS_LAUNCH_Z(KC)                       \
  do {                                        \
    if (Z == 1) RS_LAUNCH(KC, 1);             \
    else if (Z == 2) RS_LAUNCH(KC, 2);        \
    else if (Z <= 4) RS_LAUNCH(KC, 4);        \
    else RS_LAUNCH(KC, 8);                    \
  } while (0)
  if (K == 2) RS_LAUNCH_Z(2);
  else if (K == 3) RS_LAUNCH_Z(3);
  else if (K == 4) RS_LAUNCH_Z(4);
  else RS_LAUNCH_Z(8);
#undef RS_LAUNCH_Z
#undef RS_LAUNCH
  DT_LAUNCH_CHECK();
  return DT_OK;
}
