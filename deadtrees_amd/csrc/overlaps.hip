// Patch overlaps (deployment/overlaps.py holds the contract): for two label planes LA, LB int32 [h][w] that already sit in
// HBM, the runs of equal pair keys in flat row-major order — the raw material of the overlap table (a, b, n).
//
// key(p) = ((int64)LA[p] << 32) | (uint32)LB[p] where both labels are > 0, else 0.  A run is a maximal stretch of
// consecutive pixels with one key (a run may wrap around a row end: it adds to the same pair); pixel p is a run head iff
// p == 0 or key(p) != key(p - 1).  Every pixel lies in exactly one run, so the length of run r is start[r + 1] - start[r]
// (h * w - start[R - 1] for the last one).  Two launches, a kernel boundary between them (no workgroup waits for
// another, every loop bound is known at launch, no atomics):
//   count   a workgroup of 256 lanes per OV_CHUNK = 1024 consecutive pixels, 4 pixels per lane from one 16-byte load per
//           plane: the chunk's run heads, and how many of them carry a key other than 0
//   runs    the same walk + compaction in row-major order (ballot and popcount within a wave, LDS across the four waves):
//           key[r] and start[r] of every run
// Sorting the R runs by key and summing the lengths of equal keys is left to the caller (a sort and a scan over runs).
// The result is a pure function of the two planes.
//
// A plane handed in by a caller is read defensively: a value <= 0 is background, and a run index is checked against R.
#include "conv_host.h"

#define OV_CHUNK 1024                    // pixels per workgroup: 256 lanes of 4 consecutive pixels
static_assert(OV_CHUNK == 4 * 256, "a lane takes one 16-byte load of each plane");

__device__ __forceinline__ int64_t ov_key(int a, int b) {
  return (a > 0 && b > 0) ? (int64_t)(((uint64_t)(uint32_t)a << 32) | (uint32_t)b) : (int64_t)0;
}

// the keys of the lane's pixels p0 .. p0 + 3 (0 behind the raster's end) and, bit k, whether pixel p0 + k is a run head.
// The predecessor of a lane's first pixel is the last pixel of the lane below; the first lane of a wave loads it
__device__ __forceinline__ int ov_heads(const int32_t* __restrict__ LA, const int32_t* __restrict__ LB, int64_t n, int64_t p0,
                                        int64_t key[4]) {
  int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  if (p0 + 3 < n) {                        // p0 % 4 == 0 and the planes are 16-byte aligned
    const int4 va = *reinterpret_cast<const int4*>(LA + p0), vb = *reinterpret_cast<const int4*>(LB + p0);
    a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
    b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
  } else {                                 // the h * w % 4 tail, and the lanes behind it
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (p0 + k < n) {
        a[k] = LA[p0 + k];
        b[k] = LB[p0 + k];
      }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) key[k] = ov_key(a[k], b[k]);
  const int lane = threadIdx.x & 63;
  int pa = __shfl_up(a[3], 1, 64), pb = __shfl_up(b[3], 1, 64);
  if (lane == 0 && p0 > 0 && p0 < n) {
    pa = LA[p0 - 1];
    pb = LB[p0 - 1];
  }
  const int64_t before = ov_key(pa, pb);
  int heads = 0;
  if (p0 < n) heads |= (p0 == 0 || key[0] != before);
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (p0 + k < n) heads |= (key[k] != key[k - 1]) << k;
  return heads;
}

// counts int32 [chunks][2]: the run heads of the chunk, and those among them whose key is not 0
__global__ __launch_bounds__(256) void overlap_count_kernel(const int32_t* __restrict__ LA, const int32_t* __restrict__ LB,
                                                            int64_t n, int32_t* __restrict__ counts) {
  __shared__ int wsum[4][2];
  const int64_t p0 = (int64_t)blockIdx.x * OV_CHUNK + 4 * (int64_t)threadIdx.x;
  int64_t key[4];
  const int heads = ov_heads(LA, LB, n, p0, key);
  int all = 0, live = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    all += __popcll(__ballot(heads >> k & 1));
    live += __popcll(__ballot((heads >> k & 1) && key[k] != 0));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wsum[wave][0] = all;
    wsum[wave][1] = live;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[2 * (int64_t)blockIdx.x] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
    counts[2 * (int64_t)blockIdx.x + 1] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
  }
}

// chunk_first int32 [chunks]: the runs in front of the chunk.  Writes key[r] and start[r] of every run, r ascending with
// the run's first pixel
__global__ __launch_bounds__(256) void overlap_runs_kernel(const int32_t* __restrict__ LA, const int32_t* __restrict__ LB,
                                                           int64_t n, const int32_t* __restrict__ chunk_first, int R,
                                                           int64_t* __restrict__ run_key, int32_t* __restrict__ run_start) {
  __shared__ int wsum[4];
  const int64_t p0 = (int64_t)blockIdx.x * OV_CHUNK + 4 * (int64_t)threadIdx.x;
  int64_t key[4];
  const int heads = ov_heads(LA, LB, n, p0, key);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  int rank = 0, total = 0;                 // the heads of the wave in front of this lane's pixels, and all of them
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t m = __ballot(heads >> k & 1);
    rank += __popcll(m & below);
    total += __popcll(m);
  }
  if (lane == 0) wsum[wave] = total;
  __syncthreads();
  int r = chunk_first[blockIdx.x] + rank;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < wave) r += wsum[k];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (heads >> k & 1) {
      if ((unsigned)r < (unsigned)R) {
        run_key[r] = key[k];
        run_start[r] = (int32_t)(p0 + k);
      }
      ++r;
    }
}

// ---------------------------------------------------------------- entry points
#define OV_MAX_PIXELS 2147483646LL       // 2^31 - 2: labels are int32 and 1-based

static int ov_check(const char* tag, const int32_t* la, const int32_t* lb, int h, int w) {
  DT_REQUIRE(la && lb, "%s: null pointer", tag);
  DT_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= OV_MAX_PIXELS, "%s: raster %dx%d must hold 1..2^31-2 pixels", tag, h, w);
  DT_REQUIRE(dt_aligned16(la, lb), "%s: the label planes must be 16-byte aligned", tag);
  return DT_OK;
}

extern "C" int dt_overlap_chunk(int* chunk) {
  DT_REQUIRE(chunk, "overlap_chunk: null pointer");
  *chunk = OV_CHUNK;
  return DT_OK;
}

extern "C" int dt_overlap_count(const int32_t* labels_a, const int32_t* labels_b, int h, int w, int32_t* chunk_counts,
                                void* stream) {
  DT_TRY(ov_check("overlap_count", labels_a, labels_b, h, w));
  DT_REQUIRE(chunk_counts, "overlap_count: null pointer");
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(overlap_count_kernel, dim3((unsigned)((n + OV_CHUNK - 1) / OV_CHUNK)), dim3(256), 0, (hipStream_t)stream,
                     labels_a, labels_b, n, chunk_counts);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_overlap_runs(const int32_t* labels_a, const int32_t* labels_b, int h, int w, const int32_t* chunk_first,
                               int n_runs, int64_t* run_key, int32_t* run_start, void* stream) {
  DT_TRY(ov_check("overlap_runs", labels_a, labels_b, h, w));
  DT_REQUIRE(chunk_first && run_key && run_start, "overlap_runs: null pointer");
  const int64_t n = (int64_t)h * w;
  DT_REQUIRE(n_runs >= 1 && n_runs <= n, "overlap_runs: n_runs=%d for %lld pixels", n_runs, (long long)n);
  hipLaunchKernelGGL(overlap_runs_kernel, dim3((unsigned)((n + OV_CHUNK - 1) / OV_CHUNK)), dim3(256), 0, (hipStream_t)stream,
                     labels_a, labels_b, n, chunk_first, n_runs, run_key, run_start);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
