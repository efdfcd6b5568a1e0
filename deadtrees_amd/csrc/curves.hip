// Operating points (deadtrees_amd/loss/curves.py holds the contract): the per-class histogram of the predicted
// probability split by ground truth, accumulated on the device during validation, and the decision kernel that applies a
// threshold per class to stitched probabilities.  Both ends quantise a probability to the same 16-bit integer q (the rule
// of attributes.hip's confidence: clip to [0, 1], NaN -> 0, floor(p * 65535 + 0.5) in two fp32 roundings), so a curve
// read at a threshold describes the maps decided at that threshold exactly.  Counts are integers: the histogram does not
// depend on the order in which pixels, workgroups, batches or ranks arrive.
//
// dt_prob_histogram: one 256-lane workgroup per CURVE_CHUNK consecutive pixels of the B * H * W pixel axis (a chunk may
// straddle two images), uncapped grid.  A lane takes 4 consecutive pixels per step: one 16-byte load per class plane
// where that plane's offset is a multiple of 4 floats (plane starts are H * W floats apart: with H * W % 4 != 0 the planes
// that do not line up, and every group that straddles an image or the end, are read scalar-wise).  Logits go through
// loss_softmax, the project's one softmax.  The workgroup's histogram is 2 * K * 2 * 256 uint32 counters in LDS (32 KB at
// K = 8; a chunk cannot overflow 32 bits).  A real map puts almost every pixel of a wave into the same two counters per
// class, which plain LDS atomics would serialise: the lanes that share the counter of the first pending lane are found
// with a ballot and added as ONE popcount by that lane, CURVE_ROUNDS times; what is left goes through plain LDS atomics.
// The forest-mask bit travels in the key, so a group's leader adds to both planes.  Non-zero counters are flushed with
// 64-bit integer atomics.  No workgroup waits for another, no scalar leaves the device.
#include <limits.h>

#include "conv_host.h"
#include "loss_softmax.h"

#define CURVE_CHUNK 16384                // pixels per workgroup: 512 workgroups at B = 32, 512 x 512
#define CURVE_MAXK 8                     // classes
#define CURVE_BINS 256                   // bin = q >> 8
#define CURVE_ROUNDS 2                   // ballot rounds before the plain atomics
#define CURVE_STEP (256 * 4)             // pixels a workgroup takes per step

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

static_assert(CURVE_CHUNK % CURVE_STEP == 0, "a chunk is a whole number of steps");

// THE quantisation of the contract: two roundings, never fused
__device__ __forceinline__ unsigned curve_q(float p) {
  const float clipped = fminf(p > 0.f ? p : 0.f, 1.f);                               // NaN -> 0
  return (unsigned)floorf(__fadd_rn(__fmul_rn(clipped, 65535.f), 0.5f));
}

// 4 consecutive int64 from element g on (zeros past n); two 16-byte loads where the group is whole and the plane aligned
__device__ __forceinline__ void curve_load4_i64(const int64_t* __restrict__ base, int64_t g, int64_t n, bool vec,
                                                int64_t (&out)[4]) {
  if (vec && g + 3 < n) {
    const i64x2 a = *reinterpret_cast<const i64x2*>(base + g), b = *reinterpret_cast<const i64x2*>(base + g + 2);
    out[0] = a[0], out[1] = a[1], out[2] = b[0], out[3] = b[1];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = g + j < n ? base[g + j] : 0;
  }
}

// One count of counter key >> 1 in plane 0 and, with bit 0 of the key, in plane 1.  Every lane of the wave calls it.
template <int K>
__device__ __forceinline__ void curve_count(unsigned* __restrict__ h, unsigned key, bool pending, int lane) {
  constexpr int PLANE = K * 2 * CURVE_BINS;
#pragma unroll
  for (int r = 0; r < CURVE_ROUNDS; ++r) {
    const unsigned long long live = __ballot(pending);
    if (live == 0) return;
    const int leader = __ffsll((long long)live) - 1;
    const unsigned lk = (unsigned)__shfl((int)key, leader, 64);
    const bool same = pending && key == lk;
    const unsigned long long group = __ballot(same);
    if (lane == leader) {
      const unsigned cnt = (unsigned)__popcll(group);
      atomicAdd(&h[lk >> 1], cnt);
      if (lk & 1u) atomicAdd(&h[PLANE + (lk >> 1)], cnt);
    }
    pending = pending && !same;
  }
  if (pending) {
    atomicAdd(&h[key >> 1], 1u);
    if (key & 1u) atomicAdd(&h[PLANE + (key >> 1)], 1u);
  }
}

// align: bit 0 src, bit 1 labels, bit 2 lu, bit 3 q_out are 16-byte (q_out: 8-byte) aligned
template <int K, bool LOGITS>
__global__ __launch_bounds__(256) void prob_histogram_kernel(const float* __restrict__ src, const int64_t* __restrict__ labels,
                                                             const int64_t* __restrict__ lu,
                                                             unsigned long long* __restrict__ hist, int32_t* __restrict__ err,
                                                             uint16_t* __restrict__ q_out, int64_t n, int64_t HW, int align) {
  constexpr int NH = 2 * K * 2 * CURVE_BINS;
  __shared__ unsigned h[NH];
  const int t = threadIdx.x, lane = t & 63;
  for (int i = t; i < NH; i += 256) h[i] = 0;
  __syncthreads();
  const int64_t c0 = (int64_t)blockIdx.x * CURVE_CHUNK;
  const int64_t c1 = c0 + CURVE_CHUNK < n ? c0 + CURVE_CHUNK : n;
  for (int64_t s0 = c0; s0 < c1; s0 += CURVE_STEP) {
    if (s0 + (t - lane) * 4 >= c1) break;                // the whole wave is past the chunk (wave-uniform)
    const int64_t g = s0 + 4 * t;                        // this lane's pixels g .. g + 3; c1 - c0 % 4 == 0 unless c1 == n
    const int64_t b = g / HW, p = g - b * HW;
    const bool whole = g + 3 < n && p + 3 < HW;          // four pixels of one image
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t off = (b * K + k) * HW + p;
      if (whole && (align & 1) && (off & 3) == 0) {
        const f32x4 q4 = *reinterpret_cast<const f32x4*>(src + off);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = q4[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t i = g + j, bj = i / HW;
          v[k][j] = i < n ? src[(bj * K + k) * HW + (i - bj * HW)] : 0.f;
        }
      }
    }
    int64_t lab[4], forest[4] = {0, 0, 0, 0};
    curve_load4_i64(labels, g, n, (align & 2) != 0, lab);
    if (lu) curve_load4_i64(lu, g, n, (align & 4) != 0, forest);
    unsigned q[K][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float z[K];
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = v[k][j];
      if constexpr (LOGITS) loss_softmax<K>(z, z);
#pragma unroll
      for (int k = 0; k < K; ++k) q[k][j] = curve_q(z[k]);
    }
    if (q_out) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t off = (b * K + k) * HW + p;
        if (whole && (align & 8) && (off & 3) == 0) {
          *reinterpret_cast<u16x4*>(q_out + off) =
              u16x4{(unsigned short)q[k][0], (unsigned short)q[k][1], (unsigned short)q[k][2], (unsigned short)q[k][3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int64_t i = g + j, bj = i / HW;
            if (i < n) q_out[(bj * K + k) * HW + (i - bj * HW)] = (uint16_t)q[k][j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool there = g + j < n;
      const bool ok = there && lab[j] >= 0 && lab[j] < K;      // dt_confusion_matrix's rule: flag and skip
      if (there && !ok) err[0] = 1;
      const unsigned masked = forest[j] == 1 ? 1u : 0u;         // lu NULL: nothing enters plane 1
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const unsigned truth = lab[j] == k ? 1u : 0u;
        const unsigned key = (((unsigned)k * 2u + truth) * CURVE_BINS + (q[k][j] >> 8)) * 2u + masked;
        curve_count<K>(h, key, ok, lane);
      }
    }
  }
  __syncthreads();
  for (int i = t; i < NH; i += 256)
    if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// ---------------------------------------------------------------- entry points
extern "C" int dt_curve_chunk(int* chunk) {
  DT_REQUIRE(chunk, "curve_chunk: null pointer");
  *chunk = CURVE_CHUNK;
  return DT_OK;
}

template <int K>
static void curve_launch(bool logits, dim3 grid, hipStream_t st, const float* src, const int64_t* labels, const int64_t* lu,
                         int64_t* hist, int32_t* err, uint16_t* q_out, int64_t n, int64_t HW, int align) {
  if (logits)
    hipLaunchKernelGGL((prob_histogram_kernel<K, true>), grid, dim3(256), 0, st, src, labels, lu, (unsigned long long*)hist, err,
                       q_out, n, HW, align);
  else
    hipLaunchKernelGGL((prob_histogram_kernel<K, false>), grid, dim3(256), 0, st, src, labels, lu, (unsigned long long*)hist, err,
                       q_out, n, HW, align);
}

static inline bool curve_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

extern "C" int dt_prob_histogram(const float* src, const int64_t* labels, const int64_t* lu, int64_t* hist, int32_t* err_flag,
                                 uint16_t* q_out, int B, int K, int H, int W, int is_logits, void* stream) {
  DT_REQUIRE(src && labels && hist && err_flag, "prob_histogram: null pointer");
  DT_REQUIRE(B > 0 && H > 0 && W > 0, "prob_histogram: B=%d H=%d W=%d must be positive", B, H, W);
  DT_REQUIRE(K >= 2 && K <= CURVE_MAXK, "prob_histogram: K=%d unsupported (2..%d)", K, CURVE_MAXK);
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const int64_t chunks = (n + CURVE_CHUNK - 1) / CURVE_CHUNK;
  DT_REQUIRE(chunks <= INT_MAX, "prob_histogram: %lld pixels are more than one launch takes", (long long)n);
  const int align = (curve_aligned(src, 16) ? 1 : 0) | (curve_aligned(labels, 16) ? 2 : 0) |
                    (lu && curve_aligned(lu, 16) ? 4 : 0) | (q_out && curve_aligned(q_out, 8) ? 8 : 0);
  const dim3 grid((unsigned)chunks);
  hipStream_t st = (hipStream_t)stream;
#define CURVE_CASE(k) \
  case k: curve_launch<k>(is_logits != 0, grid, st, src, labels, lu, hist, err_flag, q_out, n, HW, align); break
  switch (K) {
    CURVE_CASE(2);
    CURVE_CASE(3);
    CURVE_CASE(4);
    CURVE_CASE(5);
    CURVE_CASE(6);
    CURVE_CASE(7);
    CURVE_CASE(8);
  }
#undef CURVE_CASE
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---------------------------------------------------------------- decision
// Pixel i takes the class c >= 1 with the largest q_c(i) among those with q_c(i) >= T_c (ties -> the smallest c), class 0
// without one.  4 pixels per lane, one 16-byte load per class plane where it lines up; plane 0 is never read.
struct curve_thresholds {
  unsigned t[CURVE_MAXK];
};

__global__ __launch_bounds__(256) void decide_classes_kernel(const float* __restrict__ probs, curve_thresholds thr,
                                                             uint8_t* __restrict__ out, int K, int64_t n, int align) {
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g >= n) return;
  const bool whole = g + 3 < n;
  unsigned best[4] = {0u, 0u, 0u, 0u}, bq[4] = {0u, 0u, 0u, 0u};
  for (int c = 1; c < K; ++c) {
    const int64_t off = (int64_t)c * n + g;
    float v[4];
    if (whole && (align & 1) && (off & 3) == 0) {
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(probs + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q4[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = g + j < n ? probs[off + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned q = curve_q(v[j]);
      if (q >= thr.t[c] && (best[j] == 0u || q > bq[j])) {
        best[j] = (unsigned)c;
        bq[j] = q;
      }
    }
  }
  if (whole && (align & 2)) {
    *reinterpret_cast<unsigned*>(out + g) = best[0] | (best[1] << 8) | (best[2] << 16) | (best[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (g + j < n) out[g + j] = (uint8_t)best[j];
  }
}

extern "C" int dt_decide_classes_u8(const float* probs, const uint16_t* thresholds, uint8_t* out_u8, int K, int64_t n,
                                    void* stream) {
  DT_REQUIRE(probs && thresholds && out_u8, "decide_classes_u8: null pointer");
  DT_REQUIRE(K >= 2 && K <= CURVE_MAXK, "decide_classes_u8: K=%d unsupported (2..%d)", K, CURVE_MAXK);
  DT_REQUIRE(n >= 1, "decide_classes_u8: n=%lld pixels", (long long)n);
  curve_thresholds thr;
  for (int c = 0; c < CURVE_MAXK; ++c) thr.t[c] = 0u;
  for (int c = 1; c < K; ++c) {
    DT_REQUIRE(thresholds[c] >= 1, "decide_classes_u8: the threshold of class %d must be in 1..65535", c);
    thr.t[c] = thresholds[c];
  }
  const int64_t groups = (n + CURVE_STEP - 1) / CURVE_STEP;
  DT_REQUIRE(groups <= INT_MAX, "decide_classes_u8: %lld pixels are more than one launch takes", (long long)n);
  const int align = (curve_aligned(probs, 16) ? 1 : 0) | (curve_aligned(out_u8, 4) ? 2 : 0);
  hipLaunchKernelGGL(decide_classes_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, probs, thr, out_u8, K, n,
                     align);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
