// Operating points (deadtrees_amd/loss/curves.py holds the contract): the per-class histogram of the predicted
// probability split by ground truth, accumulated on the device during validation, and the decision kernel that applies a
// threshold per class to stitched probabilities, pixel by pixel or patch by patch (hysteresis and a confidence filter: the
// last part of this file).  All of them quantise a probability to the same 16-bit integer q (the rule
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
#include "patch_runs.h"

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
// without one.  4 pixels per lane, one 16-byte load per class plane where it lines up; plane 0 is never read.  QOWN (the
// candidates of a patch-wise decision): the winner's q goes into a uint16 plane as well, 0 on class 0.
struct curve_thresholds {
  unsigned t[CURVE_MAXK];
};

// align: bit 0 probs 16-byte, bit 1 out 4-byte, bit 2 q_own 8-byte aligned
template <bool QOWN>
__global__ __launch_bounds__(256) void decide_classes_kernel(const float* __restrict__ probs, curve_thresholds thr,
                                                             uint8_t* __restrict__ out, uint16_t* __restrict__ q_own, int K,
                                                             int64_t n, int align) {
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
  if constexpr (QOWN) {
    if (whole && (align & 4)) {
      *reinterpret_cast<u16x4*>(q_own + g) =
          u16x4{(unsigned short)bq[0], (unsigned short)bq[1], (unsigned short)bq[2], (unsigned short)bq[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g + j < n) q_own[g + j] = (uint16_t)bq[j];
    }
  }
}

// thresholds[1 .. K - 1] -> thr, each in 1..65535
static int curve_read_thresholds(const char* tag, const uint16_t* thresholds, int K, curve_thresholds& thr) {
  for (int c = 0; c < CURVE_MAXK; ++c) thr.t[c] = 0u;
  for (int c = 1; c < K; ++c) {
    DT_REQUIRE(thresholds[c] >= 1, "%s: the threshold of class %d must be in 1..65535", tag, c);
    thr.t[c] = thresholds[c];
  }
  return DT_OK;
}

extern "C" int dt_decide_classes_u8(const float* probs, const uint16_t* thresholds, uint8_t* out_u8, int K, int64_t n,
                                    void* stream) {
  DT_REQUIRE(probs && thresholds && out_u8, "decide_classes_u8: null pointer");
  DT_REQUIRE(K >= 2 && K <= CURVE_MAXK, "decide_classes_u8: K=%d unsupported (2..%d)", K, CURVE_MAXK);
  DT_REQUIRE(n >= 1, "decide_classes_u8: n=%lld pixels", (long long)n);
  curve_thresholds thr;
  DT_TRY(curve_read_thresholds("decide_classes_u8", thresholds, K, thr));
  const int64_t groups = (n + CURVE_STEP - 1) / CURVE_STEP;
  DT_REQUIRE(groups <= INT_MAX, "decide_classes_u8: %lld pixels are more than one launch takes", (long long)n);
  const int align = (curve_aligned(probs, 16) ? 1 : 0) | (curve_aligned(out_u8, 4) ? 2 : 0);
  hipLaunchKernelGGL(decide_classes_kernel<false>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, probs, thr,
                     out_u8, (uint16_t*)nullptr, K, n, align);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---------------------------------------------------------------- patch-wise decision (hysteresis, confidence filter)
// Candidates at the low thresholds (decide_classes_kernel<true>), their label plane (patches.hip), then two launches here:
// the support of every patch — the maximum, the sum and the count of its pixels' own q, in planes indexed by the root
// (label - 1) — and the rejection of the patches that lack a pixel at T_c or a mean of M_c.  Integers only: the planes do
// not depend on the order in which runs arrive.
//
// patch_support_kernel walks the pixels as patch_attributes_kernel does: a wave owns HY_SPAN consecutive 64-pixel chunks,
// pt_runs finds the runs of equal label (a run may wrap a row end: nothing here is geometry), a segmented scan gives every
// run its maximum and its 32-bit partial sum (64 terms of at most 65535), the run still open at the end of a chunk is
// carried in 64 bits, and a finished run writes once per quantity.  Two things keep one raster-sized patch from queueing
// every wave on one address: the atomic max is skipped when a relaxed load already shows a value that is large enough (a
// hint: a stale value only costs the atomic), and the runs the four waves of a workgroup END with go through LDS, where
// equal labels are combined before one lane writes them — a workgroup inside one patch issues one write per quantity.
#define HY_SPAN 16                       // 64-pixel chunks per wave
#define HY_MAX_SIDE 16384
#define HY_MAX_PIXELS 2147483646ll       // labels are int32 and 1-based
#define HY_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct hy_run {
  int label, qmax, count;
  unsigned long long sum;
};

template <bool SUMS>
__device__ __forceinline__ void hy_emit(const hy_run& r, int32_t* __restrict__ qmax, unsigned long long* __restrict__ qsum,
                                        int32_t* __restrict__ area) {
  const int root = r.label - 1;
  if (HY_LOAD(&qmax[root]) < r.qmax) atomicMax(&qmax[root], r.qmax);
  if constexpr (SUMS) {
    atomicAdd(&qsum[root], r.sum);
    atomicAdd(&area[root], r.count);
  }
}

__device__ __forceinline__ void hy_merge(hy_run& into, const hy_run& other) {
  into.qmax = max(into.qmax, other.qmax);
  into.sum += other.sum;
  into.count += other.count;
}

template <bool SUMS>
__global__ __launch_bounds__(256) void patch_support_kernel(const int32_t* __restrict__ labels,
                                                            const uint16_t* __restrict__ q_own, int64_t n,
                                                            int32_t* __restrict__ qmax, unsigned long long* __restrict__ qsum,
                                                            int32_t* __restrict__ area) {
  __shared__ hy_run tail[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * (HY_SPAN * 64);
  hy_run carry = {0, 0, 0, 0ull};                          // wave-uniform: the run left open by the previous chunk
  for (int j = 0; j < HY_SPAN; ++j) {
    const int64_t i = base + j * 64 + lane;
    if (i - lane >= n) break;
    const int label = pt_label_at(labels, i, n);
    if (__ballot(label != 0) == 0) {                      // background only, most chunks of a real map: q_own is not read
      if (lane == 0 && carry.label) hy_emit<SUMS>(carry, qmax, qsum, area);
      carry.label = 0;
      continue;
    }
    const unsigned q = label ? q_own[i] : 0u;             // a label implies i < n
    bool head;
    int len;
    uint64_t heads;
    pt_runs(label, false, lane, head, len, heads);        // len: the distance to the next head, in every lane
    // maximum and sum over the lanes lane .. lane + len - 1; background is never written out, so its lanes take no partner
    const int reach = label ? len : 1;
    unsigned hi = q, sum = q;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = d < reach;
      if (__ballot(take) == 0) break;
      const unsigned other_hi = __shfl_down(hi, d, 64);
      if (take) hi = max(hi, other_hi);
      if constexpr (SUMS) {
        const unsigned other_sum = __shfl_down(sum, d, 64);
        if (take) sum += other_sum;
      }
    }
    hy_run run = {label, (int)hi, len, (unsigned long long)sum};
    const int first = __shfl(label, 0, 64), last_head = 63 - __clzll((long long)heads);
    if (lane == 0 && carry.label) {
      if (carry.label == first) hy_merge(run, carry);
      else hy_emit<SUMS>(carry, qmax, qsum, area);
    }
    if (head && lane != last_head && label) hy_emit<SUMS>(run, qmax, qsum, area);
    carry.label = __shfl(run.label, last_head, 64);
    carry.qmax = __shfl(run.qmax, last_head, 64);
    carry.count = __shfl(run.count, last_head, 64);
    carry.sum = __shfl(run.sum, last_head, 64);
  }
  // the runs the four waves end with (label 0: none; a wave past the plane has none): equal neighbours become one write
  if (lane == 0) tail[wave] = carry;
  __syncthreads();
  if (threadIdx.x != 0) return;
  hy_run open = {0, 0, 0, 0ull};
  for (int k = 0; k < 4; ++k) {
    const hy_run t = tail[k];
    if (t.label == 0) continue;
    if (t.label == open.label) {
      hy_merge(open, t);
    } else {
      if (open.label) hy_emit<SUMS>(open, qmax, qsum, area);
      open = t;
    }
  }
  if (open.label) hy_emit<SUMS>(open, qmax, qsum, area);
}

// In place: a labelled pixel whose patch fails the core test or the confidence filter becomes class 0.  4 pixels per lane,
// one 16-byte load of the labels and one packed 4-byte load and store of the classes where they line up.
// align: bit 0 labels 16-byte, bit 1 classes 4-byte aligned
template <bool SUMS>
__global__ __launch_bounds__(256) void reject_patches_kernel(uint8_t* __restrict__ classes, const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ qmax,
                                                             const long long* __restrict__ qsum,
                                                             const int32_t* __restrict__ area, curve_thresholds thr,
                                                             curve_thresholds conf, int K, int64_t n, int align) {
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (g >= n) return;
  const bool whole = g + 3 < n;
  int label[4];
  if (whole && (align & 1)) {
    const i32x4 l4 = *reinterpret_cast<const i32x4*>(labels + g);
#pragma unroll
    for (int j = 0; j < 4; ++j) label[j] = l4[j] > 0 && l4[j] <= n ? l4[j] : 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) label[j] = pt_label_at(labels, g + j, n);
  }
  if ((label[0] | label[1] | label[2] | label[3]) == 0) return;      // (labels are >= 0 here) background: nothing to write
  const bool packed = whole && (align & 2);
  unsigned cls[4];
  if (packed) {
    const unsigned c4 = *reinterpret_cast<const unsigned*>(classes + g);
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[j] = (c4 >> (8 * j)) & 255u;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[j] = label[j] ? classes[g + j] : 0u;
  }
  // the class a pixel keeps: its own on background and in a kept patch, 0 in a rejected one
  unsigned kept[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned c = cls[j];
    const int root = label[j] ? label[j] - 1 : 0;         // (entry 0 is read for nothing on background)
    bool keep = c >= 1u && c < (unsigned)K && (unsigned)qmax[root] >= thr.t[c & (CURVE_MAXK - 1)];
    if constexpr (SUMS) {
      const unsigned m = conf.t[c & (CURVE_MAXK - 1)];
      if (keep && m) keep = qsum[root] >= (long long)m * area[root];
    }
    kept[j] = keep || label[j] == 0 ? c : 0u;
  }
  if (kept[0] == cls[0] && kept[1] == cls[1] && kept[2] == cls[2] && kept[3] == cls[3]) return;
  if (packed) {
    *reinterpret_cast<unsigned*>(classes + g) = kept[0] | (kept[1] << 8) | (kept[2] << 16) | (kept[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (label[j]) classes[g + j] = (uint8_t)kept[j];
  }
}

static int hy_check_size(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1 && h <= HY_MAX_SIDE && w <= HY_MAX_SIDE && (int64_t)h * w <= HY_MAX_PIXELS,
             "%s: raster %dx%d: sides must be in 1..%d and h * w <= 2^31 - 2", tag, h, w, HY_MAX_SIDE);
  return DT_OK;
}

extern "C" int dt_support_span(int* chunks) {
  DT_REQUIRE(chunks, "support_span: null pointer");
  *chunks = HY_SPAN;
  return DT_OK;
}

extern "C" int dt_decide_candidates_u8(const float* probs, const uint16_t* low, uint8_t* out_u8, uint16_t* q_own, int K,
                                       int64_t n, void* stream) {
  DT_REQUIRE(probs && low && out_u8 && q_own, "decide_candidates_u8: null pointer");
  DT_REQUIRE(K >= 2 && K <= CURVE_MAXK, "decide_candidates_u8: K=%d unsupported (2..%d)", K, CURVE_MAXK);
  DT_REQUIRE(n >= 1 && n <= HY_MAX_PIXELS, "decide_candidates_u8: n=%lld pixels (1 .. 2^31 - 2)", (long long)n);
  curve_thresholds thr;
  DT_TRY(curve_read_thresholds("decide_candidates_u8", low, K, thr));
  const int64_t groups = (n + CURVE_STEP - 1) / CURVE_STEP;
  const int align = (curve_aligned(probs, 16) ? 1 : 0) | (curve_aligned(out_u8, 4) ? 2 : 0) | (curve_aligned(q_own, 8) ? 4 : 0);
  hipLaunchKernelGGL(decide_classes_kernel<true>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, probs, thr,
                     out_u8, q_own, K, n, align);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_patch_support(const int32_t* labels, const uint16_t* q_own, int h, int w, int32_t* qmax, int64_t* qsum,
                                int32_t* area, void* stream) {
  DT_REQUIRE(labels && q_own && qmax, "patch_support: null pointer");
  DT_REQUIRE((qsum == nullptr) == (area == nullptr), "patch_support: the sum plane comes with the area plane");
  DT_TRY(hy_check_size("patch_support", h, w));
  const int64_t n = (int64_t)h * w;
  const dim3 grid((unsigned)((n + 4 * HY_SPAN * 64 - 1) / (4 * HY_SPAN * 64)));
  if (qsum)
    hipLaunchKernelGGL(patch_support_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, labels, q_own, n, qmax,
                       (unsigned long long*)qsum, area);
  else
    hipLaunchKernelGGL(patch_support_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, labels, q_own, n, qmax,
                       (unsigned long long*)nullptr, (int32_t*)nullptr);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_reject_patches_u8(uint8_t* classes, const int32_t* labels, const int32_t* qmax, const int64_t* qsum,
                                    const int32_t* area, const uint16_t* thresholds, const uint16_t* min_confidence, int K,
                                    int h, int w, void* stream) {
  DT_REQUIRE(classes && labels && qmax && thresholds, "reject_patches_u8: null pointer");
  DT_REQUIRE((qsum == nullptr) == (area == nullptr), "reject_patches_u8: the sum plane comes with the area plane");
  DT_REQUIRE(K >= 2 && K <= CURVE_MAXK, "reject_patches_u8: K=%d unsupported (2..%d)", K, CURVE_MAXK);
  DT_TRY(hy_check_size("reject_patches_u8", h, w));
  curve_thresholds thr, conf;
  DT_TRY(curve_read_thresholds("reject_patches_u8", thresholds, K, thr));
  bool filter = false;
  for (int c = 0; c < CURVE_MAXK; ++c) conf.t[c] = 0u;
  for (int c = 1; c < K && min_confidence; ++c) {
    conf.t[c] = min_confidence[c];
    filter = filter || conf.t[c] != 0u;
  }
  DT_REQUIRE(!filter || qsum, "reject_patches_u8: a confidence filter needs the sum and area planes");
  const int64_t n = (int64_t)h * w;
  const dim3 grid((unsigned)((n + CURVE_STEP - 1) / CURVE_STEP));
  const int align = (curve_aligned(labels, 16) ? 1 : 0) | (curve_aligned(classes, 4) ? 2 : 0);
  if (filter)
    hipLaunchKernelGGL(reject_patches_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, classes, labels, qmax,
                       (const long long*)qsum, area, thr, conf, K, n, align);
  else
    hipLaunchKernelGGL(reject_patches_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, classes, labels, qmax,
                       (const long long*)nullptr, (const int32_t*)nullptr, thr, conf, K, n, align);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
