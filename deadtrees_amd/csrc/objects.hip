// Crown-level validation curves (deadtrees_amd/loss/objects.py holds the contract): per validation batch ONE labelling of
// the candidates at the low thresholds and one of the target, the matching of predicted patches to target crowns above an
// IoU of at least 1/2, and one histogram entry per predicted patch — (class, matched, qmax >> 8, mean q >> 8) — from which
// the host reads crown-level TP / FP / FN for every (T, M) at once.  Integers only: nothing depends on the order in which
// pixels, waves, workgroups or batches arrive.  No workgroup waits for another, no scalar leaves the device, no sort.
//
// The B images lie in ONE plane of (H + 1) x (W + 1) cells, `cols` cells per row: the last row and column of a cell, the
// cells past image B - 1 and the columns past the last cell are class 0, so no patch joins two images and the unchanged
// single-raster kernels (dt_label_patches_u8, dt_patch_areas, dt_patch_support) label and measure the whole batch.
//
// dt_object_planes    q uint16 [B][K][H][W] and the target -> the candidates' class plane, their own q and the target's
//                     class plane.  4 plane pixels per lane, 8- / 16-byte loads where the image offset allows.
// dt_object_vote      above an IoU of 1/2 the partner of a target patch a covers more than half of a: it is the strict
//                     majority of the predicted labels over a's pixels, 0 (no patch) being a value like any other.  A
//                     majority summary (candidate, count) merges like this: equal candidates add, others subtract, the
//                     larger side stays.  A strict majority survives EVERY merge tree (Boyer-Moore; Misra-Gries with one
//                     counter is a mergeable summary), so the result that matters does not depend on the arrival order.
//                     The walk is dt_patch_support's: a wave owns OB_SPAN consecutive 64-pixel chunks, pt_runs finds the
//                     runs of equal TARGET label, a segmented scan merges the per-pixel summaries (predicted label, 1) of
//                     a run, the open run is carried, the runs the four waves of a workgroup end with are merged through
//                     LDS, and a finished run merges into vote[target label - 1], a packed (candidate:32, count:32)
//                     word, through a 64-bit compare-and-swap: lock-free, a failed swap means another lane's succeeded.
// dt_object_inter     the same walk: the pixels of a whose predicted label is a's candidate, an int32 atomicAdd per run.
// dt_object_targets   over the target roots: targets[c] += 1, and where n * q > p * (A_a + A_b - n), the classes agree and
//                     A_b >= min_pixels, matched[b] = 1.  Without a majority the candidate is arbitrary but then
//                     n <= A_a / 2 <= union / 2 fails the test: matched is deterministic.  One writer per b at most (two
//                     disjoint targets cannot each hold more than half of b).
// dt_object_histogram over the predicted roots with A >= min_pixels: one 64-bit add into hist[c][matched][jT][jM].
#include <limits.h>

#include "conv_host.h"
#include "patch_runs.h"

#define OB_SPAN 16                       // 64-pixel chunks per wave
#define OB_MAXK 8
#define OB_MAX_SIDE 16384
#define OB_MAX_PIXELS 2147483646ll       // labels are int32 and 1-based
#define OB_ROUNDS 2                      // ballot rounds before the plain atomics of the histogram
#define OB_ROOT_STEPS 8                  // 256-pixel steps per workgroup of dt_object_targets

typedef long long ob_i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned short ob_u16x4 __attribute__((ext_vector_type(4)));

struct ob_thresholds {
  unsigned t[OB_MAXK];
};

struct ob_layout {
  int B, K, H, W, cols, ph, pw;
};

static inline bool ob_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// ---------------------------------------------------------------- the batch plane
// candidates: the class c >= 1 with the largest q_c among those with q_c >= L_c (ties -> the smallest c), 0 without one
__device__ __forceinline__ void ob_candidate(unsigned c, unsigned q, const ob_thresholds& low, unsigned& best, unsigned& bq) {
  if (q >= low.t[c] && (best == 0u || q > bq)) {
    best = c;
    bq = q;
  }
}

// align: bit 0 q 8-byte, bit 1 target 16-byte, bit 2 cand and tcls 4-byte, bit 3 q_own 8-byte aligned
__global__ __launch_bounds__(256) void object_planes_kernel(const uint16_t* __restrict__ q, const int64_t* __restrict__ target,
                                                            ob_thresholds low, ob_layout L, uint8_t* __restrict__ cand,
                                                            uint16_t* __restrict__ q_own, uint8_t* __restrict__ tcls,
                                                            int32_t* __restrict__ err, int align) {
  const int gw = (L.pw + 3) / 4;                             // groups of 4 pixels per plane row
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)L.ph * gw) return;
  const int py = (int)(gid / gw), px0 = (int)(gid - (int64_t)py * gw) * 4;
  const int cr = py / (L.H + 1), y = py - cr * (L.H + 1);
  unsigned best[4] = {0u, 0u, 0u, 0u}, bq[4] = {0u, 0u, 0u, 0u}, tc[4] = {0u, 0u, 0u, 0u};
  bool bad = false;
  if (y < L.H) {                                             // (the last row of a cell is a gutter)
    const int cc0 = px0 / (L.W + 1), x0 = px0 - cc0 * (L.W + 1);
    const int64_t b0 = (int64_t)cr * L.cols + cc0;
    if (cc0 < L.cols && b0 < L.B && x0 + 3 < L.W) {          // four pixels of one image row
      const int64_t toff = (b0 * L.H + y) * L.W + x0;
      int64_t lab[4];
      if ((align & 2) && (toff & 1) == 0) {
        const ob_i64x2 a = *reinterpret_cast<const ob_i64x2*>(target + toff);
        const ob_i64x2 b = *reinterpret_cast<const ob_i64x2*>(target + toff + 2);
        lab[0] = a[0], lab[1] = a[1], lab[2] = b[0], lab[3] = b[1];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) lab[j] = target[toff + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = lab[j] >= 0 && lab[j] < L.K;
        bad = bad || !ok;
        tc[j] = ok ? (unsigned)lab[j] : 0u;
      }
      for (int c = 1; c < L.K; ++c) {
        const int64_t off = ((b0 * L.K + c) * L.H + y) * L.W + x0;
        unsigned v[4];
        if ((align & 1) && (off & 3) == 0) {
          const ob_u16x4 q4 = *reinterpret_cast<const ob_u16x4*>(q + off);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = q4[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = q[off + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ob_candidate((unsigned)c, v[j], low, best[j], bq[j]);
      }
    } else {                                                 // a group that meets a gutter, an empty cell or the plane's end
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int px = px0 + j, cc = px / (L.W + 1), x = px - cc * (L.W + 1);
        const int64_t b = (int64_t)cr * L.cols + cc;
        if (px >= L.pw || cc >= L.cols || x >= L.W || b >= L.B) continue;
        const int64_t lab = target[(b * L.H + y) * L.W + x];
        const bool ok = lab >= 0 && lab < L.K;
        bad = bad || !ok;
        tc[j] = ok ? (unsigned)lab : 0u;
        for (int c = 1; c < L.K; ++c)
          ob_candidate((unsigned)c, q[((b * L.K + c) * L.H + y) * L.W + x], low, best[j], bq[j]);
      }
    }
  }
  if (bad) err[0] = 1;                                       // dt_prob_histogram's rule: flag, and the pixel is background
  const int64_t o = (int64_t)py * L.pw + px0;
  const bool whole = px0 + 3 < L.pw && (o & 3) == 0;
  if (whole && (align & 4)) {
    *reinterpret_cast<unsigned*>(cand + o) = best[0] | (best[1] << 8) | (best[2] << 16) | (best[3] << 24);
    *reinterpret_cast<unsigned*>(tcls + o) = tc[0] | (tc[1] << 8) | (tc[2] << 16) | (tc[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (px0 + j < L.pw) cand[o + j] = (uint8_t)best[j], tcls[o + j] = (uint8_t)tc[j];
  }
  if (whole && (align & 8)) {
    *reinterpret_cast<ob_u16x4*>(q_own + o) =
        ob_u16x4{(unsigned short)bq[0], (unsigned short)bq[1], (unsigned short)bq[2], (unsigned short)bq[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (px0 + j < L.pw) q_own[o + j] = (uint16_t)bq[j];
  }
}

// ---------------------------------------------------------------- the walk of both label planes
// VOTE: (cand, count) is a majority summary of predicted labels; otherwise count is a pixel count and cand is not used
struct ob_run {
  int label;                             // the target label the run belongs to, 0: none
  unsigned cand, count;
};

template <bool VOTE>
__device__ __forceinline__ void ob_merge(unsigned& cand, unsigned& count, unsigned other_cand, unsigned other_count) {
  if constexpr (VOTE) {
    if (cand == other_cand) {
      count += other_count;
    } else if (count >= other_count) {
      count -= other_count;
    } else {
      cand = other_cand;
      count = other_count - count;
    }
  } else {
    count += other_count;
  }
}

template <bool VOTE>
__device__ __forceinline__ void ob_emit(const ob_run& r, unsigned long long* __restrict__ vote, int32_t* __restrict__ inter) {
  if (r.count == 0u) return;                               // an empty summary changes no word
  const int root = r.label - 1;
  if constexpr (VOTE) {
    unsigned long long seen = __hip_atomic_load(&vote[root], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), assumed;
    do {
      assumed = seen;
      unsigned c = (unsigned)(assumed >> 32), n = (unsigned)assumed;
      ob_merge<true>(c, n, r.cand, r.count);
      seen = atomicCAS(&vote[root], assumed, ((unsigned long long)c << 32) | n);
    } while (seen != assumed);
  } else {
    atomicAdd(&inter[root], (int)r.count);
  }
}

// vote: written (VOTE) or read; inter: written (!VOTE)
template <bool VOTE>
__global__ __launch_bounds__(256) void object_walk_kernel(const int32_t* __restrict__ lt_plane,
                                                          const int32_t* __restrict__ lp_plane, int64_t n,
                                                          unsigned long long* vote, int32_t* __restrict__ inter) {
  __shared__ ob_run tail[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * (OB_SPAN * 64);
  ob_run carry = {0, 0u, 0u};                              // wave-uniform: the run left open by the previous chunk
  for (int j = 0; j < OB_SPAN; ++j) {
    const int64_t i = base + j * 64 + lane;
    if (i - lane >= n) break;
    const int lt = pt_label_at(lt_plane, i, n);
    if (__ballot(lt != 0) == 0) {                          // no target here, most chunks of a real map: lp is not read
      if (lane == 0 && carry.label) ob_emit<VOTE>(carry, vote, inter);
      carry.label = 0;
      continue;
    }
    const int lp = lt ? pt_label_at(lp_plane, i, n) : 0;   // a label implies i < n
    unsigned cand = 0u, count = 0u;
    if constexpr (VOTE) {
      cand = (unsigned)lp;
      count = lt ? 1u : 0u;
    } else {
      count = lt && (unsigned)(vote[lt - 1] >> 32) == (unsigned)lp ? 1u : 0u;
    }
    bool head;
    int len;
    uint64_t heads;
    pt_runs(lt, false, lane, head, len, heads);            // len: the distance to the next head, in every lane
    const int reach = lt ? len : 1;                        // background is never written out: its lanes take no partner
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = d < reach;
      if (__ballot(take) == 0) break;
      const unsigned other_cand = __shfl_down(cand, d, 64), other_count = __shfl_down(count, d, 64);
      if (take) ob_merge<VOTE>(cand, count, other_cand, other_count);
    }
    ob_run run = {lt, cand, count};
    const int first = __shfl(lt, 0, 64), last_head = 63 - __clzll((long long)heads);
    if (lane == 0 && carry.label) {
      if (carry.label == first) ob_merge<VOTE>(run.cand, run.count, carry.cand, carry.count);
      else ob_emit<VOTE>(carry, vote, inter);
    }
    if (head && lane != last_head && lt) ob_emit<VOTE>(run, vote, inter);
    carry.label = __shfl(run.label, last_head, 64);
    carry.cand = __shfl(run.cand, last_head, 64);
    carry.count = __shfl(run.count, last_head, 64);
  }
  // the runs the four waves end with (label 0: none): equal neighbours become one write
  if (lane == 0) tail[wave] = carry;
  __syncthreads();
  if (threadIdx.x != 0) return;
  ob_run open = {0, 0u, 0u};
  for (int k = 0; k < 4; ++k) {
    const ob_run t = tail[k];
    if (t.label == 0) continue;
    if (t.label == open.label) {
      ob_merge<VOTE>(open.cand, open.count, t.cand, t.count);
    } else {
      if (open.label) ob_emit<VOTE>(open, vote, inter);
      open = t;
    }
  }
  if (open.label) ob_emit<VOTE>(open, vote, inter);
}

// ---------------------------------------------------------------- the roots
__global__ __launch_bounds__(256) void object_targets_kernel(const int32_t* __restrict__ lt_plane, const uint8_t* __restrict__ tcls,
                                                             const uint8_t* __restrict__ cand,
                                                             const unsigned long long* __restrict__ vote,
                                                             const int32_t* __restrict__ inter, const int32_t* __restrict__ area_t,
                                                             const int32_t* __restrict__ area_p, int K, int64_t n,
                                                             long long min_pixels, long long iou_p, long long iou_q,
                                                             unsigned long long* __restrict__ targets,
                                                             uint8_t* __restrict__ matched) {
  __shared__ unsigned found[OB_MAXK];
  if (threadIdx.x < OB_MAXK) found[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // OB_ROOT_STEPS x 256 consecutive pixels per workgroup: the roots of a class are counted per wave (ballot) and per
  // workgroup (LDS), so that the one counter targets[c] takes one add per workgroup
  for (int step = 0; step < OB_ROOT_STEPS; ++step) {
    const int64_t i = ((int64_t)blockIdx.x * OB_ROOT_STEPS + step) * 256 + threadIdx.x;
    if (i - threadIdx.x >= n) break;                        // (the same for the whole workgroup)
    unsigned c = 0u;
    if (i < n && pt_label_at(lt_plane, i, n) == i + 1) c = tcls[i];
    if (c >= (unsigned)K) c = 0u;
    if (c) {
      const unsigned b_label = (unsigned)(vote[i] >> 32);   // a value of the predicted label plane: 0 .. n
      if (b_label) {
        const int64_t b = (int64_t)b_label - 1;
        const long long shared = inter[i], aa = area_t[i], ab = area_p[b];
        if (cand[b] == c && ab >= min_pixels && shared * iou_q > iou_p * (aa + ab - shared)) matched[b] = 1;
      }
    }
    if (__ballot(c != 0u) == 0) continue;                   // (wave-uniform)
    for (unsigned k = 1; k < (unsigned)K; ++k) {
      const unsigned long long here = __ballot(c == k);
      if (lane == 0 && here) atomicAdd(&found[k], (unsigned)__popcll(here));
    }
  }
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x < K && found[threadIdx.x])
    atomicAdd(&targets[threadIdx.x], (unsigned long long)found[threadIdx.x]);
}

__global__ __launch_bounds__(256) void object_histogram_kernel(const int32_t* __restrict__ lp_plane, const uint8_t* __restrict__ cand,
                                                               const int32_t* __restrict__ qmax, const long long* __restrict__ qsum,
                                                               const int32_t* __restrict__ area, const uint8_t* __restrict__ matched,
                                                               int K, int64_t n, long long min_pixels,
                                                               unsigned long long* __restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pending = false;
  unsigned key = 0u;
  if (i < n && pt_label_at(lp_plane, i, n) == i + 1) {
    const unsigned c = cand[i];
    const long long a = area[i];
    if (c >= 1u && c < (unsigned)K && a >= 1 && a >= min_pixels) {
      const unsigned jt = ((unsigned)qmax[i] >> 8) & 255u, jm = ((unsigned)(qsum[i] / a) >> 8) & 255u;
      key = (((c * 2u + (matched[i] ? 1u : 0u)) * 256u + jt) * 256u) + jm;
      pending = true;
    }
  }
  // patches of one kind share a counter: the lanes that share the first pending lane's are added as one count
#pragma unroll
  for (int r = 0; r < OB_ROUNDS; ++r) {
    const unsigned long long live = __ballot(pending);
    if (live == 0) return;
    const int leader = __ffsll((long long)live) - 1;
    const unsigned lk = (unsigned)__shfl((int)key, leader, 64);
    const bool same = pending && key == lk;
    const unsigned long long group = __ballot(same);
    if (lane == leader) atomicAdd(&hist[lk], (unsigned long long)__popcll(group));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&hist[key], 1ull);
}

// ---------------------------------------------------------------- entry points
static int ob_check_plane(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1 && h <= OB_MAX_SIDE && w <= OB_MAX_SIDE && (int64_t)h * w <= OB_MAX_PIXELS,
             "%s: plane %dx%d: sides must be in 1..%d and h * w <= 2^31 - 2", tag, h, w, OB_MAX_SIDE);
  return DT_OK;
}

static inline dim3 ob_pixel_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
static inline dim3 ob_walk_grid(int64_t n) { return dim3((unsigned)((n + 4 * OB_SPAN * 64 - 1) / (4 * OB_SPAN * 64))); }

extern "C" int dt_object_planes(const uint16_t* q, const int64_t* target, const uint16_t* low, int B, int K, int H, int W,
                                int cols, int ph, int pw, uint8_t* cand, uint16_t* q_own, uint8_t* tcls, int32_t* err_flag,
                                void* stream) {
  DT_REQUIRE(q && target && low && cand && q_own && tcls && err_flag, "object_planes: null pointer");
  DT_REQUIRE(B > 0 && H > 0 && W > 0, "object_planes: B=%d H=%d W=%d must be positive", B, H, W);
  DT_REQUIRE(K >= 2 && K <= OB_MAXK, "object_planes: K=%d unsupported (2..%d)", K, OB_MAXK);
  DT_REQUIRE(H < OB_MAX_SIDE && W < OB_MAX_SIDE && cols >= 1 && cols <= B, "object_planes: %d cells per row for B=%d, H=%d, W=%d",
             cols, B, H, W);
  const int64_t rows = ((int64_t)B + cols - 1) / cols;
  DT_REQUIRE(ph == rows * (H + 1) && pw >= (int64_t)cols * (W + 1),
             "object_planes: a plane of %dx%d does not hold %d rows of %d cells of %dx%d", ph, pw, (int)rows, cols, H + 1, W + 1);
  DT_TRY(ob_check_plane("object_planes", ph, pw));
  ob_thresholds thr;
  for (int c = 0; c < OB_MAXK; ++c) thr.t[c] = 0u;
  for (int c = 1; c < K; ++c) {
    DT_REQUIRE(low[c] >= 1, "object_planes: the low threshold of class %d must be in 1..65535", c);
    thr.t[c] = low[c];
  }
  const ob_layout L = {B, K, H, W, cols, ph, pw};
  const int align = (ob_aligned(q, 8) ? 1 : 0) | (ob_aligned(target, 16) ? 2 : 0) |
                    (ob_aligned(cand, 4) && ob_aligned(tcls, 4) ? 4 : 0) | (ob_aligned(q_own, 8) ? 8 : 0);
  const int64_t groups = (int64_t)ph * ((pw + 3) / 4);
  hipLaunchKernelGGL(object_planes_kernel, ob_pixel_grid(groups), dim3(256), 0, (hipStream_t)stream, q, target, thr, L, cand,
                     q_own, tcls, err_flag, align);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_object_vote(const int32_t* labels_t, const int32_t* labels_p, int h, int w, int64_t* vote, void* stream) {
  DT_REQUIRE(labels_t && labels_p && vote, "object_vote: null pointer");
  DT_TRY(ob_check_plane("object_vote", h, w));
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(object_walk_kernel<true>, ob_walk_grid(n), dim3(256), 0, (hipStream_t)stream, labels_t, labels_p, n,
                     (unsigned long long*)vote, (int32_t*)nullptr);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_object_inter(const int32_t* labels_t, const int32_t* labels_p, const int64_t* vote, int h, int w,
                               int32_t* inter, void* stream) {
  DT_REQUIRE(labels_t && labels_p && vote && inter, "object_inter: null pointer");
  DT_TRY(ob_check_plane("object_inter", h, w));
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(object_walk_kernel<false>, ob_walk_grid(n), dim3(256), 0, (hipStream_t)stream, labels_t, labels_p, n,
                     (unsigned long long*)vote, inter);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_object_targets(const int32_t* labels_t, const uint8_t* tcls, const uint8_t* cand, const int64_t* vote,
                                 const int32_t* inter, const int32_t* area_t, const int32_t* area_p, int K, int h, int w,
                                 int64_t min_pixels, int64_t iou_p, int64_t iou_q, int64_t* targets, uint8_t* matched,
                                 void* stream) {
  DT_REQUIRE(labels_t && tcls && cand && vote && inter && area_t && area_p && targets && matched, "object_targets: null pointer");
  DT_REQUIRE(K >= 2 && K <= OB_MAXK, "object_targets: K=%d unsupported (2..%d)", K, OB_MAXK);
  DT_REQUIRE(min_pixels >= 0, "object_targets: min_pixels=%lld must not be negative", (long long)min_pixels);
  DT_REQUIRE(iou_q >= 1 && iou_q <= 1000000 && 2 * iou_p >= iou_q && iou_p < iou_q,
             "object_targets: min_iou %lld / %lld must lie in [1/2, 1) with a denominator of at most 10^6", (long long)iou_p,
             (long long)iou_q);
  DT_TRY(ob_check_plane("object_targets", h, w));
  const int64_t n = (int64_t)h * w;
  const dim3 grid = ob_pixel_grid((n + OB_ROOT_STEPS - 1) / OB_ROOT_STEPS);
  hipLaunchKernelGGL(object_targets_kernel, grid, dim3(256), 0, (hipStream_t)stream, labels_t, tcls, cand,
                     (const unsigned long long*)vote, inter, area_t, area_p, K, n, (long long)min_pixels, (long long)iou_p,
                     (long long)iou_q, (unsigned long long*)targets, matched);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_object_histogram(const int32_t* labels_p, const uint8_t* cand, const int32_t* qmax, const int64_t* qsum,
                                   const int32_t* area, const uint8_t* matched, int K, int h, int w, int64_t min_pixels,
                                   int64_t* hist, void* stream) {
  DT_REQUIRE(labels_p && cand && qmax && qsum && area && matched && hist, "object_histogram: null pointer");
  DT_REQUIRE(K >= 2 && K <= OB_MAXK, "object_histogram: K=%d unsupported (2..%d)", K, OB_MAXK);
  DT_REQUIRE(min_pixels >= 0, "object_histogram: min_pixels=%lld must not be negative", (long long)min_pixels);
  DT_TRY(ob_check_plane("object_histogram", h, w));
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(object_histogram_kernel, ob_pixel_grid(n), dim3(256), 0, (hipStream_t)stream, labels_p, cand, qmax,
                     (const long long*)qsum, area, matched, K, n, (long long)min_pixels, (unsigned long long*)hist);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
