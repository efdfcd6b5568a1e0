// Crowns (deployment/crowns.py holds the contract): touching dead crowns split by their inscribed depth, on the class map and
// the label plane that already sit in HBM.  Integers only.
//
//   depth    depth2[p] = min(cap2, the squared distance from p to the nearest pixel INSIDE the raster of another class), the
//            two passes of the separable exact transform (distmap.hip):
//              columns  per pixel the vertical distance g to the nearest pixel of its column with another class (CR_NONE:
//                       none).  The column is cut into segments of CR_SEG rows chained by one lane per column, as
//                       proximity.hip does: (1) what a segment leaves behind in both directions when it starts from nothing,
//                       (2) one lane per column chains these into the state every segment starts from, (3) the segments
//                       again, from that state: down writes the distance upwards, up folds the distance downwards in.
//              rows     min over x' of (x - x')^2 + (cls[y, x'] == c ? g[y, x']^2 : 0), walking outward from x while
//                       dx^2 < min(best, cap2): a pixel reads at most 2 sqrt(cap2) entries, staged in LDS with that halo.
//            The same pass writes the core class plane (the class where depth2 >= E).
//   grow     ONE Jacobi round per launch, ping-pong between two planes: a waiting pixel (class != 0, S == 0) takes the
//            minimum S of its same-class neighbours that have one.  The launch boundary is the only ordering the rule needs;
//            a lane that labelled a pixel ORs into the round's own flag slot, which the host reads once per group of rounds.
//   remainder  the class plane of the pixels no core reached, and the not-converged bit: a waiting pixel next to a reached
//            one of its class (it is read here, where S is still whole).
//   merge    seg = S or the remainder's label; first[seg - 1] = min pixel, depth[seg - 1] = max depth2, integer atomics with
//            the lanes of a wave that share a seg combined first: the planes do not depend on the order of arrival.
//   relabel  crowns = 1 + first[seg - 1]; the pixel a seg is named after moves the seg's depth to the crown's root.
// No workgroup waits for another, every loop bound is known at launch, every grid follows the pixel count.
#include <limits.h>

#include "conv_host.h"
#include "patch_runs.h"

#define CR_SEG 64                        // rows per column segment
#define CR_BATCH 8                       // rows of a segment whose classes a lane loads before it walks them
#define CR_WINDOW 1024                   // pixels of one row per workgroup of the row pass: 256 lanes, 4 pixels each
#define CR_NONE 0xffffu                  // the distance column's "no such pixel"
#define CR_INF2 (1u << 30)               // its square: at or above every cap
#define CR_MAX_SIDE 16384                // column distances fit uint16 below the sentinel, d2 < 2^30
#define CR_MAX_PIXELS 2147483646LL       // 2^31 - 2: labels are int32 and 1-based
#define CR_MAX_DEPTH2 (1 << 30)
static_assert(CR_WINDOW == 4 * 256, "a lane takes four pixels of the window");
#define CR_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// flag |= 1 by the first lane of a wave in which `any` lane asks for it.  Thousands of waves ask for the same word: whoever
// finds the bit set already leaves the atomic out (a stale 0 costs one atomic more, never a missing bit)
__device__ __forceinline__ void cr_raise(int32_t* flag, bool any) {
  if (__ballot(any) != 0 && (threadIdx.x & 63) == 0 && (CR_LOAD(flag) & 1) == 0) atomicOr(flag, 1);
}

// ---------------------------------------------------------------- columns
// walking a column: the class of the pixel just passed (-1: none yet) and the row of the nearest pixel passed whose class
// differs from it (-1: none)
struct cr_state {
  int c, other;
};

// `before`: the row just passed when y is entered (y - 1 walking down, y + 1 walking up)
__device__ __forceinline__ void cr_step(cr_state& s, int before, int v) {
  if (v == s.c) return;
  if (s.c >= 0) s.other = before;
  s.c = v;
}

// the state behind a segment that leaves `seg` when started from nothing, entered with `in`; `before`: the row in front of it
__device__ __forceinline__ cr_state cr_chain(const cr_state& in, const cr_state& seg, int before) {
  if (seg.other >= 0 || in.c < 0) return seg;
  return {seg.c, in.c == seg.c ? in.other : before};       // one class throughout: the other one comes from before it
}

// grid (ceil(w / 64), segments), 64 lanes: one walk down the segment gives both directions' states from nothing — down: the
// last class and the nearest other row above the end; up: the first class and the first row whose class differs from it
__global__ __launch_bounds__(64) void crown_segment_kernel(const uint8_t* __restrict__ cls, int h, int w,
                                                           int4* __restrict__ carry) {
  const int x = blockIdx.x * 64 + threadIdx.x, seg = blockIdx.y;
  if (x >= w) return;
  const int y0 = seg * CR_SEG, rows = min(h, y0 + CR_SEG) - y0;
  cr_state down = {-1, -1};
  int first = -1, first_other = -1;
  for (int k0 = 0; k0 < rows; k0 += CR_BATCH) {                 // the loads of a batch are in flight together
    int v[CR_BATCH];
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) v[j] = k0 + j < rows ? cls[(int64_t)(y0 + k0 + j) * w + x] : 0;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      const int y = y0 + k0 + j;
      if (k0 + j >= rows) break;
      cr_step(down, y - 1, v[j]);
      if (first < 0) first = v[j];
      else if (first_other < 0 && v[j] != first) first_other = y;
    }
  }
  carry[(int64_t)seg * w + x] = make_int4(down.c, down.other, first, first_other);
}

// grid (ceil(w / 64)), 64 lanes: a lane chains the segments of its column, downwards and upwards, and replaces every segment's
// own states by the states it starts from
__global__ __launch_bounds__(64) void crown_chain_kernel(int h, int w, int segs, int4* __restrict__ carry) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  cr_state s = {-1, -1};
  for (int k = 0; k < segs; ++k) {
    const int64_t at = (int64_t)k * w + x;
    const int4 c = carry[at];
    carry[at] = make_int4(s.c, s.other, c.z, c.w);
    s = cr_chain(s, {c.x, c.y}, k * CR_SEG - 1);
  }
  s = {-1, -1};
  for (int k = segs - 1; k >= 0; --k) {
    const int64_t at = (int64_t)k * w + x;
    const int4 c = carry[at];
    carry[at] = make_int4(c.x, c.y, s.c, s.other);
    s = cr_chain(s, {c.z, c.w}, min(h, (k + 1) * CR_SEG));
  }
}

// grid (ceil(w / 64), segments), 64 lanes: down from the chained state g = the distance upwards, then up from the chained
// state g = min(g, the distance downwards); a lane re-reads only what it wrote itself
__global__ __launch_bounds__(64) void crown_columns_kernel(const uint8_t* __restrict__ cls, int h, int w,
                                                           const int4* __restrict__ carry, uint16_t* g) {
  const int x = blockIdx.x * 64 + threadIdx.x, seg = blockIdx.y;
  if (x >= w) return;
  const int y0 = seg * CR_SEG, rows = min(h, y0 + CR_SEG) - y0;
  const int4 in = carry[(int64_t)seg * w + x];
  cr_state s = {in.x, in.y};
  for (int k0 = 0; k0 < rows; k0 += CR_BATCH) {
    int v[CR_BATCH];
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) v[j] = k0 + j < rows ? cls[(int64_t)(y0 + k0 + j) * w + x] : 0;
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      const int y = y0 + k0 + j;
      if (k0 + j >= rows) break;
      cr_step(s, y - 1, v[j]);
      g[(int64_t)y * w + x] = (uint16_t)(s.other < 0 ? CR_NONE : (unsigned)(y - s.other));
    }
  }
  s = {in.z, in.w};
  for (int k0 = 0; k0 < rows; k0 += CR_BATCH) {
    int v[CR_BATCH], up[CR_BATCH];
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      const int64_t p = (int64_t)(y0 + rows - 1 - k0 - j) * w + x;
      v[j] = k0 + j < rows ? cls[p] : 0;
      up[j] = k0 + j < rows ? g[p] : 0;
    }
#pragma unroll
    for (int j = 0; j < CR_BATCH; ++j) {
      const int y = y0 + rows - 1 - k0 - j;
      if (k0 + j >= rows) break;
      cr_step(s, y + 1, v[j]);
      const int dn = s.other < 0 ? (int)CR_NONE : s.other - y;
      if (dn < up[j]) g[(int64_t)y * w + x] = (uint16_t)dn;
    }
  }
}

// ---------------------------------------------------------------- rows
// a staged entry: g << 8 | class
__device__ __forceinline__ uint32_t cr_offer2(uint32_t e, uint32_t c) {
  if ((e & 0xffu) != c) return 0u;                         // the pixel itself is of another class
  const uint32_t gg = e >> 8;
  return gg == CR_NONE ? CR_INF2 : gg * gg;
}

// grid (ceil(w / CR_WINDOW), h), 256 lanes; LDS: the window and `halo` entries on either side, halo^2 >= cap2
__global__ __launch_bounds__(256) void crown_rows_kernel(const uint8_t* __restrict__ cls, const uint16_t* __restrict__ g,
                                                         int h, int w, int K, int halo, uint32_t cap2, uint32_t core2,
                                                         int32_t* __restrict__ depth2, uint8_t* __restrict__ core,
                                                         int32_t* err) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cr_row[];
  const int y = blockIdx.y, x0 = blockIdx.x * CR_WINDOW;
  const int lo = max(0, x0 - halo), hi = min(w, x0 + CR_WINDOW + halo);
  const int64_t row0 = (int64_t)y * w;
  for (int i = lo + threadIdx.x; i < hi; i += 256) cr_row[i - lo] = ((uint32_t)g[row0 + i] << 8) | cls[row0 + i];
  __syncthreads();
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + 256 * k + threadIdx.x;
    if (x >= w) continue;
    const uint32_t e = cr_row[x - lo];
    uint32_t c = e & 0xffu, best = 0;
    if (c >= (uint32_t)K) {
      bad = true;
      c = 0;
    }
    if (c) {
      best = min(cap2, cr_offer2(e, c));
      for (int d = 1; d < w; ++d) {
        const uint32_t dd = (uint32_t)d * (uint32_t)d;
        const int xl = x - d, xr = x + d;
        if (dd >= best || (xl < 0 && xr >= w)) break;
        if (xl >= 0) best = min(best, dd + cr_offer2(cr_row[xl - lo], c));
        if (xr < w) best = min(best, dd + cr_offer2(cr_row[xr - lo], c));
      }
    }
    depth2[row0 + x] = (int32_t)best;
    if (core) core[row0 + x] = (uint8_t)(best >= core2 ? c : 0);
  }
  cr_raise(err, bad);
}

// ---------------------------------------------------------------- growth
// the neighbour q of a waiting pixel of class c: its S if it has the class and a label
__device__ __forceinline__ void cr_look(const uint8_t* __restrict__ cls, const int32_t* __restrict__ S, int64_t q, int c,
                                        int& best) {
  if (cls[q] != c) return;
  const int v = S[q];
  if (v > 0 && v < best) best = v;
}

// INT_MAX when no neighbour of (y, x) has the class c and a label
template <bool CONN8>
__device__ __forceinline__ int cr_neighbours(const uint8_t* __restrict__ cls, const int32_t* __restrict__ S, int h, int w,
                                             int y, int x, int c) {
  const int64_t p = (int64_t)y * w + x;
  int best = INT_MAX;
  if (y > 0) {
    if (CONN8 && x > 0) cr_look(cls, S, p - w - 1, c, best);
    cr_look(cls, S, p - w, c, best);
    if (CONN8 && x + 1 < w) cr_look(cls, S, p - w + 1, c, best);
  }
  if (x > 0) cr_look(cls, S, p - 1, c, best);
  if (x + 1 < w) cr_look(cls, S, p + 1, c, best);
  if (y + 1 < h) {
    if (CONN8 && x > 0) cr_look(cls, S, p + w - 1, c, best);
    cr_look(cls, S, p + w, c, best);
    if (CONN8 && x + 1 < w) cr_look(cls, S, p + w + 1, c, best);
  }
  return best;
}

// one round: dst = src, and a waiting pixel takes its neighbours' minimum of src.  A lane takes 4 consecutive pixels (16-byte
// accesses; the planes are 16-byte aligned, the class map 4-byte); the last lane of a ragged plane goes pixel by pixel
template <bool CONN8>
__global__ __launch_bounds__(256) void crown_grow_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ src,
                                                         int32_t* __restrict__ dst, int h, int w, int64_t n,
                                                         int32_t* slot) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  bool took = false;
  if (i0 < n) {
    const bool whole = i0 + 3 < n;
    int s[4], c[4];
    if (whole) {
      const int4 v = *reinterpret_cast<const int4*>(src + i0);
      const uchar4 u = *reinterpret_cast<const uchar4*>(cls + i0);
      s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
      c[0] = u.x, c[1] = u.y, c[2] = u.z, c[3] = u.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = i0 + j < n ? src[i0 + j] : 0;
        c[j] = i0 + j < n ? cls[i0 + j] : 0;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c[j] == 0 || s[j] != 0) continue;
      const uint32_t p = (uint32_t)(i0 + j), y = p / (uint32_t)w;
      const int best = cr_neighbours<CONN8>(cls, src, h, w, (int)y, (int)(p - y * (uint32_t)w), c[j]);
      if (best != INT_MAX) {
        s[j] = best;
        took = true;
      }
    }
    if (whole) {
      *reinterpret_cast<int4*>(dst + i0) = make_int4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) dst[i0 + j] = s[j];
    }
  }
  cr_raise(slot, took);
}

// rem = the class where S == 0, else 0; flag |= 1 when a waiting pixel has a reached neighbour of its class
template <bool CONN8>
__global__ __launch_bounds__(256) void crown_remainder_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ S,
                                                              int h, int w, int64_t n, uint8_t* __restrict__ rem,
                                                              int32_t* flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool open = false;
  if (i < n) {
    const int c = cls[i];
    const bool waits = S[i] == 0;
    rem[i] = (uint8_t)(waits ? c : 0);
    if (waits && c) {
      const uint32_t p = (uint32_t)i, y = p / (uint32_t)w;
      open = cr_neighbours<CONN8>(cls, S, h, w, (int)y, (int)(p - y * (uint32_t)w), c) != INT_MAX;
    }
  }
  cr_raise(flag, open);
}

// ---------------------------------------------------------------- merge and relabel
// seg (in place over the remainder's labels), first[seg - 1] = min p, depth[seg - 1] = max depth2.  The head lane of a run of
// equal segs holds the run's smallest pixel; after the steps the last lane of a run holds at least the run's largest depth
// and nothing but depths of its own seg
__global__ __launch_bounds__(256) void crown_merge_kernel(const int32_t* __restrict__ S, int32_t* __restrict__ seg_plane,
                                                          const int32_t* __restrict__ depth2, int64_t n,
                                                          int32_t* first, int32_t* depth) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int seg = 0, d = 0;
  if (p < n) {
    const int s = S[p];
    seg = s ? s : seg_plane[p];
    if (seg < 0 || seg > n) seg = 0;                       // no id of an n-pixel plane: no index from it leaves the planes
    seg_plane[p] = seg;
    if (seg) d = depth2[p];
  }
  bool head;
  int len;
  uint64_t heads;
  pt_runs(seg, false, lane, head, len, heads);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int oseg = __shfl_up(seg, off, 64), od = __shfl_up(d, off, 64);
    if (lane >= off && oseg == seg && od > d) d = od;
  }
  const int next = __shfl_down(seg, 1, 64);
  if (seg == 0) return;
  // both words only move one way, so a value read before the atomic — however old — says when the atomic cannot change it: a
  // raster-sized seg is two atomics per wave otherwise, all on one pair of words
  if (head && (int)p < CR_LOAD(&first[seg - 1])) atomicMin(&first[seg - 1], (int)p);
  if ((lane == 63 || next != seg) && d > CR_LOAD(&depth[seg - 1])) atomicMax(&depth[seg - 1], d);
}

__global__ __launch_bounds__(256) void crown_relabel_kernel(const int32_t* __restrict__ seg_plane,
                                                            const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ depth, int64_t n,
                                                            int32_t* __restrict__ crowns, int32_t* __restrict__ crown_depth) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int seg = seg_plane[p];
  int label = 0;
  if (seg > 0 && seg <= n) {
    const int f = first[seg - 1];
    if ((unsigned)f < (unsigned)n) {                       // merge met the seg: its first pixel
      label = f + 1;
      if (p == seg - 1) crown_depth[f] = depth[seg - 1];   // every seg names one pixel of its own: one writer per crown
    }
  }
  crowns[p] = label;
}

// ---------------------------------------------------------------- entry points
static int cr_check(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1 && h <= CR_MAX_SIDE && w <= CR_MAX_SIDE, "%s: raster %dx%d: sides must be in 1..%d", tag, h, w,
             CR_MAX_SIDE);
  DT_REQUIRE((int64_t)h * w <= CR_MAX_PIXELS, "%s: raster %dx%d must hold at most 2^31-2 pixels", tag, h, w);
  return DT_OK;
}
static int cr_check_conn(const char* tag, int connectivity) {
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity must be 4 or 8, got %d", tag, connectivity);
  return DT_OK;
}
static inline unsigned cr_grid(int64_t items) { return (unsigned)((items + 255) / 256); }

extern "C" int dt_crown_segment(int* rows) {
  DT_REQUIRE(rows, "crown_segment: null pointer");
  *rows = CR_SEG;
  return DT_OK;
}

extern "C" int dt_patch_depth2_u8(const uint8_t* classes, int h, int w, int K, int cap2, int core2, uint16_t* column,
                                  int32_t* carry, int32_t* depth2, uint8_t* core, int32_t* err_flag, void* stream) {
  DT_TRY(cr_check("patch_depth2_u8", h, w));
  DT_REQUIRE(classes && column && carry && depth2 && err_flag, "patch_depth2_u8: null pointer");
  DT_REQUIRE(K >= 2 && K <= 8, "patch_depth2_u8: K=%d unsupported (2..8)", K);
  DT_REQUIRE(cap2 >= 1 && cap2 <= CR_MAX_DEPTH2, "patch_depth2_u8: cap2 must be in 1..2^30, got %d", cap2);
  DT_REQUIRE(!core || (core2 >= 1 && core2 <= cap2), "patch_depth2_u8: core2 must be in 1..cap2 = %d, got %d", cap2, core2);
  DT_REQUIRE(dt_aligned16(carry), "patch_depth2_u8: carry must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int segs = dt_cdiv(h, CR_SEG), cols = dt_cdiv(w, 64);
  hipLaunchKernelGGL(crown_segment_kernel, dim3(cols, segs), dim3(64), 0, st, classes, h, w, (int4*)carry);
  hipLaunchKernelGGL(crown_chain_kernel, dim3(cols), dim3(64), 0, st, h, w, segs, (int4*)carry);
  hipLaunchKernelGGL(crown_columns_kernel, dim3(cols, segs), dim3(64), 0, st, classes, h, w, (const int4*)carry, column);
  int halo = 1;                                               // the smallest with halo^2 >= cap2; beyond w the whole row
  while (halo < w && (int64_t)halo * halo < cap2) ++halo;
  const int64_t staged = (int64_t)CR_WINDOW + 2 * (int64_t)halo;
  const size_t lds = (size_t)(staged < w ? staged : w) * sizeof(uint32_t);
  hipLaunchKernelGGL(crown_rows_kernel, dim3(dt_cdiv(w, CR_WINDOW), h), dim3(256), lds, st, classes, column, h, w, K, halo,
                     (uint32_t)cap2, (uint32_t)core2, depth2, core, err_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_crown_grow(const uint8_t* classes, const int32_t* src, int32_t* dst, int h, int w, int connectivity,
                             int32_t* slot, void* stream) {
  DT_TRY(cr_check("crown_grow", h, w));
  DT_TRY(cr_check_conn("crown_grow", connectivity));
  DT_REQUIRE(classes && src && dst && slot && src != dst, "crown_grow: null pointer, or src is dst");
  DT_REQUIRE(dt_aligned16(src, dst) && ((uintptr_t)classes & 3) == 0,
             "crown_grow: the planes must be 16-byte aligned, the class map 4-byte");
  const int64_t n = (int64_t)h * w;
  if (connectivity == 8)
    hipLaunchKernelGGL(crown_grow_kernel<true>, dim3(cr_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, classes, src,
                       dst, h, w, n, slot);
  else
    hipLaunchKernelGGL(crown_grow_kernel<false>, dim3(cr_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, classes, src,
                       dst, h, w, n, slot);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_crown_remainder(const uint8_t* classes, const int32_t* grown, int h, int w, int connectivity,
                                  uint8_t* remainder, int32_t* flag, void* stream) {
  DT_TRY(cr_check("crown_remainder", h, w));
  DT_TRY(cr_check_conn("crown_remainder", connectivity));
  DT_REQUIRE(classes && grown && remainder && flag, "crown_remainder: null pointer");
  const int64_t n = (int64_t)h * w;
  if (connectivity == 8)
    hipLaunchKernelGGL(crown_remainder_kernel<true>, dim3(cr_grid(n)), dim3(256), 0, (hipStream_t)stream, classes, grown, h,
                       w, n, remainder, flag);
  else
    hipLaunchKernelGGL(crown_remainder_kernel<false>, dim3(cr_grid(n)), dim3(256), 0, (hipStream_t)stream, classes, grown, h,
                       w, n, remainder, flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_crown_merge(const int32_t* grown, int32_t* seg, const int32_t* depth2, int h, int w, int32_t* first,
                              int32_t* depth, void* stream) {
  DT_TRY(cr_check("crown_merge", h, w));
  DT_REQUIRE(grown && seg && depth2 && first && depth, "crown_merge: null pointer");
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(crown_merge_kernel, dim3(cr_grid(n)), dim3(256), 0, (hipStream_t)stream, grown, seg, depth2, n, first,
                     depth);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_crown_relabel(const int32_t* seg, const int32_t* first, const int32_t* depth, int h, int w, int32_t* crowns,
                                int32_t* crown_depth, void* stream) {
  DT_TRY(cr_check("crown_relabel", h, w));
  DT_REQUIRE(seg && first && depth && crowns && crown_depth, "crown_relabel: null pointer");
  DT_REQUIRE(crowns != first && crowns != depth && crowns != seg, "crown_relabel: crowns must be a plane of its own");
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(crown_relabel_kernel, dim3(cr_grid(n)), dim3(256), 0, (hipStream_t)stream, seg, first, depth, n, crowns,
                     crown_depth);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
