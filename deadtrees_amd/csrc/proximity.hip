// Nearest-patch distances (deployment/proximity.py holds the contract): for a source label plane LS and a query label plane
// LQ, int32 [h][w] in HBM, per query patch the lexicographic minimum of (d2, source root) over the pairs of a query pixel
// and an admissible source pixel, d2 = dy^2 + dx^2 between pixel centres.  Integers only.
//
// The search is separable: a source pixel at minimum distance from p is the nearest admissible pixel of its own column
// above or below p's row.  So
//   columns  per pixel and vertical direction (0: at or above the row, 1: at or below) the distance and the label of the
//            nearest labelled pixel of the column, and with `second` of the nearest labelled pixel whose label differs
//            from that one (what a query of the first one's own patch takes in exclude_own mode).  The column is cut into
//            segments of PX_SEG rows so that h / PX_SEG * w lanes work instead of w: (1) the state a segment leaves
//            behind when it starts from nothing, (2) one lane per column chains the segments' states into the state every
//            segment starts from — the carried fix-up, h / PX_SEG steps —, (3) the segments again, from that state, write
//            the tables.  Three launches, a kernel boundary between them.
//   query    a workgroup takes PX_WINDOW consecutive pixels of one row, compacts the labelled ones in ascending x (ballot
//            and popcount within a wave, LDS across the four waves) and gives one lane to each: it walks outward along
//            the row, dx = 0, 1, 2, ..., while dx^2 <= min(best so far, limit2), reads the candidates of both directions
//            at x - dx and x + dx from the tables through L2, and folds d2 << 32 | root into best[row] with a 64-bit
//            atomicMin, equal rows of neighbouring lanes combined first.  A minimum does not depend on the order.
// No workgroup waits for another, every loop bound is known when its loop starts, no scalar leaves the device.
//
// Planes handed in by a caller are read defensively: a value <= 0 is background, a row is checked against n.
#include "conv_host.h"

#define PX_SEG 64                        // rows per column segment
#define PX_BATCH 8                       // rows of a segment whose labels a lane loads before it walks them
#define PX_WINDOW 1024                   // pixels of one row per query workgroup: 256 lanes, 4 pixels each
#define PX_NONE 0xffffu                  // the distance column's "no such pixel"
#define PX_MAX_SIDE 16384                // column distances fit uint16 below the sentinel, d2 < 2^30
#define PX_MAX_PIXELS 2147483646LL       // 2^31 - 2: labels are int32 and 1-based
static_assert(PX_WINDOW == 4 * 256, "a lane takes four pixels of the window");

// the nearest labelled pixel met so far (row r1, label l1) and the nearest whose label differs from l1 (r2, l2); r < 0: none
struct px_state {
  int r1, l1, r2, l2;
};

__device__ __forceinline__ void px_step(px_state& s, int y, int label) {
  if (label <= 0) return;
  if (s.r1 < 0 || label != s.l1) {         // the pixel left behind is the nearest one of another label
    s.r2 = s.r1;
    s.l2 = s.l1;
    s.l1 = label;
  }
  s.r1 = y;
}

// the state behind a segment that leaves `seg` when started from nothing, entered with `in`
__device__ __forceinline__ px_state px_chain(const px_state& in, const px_state& seg) {
  if (seg.r1 < 0) return in;
  px_state out = seg;
  if (seg.r2 < 0 && in.r1 >= 0) {          // the segment holds one label only: the other one comes from before it
    if (in.l1 != seg.l1) {
      out.r2 = in.r1;
      out.l2 = in.l1;
    } else {
      out.r2 = in.r2;
      out.l2 = in.l2;
    }
  }
  return out;
}

// grid (ceil(w / 64), segments, 2 directions), 64 lanes: a lane walks its column through one segment, downwards for
// direction 0 and upwards for direction 1.  WRITE false: from nothing, the state left behind goes to carry[dir][seg][x].
// WRITE true: from carry[dir][seg][x], the tables' entries of the segment are written
template <bool WRITE>
__global__ __launch_bounds__(64) void proximity_segment_kernel(const int32_t* __restrict__ LS, int h, int w, int segs,
                                                               int second, int4* __restrict__ carry,
                                                               uint16_t* __restrict__ dist, int32_t* __restrict__ near,
                                                               int32_t* __restrict__ flag) {
  const int x = blockIdx.x * 64 + threadIdx.x, seg = blockIdx.y, dir = blockIdx.z;
  if (!WRITE && x == 0 && seg == 0 && dir == 0) *flag = 0;      // the chain kernel behind this one sets it
  if (x >= w) return;
  const int y0 = seg * PX_SEG, y1 = min(h, y0 + PX_SEG);
  const int64_t at = ((int64_t)dir * segs + seg) * w + x;
  px_state s = {-1, 0, -1, 0};
  if (WRITE) {
    const int4 c = carry[at];
    s = {c.x, c.y, c.z, c.w};
  }
  const int64_t plane = (int64_t)h * w;
  const int rows = y1 - y0;
  for (int k0 = 0; k0 < rows; k0 += PX_BATCH) {                 // the loads of a batch are in flight together
    int label[PX_BATCH];
#pragma unroll
    for (int j = 0; j < PX_BATCH; ++j) {
      const int k = k0 + j, y = dir ? y1 - 1 - k : y0 + k;
      label[j] = k < rows ? LS[(int64_t)y * w + x] : 0;
    }
#pragma unroll
    for (int j = 0; j < PX_BATCH; ++j) {
      const int k = k0 + j, y = dir ? y1 - 1 - k : y0 + k;
      if (k >= rows) break;
      const int64_t p = (int64_t)y * w + x;
      px_step(s, y, label[j]);
      if (WRITE) {
        dist[dir * plane + p] = s.r1 < 0 ? (uint16_t)PX_NONE : (uint16_t)abs(y - s.r1);
        near[dir * plane + p] = s.r1 < 0 ? 0 : s.l1;
        if (second) {
          dist[(2 + dir) * plane + p] = s.r2 < 0 ? (uint16_t)PX_NONE : (uint16_t)abs(y - s.r2);
          near[(2 + dir) * plane + p] = s.r2 < 0 ? 0 : s.l2;
        }
      }
    }
  }
  if (!WRITE) carry[at] = make_int4(s.r1, s.l1, s.r2, s.l2);
}

// grid (ceil(w / 64), 2 directions): a lane chains the segments of its column in the direction's order and replaces every
// segment's own state by the state it starts from.  flag |= 1 when the plane holds a labelled pixel at all
__global__ __launch_bounds__(64) void proximity_chain_kernel(int w, int segs, int4* __restrict__ carry,
                                                             int32_t* __restrict__ flag) {
  const int x = blockIdx.x * 64 + threadIdx.x, dir = blockIdx.y;
  px_state s = {-1, 0, -1, 0};
  if (x < w)
    for (int k = 0; k < segs; ++k) {
      const int seg = dir ? segs - 1 - k : k;
      const int64_t at = ((int64_t)dir * segs + seg) * w + x;
      const int4 c = carry[at];
      carry[at] = make_int4(s.r1, s.l1, s.r2, s.l2);
      s = px_chain(s, {c.x, c.y, c.z, c.w});
    }
  if (dir == 0 && __ballot(s.r1 >= 0) != 0 && threadIdx.x == 0) atomicOr(flag, 1);
}

// folds the candidate (g, label) of column distance dx2 into the lane's best key and bound
__device__ __forceinline__ void px_fold(const uint16_t* __restrict__ dist, const int32_t* __restrict__ near, int64_t plane,
                                        int64_t p, int own, uint32_t dx2, uint64_t& key, uint32_t& bound) {
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    uint32_t g = dist[dir * plane + p];
    if (g == PX_NONE) continue;
    int label = near[dir * plane + p];
    if (label == own) {                    // exclude_own (own is 0 otherwise): the nearest pixel of another label
      g = dist[(2 + dir) * plane + p];
      if (g == PX_NONE) continue;
      label = near[(2 + dir) * plane + p];
    }
    const uint32_t d2 = dx2 + g * g;
    if (label <= 0 || d2 > bound) continue;
    const uint64_t k = ((uint64_t)d2 << 32) | (uint32_t)(label - 1);
    if (k < key) {
      key = k;
      bound = d2;
    }
  }
}

// grid (ceil(w / PX_WINDOW), h), 256 lanes
__global__ __launch_bounds__(256) void proximity_query_kernel(const uint16_t* __restrict__ dist,
                                                              const int32_t* __restrict__ near,
                                                              const int32_t* __restrict__ flag,
                                                              const int32_t* __restrict__ LQ, int h, int w,
                                                              const int32_t* __restrict__ dense, int rows, int exclude_own,
                                                              uint32_t limit, unsigned long long* __restrict__ best) {
  __shared__ int wsum[4][4];
  __shared__ uint16_t qx[PX_WINDOW];
  __shared__ int32_t ql[PX_WINDOW];
  if (*flag == 0) return;                  // no source pixel anywhere: every entry of best stays all ones
  const int y = blockIdx.y, x0 = blockIdx.x * PX_WINDOW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const int64_t row0 = (int64_t)y * w, plane = (int64_t)h * w;
  // compaction in ascending x = x0 + 256 k + 64 wave + lane
  int label[4], rank[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + 256 * k + threadIdx.x;
    label[k] = x < w ? LQ[row0 + x] : 0;
    const uint64_t m = __ballot(label[k] > 0);
    rank[k] = __popcll(m & below);
    if (lane == 0) wsum[k][wave] = __popcll(m);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int first = total;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < wave) first += wsum[k][v];
      total += wsum[k][v];
    }
    if (label[k] > 0) {
      qx[first + rank[k]] = (uint16_t)(x0 + 256 * k + threadIdx.x);
      ql[first + rank[k]] = label[k];
    }
  }
  __syncthreads();
  for (int i0 = 64 * wave; i0 < total; i0 += 256) {            // wave-uniform: the shuffles below need every lane
    const int i = i0 + lane;
    int row = -1;
    uint64_t key = ~(uint64_t)0;
    if (i < total) {
      const int x = qx[i], own = ql[i];
      const int r = own <= plane ? dense[own - 1] : -1;       // a label beyond the raster names no root
      if ((unsigned)r < (unsigned)rows) {
        row = r;
        // the patch's best so far is reached by some pair: nothing beyond it can lower the patch's minimum
        const unsigned long long seen = __hip_atomic_load(&best[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t reached = (uint32_t)(seen >> 32);
        uint32_t bound = reached < limit ? reached : limit;
        const int other = exclude_own ? own : 0;
        for (int dx = 0; dx < w; ++dx) {
          const uint32_t dx2 = (uint32_t)dx * (uint32_t)dx;
          const bool left = x - dx >= 0, right = dx > 0 && x + dx < w;
          if (dx2 > bound || !(left || right)) break;
          if (left) px_fold(dist, near, plane, row0 + x - dx, other, dx2, key, bound);
          if (right) px_fold(dist, near, plane, row0 + x + dx, other, dx2, key, bound);
        }
      }
    }
    // equal rows of neighbouring lanes: after the steps the last lane of a stretch of one row holds the stretch's minimum
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int orow = __shfl_up(row, off, 64);
      const uint64_t okey = (uint64_t)__shfl_up((long long)key, off, 64);
      if (lane >= off && orow == row && okey < key) key = okey;
    }
    const int next = __shfl_down(row, 1, 64);
    if (row >= 0 && key != ~(uint64_t)0 && (lane == 63 || next != row))
      __hip_atomic_fetch_min(&best[row], (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- entry points
static int px_check(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1 && h <= PX_MAX_SIDE && w <= PX_MAX_SIDE, "%s: raster %dx%d: sides must be in 1..%d", tag, h, w,
             PX_MAX_SIDE);
  DT_REQUIRE((int64_t)h * w <= PX_MAX_PIXELS, "%s: raster %dx%d must hold at most 2^31-2 pixels", tag, h, w);
  return DT_OK;
}

extern "C" int dt_proximity_segment(int* rows) {
  DT_REQUIRE(rows, "proximity_segment: null pointer");
  *rows = PX_SEG;
  return DT_OK;
}

extern "C" int dt_proximity_window(int* pixels) {
  DT_REQUIRE(pixels, "proximity_window: null pointer");
  *pixels = PX_WINDOW;
  return DT_OK;
}

extern "C" int dt_proximity_columns(const int32_t* labels_src, int h, int w, int second, uint16_t* dist, int32_t* nearest,
                                    int32_t* carry, int32_t* flag, void* stream) {
  DT_TRY(px_check("proximity_columns", h, w));
  DT_REQUIRE(labels_src && dist && nearest && carry && flag, "proximity_columns: null pointer");
  DT_REQUIRE(dt_aligned16(carry), "proximity_columns: carry must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int segs = dt_cdiv(h, PX_SEG), cols = dt_cdiv(w, 64);
  hipLaunchKernelGGL(proximity_segment_kernel<false>, dim3(cols, segs, 2), dim3(64), 0, st, labels_src, h, w, segs,
                     second != 0, (int4*)carry, dist, nearest, flag);
  hipLaunchKernelGGL(proximity_chain_kernel, dim3(cols, 2), dim3(64), 0, st, w, segs, (int4*)carry, flag);
  hipLaunchKernelGGL(proximity_segment_kernel<true>, dim3(cols, segs, 2), dim3(64), 0, st, labels_src, h, w, segs,
                     second != 0, (int4*)carry, dist, nearest, flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_proximity_query(const uint16_t* dist, const int32_t* nearest, const int32_t* flag,
                                  const int32_t* labels_qry, int h, int w, const int32_t* dense_plane, int n, int exclude_own,
                                  int second, int64_t limit2, uint64_t* best, void* stream) {
  DT_TRY(px_check("proximity_query", h, w));
  DT_REQUIRE(n >= 0 && n <= (int64_t)h * w, "proximity_query: n=%d rows for %lld pixels", n, (long long)h * w);
  if (n == 0) return DT_OK;
  DT_REQUIRE(dist && nearest && flag && labels_qry && dense_plane && best, "proximity_query: null pointer");
  DT_REQUIRE(!exclude_own || second, "proximity_query: exclude_own needs tables built with second != 0");
  const uint32_t limit = limit2 < 0 || limit2 > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)limit2;
  hipLaunchKernelGGL(proximity_query_kernel, dim3(dt_cdiv(w, PX_WINDOW), h), dim3(256), 0, (hipStream_t)stream, dist, nearest,
                     flag, labels_qry, h, w, dense_plane, n, exclude_own != 0, limit, (unsigned long long*)best);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
