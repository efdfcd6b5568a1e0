// Dead-tree patch outlines (deployment/outlines.py holds the contract): the boundary of every patch of a label plane that
// already sits in HBM, traced into rings — one vertex per corner, in the canonical order — before anything is downloaded.
//
// A labelled pixel p = i * w + j owns side s (0 top, 1 right, 2 bottom, 3 left) iff the neighbour across it carries another
// label; the edge key is 4 p + s and every edge has exactly one successor on its ring (a left turn, straight on, or a right
// turn, chosen from the two pixels ahead).  The rings are the cycles of that permutation.  The phases, each a launch of its
// own (kernel boundaries order them: no kernel waits for another workgroup, every loop bound is known at launch):
//   count    a workgroup per OL_CHUNK consecutive pixels: owned sides and corners of the chunk
//   first    the same walk + an in-workgroup scan: first[p], the compact index of p's first edge, and every edge's key.
//            Compaction in row-major order makes compact order key order
//   link     per edge: its successor's compact index = first[q] + the owned sides of q below the successor's side
//   jump     ceil(log2 E) rounds of pointer jumping, double-buffered: per edge (m, d, ws, j) = the smallest edge of the
//            window of 2^k edges from it on, the corners in front of that minimum, the corners of the whole window, the
//            edge behind the window.  At the end m is the ring id and d the corners between the edge and the ring's head
//   rings    per ring head: its corner count and label;  scatter  per corner edge: its vertex to ring_offsets[row] + index
// Ordering the rings by (label, id) and scanning their corner counts in between is left to the caller (a sort and a
// scan over rings).  Integers only; no atomics: the result is a pure function of the label plane.
//
// A label plane handed in by a caller is read defensively: a value <= 0 is background, every index derived from the
// plane is a pixel of the plane or a compact edge index below E, and the scatter checks its target against V.
#include "conv_host.h"

#define OL_CHUNK 1024                    // pixels per workgroup in the count / first launches: 4 steps of 256 lanes
#define OL_MAX_SIDE 16384                // 4 * h * w + 3 fits 31 bits: bit 31 of an edge word is its corner flag
#define OL_CORNER 0x80000000u
static_assert(OL_CHUNK % 256 == 0, "a chunk is walked in steps of one workgroup");

__device__ __forceinline__ int ol_at(const int32_t* __restrict__ L, int h, int w, int i, int j) {
  if ((unsigned)i >= (unsigned)h || (unsigned)j >= (unsigned)w) return 0;
  const int l = L[(int64_t)i * w + j];
  return l > 0 ? l : 0;
}

// the pixel across side s, the pixel B ahead of side s, and A = B's neighbour across side s, as offsets (di, dj)
__device__ __forceinline__ int ol_across_di(int s) { return (s == 2) - (s == 0); }
__device__ __forceinline__ int ol_across_dj(int s) { return (s == 1) - (s == 3); }
__device__ __forceinline__ int ol_ahead_di(int s) { return (s == 1) - (s == 3); }
__device__ __forceinline__ int ol_ahead_dj(int s) { return (s == 0) - (s == 2); }

// bit s: pixel (i, j) with label l owns side s
__device__ __forceinline__ int ol_sides(const int32_t* __restrict__ L, int h, int w, int i, int j, int l) {
  if (l == 0) return 0;
  return (ol_at(L, h, w, i - 1, j) != l) | (ol_at(L, h, w, i, j + 1) != l) << 1 | (ol_at(L, h, w, i + 1, j) != l) << 2 |
         (ol_at(L, h, w, i, j - 1) != l) << 3;
}

// straight on from side s: B carries the label and A does not (the same for both connectivities)
__device__ __forceinline__ bool ol_straight(const int32_t* __restrict__ L, int h, int w, int i, int j, int l, int s) {
  const int bi = i + ol_ahead_di(s), bj = j + ol_ahead_dj(s);
  return ol_at(L, h, w, bi, bj) == l && ol_at(L, h, w, bi + ol_across_di(s), bj + ol_across_dj(s)) != l;
}

// bit s: side s is owned and its end point is a corner
__device__ __forceinline__ int ol_corners(const int32_t* __restrict__ L, int h, int w, int i, int j, int l, int sides) {
  int corners = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if ((sides >> s & 1) && !ol_straight(L, h, w, i, j, l, s)) corners |= 1 << s;
  return corners;
}

// the successor of edge (p = (i, j), s) as a compact index.  A pixel that carries l > 0 lies inside the raster, so every
// first[] entry read belongs to the plane
__device__ __forceinline__ int ol_successor(const int32_t* __restrict__ L, const int32_t* __restrict__ first, int h, int w,
                                            int conn8, int i, int j, int s) {
  const int l = ol_at(L, h, w, i, j);
  if (l == 0) return -1;                                                     // no edge of this plane: the callers stay put
  const int bi = i + ol_ahead_di(s), bj = j + ol_ahead_dj(s);
  const int ai = bi + ol_across_di(s), aj = bj + ol_across_dj(s);
  const bool same_b = ol_at(L, h, w, bi, bj) == l, same_a = ol_at(L, h, w, ai, aj) == l;
  int qi = i, qj = j, t = (s + 1) & 3;                                       // right: the next side of p
  if (conn8 ? same_a : (same_a && same_b)) { qi = ai; qj = aj; t = (s + 3) & 3; }      // left: around the corner to A
  else if (same_b) { qi = bi; qj = bj; t = s; }                              // straight: the same side of B
  const int below = ol_sides(L, h, w, qi, qj, l) & ((1 << t) - 1);
  return first[(int64_t)qi * w + qj] + __popc(below);
}

// exclusive prefix sum of v over the 256 lanes of the workgroup in lane order; `total`: the sum.  wsum: 4 ints of LDS
__device__ __forceinline__ int ol_block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = wsum[k];
    if (k < wave) base += s;
    total += s;
  }
  __syncthreads();                                                         // wsum is free again
  return base + inc - v;
}

// counts int32 [chunks][2]: owned sides and corners of the chunk's pixels
__global__ __launch_bounds__(256) void outline_count_kernel(const int32_t* __restrict__ L, int h, int w, int64_t n,
                                                            int32_t* __restrict__ counts) {
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * OL_CHUNK;
  int edges = 0, corners = 0;
  for (int k = 0; k < OL_CHUNK / 256; ++k) {
    const int64_t p = base + k * 256 + threadIdx.x;
    if (p >= n) break;
    const int i = (int)((uint32_t)p / (uint32_t)w), j = (int)((uint32_t)p % (uint32_t)w);
    const int l = ol_at(L, h, w, i, j);
    const int sides = ol_sides(L, h, w, i, j, l);
    edges += __popc(sides);
    corners += __popc(ol_corners(L, h, w, i, j, l, sides));
  }
  int total_edges, total_corners;
  ol_block_scan(edges, wsum, total_edges);
  ol_block_scan(corners, wsum, total_corners);
  if (threadIdx.x == 0) {
    counts[2 * (int64_t)blockIdx.x] = total_edges;
    counts[2 * (int64_t)blockIdx.x + 1] = total_corners;
  }
}

// chunk_first int32 [chunks]: edges in front of the chunk.  Writes first[p] for every pixel and the word of every edge:
// 4 p + s, OL_CORNER set when its end point is a corner
__global__ __launch_bounds__(256) void outline_first_kernel(const int32_t* __restrict__ L, int h, int w, int64_t n,
                                                            const int32_t* __restrict__ chunk_first, int E,
                                                            int32_t* __restrict__ first, uint32_t* __restrict__ edge) {
  __shared__ int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * OL_CHUNK;
  int at = chunk_first[blockIdx.x];
  for (int k = 0; k < OL_CHUNK / 256; ++k) {               // uniform trip count: every lane reaches the barriers of the scan
    const int64_t p = base + k * 256 + threadIdx.x;
    int sides = 0, corners = 0;
    if (p < n) {
      const int i = (int)((uint32_t)p / (uint32_t)w), j = (int)((uint32_t)p % (uint32_t)w);
      const int l = ol_at(L, h, w, i, j);
      sides = ol_sides(L, h, w, i, j, l);
      corners = ol_corners(L, h, w, i, j, l, sides);
    }
    int total;
    int e = at + ol_block_scan(__popc(sides), wsum, total);
    at += total;
    if (p < n) {
      first[p] = e;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (sides >> s & 1) {
          if ((unsigned)e < (unsigned)E) edge[e] = (uint32_t)(4 * p + s) | ((corners >> s & 1) ? OL_CORNER : 0u);
          ++e;
        }
    }
  }
}

// state[e] = (e, 0, corner(e), successor(e)): the window of one edge
__global__ __launch_bounds__(256) void outline_link_kernel(const int32_t* __restrict__ L, const int32_t* __restrict__ first,
                                                           int h, int w, int conn8, const uint32_t* __restrict__ edge, int E,
                                                           int4* __restrict__ state) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const uint32_t word = edge[e], key = word & ~OL_CORNER;
  const uint32_t p = key >> 2;
  int succ = ol_successor(L, first, h, w, conn8, (int)(p / (uint32_t)w), (int)(p % (uint32_t)w), (int)(key & 3u));
  if ((unsigned)succ >= (unsigned)E) succ = e;             // cannot happen with first[] of this plane: stay inside the arrays
  state[e] = make_int4(e, 0, (int)(word >> 31), succ);
}

// one round: the window of e and the window behind it become one
__global__ __launch_bounds__(256) void outline_jump_kernel(const int4* __restrict__ in, int4* __restrict__ out, int E) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int4 a = in[e];
  const int4 b = in[a.w];
  if (b.x < a.x) {                    // strictly: a window that wraps around its ring keeps the first occurrence
    a.y = a.z + b.y;
    a.x = b.x;
  }
  a.z += b.z;
  a.w = b.w;
  out[e] = a;
}

__global__ __launch_bounds__(256) void outline_heads_kernel(const int4* __restrict__ state, int E, uint8_t* __restrict__ head) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) head[e] = state[e].x == e;
}

// ring r (in ascending id) with head edge heads[r]: its corner count = the corners from the head's successor back to the
// head + the head's own, and the label of its pixels
__global__ __launch_bounds__(256) void outline_rings_kernel(const int32_t* __restrict__ L, const int32_t* __restrict__ first,
                                                            int h, int w, int conn8, const uint32_t* __restrict__ edge,
                                                            const int4* __restrict__ state, int E,
                                                            const int64_t* __restrict__ heads, int R,
                                                            int32_t* __restrict__ corners, int32_t* __restrict__ label) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t e = heads[r];
  if (e < 0 || e >= E) {
    corners[r] = 0;
    label[r] = 0;
    return;
  }
  const uint32_t word = edge[e], key = word & ~OL_CORNER;
  const uint32_t p = key >> 2;
  const int i = (int)(p / (uint32_t)w), j = (int)(p % (uint32_t)w);
  int succ = ol_successor(L, first, h, w, conn8, i, j, (int)(key & 3u));
  if ((unsigned)succ >= (unsigned)E) succ = (int)e;
  corners[r] = state[succ].y + (int)(word >> 31);
  label[r] = ol_at(L, h, w, i, j);
}

// every corner edge writes its end point, in 1/256 pixel, to its place in its ring: ring_offsets[row] + (0 for the head,
// else the ring's corner count - the corners from the edge to the head)
__global__ __launch_bounds__(256) void outline_scatter_kernel(const uint32_t* __restrict__ edge,
                                                              const int4* __restrict__ state, int E, int w,
                                                              const int32_t* __restrict__ row_of,
                                                              const int64_t* __restrict__ ring_offsets, int R, int64_t V,
                                                              int32_t* __restrict__ xy) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const uint32_t word = edge[e];
  if (!(word & OL_CORNER)) return;
  const int4 st = state[e];
  if ((unsigned)st.x >= (unsigned)E) return;
  const int row = row_of[st.x];
  if ((unsigned)row >= (unsigned)R) return;
  const int64_t off = ring_offsets[row], count = ring_offsets[row + 1] - off;
  const int64_t at = off + (st.x == e ? 0 : count - st.y);
  if (at < off || at >= off + count || at >= V) return;
  const uint32_t key = word & ~OL_CORNER, p = key >> 2;
  const int s = (int)(key & 3u), i = (int)(p / (uint32_t)w), j = (int)(p % (uint32_t)w);
  xy[2 * at] = 256 * (j + (s < 2));
  xy[2 * at + 1] = 256 * (i + (s == 1 || s == 2));
}

// ---------------------------------------------------------------- entry points
static int ol_check_size(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1 && h <= OL_MAX_SIDE && w <= OL_MAX_SIDE, "%s: raster %dx%d must be 1..%d in height and width",
             tag, h, w, OL_MAX_SIDE);
  return DT_OK;
}
static int ol_check_connectivity(const char* tag, int connectivity) {
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity must be 4 or 8, got %d", tag, connectivity);
  return DT_OK;
}
static inline unsigned ol_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int dt_outline_chunk(int* chunk) {
  DT_REQUIRE(chunk, "outline_chunk: null pointer");
  *chunk = OL_CHUNK;
  return DT_OK;
}

extern "C" int dt_outline_count(const int32_t* labels, int h, int w, int32_t* chunk_counts, void* stream) {
  DT_REQUIRE(labels && chunk_counts, "outline_count: null pointer");
  DT_TRY(ol_check_size("outline_count", h, w));
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(outline_count_kernel, dim3((unsigned)((n + OL_CHUNK - 1) / OL_CHUNK)), dim3(256), 0, (hipStream_t)stream,
                     labels, h, w, n, chunk_counts);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_outline_edges(const int32_t* labels, int h, int w, int connectivity, const int32_t* chunk_first,
                                int n_edges, int32_t* first, uint32_t* edges, int32_t* state, void* stream) {
  DT_REQUIRE(labels && chunk_first && first, "outline_edges: null pointer");
  DT_TRY(ol_check_size("outline_edges", h, w));
  DT_TRY(ol_check_connectivity("outline_edges", connectivity));
  DT_REQUIRE(n_edges >= 0 && n_edges <= 4 * (int64_t)h * w, "outline_edges: n_edges=%d for %lld pixels", n_edges,
             (long long)h * w);
  DT_REQUIRE(n_edges == 0 || (edges && state), "outline_edges: null edge arrays");
  DT_REQUIRE(dt_aligned16(state), "outline_edges: state must be 16-byte aligned");
  const int64_t n = (int64_t)h * w;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(outline_first_kernel, dim3((unsigned)((n + OL_CHUNK - 1) / OL_CHUNK)), dim3(256), 0, st, labels, h, w, n,
                     chunk_first, n_edges, first, edges);
  if (n_edges)
    hipLaunchKernelGGL(outline_link_kernel, dim3(ol_grid(n_edges)), dim3(256), 0, st, labels, first, h, w,
                       connectivity == 8, edges, n_edges, (int4*)state);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_outline_rounds(int n_edges) {
  int rounds = 0;
  while (((int64_t)1 << rounds) < n_edges) ++rounds;
  return rounds;
}

extern "C" int dt_outline_jump(int32_t* state, int32_t* scratch, int n_edges, uint8_t* head, void* stream) {
  DT_REQUIRE(n_edges >= 1, "outline_jump: n_edges must be >= 1, got %d", n_edges);
  DT_REQUIRE(state && scratch && head && state != scratch, "outline_jump: null or aliased buffers");
  DT_REQUIRE(dt_aligned16(state, scratch), "outline_jump: state buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int4 *in = (int4*)state, *out = (int4*)scratch;
  const int rounds = dt_outline_rounds(n_edges);
  for (int k = 0; k < rounds; ++k) {
    hipLaunchKernelGGL(outline_jump_kernel, dim3(ol_grid(n_edges)), dim3(256), 0, st, in, out, n_edges);
    int4* t = in;
    in = out;
    out = t;
  }
  hipLaunchKernelGGL(outline_heads_kernel, dim3(ol_grid(n_edges)), dim3(256), 0, st, in, n_edges, head);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_outline_rings(const int32_t* labels, int h, int w, int connectivity, const int32_t* first,
                                const uint32_t* edges, const int32_t* state, int n_edges, const int64_t* heads, int n_rings,
                                int32_t* ring_corners, int32_t* ring_label, void* stream) {
  DT_REQUIRE(labels && first && edges && state && heads && ring_corners && ring_label, "outline_rings: null pointer");
  DT_TRY(ol_check_size("outline_rings", h, w));
  DT_TRY(ol_check_connectivity("outline_rings", connectivity));
  DT_REQUIRE(n_edges >= 1 && n_rings >= 1 && n_rings <= n_edges, "outline_rings: %d rings of %d edges", n_rings, n_edges);
  hipLaunchKernelGGL(outline_rings_kernel, dim3(ol_grid(n_rings)), dim3(256), 0, (hipStream_t)stream, labels, first, h, w,
                     connectivity == 8, edges, (const int4*)state, n_edges, heads, n_rings, ring_corners, ring_label);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_outline_scatter(const uint32_t* edges, const int32_t* state, int n_edges, int w, const int32_t* row_of,
                                  const int64_t* ring_offsets, int n_rings, int64_t n_vertices, int32_t* xy, void* stream) {
  DT_REQUIRE(edges && state && row_of && ring_offsets && xy, "outline_scatter: null pointer");
  DT_REQUIRE(n_edges >= 1 && n_rings >= 1 && n_vertices >= 1 && w >= 1 && w <= OL_MAX_SIDE,
             "outline_scatter: bad sizes (edges=%d, rings=%d, vertices=%lld, w=%d)", n_edges, n_rings, (long long)n_vertices, w);
  hipLaunchKernelGGL(outline_scatter_kernel, dim3(ol_grid(n_edges)), dim3(256), 0, (hipStream_t)stream, edges,
                     (const int4*)state, n_edges, w, row_of, ring_offsets, n_rings, n_vertices, xy);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
