// Dead-tree patches (deployment/patches.py holds the contract): connected components of a uint8 class map that already sits
// in HBM, their areas, an area sieve and the per-patch table, all before the map is downloaded.
//
// A patch is a maximal set of pixels of one class c, 1 <= c < K, connected through 4- or 8-neighbourhoods.  The label plane
// doubles as the union-find forest: labels[i] = 1 + parent(i), 0 on background, and parent(i) <= i ALWAYS.  A root is a
// pixel with labels[i] == i + 1, and because parents never exceed their children the root of a finished tree is the
// smallest index of its patch: the final label 1 + min(y * w + x) needs no renumbering pass and is unique.
//
// dt_label_patches_u8 is three launches; the kernel boundaries order the phases (no grid barrier, no cooperative launch):
//   local    one workgroup per PT_TH x PT_TW tile, union-find in LDS, writes 1 + global index of the in-tile root
//   merge    one lane per pixel of a tile border: unions across it, lock-free in global memory
//   flatten  every labelled pixel chases its parent to the root
//
// Termination, by construction.  find: x -> parent(x) strictly decreases until parent(x) == x.  union(a, b): a, b <- their
// roots; with a > b, old = atomicMin(&parent[a], b).  old == a: a was a root and now hangs under b, done.  Otherwise another
// lane got there first and old < a; whichever of old and b the slot now holds, the other one still has to meet it, so the
// loop goes on with (old, b): max(a, b) strictly decreases.  A lane never waits for another lane: no spin, no lock.
//
// Stale reads.  Every value a parent slot ever held is an ancestor (<= the slot's index), so an OLD value only costs a
// longer walk or one more round of the union loop, never a wrong answer; a "root" that is no longer one is caught by the
// atomicMin's return value, which is never stale.  The MI355X has one L2 per XCD, so in the merge and flatten kernels parent
// slots are read with agent-scope atomic loads (served past the L1) and written only with agent-scope atomics.
//
// Areas and the table are integer atomics pre-combined across a wave: consecutive lanes of a row nearly always share a
// root, so a wave finds its runs of equal labels with one ballot, the head lane of a run speaks for it, and the run that
// is still open at the end of a 64-pixel chunk is carried into the next one (a wave owns PT_SPAN consecutive chunks).  A
// raster-sized single patch is one atomic per 1024 pixels, not one per pixel.
#include <limits.h>

#include "conv_host.h"
#include "patch_runs.h"

#define PT_TH 32                         // tile rows
#define PT_TW 64                         // tile columns: one wave per tile row, 64 consecutive class bytes per load
#define PT_N (PT_TH * PT_TW)
#define PT_SPAN 16                       // 64-pixel chunks per wave in the area / measure kernels
#define PT_MAXK 8
#define PT_MAX_PIXELS 2147483646ll       // labels are int32 and 1-based
static_assert(PT_TW == 64, "a tile row is one wave");

#define PT_LOAD_LDS(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define PT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PT_MIN(p, v, scope) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, scope)

// ---------------------------------------------------------------- union-find over 0-based parents (LDS, inside one tile)
__device__ __forceinline__ int pt_lds_find(int* par, int x) {
  int p;
  while ((p = PT_LOAD_LDS(&par[x])) != x) x = p;          // p <= x: strictly decreasing
  return x;
}
__device__ __forceinline__ void pt_lds_union(int* par, int a, int b) {
  for (;;) {
    a = pt_lds_find(par, a);
    b = pt_lds_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = PT_MIN(&par[a], b, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;                                              // old < a: max(a, b) went down
  }
}

// ---------------------------------------------------------------- the same over the label plane (1-based, global memory)
__device__ __forceinline__ int pt_find(int32_t* lab, int x) {
  int p;
  while ((p = PT_LOAD(&lab[x]) - 1) != x) x = p;
  return x;
}
__device__ __forceinline__ void pt_union(int32_t* lab, int a, int b) {
  for (;;) {
    a = pt_find(lab, a);
    b = pt_find(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = PT_MIN(&lab[a], b + 1, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (old == a) return;
    a = old;
  }
}

// tile t of the row-major tile grid; lanes = tile columns, the four waves take the rows r = wave, wave + 4, ...
__global__ __launch_bounds__(256) void patch_local_kernel(const uint8_t* __restrict__ classes, int h, int w, int ntx, int K,
                                                          int conn8, int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ err) {
  __shared__ int par[PT_N];
  __shared__ uint8_t cls[PT_N];
  const int ty0 = (int)(blockIdx.x / (unsigned)ntx) * PT_TH, tx0 = (int)(blockIdx.x % (unsigned)ntx) * PT_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gx = tx0 + lane;
  bool bad = false;
  for (int r = wave; r < PT_TH; r += 4) {
    const int gy = ty0 + r;
    int c = 0;
    if (gy < h && gx < w) {
      c = classes[(int64_t)gy * w + gx];
      if (c >= K) { bad = true; c = 0; }
    }
    // a horizontal run of one class starts united: parent = the run's first pixel
    const int left = __shfl_up(c, 1, 64);
    const uint64_t heads = __ballot(lane == 0 || left != c);
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));     // bit 0 is always set
    cls[r * PT_TW + lane] = (uint8_t)c;
    par[r * PT_TW + lane] = r * PT_TW + start;
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(err, 1);
  __syncthreads();
  for (int r = wave < 1 ? 4 : wave; r < PT_TH; r += 4) {      // rows >= 1 meet the row above
    const int i = r * PT_TW + lane, up = i - PT_TW;
    const int c = cls[i];
    if (c == 0) continue;
    if (cls[up] == c) {
      pt_lds_union(par, i, up);       // its equal-class neighbours in that row are in up's run already
    } else if (conn8) {
      if (lane > 0 && cls[up - 1] == c) pt_lds_union(par, i, up - 1);
      if (lane < 63 && cls[up + 1] == c) pt_lds_union(par, i, up + 1);
    }
  }
  __syncthreads();
  for (int r = wave; r < PT_TH; r += 4) {
    const int gy = ty0 + r, i = r * PT_TW + lane;
    if (gy >= h || gx >= w) continue;
    int32_t label = 0;
    if (cls[i]) {
      const int root = pt_lds_find(par, i);
      label = 1 + (ty0 + root / PT_TW) * w + tx0 + root % PT_TW;
    }
    labels[(int64_t)gy * w + gx] = label;
  }
}

// pixel i = (y, x) and its neighbour (qy, qx) across a tile border: one patch when both carry the same labelled class
__device__ __forceinline__ void pt_join(const uint8_t* __restrict__ classes, int32_t* lab, int h, int w, int y, int x, int qy,
                                        int qx) {
  if (qy < 0 || qy >= h || qx < 0 || qx >= w) return;
  const int i = y * w + x, q = qy * w + qx;
  if (classes[i] != classes[q] || PT_LOAD(&lab[i]) == 0) return;     // label 0: background or a class >= K, on both sides
  pt_union(lab, i, q);
}

// items [0, nhb * w): pixel x of the top row of tile row b + 1 meets the row above it; then [.., + nvb * h): pixel y of the
// left column of tile column b + 1 meets the column left of it.  With 8-neighbourhoods a top-row pixel also looks north-west
// and north-east, a left-column pixel north-west and SOUTH-west: together every diagonal pair that straddles a border or a
// tile corner (north-east of p across a vertical border is south-west of its partner, which sits on a left column).
__global__ __launch_bounds__(256) void patch_merge_kernel(const uint8_t* __restrict__ classes, int h, int w, int nhb, int nvb,
                                                          int conn8, int32_t* lab) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t horizontal = (int64_t)nhb * w;
  if (t < horizontal) {
    const int y = ((int)(t / w) + 1) * PT_TH, x = (int)(t % w);
    pt_join(classes, lab, h, w, y, x, y - 1, x);
    if (conn8) {
      pt_join(classes, lab, h, w, y, x, y - 1, x - 1);
      pt_join(classes, lab, h, w, y, x, y - 1, x + 1);
    }
    return;
  }
  t -= horizontal;
  if (t >= (int64_t)nvb * h) return;
  const int x = ((int)(t / h) + 1) * PT_TW, y = (int)(t % h);
  pt_join(classes, lab, h, w, y, x, y, x - 1);
  if (conn8) {
    if (y % PT_TH) pt_join(classes, lab, h, w, y, x, y - 1, x - 1);   // on a tile's top row the first branch did it
    pt_join(classes, lab, h, w, y, x, y + 1, x - 1);
  }
}

__global__ __launch_bounds__(256) void patch_flatten_kernel(int32_t* lab, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || PT_LOAD(&lab[i]) == 0) return;
  const int root = pt_find(lab, (int)i);
  __hip_atomic_store(&lab[i], root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// area_plane[root] += pixels of that root.  A wave owns PT_SPAN * 64 consecutive pixels
__global__ __launch_bounds__(256) void patch_areas_kernel(const int32_t* __restrict__ labels, int64_t n,
                                                          int32_t* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (PT_SPAN * 64);
  int carry_label = 0, carry_n = 0;                       // wave-uniform: the run left open by the previous chunk
  for (int k = 0; k < PT_SPAN; ++k) {
    const int64_t i = base + k * 64 + lane;
    if (i - lane >= n) break;
    const int label = pt_label_at(labels, i, n);
    bool head;
    int len;
    uint64_t heads;
    pt_runs(label, false, lane, head, len, heads);
    const int first = __shfl(label, 0, 64), last_head = 63 - __clzll((long long)heads);
    if (lane == 0) {
      if (carry_label == first) len += carry_n;
      else if (carry_label) atomicAdd(&area[carry_label - 1], carry_n);
    }
    if (head && lane != last_head && label) atomicAdd(&area[label - 1], len);
    carry_label = __shfl(label, last_head, 64);
    carry_n = __shfl(len, last_head, 64);
  }
  if (lane == 0 && carry_label) atomicAdd(&area[carry_label - 1], carry_n);
}

__global__ __launch_bounds__(256) void patch_sieve_kernel(uint8_t* __restrict__ classes, int32_t* __restrict__ labels,
                                                          int32_t* area, int64_t n, int min_pixels) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int label = pt_label_at(labels, i, n);
    if (label == 0) continue;
    // a small root zeroes its own entry while its pixels still read it: 0 is below min_pixels (>= 2) as well
    if (PT_LOAD(&area[label - 1]) >= min_pixels) continue;
    classes[i] = 0;
    labels[i] = 0;
    if (label == i + 1) __hip_atomic_store(&area[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- the table
struct pt_box {
  int y0, x0, y1, x1;
  long long sy, sx;
};
__device__ __forceinline__ pt_box pt_box_merge(const pt_box& a, const pt_box& b) {
  return {min(a.y0, b.y0), min(a.x0, b.x0), max(a.y1, b.y1), max(a.x1, b.x1), a.sy + b.sy, a.sx + b.sx};
}
__device__ __forceinline__ pt_box pt_box_from(const pt_box& v, int src) {
  return {__shfl(v.y0, src, 64), __shfl(v.x0, src, 64), __shfl(v.y1, src, 64), __shfl(v.x1, src, 64),
          __shfl(v.sy, src, 64), __shfl(v.sx, src, 64)};
}
__device__ __forceinline__ void pt_box_flush(const pt_box& v, int row, int rows, int32_t* __restrict__ bbox,
                                             unsigned long long* __restrict__ sum_y,
                                             unsigned long long* __restrict__ sum_x) {
  if ((unsigned)row >= (unsigned)rows) return;               // a root the dense plane does not know: no row to write
  atomicMin(&bbox[4 * (int64_t)row + 0], v.y0);
  atomicMin(&bbox[4 * (int64_t)row + 1], v.x0);
  atomicMax(&bbox[4 * (int64_t)row + 2], v.y1);
  atomicMax(&bbox[4 * (int64_t)row + 3], v.x1);
  atomicAdd(&sum_y[row], (unsigned long long)v.sy);
  atomicAdd(&sum_x[row], (unsigned long long)v.sx);
}

__global__ __launch_bounds__(256) void patch_table_init_kernel(int n, int32_t* __restrict__ bbox, int64_t* __restrict__ sum_y,
                                                               int64_t* __restrict__ sum_x) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bbox[4 * (int64_t)r + 0] = INT_MAX;
  bbox[4 * (int64_t)r + 1] = INT_MAX;
  bbox[4 * (int64_t)r + 2] = -1;
  bbox[4 * (int64_t)r + 3] = -1;
  sum_y[r] = 0;
  sum_x[r] = 0;
}

// a run never crosses a row start here, so the head lane knows its run in closed form: row y, columns x .. x + len - 1
__global__ __launch_bounds__(256) void patch_measure_kernel(const int32_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ classes, int64_t n, int w,
                                                            const int32_t* __restrict__ dense, int rows,
                                                            uint8_t* __restrict__ cls,
                                                            int32_t* __restrict__ bbox, unsigned long long* __restrict__ sum_y,
                                                            unsigned long long* __restrict__ sum_x) {
  const int lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (PT_SPAN * 64);
  int carry_label = 0;
  pt_box carry = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < PT_SPAN; ++k) {
    const int64_t i = base + k * 64 + lane;
    if (i - lane >= n) break;
    const int label = pt_label_at(labels, i, n);
    const int y = i < n ? (int)((uint32_t)i / (uint32_t)w) : 0, x = i < n ? (int)((uint32_t)i % (uint32_t)w) : 0;
    if (label == i + 1 && (unsigned)dense[i] < (unsigned)rows) cls[dense[i]] = classes[i];   // the root pixel names the class
    bool head;
    int len;
    uint64_t heads;
    pt_runs(label, x == 0, lane, head, len, heads);
    pt_box box = {y, x, y, x + len - 1, (long long)len * y, (long long)len * x + (long long)len * (len - 1) / 2};
    const int first = __shfl(label, 0, 64), last_head = 63 - __clzll((long long)heads);
    if (lane == 0) {
      if (carry_label == first) box = pt_box_merge(box, carry);
      else if (carry_label) pt_box_flush(carry, dense[carry_label - 1], rows, bbox, sum_y, sum_x);
    }
    if (head && lane != last_head && label) pt_box_flush(box, dense[label - 1], rows, bbox, sum_y, sum_x);
    carry_label = __shfl(label, last_head, 64);
    carry = pt_box_from(box, last_head);
  }
  if (lane == 0 && carry_label) pt_box_flush(carry, dense[carry_label - 1], rows, bbox, sum_y, sum_x);
}

// ---------------------------------------------------------------- entry points
static int pt_check_size(const char* tag, int h, int w) {
  DT_REQUIRE(h >= 1 && w >= 1, "%s: h and w must be >= 1 (h=%d, w=%d)", tag, h, w);
  DT_REQUIRE((int64_t)h * w <= PT_MAX_PIXELS, "%s: %lld pixels do not fit int32 labels (h * w <= 2^31 - 2)", tag,
             (long long)h * w);
  return DT_OK;
}
static inline unsigned pt_wave_grid(int64_t n) { return (unsigned)((n + 4 * PT_SPAN * 64 - 1) / (4 * PT_SPAN * 64)); }

extern "C" int dt_patch_tile(int* th, int* tw) {
  DT_REQUIRE(th && tw, "patch_tile: null pointer");
  *th = PT_TH;
  *tw = PT_TW;
  return DT_OK;
}

extern "C" int dt_label_patches_u8(const uint8_t* classes, int h, int w, int K, int connectivity, int32_t* labels,
                                   int32_t* err_flag, void* stream) {
  DT_REQUIRE(classes && labels && err_flag, "label_patches_u8: null pointer");
  DT_TRY(pt_check_size("label_patches_u8", h, w));
  DT_REQUIRE(K >= 2 && K <= PT_MAXK, "label_patches_u8: K=%d unsupported (2..%d)", K, PT_MAXK);
  DT_REQUIRE(connectivity == 4 || connectivity == 8, "label_patches_u8: connectivity must be 4 or 8, got %d", connectivity);
  hipStream_t st = (hipStream_t)stream;
  const int nty = dt_cdiv(h, PT_TH), ntx = dt_cdiv(w, PT_TW), conn8 = connectivity == 8;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(patch_local_kernel, dim3((unsigned)((int64_t)nty * ntx)), dim3(256), 0, st, classes, h, w, ntx, K,
                     conn8, labels, err_flag);
  const int64_t items = (int64_t)(nty - 1) * w + (int64_t)(ntx - 1) * h;
  if (items > 0) {
    hipLaunchKernelGGL(patch_merge_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, classes, h, w, nty - 1,
                       ntx - 1, conn8, labels);
    hipLaunchKernelGGL(patch_flatten_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, labels, n);
  }
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_patch_areas(const int32_t* labels, int h, int w, int32_t* area_plane, void* stream) {
  DT_REQUIRE(labels && area_plane, "patch_areas: null pointer");
  DT_TRY(pt_check_size("patch_areas", h, w));
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(patch_areas_kernel, dim3(pt_wave_grid(n)), dim3(256), 0, (hipStream_t)stream, labels, n, area_plane);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_sieve_patches_u8(uint8_t* classes, int32_t* labels, int32_t* area_plane, int h, int w, int min_pixels,
                                   void* stream) {
  DT_REQUIRE(classes && labels && area_plane, "sieve_patches_u8: null pointer");
  DT_TRY(pt_check_size("sieve_patches_u8", h, w));
  DT_REQUIRE(min_pixels >= 0, "sieve_patches_u8: min_pixels must be >= 0, got %d", min_pixels);
  if (min_pixels <= 1) return DT_OK;       // every patch has at least one pixel
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(patch_sieve_kernel, dim3(dt_ew_grid(n, 4096)), dim3(256), 0, (hipStream_t)stream, classes, labels,
                     area_plane, n, min_pixels);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_patch_measure(const int32_t* labels, const uint8_t* classes, int h, int w, const int32_t* dense_plane,
                                int n, uint8_t* cls, int32_t* bbox, int64_t* sum_y, int64_t* sum_x, void* stream) {
  DT_REQUIRE(labels && classes && dense_plane, "patch_measure: null pointer");
  DT_TRY(pt_check_size("patch_measure", h, w));
  DT_REQUIRE(n >= 0 && n <= (int64_t)h * w, "patch_measure: n=%d rows for %lld pixels", n, (long long)h * w);
  if (n == 0) return DT_OK;
  DT_REQUIRE(cls && bbox && sum_y && sum_x, "patch_measure: null table");
  const int64_t pixels = (int64_t)h * w;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(patch_table_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, bbox, sum_y, sum_x);
  hipLaunchKernelGGL(patch_measure_kernel, dim3(pt_wave_grid(pixels)), dim3(256), 0, st, labels, classes, pixels, w,
                     dense_plane, n, cls, bbox, (unsigned long long*)sum_y, (unsigned long long*)sum_x);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
