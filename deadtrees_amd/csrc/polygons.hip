// Masks and zones from polygons: exact all-touched rasterisation (the array arithmetic of the reference's
// scripts/createmasks.py: rio.clip(all_touched=True) per class, argmax over the classes; deadtrees_amd/data/polygons.py states
// the contract in numpy).  Vertices are snapped on the host to 1/256 pixel (|q| <= 2^23, raster sides <= 16384), so every
// coordinate difference fits int32 and every cross product is one 32 x 32 -> 64 multiply-add: integers only, no floating
// point.  A polygon (even-odd over all its rings) burns pixel (i, j) iff
//   centre  the centre c = (256 j + 128, 256 i + 128) is inside: an edge taken upwards (ay < by) crosses the centre line iff
//           ay <= cy < by, and the crossing lies on the ray to +x iff cross(b - a, c - a) > 0;
//   touch   (all_touched) an edge meets the pixel's OPEN square: its bounding box strictly overlaps the square in x and y and
//           the cross products of the four corners against the edge satisfy min < 0 < max;
// and a pixel gets the MINIMUM value (1..255) among the polygons that burn it, 0 if none does.
//
// Tables (PolygonSet.tables()): edges int32 [E][4] = (ax, ay, bx, by), every ring closed, taken upwards (ay < by, or ay == by
// and ax < bx), zero-length segments left out; polys int32 [P][8] = (minx, miny, maxx, maxy, e0, e1, value, 0).
//
// One launch, one 256-thread workgroup per 32 x 64 pixel tile (the patches.hip tile); a lane owns 8 pixels side by side in one
// row, so the centre line, the row slab and the two corner rows are the lane's own and an edge costs it one row test, and, when
// that passes, nine cross products (one multiply-add and eight additions of the column step) per corner row.
//   A  the workgroup walks the polygon table 256 rows at a time and keeps those whose bounding box strictly overlaps the tile's
//      open extent, by ordered ballot compaction into an LDS list;
//   B  per kept polygon its edges stream through LDS 256 at a time, compacted likewise to those whose y range meets the tile's
//      rows and that do not lie wholly left of it (such an edge is on the far side of every ray and touches nothing); every
//      lane reads the kept edges as LDS broadcasts and accumulates 8 parity bits (XOR) and 8 touch bits (OR); after the
//      polygon the burnt pixels take min(value).
// Both lists are chunks of a stream, not capacities: any number of polygons per tile and of edges per polygon.  XOR, OR and min
// are order-free and there is no atomic: the map is a pure function of the tables.  Every pixel of the raster is written (zeros
// included), by byte stores inside h x w only: `out` may start at any byte, e.g. inside a larger staged buffer.
//
// Magnitudes: |coordinate| <= 2^23 and corners <= 2^22 give differences < 2^25 and cross products < 2^51.
#include "conv_host.h"

#define PG_THREADS 256
#define PG_TH 32                      // tile rows
#define PG_TW 64                      // tile columns
#define PG_PX 8                       // pixels per lane, side by side
#define PG_SUB 256                    // fixed-point units per pixel
#define PG_MAX_SIDE 16384

typedef int pg_i32x4 __attribute__((ext_vector_type(4)));

// ordered compaction of one flag per thread: the thread's position among the kept ones and their total.  Two barriers;
// `wcnt` is rewritten by the next call only after its own first barrier, which every wave reaches after reading it here.
__device__ __forceinline__ int pg_compact(bool keep, int* __restrict__ wcnt, int& total) {
  const unsigned long long b = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
  total = c0 + c1 + c2 + c3;
  const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(PG_THREADS) void rasterize_polygons_kernel(const pg_i32x4* __restrict__ edges, int64_t n_edges,
                                                                        const pg_i32x4* __restrict__ polys, int n_polys,
                                                                        int h, int w, int tiles_x, int all_touched,
                                                                        uint8_t* __restrict__ out) {
  __shared__ pg_i32x4 s_edge[PG_THREADS];
  __shared__ int s_e0[PG_THREADS], s_e1[PG_THREADS], s_val[PG_THREADS];
  __shared__ int s_wcnt[PG_THREADS / 64];

  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x % (unsigned)tiles_x);
  const int row = ty * PG_TH + (tid >> 3), col0 = tx * PG_TW + (tid & 7) * PG_PX;
  // the tile's open extent and the lane's row, in fixed point
  const int TX0 = tx * PG_TW * PG_SUB, TX1 = TX0 + PG_TW * PG_SUB, TY0 = ty * PG_TH * PG_SUB, TY1 = TY0 + PG_TH * PG_SUB;
  const int Y0 = row * PG_SUB, Y1 = Y0 + PG_SUB, cy = Y0 + PG_SUB / 2;
  const int X0 = col0 * PG_SUB, XE = X0 + PG_PX * PG_SUB, cx0 = X0 + PG_SUB / 2;

  uint32_t val[PG_PX];
#pragma unroll
  for (int k = 0; k < PG_PX; ++k) val[k] = 0u;

  for (int pbase = 0; pbase < n_polys; pbase += PG_THREADS) {
    // ---- A: the polygons of this chunk whose bounding box strictly overlaps the tile
    const int p = pbase + tid;
    bool keep = false;
    int e0 = 0, e1 = 0, value = 0;
    if (p < n_polys) {
      const pg_i32x4 box = polys[2 * (int64_t)p], info = polys[2 * (int64_t)p + 1];
      keep = box[0] < TX1 && box[2] > TX0 && box[1] < TY1 && box[3] > TY0;
      const int64_t lo = info[0] < 0 ? 0 : info[0], hi = info[1] < n_edges ? info[1] : n_edges;   // never past the edge table
      e0 = (int)lo;
      e1 = (int)(hi > lo ? hi : lo);
      value = info[2] & 0xff;
      keep = keep && e1 > e0 && value != 0;
    }
    int n_kept;
    const int at = pg_compact(keep, s_wcnt, n_kept);
    if (keep) {
      s_e0[at] = e0;
      s_e1[at] = e1;
      s_val[at] = value;
    }
    __syncthreads();

    // ---- B: one kept polygon after the other
    for (int q = 0; q < n_kept; ++q) {
      const int pe0 = s_e0[q], pe1 = s_e1[q];
      const uint32_t pval = (uint32_t)s_val[q];
      uint32_t par = 0u, tch = 0u;
      for (int ebase = pe0; ebase < pe1; ebase += PG_THREADS) {
        const int e = ebase + tid;
        bool ekeep = false;
        pg_i32x4 ed = {0, 0, 0, 0};
        if (e < pe1) {
          ed = edges[e];
          const int mx = ed[0] > ed[2] ? ed[0] : ed[2];
          ekeep = ed[1] < TY1 && ed[3] > TY0 && mx > TX0;          // ay <= by: rows met, and not wholly left of the tile
        }
        int n_e;
        const int eat = pg_compact(ekeep, s_wcnt, n_e);           // (its first barrier also ends the last chunk's reads)
        if (ekeep) s_edge[eat] = ed;
        __syncthreads();

        for (int i = 0; i < n_e; ++i) {
          const pg_i32x4 g = s_edge[i];
          const int ax = g[0], ay = g[1], bx = g[2], by = g[3];
          const bool crosses = ay <= cy && cy < by;
          const bool slab = all_touched && ay < Y1 && by > Y0;
          if (!(crosses || slab)) continue;
          const int64_t ux = bx - ax, uy = by - ay;
          const int64_t step = uy * PG_SUB;                        // one column to the right lowers a cross product by this
          if (crosses) {
            int64_t d = ux * (int64_t)(cy - ay) - uy * (int64_t)(cx0 - ax);
#pragma unroll
            for (int k = 0; k < PG_PX; ++k) {
              par ^= (d > 0 ? 1u : 0u) << k;
              d -= step;
            }
          }
          if (slab) {
            const int mn = ax < bx ? ax : bx, mx = ax < bx ? bx : ax;
            if (mn < XE && mx > X0) {
              int64_t c = ux * (int64_t)(Y0 - ay) - uy * (int64_t)(X0 - ax);    // corner (X0, Y0); (., Y1) is c + down
              const int64_t down = ux * PG_SUB;
              uint32_t neg = 0u, pos = 0u;                          // bit k: some corner at x = X0 + 256 k is < 0 / > 0
#pragma unroll
              for (int k = 0; k <= PG_PX; ++k) {
                const int64_t c2 = c + down;
                neg |= ((c < 0 || c2 < 0) ? 1u : 0u) << k;
                pos |= ((c > 0 || c2 > 0) ? 1u : 0u) << k;
                c -= step;
              }
              uint32_t xov = 0u;                                    // bit k: the bounding box strictly overlaps column k in x
#pragma unroll
              for (int k = 0; k < PG_PX; ++k) xov |= ((mn < X0 + (k + 1) * PG_SUB && mx > X0 + k * PG_SUB) ? 1u : 0u) << k;
              tch |= (neg | (neg >> 1)) & (pos | (pos >> 1)) & xov;
            }
          }
        }
      }
      const uint32_t burn = (par | tch) & 0xffu;
#pragma unroll
      for (int k = 0; k < PG_PX; ++k)
        if (((burn >> k) & 1u) && (val[k] == 0u || pval < val[k])) val[k] = pval;
    }
  }

  if (row < h) {
    uint8_t* __restrict__ dst = out + (int64_t)row * w + col0;
#pragma unroll
    for (int k = 0; k < PG_PX; ++k)
      if (col0 + k < w) dst[k] = (uint8_t)val[k];
  }
}

extern "C" int dt_rasterize_polygons_u8(const int32_t* edges, int64_t n_edges, const int32_t* polys, int n_polys, int h, int w,
                                        int all_touched, uint8_t* out, void* stream) {
  DT_REQUIRE(out != nullptr, "rasterize_polygons_u8: null out");
  DT_REQUIRE(h >= 1 && h <= PG_MAX_SIDE && w >= 1 && w <= PG_MAX_SIDE,
             "rasterize_polygons_u8: raster %dx%d must be 1..%d in height and width", h, w, PG_MAX_SIDE);
  DT_REQUIRE(n_polys >= 0 && n_edges >= 0 && n_edges <= 0x7fff0000LL, "rasterize_polygons_u8: bad table sizes (%d polygons, "
             "%lld edges)", n_polys, (long long)n_edges);
  DT_REQUIRE(n_polys == 0 || polys != nullptr, "rasterize_polygons_u8: null polygon table");
  DT_REQUIRE(n_edges == 0 || edges != nullptr, "rasterize_polygons_u8: null edge table");
  DT_REQUIRE(dt_aligned16(edges, polys), "rasterize_polygons_u8: the tables must be 16-byte aligned");
  const int tiles_x = dt_cdiv(w, PG_TW), tiles_y = dt_cdiv(h, PG_TH);
  hipLaunchKernelGGL(rasterize_polygons_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(PG_THREADS), 0, (hipStream_t)stream,
                     (const pg_i32x4*)edges, n_edges, (const pg_i32x4*)polys, n_polys, h, w, tiles_x, all_touched ? 1 : 0, out);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
