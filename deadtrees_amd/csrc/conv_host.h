// Host-side plumbing shared by the kernel files: descriptor checks, environment switches, grid sizing, the launcher
// of the persistent kernels, alignment checks.
// Nothing here reaches device code.
#pragma once
#include <stdlib.h>

#include "common.h"

// return the first failure of a chain of checks
#define DT_TRY(expr)                  \
  do {                                \
    const int rc__ = (expr);          \
    if (rc__ != DT_OK) return rc__;   \
  } while (0)

// ---- convolution descriptors.  Every family (fp32 direct `conv`, `conv_bf16`, `wgrad`, `wgrad_bf16`) starts with
// dt_conv_validate_null and then runs the shared rules it has, in its own order (the first message reported is part of
// the ABI's behaviour), followed by its own rules.  `tag` prefixes the message.
static inline int dt_conv_validate_null(const dt_conv_desc* d, const char* tag) {
  DT_REQUIRE(d != nullptr, "%s: null descriptor", tag);
  return DT_OK;
}
static inline int dt_conv_validate_sizes(const dt_conv_desc* d, const char* tag) {
  DT_REQUIRE(d->B > 0 && d->Hin > 0 && d->Win > 0 && d->C0 > 0 && d->C1 >= 0 && d->Cout > 0, "%s: bad sizes", tag);
  return DT_OK;
}
// mode0 1 (nearest x2 up-sampling) and 2 (zero insertion) read a half-resolution source
static inline int dt_conv_validate_even(const dt_conv_desc* d, const char* tag) {
  DT_REQUIRE(d->mode0 == 0 || ((d->Hin & 1) == 0 && (d->Win & 1) == 0), "%s: mode0 needs even Hin/Win", tag);
  return DT_OK;
}
static inline int dt_conv_validate_split(const dt_conv_desc* d, const char* tag) {
  DT_REQUIRE(d->cout_split == 0 || ((d->cout_split % 32) == 0 && d->cout_split < d->Cout),
             "%s: cout_split must be a multiple of 32 below Cout", tag);
  return DT_OK;
}
// the output size the descriptor's input size, padding, window and stride give
static inline void dt_conv_out_size(const dt_conv_desc* d, int* ho, int* wo) {
  *ho = (d->Hin + 2 * d->pad - d->ksize) / d->stride + 1;
  *wo = (d->Win + 2 * d->pad - d->ksize) / d->stride + 1;
}
static inline int dt_conv_validate_out(const dt_conv_desc* d, const char* tag) {
  int ho, wo;
  dt_conv_out_size(d, &ho, &wo);
  DT_REQUIRE(ho == d->Ho && wo == d->Wo, "%s: Ho/Wo mismatch", tag);
  return DT_OK;
}

// ---- NAME=0 in the environment switches a kernel family off (A/B measurements); unset or anything not starting with '0'
// means on.  Read once per process (per call site).
static inline bool dt_env_read_on(const char* name) {
  const char* e = getenv(name);
  return e == nullptr || e[0] != '0';
}
#define dt_env_on(NAME) ([] { static const bool on__ = dt_env_read_on(NAME); return on__; }())

// ---- grid of a grid-stride element-wise launch: one 256-thread workgroup per 256 items, at least 1, at most `cap`
static inline int dt_ew_grid(int64_t n_items, int64_t cap) {
  const int64_t g = (n_items + 255) / 256;
  return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}
// the caps of the element-wise files.  A fused BatchNorm-backward pass writes one partial row per workgroup, so a cap is
// part of its result: a call site keeps the cap it has
#define EW_CAP (256 * 16)        // 16 workgroups per CU, grid-stride beyond
#define EW_CAP_WIDE (256 * 32)   // the 2 x 2 pool blocks of the bf16 path and the channel-slice copies
// grid of the channel-slice copies: n / 256 + 1 workgroups, one more than dt_ew_grid gives for exact multiples of 256
static inline int dt_slice_grid(int64_t n_items) {
  const int64_t g = n_items / 256 + 1;
  return (int)(g < EW_CAP_WIDE ? g : EW_CAP_WIDE);
}

// ---- persistent grids of the narrow-layer kernels (conv_narrow.hip, conv_bf16_narrow.hip): every workgroup slot of the
// device, each workgroup walking tiles blockIdx.x, + grid, ... and writing ONE statistics row / weight-gradient slab.
// DT_CUS is a constant on purpose: dt_persist_rows sizes the buffers before any launch, and the grid decides which row a
// tile's sums land in, so both are part of the result
#define DT_CUS 256
#define DT_PERSIST_MAX_PER_CU 8
// rows / slabs of a layer with `tiles` tiles: an upper bound of every variant's grid, asked before the variant is known
static inline int dt_persist_rows(int tiles) {
  return tiles < DT_PERSIST_MAX_PER_CU * DT_CUS ? tiles : DT_PERSIST_MAX_PER_CU * DT_CUS;
}
// Workgroups of an instantiation that fit one CU, from its own code object: registers (512 per lane and SIMD, granule 8,
// one wave of the workgroup per SIMD) and LDS (160 KiB).  The kernel is latency-bound by the bytes it keeps in flight
// (PMC round 3: waves parked 53 % of the time at 3 workgroups per CU = 33 KB in flight per CU -> 3.6 TB/s), so the
// persistent grid takes every slot there is — and exactly those, so that all workgroups walk the same number of tiles.
static inline int dt_occupancy(const void* kernel) {
  hipFuncAttributes at;
  if (hipFuncGetAttributes(&at, kernel) != hipSuccess) return 2;
  const int regs = ((at.numRegs + 7) / 8) * 8;
  const int by_regs = regs > 0 ? 512 / regs : DT_PERSIST_MAX_PER_CU;
  const int by_lds = at.sharedSizeBytes > 0 ? (int)(163840 / at.sharedSizeBytes) : DT_PERSIST_MAX_PER_CU;
  const int occ = by_regs < by_lds ? by_regs : by_lds;
  return occ > DT_PERSIST_MAX_PER_CU ? DT_PERSIST_MAX_PER_CU : (occ < 1 ? 1 : occ);
}
// asked once per instantiation and process (a function-local static: thread-safe, and the cache belongs to the kernel)
template <auto K>
static int dt_wgs_per_cu() {
  static const int per_cu = dt_occupancy(reinterpret_cast<const void*>(K));
  return per_cu;
}
// launches K(a, total) on min(total, slots) workgroups of 256 threads -> the grid
template <auto K, class Args>
static int dt_persist_launch(const Args& a, int total, hipStream_t st) {
  const int slots = dt_wgs_per_cu<K>() * DT_CUS, grid = total < slots ? total : slots;
  hipLaunchKernelGGL(K, dim3((unsigned)grid), dim3(256), 0, st, a, total);
  return grid;
}

// ---- the narrow layers' channel counts as compile-time block counts: f(CB, NB) with std::integral_constant arguments,
// CB = 1 for up to 16 input channels and 2 above, NB alike for the output channels.  A launcher that has no <2, 2>
// instantiation leaves it out with `if constexpr`
template <class F>
static inline int dt_narrow_blocks(int C0, int Cout, F&& f) {
  using one = std::integral_constant<int, 1>;
  using two = std::integral_constant<int, 2>;
  if (C0 <= 16 && Cout <= 16) return f(one{}, one{});
  if (C0 <= 16) return f(one{}, two{});
  if (Cout <= 16) return f(two{}, one{});
  return f(two{}, two{});
}

// ---- C channels in groups of `per` (4 fp32 or 8 bf16 = 16 bytes): the groups must divide the 256 threads of a workgroup
// wherever a thread keeps ONE group for the whole launch (fixed coefficients, partial rows combined inside the workgroup)
static inline bool dt_groups_divide_256(int C, int per) {
  return C > 0 && C % per == 0 && C / per <= 256 && 256 % (C / per) == 0;
}

// ---- rows (pixels) per workgroup of the BatchNorm-backward reductions of both precisions: 256 for small maps, grown so
// that a launch has at most ~2048 row blocks — the in-workgroup reduction and the second-stage row count then stay small
// next to the streaming part
#define BNB_RB 256
static inline int64_t bnb_rb(int64_t n_pix) {
  int64_t rb = BNB_RB;
  const int64_t want = (n_pix + 2047) / 2048;
  if (want > rb) rb = (want + BNB_RB - 1) / BNB_RB * BNB_RB;
  return rb;
}

// ---- 16-byte alignment of the arrays a kernel reads with 16-byte loads (a null pointer counts as aligned)
template <class... P>
static inline bool dt_aligned16(const P*... p) {
  return ((... | (uintptr_t)p) & 15) == 0;
}
static inline bool dt_fuse_aligned16(const dt_bn_bwd_fuse* f) {
  return dt_aligned16(f->mean, f->invstd, f->act_scale, f->act_shift);
}
// every array a fused BatchNorm-backward reduction with a virtual activation reads is there
static inline bool dt_fuse_complete(const dt_bn_bwd_fuse* f) {
  return f && f->y && f->mean && f->invstd && f->act_scale && f->act_shift;
}
#define DT_REQUIRE_COEF_ALIGNED(ok, tag) DT_REQUIRE(ok, tag ": per-channel arrays must be 16-byte aligned")
