"""The inventory of the capped launches: every kernel of ``deadtrees_amd/csrc`` that is launched on a grid with an upper bound
(``dt_ew_grid(n_items, cap)``, ``dt_slice_grid(n_items)`` of csrc/conv_host.h, or a hand-written ``if (g > N) g = N;``)
and walks the rest with a grid-stride loop, with the shapes of the GPU tests that run it past that bound.

``ROWS`` is compared with the sources by tests/test_grid_caps.py (host only: a new capped launch, or a cap that changes, fails
there until a row names a case for it); the shape lists below are what tests/test_above_cap_gpu.py parametrises over, so the
arithmetic test of test_grid_caps.py checks the sizes that really run.

Sizes: every kernel runs at ``cap * 256 + r`` items (some threads take two turns of the loop, some one) and at
``2 * cap * 256 + r'`` (a third turn: a stride that is applied once only shows here), r and r' no multiples of 256, of the
channel count or of the row width.  Maps are large by pixel count and narrow by channel count."""
from collections import namedtuple

WG = 256                          # threads per workgroup = items per workgroup of a grid-stride launch
EW_CAP = 256 * 16                 # csrc/conv_host.h
EW_CAP_WIDE = 256 * 32
ST_CAP = 256 * 16                 # csrc/stitch.hip
RS_CAP = 512                      # csrc/raster_stats.hip
ROW_BLOCK_PIXELS = 2048 * 256     # bnb_rb(n_pix) of conv_host.h grows the row block of dt_bn_bwd_reduce(_bf16) above this

ABOVE = "tests/test_above_cap_gpu.py::"

# ------------------------------------------------------------------------------------------------ shapes of the GPU cases
# (C, n_pix): dt_bn_act, items n_pix * C / 4.  C = 64: a thread keeps one channel quad (the grid stride is a multiple of
# C / 4 = 16); C = 48: C / 4 = 12 divides neither a capped stride (4096 * 256) nor the one of the small case (47 * 256)
BN_ACT_BELOW = [(64, 1000), (48, 1000)]
BN_ACT = [(64, 65_573), (64, 131_147), (48, 87_401), (48, 174_797)]
# (C, n_pix): dt_bn_bwd_reduce + dt_bn_bwd_apply(_frozen) and their bf16 twins: 524,288 + 257 and 1,310,723 pixels are past the
# row-block threshold; the apply pass (items n_pix * C / 4 resp. / 8) is past its cap once at 1,310,723 x 4 (8), twice at
# 2,097,667 x 4 (8) and eight (four) times at 524,545 x 64
BN_BWD = [(4, 524_545), (4, 1_310_723), (4, 2_097_667), (64, 524_545)]
BN_BWD_BF16 = [(8, 524_545), (8, 1_310_723), (8, 2_097_667), (64, 524_545)]
# (C, H, W) of the pooled INPUT, B = 1: items Ho * Wo * C / 4 (forward, the 2 x 2 backward of even maps, the fused
# BatchNorm sums) or H * W * C / 4 (the per-pixel backward of odd maps); bf16: C / 8.  One item is 16 bytes of output
# and 64 bytes of input, so the third turn needs a 134 MB input
MAXPOOL = [(4, 2050, 2052), (4, 2051, 2049), (8, 2050, 2052), (64, 514, 516)]
MAXPOOL_BF16 = [(8, 2050, 2052), (8, 2051, 2049), (16, 2050, 2052)]
MAXPOOL_BN = [(4, 2050, 2052), (8, 2050, 2052)]
MAXPOOL_BN_BF16 = [(8, 2050, 2052), (16, 2050, 2052)]
# (C, H, W) of the half-resolution OUTPUT, B = 1: items H * W * C / 4 (bf16: / 8)
UPSAMPLE = [(4, 1025, 1026), (8, 1025, 1026), (64, 257, 258)]
UPSAMPLE_BF16 = [(8, 1025, 1026), (16, 1025, 1026)]
# (B, C, H, W): items B * H * W pixels
LAYOUT = [(1, 3, 1100, 1000), (2, 3, 1100, 1000)]
NORMALIZE = [1_100_003, 2_200_007]                     # pixels, 4 source and 3 destination channels
BAND = [1_048_576 + 77, 2_097_152 + 333]               # bytes
# (C_narrow, C_wide, offset, n_pix): items n_pix * C_narrow / 4 (bf16: / 8) against the wide cap
SLICE = [(8, 12, 4, 1_048_576 + 131), (8, 12, 4, 2_097_152 + 77)]
SLICE_BF16 = [(16, 24, 8, 1_048_576 + 131), (16, 24, 8, 2_097_152 + 77)]
# (H, W) of RGBN tiles: the byte sums are capped at 256 workgroups x 4096 bytes, the gathers at 1024 x 256 pixels per image.
# An odd quarter turn needs a square tile
AUGMENT = [(520, 516), (518, 518), (740, 712), (726, 726)]
# (H, W) of pool tiles: items H * ceil(W / 4) (four pixels per thread) against 1024 workgroups per image; W % 4 == 2 takes
# the scalar stores, W % 4 == 0 the vector stores
POOL = [(1040, 1014), (1030, 1030), (1460, 1440)]
F32_BF16 = [8 * (1_048_576 + 37), 8 * (2_097_152 + 91)]      # elements, items of 8
BN_ACT_BF16 = [(8, 1_048_576 + 37), (8, 2_097_152 + 91), (64, 131_072 + 75), (64, 262_144 + 91)]    # (C, n_pix), items of 8
PACK_DGRAD = [(3, 256, 512), (3, 512, 512)]            # (k, Cin, Cout): items k * k * Cin * Cout weights
STEM_S2D = [(1, 2900, 2900, 3), (2, 2900, 2900, 1)]    # (B, H, W, Cin): items B * H / 2 * W / 2 against 8192 workgroups
# (B, H, W, Cin, Cout, k, stride, pad): the final reduction of the weight gradient, items k * k * Cin * Cout against 2048
WGRAD = [(1, 4, 4, 128, 512, 3, 1, 1), (1, 4, 4, 256, 512, 3, 2, 1), (1, 4, 4, 512, 512, 3, 1, 1)]
# floats: items of 4 and a scalar tail of 3; 100 quads past one cap (a ragged last workgroup), three whole workgroups past two
ADAM = [4_194_304 + 4 * 100 + 3, 2 * 4_194_304 + 4 * 256 * 3 + 3]
ADAM_RANGES = (2 * 4_194_304 + 4 * 256 * 3 + 3, [(0, 2_700_004), (4_000_000, 2 * 4_194_304 + 4 * 256 * 3 + 3)])
VOTE = [4 * (1_048_576 + 37), 4 * (2_097_152 + 91)]                   # pixels, items of 4
STITCH = [(1100, 1000, 256, 32, 2), (1100, 1000, 256, 32, 3), (1500, 1400, 256, 32, 2)]      # (h, w, d, overlap, K): items h * w
# (h, w, d, overlap, ny, nx) of the windowed gather: items ny * nx * d * d window pixels; d = 250 keeps them off multiples of 256
GATHER = [(1100, 1000, 250, 30, 5, 5), (1500, 1400, 250, 30, 7, 7)]
ZONAL = [16 * (131_072 + 37) + 5, 16 * (262_144 + 91) + 11]           # bytes: items of 16 after the aligned head
SIEVE = [(1100, 1000), (1500, 1400)]                                  # (h, w): items h * w


def _pool_out(n):
    return (n - 1) // 2 + 1


def _maxpool_items(cases, per, odd_bwd=False):
    """items of the pooled map; odd_bwd: of the input, for the maps the per-pixel backward takes"""
    if odd_bwd:
        return [H * W * (C // per) for C, H, W in cases if (H | W) & 1]
    return [_pool_out(H) * _pool_out(W) * (C // per) for C, H, W in cases]


def _even(cases):
    return [c for c in cases if not (c[1] | c[2]) & 1]


Row = namedtuple("Row", "file function cap workgroups per_wg item items tests")
Row.__doc__ = """file, function: where the launch is (the extern "C" entry point or the launcher it goes through); cap: the
expression as written in the source; workgroups: its value; per_wg: items one workgroup takes per turn; item: what one item
is; items: the item counts of the named tests' cases, every one past ``workgroups * per_wg``; tests: the GPU tests"""


def _row(file, function, cap, workgroups, item, items, tests, per_wg=WG):
    return Row(file, function, cap, workgroups, per_wg, item, tuple(items), tuple(tests))


ROWS = [
    # ---- elementwise.hip
    _row("elementwise.hip", "dt_channel_slice", "dt_slice_grid(n4)", EW_CAP_WIDE, "4 floats",
         [n * Cn // 4 for Cn, _, _, n in SLICE], [ABOVE + "test_channel_slice"]),
    _row("elementwise.hip", "dt_bn_act", "dt_ew_grid(n4, EW_CAP)", EW_CAP, "4 floats",
         [n * C // 4 for C, n in BN_ACT], [ABOVE + "test_bn_act", ABOVE + "test_bn_backward"]),
    _row("elementwise.hip", "bn_bwd_apply_impl", "dt_ew_grid(n4, EW_CAP)", EW_CAP, "4 floats",
         [n * C // 4 for C, n in BN_BWD[1:]], [ABOVE + "test_bn_backward"]),
    _row("elementwise.hip", "dt_maxpool3x3s2", "dt_ew_grid(total, EW_CAP)", EW_CAP, "4 floats of the pooled map",
         _maxpool_items(MAXPOOL, 4), [ABOVE + "test_maxpool"]),
    _row("elementwise.hip", "dt_maxpool3x3s2_bwd_bn_rows", "dt_ew_grid((int64_t)B * (H / 2) * (W / 2) * (C / 4), EW_CAP)",
         EW_CAP, "a 2 x 2 block of 4 floats; rows = grid", _maxpool_items(MAXPOOL_BN, 4), [ABOVE + "test_maxpool_backward_bn"]),
    _row("elementwise.hip", "dt_maxpool3x3s2_bwd", "dt_ew_grid((int64_t)B * Ho * Wo * (C / 4), EW_CAP)", EW_CAP,
         "a 2 x 2 block of 4 floats (even maps)", _maxpool_items(_even(MAXPOOL), 4), [ABOVE + "test_maxpool"]),
    _row("elementwise.hip", "dt_maxpool3x3s2_bwd", "dt_ew_grid(total, EW_CAP)", EW_CAP, "4 floats of the input (odd maps)",
         _maxpool_items(MAXPOOL, 4, odd_bwd=True), [ABOVE + "test_maxpool"]),
    _row("elementwise.hip", "dt_upsample2x_bwd", "dt_ew_grid(total, EW_CAP)", EW_CAP, "4 floats of the output",
         [H * W * C // 4 for C, H, W in UPSAMPLE], [ABOVE + "test_upsample_backward"]),
    _row("elementwise.hip", "dt_upsample2x_bwd_bn_rows", "dt_ew_grid((int64_t)B * H * W * (C / 4), EW_CAP)", EW_CAP,
         "4 floats of the output; rows = grid", [H * W * C // 4 for C, H, W in UPSAMPLE], [ABOVE + "test_upsample_backward"]),
    _row("elementwise.hip", "dt_nchw_to_nhwc", "dt_ew_grid(B * HW, EW_CAP)", EW_CAP, "one pixel",
         [B * H * W for B, _, H, W in LAYOUT], [ABOVE + "test_layout_shuttles"]),
    _row("elementwise.hip", "dt_nhwc_to_nchw", "dt_ew_grid(B * HW, EW_CAP)", EW_CAP, "one pixel",
         [B * H * W for B, _, H, W in LAYOUT], [ABOVE + "test_layout_shuttles"]),
    _row("elementwise.hip", "dt_normalize_u8", "dt_ew_grid(n_pix, EW_CAP)", EW_CAP, "one pixel", NORMALIZE,
         [ABOVE + "test_normalize_u8"]),
    _row("elementwise.hip", "dt_band_has_data", "dt_ew_grid(n, EW_CAP)", EW_CAP, "one byte", BAND,
         [ABOVE + "test_band_has_data"]),
    _row("elementwise.hip", "dt_augment_normalize_u8", "if (gx > 256) gx = 256;", 256, "one byte of one image",
         [H * W * 4 for H, W in AUGMENT], [ABOVE + "test_augment"], per_wg=256 * 16),
    _row("elementwise.hip", "dt_augment_normalize_u8", "if (gp > 1024) gp = 1024;", 1024, "one pixel of one image",
         [H * W for H, W in AUGMENT], [ABOVE + "test_augment"]),
    _row("elementwise.hip", "dt_augment_labels", "if (gp > 1024) gp = 1024;", 1024, "one pixel of one image",
         [H * W for H, W in AUGMENT], [ABOVE + "test_augment"]),
    # ---- pool.hip
    _row("pool.hip", "pool_gather_launch", "if (gx > 1024) gx = 1024;", 1024, "four pixels of one image",
         [H * ((W + 3) // 4) for H, W in POOL], [ABOVE + "test_pool_gather"]),
    # ---- elementwise_bf16.hip
    _row("elementwise_bf16.hip", "dt_bn_bwd_apply_bf16", "dt_ew_grid(n8, EW_CAP)", EW_CAP, "8 bf16",
         [n * C // 8 for C, n in BN_BWD_BF16[1:]], [ABOVE + "test_bn_backward_bf16"]),
    _row("elementwise_bf16.hip", "dt_maxpool3x3s2_bf16_amax", "dt_ew_grid(total, EW_CAP)", EW_CAP, "8 bf16 of the pooled map",
         _maxpool_items(MAXPOOL_BF16, 8), [ABOVE + "test_maxpool_bf16"]),
    _row("elementwise_bf16.hip", "dt_maxpool3x3s2_bwd_bn_bf16_rows",
         "dt_ew_grid((int64_t)B * (H / 2) * (W / 2) * (C / 8), EW_CAP)", EW_CAP, "a 2 x 2 block of 8 bf16; rows = grid",
         _maxpool_items(MAXPOOL_BN_BF16, 8), [ABOVE + "test_maxpool_backward_bn"]),
    _row("elementwise_bf16.hip", "dt_maxpool3x3s2_bwd_bf16", "dt_ew_grid((int64_t)B * Ho * Wo * (C / 8), EW_CAP_WIDE)",
         EW_CAP_WIDE, "a 2 x 2 block of 8 bf16 (even maps)", _maxpool_items(_even(MAXPOOL_BF16)[-1:], 8),
         [ABOVE + "test_maxpool_bf16"]),
    _row("elementwise_bf16.hip", "dt_maxpool3x3s2_bwd_bf16", "dt_ew_grid(total, EW_CAP)", EW_CAP,
         "8 bf16 of the input (odd maps)", _maxpool_items(MAXPOOL_BF16, 8, odd_bwd=True), [ABOVE + "test_maxpool_bf16"]),
    _row("elementwise_bf16.hip", "upsample2x_bwd_bf16_launch", "dt_ew_grid(total, EW_CAP)", EW_CAP, "8 bf16 of the output",
         [H * W * C // 8 for C, H, W in UPSAMPLE_BF16], [ABOVE + "test_upsample_backward_bf16"]),
    _row("elementwise_bf16.hip", "dt_channel_slice_bf16", "dt_slice_grid(n8)", EW_CAP_WIDE, "8 bf16",
         [n * Cn // 8 for Cn, _, _, n in SLICE_BF16], [ABOVE + "test_channel_slice_bf16"]),
    _row("elementwise_bf16.hip", "dt_upsample2x_bwd_bn_bf16_rows", "dt_ew_grid((int64_t)B * H * W * (C / 8), EW_CAP)", EW_CAP,
         "8 bf16 of the output; rows = grid", [H * W * C // 8 for C, H, W in UPSAMPLE_BF16],
         [ABOVE + "test_upsample_backward_bf16"]),
    _row("elementwise_bf16.hip", "dt_f32_to_bf16", "dt_ew_grid(n / 8, EW_CAP)", EW_CAP, "8 floats",
         [n // 8 for n in F32_BF16], [ABOVE + "test_precision_converters"]),
    # ---- conv_bf16.hip  (dt_pack_weights_bf16 launches a three-dimensional grid of 32 x 32 tiles: no cap)
    _row("conv_bf16.hip", "dt_pack_dgrad_weights_bf16", "dt_ew_grid(per_tap * ksize * ksize, 4096)", 4096, "one weight",
         [k * k * ci * co for k, ci, co in PACK_DGRAD], [ABOVE + "test_pack_dgrad_weights_bf16"]),
    _row("conv_bf16.hip", "dt_stem_s2d_bf16", "dt_ew_grid((int64_t)B * (H / 2) * (W / 2), 8192)", 8192,
         "one pixel of the half-resolution image (16 bf16)", [B * (H // 2) * (W // 2) for B, H, W, _ in STEM_S2D],
         [ABOVE + "test_stem_space_to_depth_bf16"]),
    _row("conv_bf16.hip", "dt_bn_act_bf16", "dt_ew_grid(n8, 4096)", 4096, "8 bf16", [n * C // 8 for C, n in BN_ACT_BF16],
         [ABOVE + "test_bn_act_bf16"]),
    _row("conv_bf16.hip", "dt_maxpool3x3s2_bf16", "dt_ew_grid(total, 4096)", 4096, "8 bf16 of the pooled map",
         _maxpool_items(MAXPOOL_BF16, 8), [ABOVE + "test_maxpool_bf16"]),
    _row("conv_bf16.hip", "dt_bf16_to_f32", "dt_ew_grid(n / 8, 4096)", 4096, "8 bf16", [n // 8 for n in F32_BF16],
         [ABOVE + "test_precision_converters"]),
    # ---- conv_wgrad.hip  (dt_conv2d_wgrad and dt_conv2d_wgrad_stem_dy_bf16 share wgrad_impl; a stem has 9,408 .. 12,544
    # weights, so only the wide layers of dt_conv2d_wgrad reach the cap)
    _row("conv_wgrad.hip", "wgrad_impl", "dt_ew_grid(E, 256 * 8)", 256 * 8, "one weight",
         [k * k * ci * co for _, _, _, ci, co, k, _, _ in WGRAD], [ABOVE + "test_weight_gradient_tail"]),
    # ---- optim.hip
    _row("optim.hip", "dt_adam_step", "dt_ew_grid(n >> 2, 256 * 16)", 256 * 16, "4 floats", [n >> 2 for n in ADAM],
         [ABOVE + "test_flat_adam"]),
    _row("optim.hip", "dt_adam_step_dev", "dt_ew_grid(n >> 2, 256 * 16)", 256 * 16, "4 floats", [n >> 2 for n in ADAM],
         [ABOVE + "test_flat_adam"]),
    _row("optim.hip", "dt_adam_step_ranges", "if (grid > 256 * 16 / nranges) grid = 256 * 16 / nranges;",
         256 * 16 // len(ADAM_RANGES[1]), "4 floats of one range", [(hi - lo) >> 2 for lo, hi in ADAM_RANGES[1]],
         [ABOVE + "test_flat_adam_trainable_ranges"]),
    _row("optim.hip", "dt_weight_average", "dt_ew_grid(n >> 2, 256 * 16)", 256 * 16, "4 floats", [n >> 2 for n in ADAM],
         [ABOVE + "test_weight_average"]),
    # ---- head_loss.hip
    _row("head_loss.hip", "dt_seg_loss_bwd", "dt_ew_grid(total, 256 * 16)", 256 * 16, "one pixel", [5 * 512 * 512],
         ["tests/test_loss_kernels_gpu.py::test_values_and_gradients_at_the_training_tile_size"]),      # the B = 5 case
    _row("head_loss.hip", "dt_confusion_matrix", "if (g > 2048) g = 2048;", 2048, "one pixel", [2048 * 4096 + 4097],
         ["tests/test_loss_kernels_gpu.py::test_confusion_matrix_sizes_and_classes"], per_wg=256 * 16),
    _row("head_loss.hip", "dt_ensemble_vote", "dt_ew_grid(n4, 4096)", 4096, "4 pixels", [n // 4 for n in VOTE],
         [ABOVE + "test_ensemble_vote"]),
    # ---- stitch.hip  (dt_split_normalize_u8 of elementwise.hip goes through dt_window_normalize_u8)
    _row("stitch.hip", "dt_window_normalize_u8", "dt_ew_grid(n_pix, ST_CAP)", ST_CAP, "one pixel of one window",
         [ny * nx * d * d for _, _, d, _, ny, nx in GATHER], [ABOVE + "test_window_gather"]),
    _row("stitch.hip", "dt_stitch_accumulate", "dt_ew_grid(n_pix, ST_CAP)", ST_CAP, "one raster pixel",
         [h * w for h, w, _, _, _ in STITCH], [ABOVE + "test_stitch_accumulate_and_finalize"]),
    _row("stitch.hip", "dt_stitch_finalize", "dt_ew_grid(n_pix, ST_CAP)", ST_CAP, "one raster pixel",
         [h * w for h, w, _, _, _ in STITCH], [ABOVE + "test_stitch_accumulate_and_finalize"]),
    _row("stitch.hip", "dt_stitch_classes_u8", "dt_ew_grid(n_pix, ST_CAP)", ST_CAP, "one raster pixel",
         [h * w for h, w, _, _, _ in STITCH[1:]], [ABOVE + "test_stitch_classes"]),
    # ---- raster_stats.hip, patches.hip
    _row("raster_stats.hip", "dt_zonal_counts_u8", "dt_ew_grid(nvec, RS_CAP)", RS_CAP, "16 pixels", [n // 16 for n in ZONAL],
         [ABOVE + "test_zonal_counts"]),
    _row("patches.hip", "dt_sieve_patches_u8", "dt_ew_grid(n, 4096)", 4096, "one pixel", [h * w for h, w in SIEVE],
         [ABOVE + "test_sieve"]),
]

# the row-block regime of the two-pass BatchNorm backward: not a grid cap, a threshold of the same kind.  (entry point, rows
# query, pixel counts of the cases, tests)
ROW_BLOCK_ROWS = [
    ("dt_bn_bwd_reduce", "dt_bn_bwd_rows", sorted({n for _, n in BN_BWD}), (ABOVE + "test_bn_backward",)),
    ("dt_bn_bwd_reduce_bf16", "dt_bn_bwd_rows_bf16", sorted({n for _, n in BN_BWD_BF16}), (ABOVE + "test_bn_backward_bf16",)),
]
