/* deadtrees_hip.h — C ABI of libdeadtrees_hip.so (MI355X / gfx950 only).
 *
 * The reference (cwerner/deadtrees) has NO native code and no FFI: its hot path is
 * `self.model(img)` (deadtrees/network/segmodel.py:214,235,280; deployment/inference.py:60) on
 * smp.Unet(resnet34) plus the loss callables of deadtrees/loss (segmodel.py:169-200), executed
 * by ATen.  Each entry point below replaces one ATen op family that this path launches
 * (SURVEY.md §2.3 K1..K22); the comment on each names the reference call site it serves.
 *
 * Conventions
 *   - plain pointers + sizes; all tensors are DEVICE pointers, fp32 unless stated, NHWC
 *     ("[B,H,W,C]") for activations, HWIO ("[kh][kw][Cin][Cout]") for conv weights;
 *     logits / labels / distance maps at the module boundary are NCHW like the reference.
 *   - inputs are borrowed, outputs are caller-allocated, no ownership transfer, no hidden
 *     allocation, no host synchronisation: every call only enqueues kernels on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream) and is hipGraph-capturable.
 *   - return 0 on success, a negative DT_E* code otherwise; dt_last_error() gives the message
 *     (thread-local).  Shape preconditions are validated on the host BEFORE any launch.
 */
#ifndef DEADTREES_HIP_H
#define DEADTREES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DT_OK 0
#define DT_EINVAL (-22)  /* bad shape / argument            */
#define DT_ENOSYS (-38)  /* configuration not implemented   */
#define DT_EHIP (-5)     /* HIP runtime / launch failure    */

const char* dt_last_error(void);
int dt_version(void);
/* number of HIP devices visible; <0 on error.  Does not create a context. */
int dt_device_count(void);

/* ------------------------------------------------------------------ convolution (K1,K5,K6,K7,K9,K10,K21)
 * One descriptor drives forward, data-gradient and weight-gradient kernels.
 * The LOGICAL input is cat([src0', src1], channel) of size [B,Hin,Win,C0+C1] where src0' is
 *   mode0 = 0 : src0 itself                                   [B,Hin,Win,C0]
 *   mode0 = 1 : nearest x2 upsample of src0                   [B,Hin/2,Win/2,C0]  (F.interpolate, K9)
 *   mode0 = 2 : zero-insertion x2 of src0 (transposed conv)   [B,Hin/2,Win/2,C0]  (stride-2 dgrad)
 * src1 (C1 may be 0) is always direct (the U-Net skip, torch.cat K10).
 * Output [B,Ho,Wo,Cout]; channels [0,cout_split) go to out0 (leading dim cout_split), the rest to
 * out1 (leading dim Cout-cout_split); cout_split = 0 -> everything to out0.
 */
typedef struct dt_conv_desc {
  int32_t B, Hin, Win;
  int32_t C0, C1;
  int32_t mode0;
  int32_t Ho, Wo, Cout;
  int32_t ksize;       /* 1, 3 or 7 (square) */
  int32_t stride;      /* 1 or 2             */
  int32_t pad;
  int32_t cout_split;  /* 0 or a multiple of 32 */
  int32_t accumulate;  /* !=0: out0 += result (gradient accumulation on residual / skip joins) */
} dt_conv_desc;

/* rows P of the BatchNorm partial-statistics buffer dt_conv2d writes: stats is [2][P][Cout]
 * (plane 0 = sum, plane 1 = sum of squares, one row per workgroup tile). */
int dt_conv2d_stat_rows(const dt_conv_desc* d);

/* y = conv(x, w) — replaces ATen conv2d reached from smp encoder/decoder (segmodel.py:214).
 * stats may be NULL.  fp32 MFMA (v_mfma_f32_32x32x2_f32): exact fp32 fma chains. */
int dt_conv2d(const dt_conv_desc* d, const float* src0, const float* src1, const float* w_hwio,
              float* out0, float* out1, float* stats, const float* in_scale, const float* in_shift, void* stream);
/* in_scale/in_shift (both NULL or both [C0]): source 0 is read as relu(src0*in_scale[c]+in_shift[c]) while it is
 * staged into LDS — the BatchNorm-apply + ReLU of the producing layer fused into its consumer, so that activation
 * never exists in HBM (zero padding stays zero).  Same pair on dt_conv2d_wgrad. */

/* tile configuration dt_conv2d selects for d (kernel conv_fwd_kernel<ksize,stride,tw,tn,ck>): used to
 * attribute profiler rows and roofline numbers to launches. */
int dt_conv2d_config(const dt_conv_desc* d, int* tw, int* tn, int* ck);
int dt_conv2d_uses_zi(const dt_conv_desc* d);  /* 1: parity-class tiles of the transposed (stride-2) data gradient */

/* ---- Winograd F(2x2,3x3) form of the 3x3 stride-1 pad-1 layers (same ATen conv2d / convolution_backward(input)
 * calls as dt_conv2d; 2.25x fewer multiplies, results within ~1e-6 relative of the direct form instead of an exact fma
 * chain).  u = dt_winograd_weights(w_hwio): G g G^T in the order [16 positions][Cin/8][2][Cout][4], 16*Cin*Cout floats.
 * Supported when C0, C1 are multiples of 8 and C0 + C1 of 16, Cout and cout_split multiples of 64, mode0 in {0,1}, every
 * operand below 2 GiB (dt_conv2d_winograd_supported; callers fall back to dt_conv2d otherwise).
 * stats rows: dt_conv2d_winograd_stat_rows (16x16-pixel tiles). */
int dt_conv2d_winograd_supported(const dt_conv_desc* d);
int dt_conv2d_winograd_stat_rows(const dt_conv_desc* d);
int dt_winograd_weights(const float* w_hwio, float* u, int Cin, int Cout, void* stream);
int dt_conv2d_winograd(const dt_conv_desc* d, const float* src0, const float* src1, const float* u, float* out0,
                       float* out1, float* stats, const float* in_scale, const float* in_shift, void* stream);
/* inference form (eval-mode BatchNorm): out = relu(conv(src) * scale + shift [+ residual]) — the ATen chain conv2d ->
 * batch_norm(eval) -> (add) -> relu_ of a ResNet / decoder block (reference call site deployment/inference.py:60) in ONE
 * kernel; scale / shift per output channel (dt_bn_eval_affine), residual (optional) in the layout of out.  Same
 * arithmetic as dt_conv2d_winograd followed by dt_bn_act: bit-identical.  No split outputs, joins or statistics. */
int dt_conv2d_winograd_affine(const dt_conv_desc* d, const float* src0, const float* src1, const float* u, float* out,
                              const float* scale, const float* shift, const float* residual, void* stream);
/* The same one-launch inference form for the narrow full-resolution decoder layers (3x3 stride 1 pad 1, Cin and Cout in
 * {16, 32}, maps of at least 8 x 32 pixels; dt_conv2d_narrow_supported tells): out = relu(conv(x) * scale + shift), with
 * x = src0 or — in_scale / in_shift given — relu(src0 * in_scale + in_shift) (the producer's virtual activation). */
int dt_conv2d_narrow_supported(const dt_conv_desc* d);
int dt_conv2d_narrow_affine(const dt_conv_desc* d, const float* src0, const float* w_hwio, float* out, const float* scale,
                            const float* shift, const float* in_scale, const float* in_shift, void* stream);
/* ... and for every other layer dt_conv2d takes (stem 7x7 / 2, stride-2 3x3, 1x1 down-sample, concat layers): out =
 * conv(x) * scale + shift, through ReLU when relu != 0 — bit-identical to dt_conv2d followed by dt_bn_act(relu).  No
 * input transform, split, join or statistics. */
int dt_conv2d_affine(const dt_conv_desc* d, const float* src0, const float* src1, const float* w_hwio, float* out,
                     const float* scale, const float* shift, int relu, void* stream);
/* all eligible layers in one launch: int32 table rows (w_off, u_off, Cin, Cout, first_block), blocks of a layer =
 * ceil(Cout/64) * ceil(Cin/16); `weights` = the flat parameter buffer (forward images) or its dt_weight_images mode-0
 * image with Cin/Cout swapped (data-gradient images). */
int dt_winograd_weight_images(const float* weights, float* u, const int32_t* table, int n_layers, int total_blocks,
                              void* stream);

/* wd[kh'][kw'][co][ci] = w[K-1-kh'][K-1-kw'][ci][co]: weights of the data-gradient convolution. */
int dt_weight_flip_transpose(const float* w_hwio, float* wd, int ksize, int Cin, int Cout, void* stream);

/* dW[kh][kw][ci][co] = sum_{b,oy,ox} x[b,oy*s+kh-p,ox*s+kw-p,ci] * dy[b,oy,ox,co]  (autograd of conv2d, K21).
 * workspace: fp32 scratch of at least dt_conv2d_wgrad_workspace(d) bytes (split-K partials, reduced
 * in a fixed order -> run-to-run deterministic). */
size_t dt_conv2d_wgrad_workspace(const dt_conv_desc* d);
int dt_conv2d_wgrad(const dt_conv_desc* d, const float* src0, const float* src1, const float* dy,
                    float* dw_hwio, float* workspace, size_t workspace_bytes, const float* in_scale,
                    const float* in_shift, void* stream);
/* Winograd F(2x2,3x3) form of dt_conv2d_wgrad for 3x3 stride-1 pad-1 layers whose C0, C1 and Cout are multiples of 64
 * (same arguments; 2.25x fewer multiplies, result within ~1e-6 relative of the direct form; deterministic). */
int dt_conv2d_wgrad_winograd_supported(const dt_conv_desc* d);
size_t dt_conv2d_wgrad_winograd_workspace(const dt_conv_desc* d);
int dt_conv2d_wgrad_winograd(const dt_conv_desc* d, const float* src0, const float* src1, const float* dy,
                             float* dw_hwio, float* workspace, size_t workspace_bytes, const float* in_scale,
                             const float* in_shift, void* stream);

/* ------------------------------------------------------------------ BatchNorm / ReLU / residual (K2,K3,K8,K21) */
/* stats[2][P][C] -> batch mean / biased var over `count` elements; writes mean, invstd, and the fused
 * affine scale = gamma*invstd, shift = beta - mean*scale; updates running stats with `momentum`
 * (unbiased var), as torch BatchNorm2d(train).  fp64 accumulation, fixed order. */
/* The stats buffer (also the one dt_conv2d writes) must hold dt_bn_stats_floats(P,C) floats: the
 * [2][P][C] partial rows plus a scratch tail used by the first reduction stage when P is large. */
int64_t dt_bn_stats_floats(int P, int C);
int dt_bn_finalize(float* stats, int P, int C, double count, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var,
                   float* mean, float* invstd, float* scale, float* shift, void* stream);
/* The same kernel with the momentum read from the device (float[1]) when it runs: a captured graph replays with a
 * momentum that changes every batch (cumulative average, see dt_cma_advance).  Given the same momentum value every
 * output is bit-identical to dt_bn_finalize. */
int dt_bn_finalize_dev(float* stats, int P, int C, double count, const float* gamma, const float* beta,
                       float eps, const float* momentum_dev, float* running_mean, float* running_var,
                       float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale/shift from running stats. */
int dt_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C, float* scale, float* shift, void* stream);
/* eval mode with a backward pass to follow (frozen-BatchNorm fine-tuning, F.batch_norm(training=False) backward):
 * mean = running_mean, invstd = 1/sqrt(running_var + eps) for dt_bn_bwd_reduce / dt_bn_bwd_apply_frozen. */
int dt_bn_eval_stats(const float* running_mean, const float* running_var, float eps, int C, float* mean,
                     float* invstd, void* stream);
/* out = act( y*scale[c]+shift[c] + (res ? res*rscale[c]+rshift[c] : 0) ), act = ReLU if relu == 1;
 * relu == 2: ReLU on the main branch only, out = relu(y*scale+shift) + residual (the ResUnet decoder block,
 * network/extra/resunet/decoder.py:40-52).  rscale/rshift NULL -> identity residual.  n_pix = B*H*W. */
int dt_bn_act(const float* y, const float* scale, const float* shift, const float* res,
              const float* rscale, const float* rshift, float* out, int64_t n_pix, int C, int relu,
              void* stream);
/* BN backward, pass 1: g = dout * (out>0 if out_act else 1); partial sums of g and g*xhat per channel
 * -> red[2][P][C] with P = dt_bn_bwd_rows(n_pix); `red` holds dt_bn_bwd_red_floats(n_pix,C) floats. */
int dt_bn_bwd_rows(int64_t n_pix, int C);
int64_t dt_bn_bwd_red_floats(int64_t n_pix, int C);  /* size of `red` in floats (rows + reduction scratch) */
/* ReLU mask of g: from out_act when given, else recomputed as (y*act_scale+act_shift > 0) when act_scale is
 * given (virtual activation), else none (BatchNorm without ReLU: the downsample branch). */
int dt_bn_bwd_reduce(const float* dout, const float* out_act, const float* y, const float* mean,
                     const float* invstd, const float* act_scale, const float* act_shift, float* red,
                     int64_t n_pix, int C, void* stream);
/* pass 2: reduces red -> dgamma, dbeta (fp64, fixed order) and writes
 * dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat));  if dres != NULL also dres (+)= g. */
int dt_bn_bwd_apply(const float* dout, const float* out_act, const float* y, const float* mean,
                    const float* invstd, const float* gamma, const float* act_scale, const float* act_shift,
                    float* red, int P, float* dgamma, float* dbeta, float* dy, float* dres, int dres_accumulate,
                    int64_t n_pix, int C, void* stream);
/* the same pass for eval-mode (frozen-statistics) BatchNorm: dgamma = sum g*xhat, dbeta = sum g as above, but
 * dy = gamma*invstd*g (mean / invstd do not depend on the batch) — ATen batch_norm_backward with train=False. */
int dt_bn_bwd_apply_frozen(const float* dout, const float* out_act, const float* y, const float* mean,
                           const float* invstd, const float* gamma, const float* act_scale, const float* act_shift,
                           float* red, int P, float* dgamma, float* dbeta, float* dy, float* dres,
                           int dres_accumulate, int64_t n_pix, int C, void* stream);

/* torch.cat of NHWC tensors along the channels and its backward (the dense skip connections of the Unet++ decoder:
 * reference network/extra/efficientunetplusplus/decoder.py:170-177, same wiring as smp UnetPlusPlusDecoder).
 * to_wide = 1: wide[n, offset : offset + C_narrow] = narrow[n, :] (src = narrow, dst = wide);
 * to_wide = 0: narrow[n, :] (+)= wide[n, offset : offset + C_narrow] (src = wide, dst = narrow; += when accumulate). */
int dt_channel_slice(const float* src, float* dst, int64_t n_pix, int C_narrow, int C_wide, int offset, int to_wide,
                     int accumulate, void* stream);

/* per-channel sums of g [n_pix][C] -> out[C]: the bias gradient of a biased convolution (ATen convolution_backward's
 * third output; here the 1x1 identity_conv of the ResUnet decoder).  workspace: dt_channel_sums_workspace floats. */
int64_t dt_channel_sums_workspace(int64_t n_pix, int C);
int dt_channel_sums(const float* g, float* workspace, int64_t n_pix, int C, float* out, void* stream);
/* bf16 twin (g bf16, fp32 sums; C a multiple of 8, at most 256): the identity_conv bias gradient under AMP */
int64_t dt_channel_sums_bf16_workspace(int64_t n_pix, int C);
int dt_channel_sums_bf16(const void* g_bf16, float* workspace, int64_t n_pix, int C, float* out, void* stream);

/* ------------------------------------------------------------------ pooling / resampling (K4,K9 bwd) */
/* max_pool2d(k=3,s=2,p=1) NHWC; argmax (uint8 window position, first max in scan order like ATen). */
int dt_maxpool3x3s2(const float* x, float* out, uint8_t* argmax, int B, int H, int W, int C, void* stream);
int dt_maxpool3x3s2_bwd(const float* dout, const uint8_t* argmax, float* dx, int accumulate, int B,
                        int H, int W, int C, void* stream);
/* backward of nearest x2 upsample: dx[b,y,x,c] = sum of the 2x2 block of dup; dup is [B,2H,2W,C]. */
int dt_upsample2x_bwd(const float* dup, float* dx, int accumulate, int B, int H, int W, int C, void* stream);
/* layout shuttles at the module boundary */
int dt_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, void* stream);
int dt_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, void* stream);
/* uint8 HWC tile -> normalised fp32 NHWC ((x/255-mean)/std), reference data/deadtreedata.py:148-154 */
/* mean/std are HOST arrays of Cdst floats (passed by value to the kernel). */
int dt_normalize_u8(const uint8_t* src, float* dst, int64_t n_pix, int Csrc, int Cdst, const float* mean,
                    const float* std, void* stream);
/* Tiled-inference input in one gather (reference deployment/tiler.py:121-134 zero-pad + utils/data_handling.py:9-20
 * make_blocks_vectorized + scripts/inference.py:94-96 per-tile Normalize): band-major uint8 raster [Csrc][h][w] ->
 * fp32 NHWC sub-tiles [n_blocks][d][d][Cdst] for the blocks first_block .. of the row-major block grid that is nbx blocks
 * wide; pixels beyond the raster are the tiler's zero padding (normalised like a zero byte). */
int dt_split_normalize_u8(const uint8_t* raster_chw, float* dst_nhwc, int Csrc, int h, int w, int d, int nbx,
                          int first_block, int n_blocks, int Cdst, const float* mean, const float* stdv, void* stream);

/* Overlap-stitched tiled inference (BASELINE configs[5]; the reference has no overlap).  Geometry, shared by all its
 * entry points: d = window edge, overlap o even with 0 <= o <= d/2, stride s = d - o; an axis of length L carries
 * n(L) = max(1, ceil((L - o) / s)) windows (dt_stitch_window_count; <0 on bad arguments); window k = i * nx + j has its
 * origin at (i * s, j * s), row-major; pixels beyond the raster are the tiler's zero byte; o = 0 is the block grid of
 * dt_split_normalize_u8.  A raster pixel lies in at most 2 windows per axis.  K <= 4 classes. */
int dt_stitch_window_count(int L, int d, int overlap);
/* Test-time augmentation on the stitched path.  A view is (flip: 0 none, 1 horizontal, 2 vertical; rot: k of np.rot90),
 * view = rot90^k(flip(window)) as in dt_augment_normalize_u8; windows are square, so all eight are legal.  `views` is a
 * HOST array of n_views pairs (flip_0, rot_0, flip_1, rot_1, ...), 1 <= n_views <= 8; it is read during the call and
 * travels to the kernel by value.  views == NULL with n_views == 0 is the plain window: the one identity view (NULL with
 * any other n_views is an argument error). */
/* dt_split_normalize_u8 with window origins `stride` = d - o apart (same arithmetic: bit-identical at stride == d, which is
 * how dt_split_normalize_u8 is served): windows first .. first + count - 1 of the grid that is nwx = n(w) windows wide ->
 * fp32 NHWC [count][d][d][Cdst] without views; with views [count][n_views][d][d][Cdst], tile k * n_views + v is view v of
 * window first + k - a bit-exact permutation of the plain window (zero padding included). */
int dt_window_normalize_u8(const uint8_t* raster_chw, float* dst_nhwc, int Csrc, int h, int w, int d, int stride, int nwx,
                           int first, int count, int Cdst, const float* mean, const float* stdv, const int* views,
                           int n_views, void* stream);
/* average mode.  logits: fp32 NCHW [count][K][d][d] of the windows first .. first + count - 1 ([count][n_views][K][d][d]
 * of the gather's tiles with views); acc: fp32 planar [K][h][w], zeroed before the first call.  For every window of the
 * range that covers the pixel, in ascending index: the softmax of every view is read where the window pixel sits in that
 * view, the probability vectors are summed in view order and multiplied by 1.0f / n_views (without views: the window's
 * own softmax, the same bits as the one view (0, 0)), then acc[k][gy][gx] += weight * mean_k.  weight_mode
 * DT_STITCH_WEIGHT_RAMP: r(y) * r(x), r(t) = min(1, (t + 1) / (o + 1), (d - t) / (o + 1)); DT_STITCH_WEIGHT_KEEP: 1 inside
 * the window's kept region of dt_stitch_classes_u8 and 0 outside, i.e. exactly one window per pixel.  One thread owns a
 * pixel: with calls in ascending window order the accumulator is bit-identical for every split into calls.  Several
 * models may add into one acc (soft vote), each in ascending window order; dt_stitch_finalize normalises. */
#define DT_STITCH_WEIGHT_RAMP 0
#define DT_STITCH_WEIGHT_KEEP 1
int dt_stitch_accumulate(const float* logits, float* acc, int K, int h, int w, int d, int overlap, int first, int count,
                         const int* views, int n_views, int weight_mode, void* stream);
/* classes uint8 [h][w] = argmax_k acc (ties -> lowest k, the head kernel's rule); probs (may be NULL): fp32 [K][h][w] =
 * acc_k / sum_k acc. */
int dt_stitch_finalize(const float* acc, uint8_t* classes, float* probs, int K, int h, int w, void* stream);
/* crop mode.  maps: uint8 [count][d][d] class maps of the windows first .. (the head kernel's fused argmax); window i of n
 * keeps rows (columns alike) [i * s + (i > 0) * o/2, i * s + d - (i < n - 1) * o/2) — disjoint regions that tile the
 * raster — and writes them into classes uint8 [h][w]. */
int dt_stitch_classes_u8(const uint8_t* maps, uint8_t* classes, int h, int w, int d, int overlap, int first, int count,
                         void* stream);

/* scripts/inference.py:60-62 is_valid_tile: flag[0] (int32, zero it first) = 1 iff some byte of band[n] is neither 0 nor
 * 255 (a raster whose first band is all 0 / 255 is skipped by the reference's driver). */
int dt_band_has_data(const uint8_t* band, int64_t n, int32_t* flag, void* stream);

/* Training augmentation on the device, data/deadtreedata.py:128-146 `train_transform`:
 * OneOf(HorizontalFlip, VerticalFlip), RandomRotate90, RandomBrightnessContrast(brightness_by_max=False),
 * Normalize, ToTensorV2 in ONE gather pass uint8 NHWC [B,H,W,Csrc] -> fp32 NHWC [B,H,W,Cdst].
 * The host draws the per-sample parameters: geo int32 [B][2] = (flip 0 none / 1 horizontal / 2 vertical,
 * rot k = np.rot90 count, H == W when k is odd), bc fp32 [B][2] = (alpha, beta); (1, 0) leaves the pixel values
 * unchanged, else lut(v) = uint8(clip(v*alpha + beta*mean(image), 0, 255)) as albumentations does for uint8.
 * sums_scratch: B uint64 (per-image pixel sums for the mean).  mean/std: HOST arrays of Cdst floats.
 * dt_augment_labels applies the same geometric map to int64 [B,H,W] masks / land-use maps. */
int dt_augment_normalize_u8(const uint8_t* src, float* dst, const int32_t* geo, const float* bc, uint64_t* sums_scratch,
                            int B, int H, int W, int Csrc, int Cdst, const float* mean, const float* std, void* stream);
int dt_augment_labels(const int64_t* src, int64_t* dst, const int32_t* geo, int B, int H, int W, void* stream);

/* Batch gather from a device-resident sample pool: images uint8 [N][H][W][4] (4-byte aligned), masks / lu uint8 [N][H][W]
 * (lu and lu_out may both be NULL), sums uint64 [N] = the exact sum of the 4*H*W image bytes of every sample.  For
 * b < B the sample idx[b] goes through the flip / turn geo[b] and the brightness-contrast bc[b] of
 * dt_augment_normalize_u8, with its arithmetic bit for bit, into img_out fp32 PLANAR [B][Cdst][H][W]; mask_out / lu_out
 * int64 [B][H][W] take the same pixel map.  merge_above != 0: mask labels above 1 become 1 (the reference's
 * classes == 2 rule, data/deadtreedata.py:179-180); lu is never merged.  One launch, no scratch memory.
 * The pool is never read out of range: a sample with idx[b] outside [0, N), or with an odd turn while H != W, is
 * written as zeros and ORs DT_POOL_ERR_INDEX / DT_POOL_ERR_TURN into err_flag[0] (int32, zeroed by the caller).
 * mean/std: HOST arrays of Cdst floats.  This is dt_pool_gather_combined with one source and src == NULL: the same kernel,
 * the same checks. */
#define DT_POOL_ERR_INDEX 1
#define DT_POOL_ERR_TURN 2
int dt_pool_gather_batch(const uint8_t* images, const uint8_t* masks, const uint8_t* lu, const uint64_t* sums,
                         const int32_t* idx, const int32_t* geo, const float* bc, float* img_out, int64_t* mask_out,
                         int64_t* lu_out, int32_t* err_flag, int64_t N, int B, int H, int W, int Cdst, int merge_above,
                         const float* mean, const float* std, void* stream);

/* One batch out of SEVERAL pools in one launch (the reference's main + extra shard sets, data/deadtreedata.py:348-395):
 * sources is a HOST array of n_sources (1 .. DT_POOL_MAX_SOURCES) pools laid out as dt_pool_gather_batch takes them, all
 * of one tile size H x W; slot b < B reads sample idx[b] of source src[b] (both int32 [B] on the device) with the
 * arithmetic, pixel map and stores of dt_pool_gather_batch, bit for bit.  lu_out non-NULL requires lu in every source;
 * with lu_out NULL the sources' lu are not read.  src[b] outside [0, n_sources) ORs DT_POOL_ERR_SOURCE into err_flag[0],
 * idx[b] outside [0, sources[src[b]].n) DT_POOL_ERR_INDEX, an odd turn while H != W DT_POOL_ERR_TURN; such a slot reads
 * nothing and is written as zeros.  The table travels as a kernel argument: no copy, no scratch memory.  src may be NULL
 * exactly when n_sources == 1: every slot then reads source 0 (what dt_pool_gather_batch does). */
#define DT_POOL_MAX_SOURCES 8
#define DT_POOL_ERR_SOURCE 4
typedef struct dt_pool_source {
  const uint8_t* images;
  const uint8_t* masks;
  const uint8_t* lu;
  const uint64_t* sums;
  int64_t n;
} dt_pool_source;
int dt_pool_gather_combined(const dt_pool_source* sources, int n_sources, const int32_t* src, const int32_t* idx,
                            const int32_t* geo, const float* bc, float* img_out, int64_t* mask_out, int64_t* lu_out,
                            int32_t* err_flag, int B, int H, int W, int Cdst, int merge_above, const float* mean,
                            const float* std, void* stream);

/* Data gradient of a 3x3 stride-1 layer with the BatchNorm-backward REDUCTION of the layer it feeds fused into the
 * epilogue (instead of a separate dt_bn_bwd_reduce pass over the tensor it has just written): out0 = conv(src0, w)
 * like dt_conv2d (no concat / split / accumulate / upsample), and red[2][P][Cout] (P = dt_conv2d_stat_rows(desc))
 * receives per workgroup  sum g  and  sum g * xhat  with  g = out0 * [y*act_scale + act_shift > 0],
 * xhat = (y - mean) * invstd  — exactly what dt_bn_bwd_reduce computes from (dout = out0, y) with a virtual
 * activation.  `red` must hold dt_bn_stats_floats(P, Cout) floats; pass it with P to dt_bn_bwd_apply. */
typedef struct dt_bn_bwd_fuse {
  const float* y;          /* raw conv output of the BatchNorm layer, same shape as out0 */
  const float* mean;
  const float* invstd;
  const float* act_scale;  /* scale / shift of that BatchNorm (its ReLU mask is recomputed from y) */
  const float* act_shift;
  const float* act;        /* optional: the STORED activation (block outputs, relu(bn(y) + identity)); when given the
                              mask is act > 0 and act_scale / act_shift are not read.  With it the convolution may be a
                              gradient join (desc->accumulate = 1): the sums are taken over out0 AFTER the add. */
} dt_bn_bwd_fuse;
int dt_conv2d_bn_bwd(const dt_conv_desc* desc, const float* src0, const float* w, float* out0, float* red,
                     const dt_bn_bwd_fuse* fuse, void* stream);
/* Winograd form of dt_conv2d_bn_bwd: same arguments, u = dt_winograd_weights of the flipped / transposed weights. */
int dt_conv2d_winograd_bn_bwd(const dt_conv_desc* d, const float* src0, const float* u, float* out0, float* red,
                              const dt_bn_bwd_fuse* fuse, void* stream);
/* Data gradient of a decoder conv1 — y = conv3x3(cat(nearest_upsample_x2(x), skip)) — with the up-sampling's backward in
 * the Winograd epilogue (the 2x2 outputs of a Winograd tile are one source pixel's four gradients): `desc` = the stride-1
 * data-gradient descriptor (C0 = the convolution's output channels, Cout = channels of x + skip, cout_split = channels of
 * x; multiples of 64), u = dt_winograd_weights of the flipped / transposed weights.  gx [B, Hin/2, Win/2, cout_split] =
 * gradient of x (2x2-summed, never stored at full resolution), red [2][P][cout_split] = BatchNorm-backward sums of the
 * layer that produced x (fuse: its raw output at gx's resolution, mean, invstd, act_scale, act_shift), dskip [B, Hin,
 * Win, Cout - cout_split] = gradient of the skip.  Replaces dt_conv2d_winograd (split outputs) + dt_upsample2x_bwd_bn
 * (reference: autograd of torch.cat + F.interpolate(nearest, x2) + Conv2d in smp's DecoderBlock.forward). */
int dt_conv2d_winograd_upsampled_dgrad_supported(const dt_conv_desc* desc);
int dt_conv2d_winograd_upsampled_dgrad_rows(const dt_conv_desc* desc);
int dt_conv2d_winograd_upsampled_dgrad(const dt_conv_desc* desc, const float* dy, const float* u, float* gx, float* dskip,
                                       float* red, const dt_bn_bwd_fuse* fuse, int launches /* reserved: pass 3 */,
                                       void* stream);
/* the same restricted to the up-sampled input channels [0, cout_split): no skip gradient computed or written (decoder
 * blocks 1-3 with a frozen encoder); red[2][P][cout_split], P = dt_conv2d_winograd_upsampled_dgrad_x_rows(desc) */
int dt_conv2d_winograd_upsampled_dgrad_x_rows(const dt_conv_desc* desc);
int dt_conv2d_winograd_upsampled_dgrad_x(const dt_conv_desc* desc, const float* dy, const float* u, float* gx, float* red,
                                         const dt_bn_bwd_fuse* fuse, void* stream);

/* ------------------------------------------------------------------ segmentation head (K11,K12,K19) */
/* logits[B,K,H,W] (NCHW) = conv3x3(x[B,H,W,Cin], w[K][3][3][Cin]) + bias; optional uint8/int64 argmax
 * class map (ties -> lowest index, torch.argmax) — smp SegmentationHead + inference.py:62. */
int dt_head_fwd(const float* x, const float* w_ohwi, const float* bias, float* logits_nchw,
                int64_t* argmax_i64, uint8_t* argmax_u8, int B, int H, int W, int Cin, int K, void* stream);
int dt_head_bwd_rows(int B, int H, int W);
/* floats the `red` scratch of dt_head_bwd / dt_head_bwd_finalize must hold (partial rows + reduction stage) */
int64_t dt_head_bwd_red_floats(int B, int H, int W, int Cin, int K);
/* dx[B,H,W,Cin] and one partial row of dW/dbias per workgroup into red; dt_head_bwd_finalize sums the rows
 * (two-stage, fixed order) into dw_ohwi[K][3][3][Cin] and dbias[K]. */
int dt_head_bwd(const float* x, const float* w_ohwi, const float* dlogits_nchw, float* dx, float* red,
                int B, int H, int W, int Cin, int K, void* stream);
int dt_head_bwd_finalize(float* red, int P, float* dw_ohwi, float* dbias, int Cin, int K, void* stream);

/* ------------------------------------------------------------------ losses & metrics (K12-K18) */
#define DT_LOSS_NACC 10
/* per (b,k) accumulators, fp64 [B][K][DT_LOSS_NACC]:
 *   0 count(t)  1 sum p*t  2 sum p  3 sum (1-p)^gamma * t * log(p+1e-10)  4 sum t*log(p+1e-10)
 *   5 sum p*dist  6 sum t*[p>0.5]  7 sum [p>0.5]
 *   8 sum t * wass, wass = sum_l M[label][l] * softmax(p)_l  (GWDICE, loss/gwdl.py:131-178; only when wass_m given:
 *     K x K label-distance matrix, row-major; note the SECOND softmax over the probabilities, segmodel.py:176)
 *   9 sum t * V(pixel), V = gw_possum from dt_gwdice_possum (the cross-sample sum the reference's broadcasting
 *     in gwdl.py:180-198 produces); wass_m and gw_possum are both NULL unless GWDICE is on.
 * from logits (softmax fused, never materialising the int32 one-hot of losses.py:124-141).
 * labels int64 [B,H,W]; dist may be NULL.  Also optionally writes probs[B,K,H,W].
 * acc must have room for dt_seg_loss_acc_doubles(B,K,H,W) doubles: the [B][K][NACC] result first,
 * per-workgroup partial rows behind it (fixed-order second stage, no atomics).
 * Labels outside [0,K) (the assert of losses.py:129) set err_flag[0]=1 instead of aborting the kernel. */
int64_t dt_seg_loss_acc_doubles(int B, int K, int H, int W);
int dt_seg_loss_fwd(const float* logits, const int64_t* labels, const float* dist, const float* wass_m,
                    const float* gw_possum, float gamma, double* acc, float* probs, int32_t* err_flag, int B, int K, int H, int W, void* stream);
/* dlogits = softmax-backward of g, g_k = a[b,k]*t_k + c[b,k] + wf*focal'(p_k)*t_k + wb[k]*dist_k,
 * scaled by gscale[0] (device scalar: upstream grad); coef fp32 [B][K][2] = (a,c); wfocal = [wf/M, gamma].
 * GWDICE (all NULL when unused): wass_m [K][K]; d loss / d wass of pixel (b, s) = wass_coef[b] + gw_posgrad[s]
 * (fp32 [B] and [H*W], the latter from dt_gwdice_posgrad); chained through the second softmax before it joins g. */
int dt_seg_loss_bwd(const float* logits, const int64_t* labels, const float* dist, const float* coef,
                    const float* wfocal, const float* wbound, const float* gscale, const float* wass_m,
                    const float* wass_coef, const float* gw_posgrad, float* dlogits, int B, int K, int H, int W,
                    void* stream);
/* The scalar algebra of SemSegment.calculate_loss / log_metrics (segmodel.py:169-208; gdl.py:15-27,
 * losses.py:187-291, gwdl.py:110-138, smp Fscore) on the [B][K][NACC] sums of dt_seg_loss_fwd, fp64, on the device:
 *   parts fp32 [8] = dice_loss, boundary_loss, focal_loss, ce_loss, dice (Fscore w/o background), dice_with_bg,
 *                    total_loss, total_loss (slot 7 = the differentiable scalar callers hand to backward);
 *   coef [B][K][2], wfocal [2], wbound [K] and (GWDICE) wass_a [B] (-> dt_gwdice_posgrad), wass_c [B]: the inputs of
 *   dt_seg_loss_bwd.  dice_kind 0 GDICE / 1 DICE / 2 GWDICE / 3 no dice term (single-loss callables); boundary_weight = alpha for BOUNDARY-RAMPED, else 1. */
typedef struct dt_loss_cfg {
  int32_t dice_kind, use_boundary, use_focal;
  float boundary_weight, gamma;
} dt_loss_cfg;
int dt_seg_loss_algebra(const double* acc, const dt_loss_cfg* cfg, int B, int K, int H, int W, float* parts, float* coef,
                        float* wfocal, float* wbound, float* wass_a, float* wass_c, void* stream);
/* GWDICE position passes.  loss/gwdl.py:180-198 broadcasts alpha[B,1,S] * (1 - wass)[B,S] to [B,B,S], so sample
 * i's generalised true positives are sum_s alpha_i(s) * V(s), V(s) = sum_j (1 - wass_j(s)) over the whole batch
 * (equal to the published formula only for B = 1); reproduced because the reference trains with it.
 *   dt_gwdice_possum : possum[H*W] = V                                   (forward, before dt_seg_loss_fwd)
 *   dt_gwdice_posgrad: posgrad[H*W] = sum_i sample_coef[i] * [0 < label_i(s) < K]   (backward, before dt_seg_loss_bwd;
 *                      a label outside [0,K) counts for no class, as in dt_seg_loss_fwd) */
int dt_gwdice_possum(const float* logits, const int64_t* labels, const float* wass_m, float* possum, int B, int K,
                     int H, int W, void* stream);
int dt_gwdice_posgrad(const int64_t* labels, const float* sample_coef, float* posgrad, int B, int K, int H, int W,
                      void* stream);

/* K x K confusion counts accumulated on the device (eval reductions, segmodel.py:291-309,337-365):
 * counts int64 [2][K][K] (+=): plane 0 all pixels, plane 1 pixels with lu == 1 (lu may be NULL);
 * rows = target, columns = prediction.  Give the prediction as int64 OR uint8 (the other pointer NULL). */
int dt_confusion_matrix(const int64_t* pred_i64, const uint8_t* pred_u8, const int64_t* target, const int64_t* lu,
                        int K, int64_t n, int64_t* counts, int32_t* err_flag, void* stream);

/* Fused evaluation head (validation / test epochs): ONE pass over the decoder output x[B,H,W,Cin = 16] does what
 * dt_head_fwd -> dt_seg_loss_fwd -> dt_confusion_matrix do in three, and the logits never reach memory:
 *   acc    fp64 [B][K][DT_LOSS_NACC] (overwritten): slots 0-7 as above; 8, 9 (GWDICE: they need a pass over every
 *          sample's logits first) are written as zero.  Room for dt_head_eval_acc_doubles(B,K,H,W) doubles: one
 *          partial row per workgroup behind the result, fixed-order second stage, no float atomics.
 *   counts int64 [2][K][K] (+=) as dt_confusion_matrix (lu may be NULL), arg-max ties -> lowest class.
 *   argmax_u8 [B,H,W] optional.  A label outside [0,K) sets err_flag[0] = 1 and enters no confusion count.
 * The logits come from the same device function as dt_head_fwd's: arg-max map, counts and the slots 0, 6, 7 equal
 * the three-kernel chain exactly, the real-valued slots to fp32 summation order.  2 <= K <= 4, dist [B,K,H,W] or NULL. */
int64_t dt_head_eval_acc_doubles(int B, int K, int H, int W);
int dt_head_eval(const float* x, const float* w_ohwi, const float* bias, const int64_t* labels, const int64_t* lu,
                 const float* dist, float gamma, double* acc, int64_t* counts, uint8_t* argmax_u8, int32_t* err_flag,
                 int B, int H, int W, int Cin, int K, void* stream);
int dt_head_eval_bf16(const void* x_bf16, const float* w_ohwi, const float* bias, const int64_t* labels,
                      const int64_t* lu, const float* dist, float gamma, double* acc, int64_t* counts,
                      uint8_t* argmax_u8, int32_t* err_flag, int B, int H, int W, int Cin, int K, void* stream);
/* Epoch mean of the per-batch scalars on the device: epoch[i] += weight * parts[i] for i < 8 (parts of
 * dt_seg_loss_algebra), epoch[8] += weight; fp64, one launch, no host synchronisation. */
int dt_eval_accumulate(const float* parts, double weight, double* epoch, void* stream);

/* Ensemble vote (deployment/inference.py:65-116 PyTorchEnsembleInference.run): per-pixel torch.mode over the
 * uint8 class maps of M models, maps[M][n]; ties -> the smallest class (torch.mode).  n % 4 == 0, 2 <= K <= 8.
 * Writes uint8 and/or int64 maps (either pointer may be NULL); classes >= K set err_flag[0]. */
int dt_ensemble_vote(const uint8_t* maps, int M, int64_t n, int K, uint8_t* out_u8, int64_t* out_i64,
                     int32_t* err_flag, void* stream);

/* Raster statistics (scripts/computestats_inference.py, scripts/aggregate_results.py, deployment/server.py:112): class
 * counts per zone of a uint8 class map in device memory.  counts int64 [Z][K] (+=, as dt_confusion_matrix: one buffer
 * can collect many rasters): counts[z][c] += the number of pixels i < n with zones[i] == z and classes[i] == c.  zones
 * may be NULL: Z must then be 1 and every pixel is zone 0.  2 <= K <= 8, 1 <= Z <= 8, n >= 1; any n and any byte
 * alignment of either pointer (the two may differ).  A class >= K ORs 1 into err_flag[0], a zone >= Z ORs 2; such a
 * pixel enters no count, all others are counted.  Integer arithmetic only: exact and independent of the order. */
int dt_zonal_counts_u8(const uint8_t* classes, const uint8_t* zones, int64_t n, int K, int Z, int64_t* counts,
                       int32_t* err_flag, void* stream);

/* Cover grids (deployment/cover.py states the contract): area-weighted class counts per zone and per cell of a coarser
 * grid, from a uint8 class map [h][w] in device memory, 1 <= h, w <= 16384.  The grid is two edge tables in device memory,
 * int32 in units of 1/256 pixel: yq[gy + 1] and xq[gx + 1], strictly increasing, every cell at least 256 wide, |q| <= 2^23
 * (the CALLER checks the tables; whatever they hold, nothing outside `sums` is written).  Pixel (i, j) is the square
 * (j, j + 1) x (i, i + 1); wy(g, i) = max(0, min(yq[g + 1], 256 (i + 1)) - max(yq[g], 256 i)), wx likewise.  sums int64
 * [gy][gx][Z][K] (+=): sums[g][x][z][c] += the sum of wy(g, i) * wx(x, j) over the pixels with zones == z and classes == c,
 * in units of 1/65536 pixel.  zones may be NULL: Z must then be 1.  2 <= K <= 8, 1 <= Z <= 8, gy * gx * Z * K <= 2^26; any
 * byte alignment of either map.  A class >= K ORs 1 into err_flag[0], a zone >= Z ORs 2; such a pixel enters no sum.
 * One launch over the dt_patch_tile tiles of the map, no synchronisation.  Integers only: exact, order independent. */
int dt_cover_grid_u8(const uint8_t* classes, const uint8_t* zones, int h, int w, int K, int Z, const int32_t* yq, int gy,
                     const int32_t* xq, int gx, int64_t* sums, int32_t* err_flag, void* stream);

/* Dead-tree patches (deployment/patches.py states the contract): connected components of a uint8 class map [h][w] in
 * device memory, h * w <= 2^31 - 2.  A patch is a maximal set of pixels of one class c, 1 <= c < K, connected through
 * 4- or 8-neighbourhoods; class 0 is background.  No entry point synchronises; all integers: exact, order independent.
 *
 * dt_label_patches_u8: labels int32 [h][w] (overwritten): 0 on background, elsewhere 1 + min(y * w + x) over the pixel's
 *   patch.  2 <= K <= 8, connectivity 4 or 8.  A class >= K ORs 1 into err_flag[0] and is background.  Three launches:
 *   union-find per tile in LDS, lock-free unions across the tile borders, path flattening; dt_patch_tile gives the tile.
 * dt_patch_areas: area_plane int32 [h * w], ZEROED BY THE CALLER: += the pixel count of every patch at its root's index
 *   (label - 1); other entries are not touched.
 * dt_sieve_patches_u8: in place; the pixels of every patch with area < min_pixels become class 0 / label 0 and the root's
 *   area entry becomes 0 (no fill from the neighbours); min_pixels <= 1 changes nothing.
 * dt_patch_measure: the table of n patches.  dense_plane int32 [h * w] holds at every root's index the row of that root
 *   (other entries are not read).  Overwrites cls uint8 [n] (the class), bbox int32 [n][4] (y0, x0, y1, x1, inclusive),
 *   sum_y / sum_x int64 [n] (sums of the pixels' row / column numbers). */
int dt_patch_tile(int* th, int* tw);
int dt_label_patches_u8(const uint8_t* classes, int h, int w, int K, int connectivity, int32_t* labels, int32_t* err_flag,
                        void* stream);
int dt_patch_areas(const int32_t* labels, int h, int w, int32_t* area_plane, void* stream);
int dt_sieve_patches_u8(uint8_t* classes, int32_t* labels, int32_t* area_plane, int h, int w, int min_pixels, void* stream);
int dt_patch_measure(const int32_t* labels, const uint8_t* classes, int h, int w, const int32_t* dense_plane, int n,
                     uint8_t* cls, int32_t* bbox, int64_t* sum_y, int64_t* sum_x, void* stream);

/* Dead-tree patch outlines (deployment/outlines.py states the contract): the boundaries of the patches of a label plane
 * int32 [h][w] in device memory (dt_label_patches_u8, sieved or not; a value <= 0 is background), traced into rings along
 * the pixel edges; h, w in 1..16384.  A labelled pixel p = y * w + x owns side s (0 top, 1 right, 2 bottom, 3 left) iff the
 * neighbour across it carries another label; edges are compacted in ascending key 4 p + s (E of them), the successor of
 * an edge is the next edge of its ring (connectivity 4 or 8 decides at saddle vertices), a ring's id is its smallest
 * edge and its vertices are the end points of the edges behind which the ring turns (the corners), V in all.  Integers
 * only, no atomics, no entry point synchronises; the caller reads E and V back after dt_outline_count and the ring
 * count R after dt_outline_jump (ops.patch_outlines is the driver).  Workspace: 4 bytes per pixel (first), 36 per edge
 * (edges + two states) and 1 per edge for the head flags.
 *
 * dt_outline_chunk: the pixels one workgroup of dt_outline_count takes.
 * dt_outline_count: chunk_counts int32 [ceil(h w / chunk)][2] (overwritten): owned sides and corners per chunk of
 *   consecutive row-major pixels.  The caller scans them: E and V are the totals.
 * dt_outline_edges: chunk_first int32 [chunks] = the exclusive scan of the edge counts.  Overwrites first int32 [h w] (the
 *   compact index of a pixel's first edge), edges uint32 [E] (4 p + s, bit 31: the end point is a corner) and state
 *   int32 [E][4] = (e, 0, corner, successor's compact index), 16-byte aligned.
 * dt_outline_rounds: ceil(log2(E)), the rounds dt_outline_jump runs.
 * dt_outline_jump: pointer jumping, one launch per round, ping-pong between state and scratch (same size, 16-byte
 *   aligned): the result lies in state when the round count is even, else in scratch.  Row e becomes (ring id, corners from e
 *   forward to the ring's id edge without that edge's own, -, -).  head uint8 [E] (overwritten): 1 where e is a ring id.
 * dt_outline_rings: heads int64 [R] = the ring ids ascending; overwrites ring_corners int32 [R] (the ring's vertex count)
 *   and ring_label int32 [R] (the label of its patch).  state: the result of dt_outline_jump.
 * dt_outline_scatter: row_of int32 [E] holds at every ring id the row of that ring in the caller's order (other entries are
 *   not read), ring_offsets int64 [R + 1] the scan of the rings' vertex counts in that order.  Writes xy int32 [V][2]: the
 *   vertices (x, y) in 1/256 pixel, a ring's in cycle order from its id edge on. */
int dt_outline_chunk(int* chunk);
int dt_outline_count(const int32_t* labels, int h, int w, int32_t* chunk_counts, void* stream);
int dt_outline_edges(const int32_t* labels, int h, int w, int connectivity, const int32_t* chunk_first, int n_edges,
                     int32_t* first, uint32_t* edges, int32_t* state, void* stream);
int dt_outline_rounds(int n_edges);
int dt_outline_jump(int32_t* state, int32_t* scratch, int n_edges, uint8_t* head, void* stream);
int dt_outline_rings(const int32_t* labels, int h, int w, int connectivity, const int32_t* first, const uint32_t* edges,
                     const int32_t* state, int n_edges, const int64_t* heads, int n_rings, int32_t* ring_corners,
                     int32_t* ring_label, void* stream);
int dt_outline_scatter(const uint32_t* edges, const int32_t* state, int n_edges, int w, const int32_t* row_of,
                       const int64_t* ring_offsets, int n_rings, int64_t n_vertices, int32_t* xy, void* stream);

/* Patch overlaps (deployment/overlaps.py states the contract): the runs of equal pair keys of two label planes int32
 * [h][w] in device memory (dt_label_patches_u8, sieved or not; a value <= 0 is background), 16-byte aligned, h * w <=
 * 2^31 - 2.  key(p) = ((int64)labels_a[p] << 32) | (uint32)labels_b[p] where both labels are > 0, else 0; a run is a maximal
 * stretch of consecutive pixels p = y * w + x with one key (rows are not told apart).  Integers only, no atomics, no entry
 * point synchronises, neither plane is written; the caller reads the run count R back after dt_overlap_count, sorts the
 * runs by key and sums the lengths of equal keys (ops.patch_overlaps is the driver).  Workspace: 8 bytes per chunk and 12
 * per run.
 *
 * dt_overlap_chunk: the pixels one workgroup takes.
 * dt_overlap_count: chunk_counts int32 [ceil(h w / chunk)][2] (overwritten): the run heads per chunk of consecutive
 *   row-major pixels, and those among them whose key is not 0.  The caller scans the first column: R is its total.
 * dt_overlap_runs: chunk_first int32 [chunks] = the exclusive scan of the head counts.  Overwrites run_key int64 [R] and
 *   run_start int32 [R] (the run's first pixel), runs in ascending start. */
int dt_overlap_chunk(int* chunk);
int dt_overlap_count(const int32_t* labels_a, const int32_t* labels_b, int h, int w, int32_t* chunk_counts, void* stream);
int dt_overlap_runs(const int32_t* labels_a, const int32_t* labels_b, int h, int w, const int32_t* chunk_first, int n_runs,
                    int64_t* run_key, int32_t* run_start, void* stream);

/* Nearest-patch distances (deployment/proximity.py states the contract): labels_src (LS) and labels_qry (LQ) are label planes
 * int32 [h][w] in device memory (dt_label_patches_u8, sieved or not; a value <= 0 is background) on one grid, sides <= 16384
 * and h * w <= 2^31 - 2.  d2(p, q) = (yp - yq)^2 + (xp - xq)^2 between pixel centres.  For the query patch of table row b the
 * result is the lexicographic minimum of (d2(p, q), LS[q] - 1) over the pairs with LQ[p] = 1 + its root, LS[q] > 0, with
 * exclude_own LS[q] != LQ[p], and with a limit d2(p, q) <= limit2: best[b] = d2 << 32 | (LS[q] - 1), all ones without such
 * a pair.  Integers only, no entry point synchronises, no workgroup waits for another, neither label plane is written; the
 * result is a pure function of the planes (a minimum does not depend on the order of the atomics).
 *
 * dt_proximity_segment / dt_proximity_window: the rows of one column segment of dt_proximity_columns, and the pixels of a
 *   row that one workgroup of dt_proximity_query takes.
 * dt_proximity_columns: overwrites the column tables of LS.  P = 2 planes, 4 with second != 0: plane dir (0: at or above the
 *   pixel's row, 1: at or below, the row itself included) holds for every pixel the nearest labelled pixel of its column —
 *   dist uint16 [P][h][w] the row distance (0xffff: none), nearest int32 [P][h][w] its label (0: none); plane 2 + dir the
 *   nearest labelled pixel of the column in that direction whose label differs from plane dir's.  carry int32
 *   [2][ceil(h / segment)][w][4], 16-byte aligned: workspace (the state every segment starts from).  flag int32 [1]
 *   (overwritten): 1 when LS has a labelled pixel at all, else 0.  12 bytes per pixel, 24 with second.
 * dt_proximity_query: dist / nearest / flag as dt_proximity_columns left them (second: how they were built; exclude_own
 *   needs it), dense_plane int32 [h * w]: root -> table row as dt_patch_measure takes it (a row outside 0 .. n - 1: no row),
 *   limit2 < 0: no limit.  best uint64 [n] is preset to all ones by the caller and lowered with 64-bit atomic minima;
 *   n == 0 launches nothing.  With flag == 0 every workgroup returns at once: an empty source plane costs one pass. */
int dt_proximity_segment(int* rows);
int dt_proximity_window(int* pixels);
int dt_proximity_columns(const int32_t* labels_src, int h, int w, int second, uint16_t* dist, int32_t* nearest,
                         int32_t* carry, int32_t* flag, void* stream);
int dt_proximity_query(const uint16_t* dist, const int32_t* nearest, const int32_t* flag, const int32_t* labels_qry, int h,
                       int w, const int32_t* dense_plane, int n, int exclude_own, int second, int64_t limit2, uint64_t* best,
                       void* stream);

/* Patch attributes (deployment/attributes.py states the contract): what the patches of a label plane look like in a raster
 * on the same grid and how sure the model was.  labels int32 [h][w] (dt_label_patches_u8, sieved or not; a value outside
 * 1 .. h * w is background), raster uint8 [C][h][w] planar, 1 <= C <= 8, dense_plane int32 [h * w]: root -> table row as
 * dt_patch_measure takes it (a row outside 0 .. n - 1: no row), all in device memory; sides <= 16384, h * w <= 2^31 - 2.
 * pairs: HOST array of n_pairs <= 4 band pairs (a, b), bands < C.  classes uint8 [h][w] and probs fp32 [K][h][w], 2 <= K <= 8:
 * both or neither (NULL); a class >= K counts as probability 0.
 * Per table row, over the pixels that carry its label (integers only, so the tables are a pure function of the inputs):
 *   sums int64 [n][Q], Q = 2 C + n_pairs + (probs ? 1 : 0): the C band sums, the C sums of squares, per pair the sum of
 *     t = (v_a * 65534 + (s >> 1)) / s with s = v_a + v_b (unsigned; 32767 for s == 0), then the sum of
 *     q = floor(min(max(p, 0), 1) * 65535 + 0.5) over p = probs[classes[i]][i], product and sum each rounded to fp32, NaN -> 0;
 *   extremes int32 [n][M], M = 2 C + (probs ? 1 : 0): the C band minima, the C band maxima, then the minimum of q.
 * Two launches: one presets the rows (sums 0, minima 255 / 65535, maxima 0), one walks the pixels: a wave takes
 * dt_attribute_span consecutive 64-pixel chunks, reduces every quantity per run of equal labels and issues one integer atomic
 * per quantity and finished run.  n == 0 launches nothing.  No synchronisation, no input is written. */
int dt_attribute_span(int* chunks);
int dt_patch_attributes_u8(const int32_t* labels, const uint8_t* raster, int C, int h, int w, const int32_t* dense_plane,
                           int n, const uint8_t* classes, const float* probs, int K, const int* pairs, int n_pairs,
                           int64_t* sums, int32_t* extremes, void* stream);

/* Crowns (deployment/crowns.py states the contract): touching crowns split by their inscribed depth.  classes uint8 [h][w]
 * and int32 planes [h][w] in device memory, sides <= 16384, h * w <= 2^31 - 2, connectivity 4 or 8.  Integers only, no entry
 * point synchronises, no workgroup waits for another, every grid follows the pixel count; the results are pure functions of
 * the inputs (minima and maxima do not depend on the order of the atomics).
 *
 * dt_crown_segment: the rows of one column segment of dt_patch_depth2_u8.
 * dt_patch_depth2_u8: depth2 int32 [h][w] (overwritten): 0 on class 0 and on a class >= K (which ORs 1 into err_flag[0]),
 *   elsewhere min(cap2, the squared distance to the nearest pixel inside the raster of another class), 1 <= cap2 <= 2^30.
 *   core uint8 [h][w] or NULL: the class where depth2 >= core2 (1 <= core2 <= cap2), else 0.  Workspace: column uint16 [h][w]
 *   and carry int32 [ceil(h / segment)][w][4], 16-byte aligned.  Four launches: three for the columns (segment states, one
 *   lane per column chains them, the distances), one for the rows (outward search in LDS, at most 2 sqrt(cap2) entries).
 * dt_crown_grow: ONE growth round: dst = src, except that a pixel with a class and src == 0 takes the minimum of src over its
 *   neighbours of the same class with src != 0.  src and dst are different planes, 16-byte aligned, classes 4-byte aligned.
 *   slot int32 [1]: |= 1 when the round labelled a pixel.
 * dt_crown_remainder: remainder uint8 [h][w] = the class where grown == 0, else 0; flag int32 [1] |= 1 when a pixel with a
 *   class and grown == 0 has a neighbour of its class with grown != 0 (the growth has not converged).
 * dt_crown_merge: seg (the label plane of the remainder) becomes grown where that is not 0 — a value outside 1 .. h * w is 0
 *   —, IN PLACE; first int32 [h * w] PRESET TO INT32_MAX and depth int32 [h * w] ZEROED by the caller: first[seg - 1] = the
 *   smallest pixel index of the seg, depth[seg - 1] = its largest depth2.
 * dt_crown_relabel: crowns int32 [h][w] (overwritten, a plane of its own) = 1 + first[seg - 1], 0 where seg is 0;
 *   crown_depth int32 [h * w], ZEROED by the caller: at a crown's root (label - 1) the largest depth2 of its pixels. */
int dt_crown_segment(int* rows);
int dt_patch_depth2_u8(const uint8_t* classes, int h, int w, int K, int cap2, int core2, uint16_t* column, int32_t* carry,
                       int32_t* depth2, uint8_t* core, int32_t* err_flag, void* stream);
int dt_crown_grow(const uint8_t* classes, const int32_t* src, int32_t* dst, int h, int w, int connectivity, int32_t* slot,
                  void* stream);
int dt_crown_remainder(const uint8_t* classes, const int32_t* grown, int h, int w, int connectivity, uint8_t* remainder,
                       int32_t* flag, void* stream);
int dt_crown_merge(const int32_t* grown, int32_t* seg, const int32_t* depth2, int h, int w, int32_t* first, int32_t* depth,
                   void* stream);
int dt_crown_relabel(const int32_t* seg, const int32_t* first, const int32_t* depth, int h, int w, int32_t* crowns,
                     int32_t* crown_depth, void* stream);

/* Operating points (deadtrees_amd/loss/curves.py states the contract): probability histograms of a validation epoch and the
 * decision that applies a threshold per class.  Both quantise a probability p the same way:
 * q = floor(min(max(p, 0), 1) * 65535 + 0.5), product and sum each rounded to fp32, NaN -> 0; bin = q >> 8.
 *
 * dt_curve_chunk: the consecutive pixels of the B * H * W axis one workgroup of dt_prob_histogram takes.
 * dt_prob_histogram: src fp32 [B][K][H][W], probabilities or, with is_logits != 0, logits (they pass through the channel
 *   softmax of dt_seg_loss_fwd first), labels int64 [B][H][W], lu int64 [B][H][W] or NULL, 2 <= K <= 8, any alignment.
 *   hist int64 [2][K][2][256] (+=, as dt_confusion_matrix: one buffer collects an epoch): hist[plane][c][t][bin] counts the
 *   pixels whose q of class c falls into bin, t = 1 iff label == c; plane 0 every pixel, plane 1 those with lu == 1 (lu
 *   NULL: plane 1 is not touched).  A label outside [0, K) sets err_flag[0] = 1 and the pixel enters no count.  q_out
 *   uint16 [B][K][H][W] or NULL: every q, out-of-range pixels included.  One launch, integer atomics only: exact and
 *   independent of the order; no synchronisation.
 * dt_decide_classes_u8: probs fp32 [K][n] in device memory, thresholds a HOST array uint16 [K] (entry 0 is not read, the
 *   others in 1..65535).  out_u8[i] = the class c >= 1 with the largest q_c(i) among those with q_c(i) >= thresholds[c],
 *   ties -> the smallest c; 0 without one.  Every byte of out_u8 [n] is written; plane 0 of probs is not read. */
int dt_curve_chunk(int* chunk);
int dt_prob_histogram(const float* src, const int64_t* labels, const int64_t* lu, int64_t* hist, int32_t* err_flag,
                      uint16_t* q_out, int B, int K, int H, int W, int is_logits, void* stream);
int dt_decide_classes_u8(const float* probs, const uint16_t* thresholds, uint8_t* out_u8, int K, int64_t n, void* stream);

/* Patch-wise decisions (hysteresis and a confidence filter; deadtrees_amd/loss/curves.py states the contract): candidates at
 * the low thresholds L_c, their patches (dt_label_patches_u8), per patch the maximum, the sum and the count of the
 * candidates' own q, and the rejection of every patch without a pixel at T_c or with sum < M_c * count.  Integers only.
 * Sides <= 16384, h * w <= 2^31 - 2, 2 <= K <= 8; low / thresholds / min_confidence are HOST arrays uint16 [K] (entry 0 is not
 * read; low and thresholds in 1..65535, min_confidence 0 for "no filter").  Grids follow the pixel count, uncapped.
 *
 * dt_decide_candidates_u8: dt_decide_classes_u8 at `low`, which also writes q_own uint16 [n]: the q of the class the pixel
 *   took, 0 on class 0.  Every element of out_u8 and q_own is written.
 * dt_patch_support: labels int32 [h][w] (a value outside 1 .. h * w is background) and q_own -> planes indexed by root
 *   (label - 1), which the CALLER has zeroed: qmax int32 [h * w] (atomic max), qsum int64 [h * w] and area int32 [h * w]
 *   (atomic adds).  qsum and area: both or neither (NULL: never touched).  A wave takes dt_support_span consecutive 64-pixel
 *   chunks, reduces per run of equal labels, carries the open run in 64 bits, and a workgroup combines the runs its four
 *   waves end with before it writes them.  The planes do not depend on the order of arrival.
 * dt_reject_patches_u8: IN PLACE on classes uint8 [h][w]: a labelled pixel of class c becomes 0 unless
 *   qmax[label - 1] >= thresholds[c] and, where min_confidence[c] > 0, qsum[label - 1] >= (int64) min_confidence[c] *
 *   area[label - 1].  qsum / area NULL: min_confidence must be NULL or all zero.  Unlabelled pixels are not written. */
int dt_support_span(int* chunks);
int dt_decide_candidates_u8(const float* probs, const uint16_t* low, uint8_t* out_u8, uint16_t* q_own, int K, int64_t n,
                            void* stream);
int dt_patch_support(const int32_t* labels, const uint16_t* q_own, int h, int w, int32_t* qmax, int64_t* qsum, int32_t* area,
                     void* stream);
int dt_reject_patches_u8(uint8_t* classes, const int32_t* labels, const int32_t* qmax, const int64_t* qsum,
                         const int32_t* area, const uint16_t* thresholds, const uint16_t* min_confidence, int K, int h, int w,
                         void* stream);

/* Crown-level validation curves (deadtrees_amd/loss/objects.py states the contract): the candidates of a batch at the low
 * thresholds matched, patch by patch, to the target's crowns above an IoU of iou_p / iou_q >= 1/2, and one histogram entry per
 * predicted patch.  Integers only, no synchronisation, no sort; every grid follows the pixel count, uncapped.  The B images
 * lie in ONE plane uint8 / uint16 / int32 [ph][pw] of (H + 1) x (W + 1) cells, `cols` per row, image b in cell (b / cols,
 * b % cols): ph = ceil(B / cols) * (H + 1), pw >= cols * (W + 1), sides <= 16384, ph * pw <= 2^31 - 2.  Everything outside the
 * images is class 0, so dt_label_patches_u8, dt_patch_areas and dt_patch_support run on the plane as on one raster.
 *
 * dt_object_planes: q uint16 [B][K][H][W] (dt_prob_histogram's q_out), target int64 [B][H][W], low a HOST array uint16 [K]
 *   (entry 0 is not read, the others in 1..65535), any alignment.  Every element of cand, q_own and tcls is written: cand the
 *   class c >= 1 with the largest q_c among those with q_c >= low[c] (ties -> the smallest c; 0 without one), q_own that q
 *   (0 on class 0), tcls the target's class.  A label outside [0, K) sets err_flag[0] = 1 and is class 0.
 * dt_object_vote: labels_t / labels_p int32 [h][w] (a value outside 1 .. h * w is background), vote int64 [h * w] ZEROED BY
 *   THE CALLER: at a target root, (candidate << 32) | count of a majority summary of labels_p (0 included) over the target
 *   patch's pixels.  The candidate is the strict majority where there is one, whatever the order of arrival.
 * dt_object_inter: inter int32 [h * w], zeroed by the caller: at a target root += the pixels of the patch whose labels_p
 *   value is the candidate of vote.
 * dt_object_targets: targets int64 [K] += the target patches per class; matched uint8 [h * w], zeroed by the caller:
 *   matched[b] = 1 where the candidate b of a target patch a has a's class, area_p[b] >= min_pixels and
 *   inter * iou_q > iou_p * (area_t[a] + area_p[b] - inter) (64-bit).  1 <= iou_q <= 10^6, iou_q <= 2 iou_p < 2 iou_q.
 * dt_object_histogram: hist int64 [K][2][256][256] += 1 at [cand][matched][qmax >> 8][(qsum / area) >> 8] for every root of
 *   labels_p with area >= min_pixels (qmax, qsum, area: the planes of dt_patch_support). */
int dt_object_planes(const uint16_t* q, const int64_t* target, const uint16_t* low, int B, int K, int H, int W, int cols,
                     int ph, int pw, uint8_t* cand, uint16_t* q_own, uint8_t* tcls, int32_t* err_flag, void* stream);
int dt_object_vote(const int32_t* labels_t, const int32_t* labels_p, int h, int w, int64_t* vote, void* stream);
int dt_object_inter(const int32_t* labels_t, const int32_t* labels_p, const int64_t* vote, int h, int w, int32_t* inter,
                    void* stream);
int dt_object_targets(const int32_t* labels_t, const uint8_t* tcls, const uint8_t* cand, const int64_t* vote,
                      const int32_t* inter, const int32_t* area_t, const int32_t* area_p, int K, int h, int w,
                      int64_t min_pixels, int64_t iou_p, int64_t iou_q, int64_t* targets, uint8_t* matched, void* stream);
int dt_object_histogram(const int32_t* labels_p, const uint8_t* cand, const int32_t* qmax, const int64_t* qsum,
                        const int32_t* area, const uint8_t* matched, int K, int h, int w, int64_t min_pixels, int64_t* hist,
                        void* stream);

/* Training samples from an ortho raster (the array arithmetic of scripts/createdataset.py:53-194 and
 * scripts/computestats.py:111-161; deadtrees_amd/data/rasters.py states the contract in numpy).  rgbn_chw uint8 [4][h][w]
 * with 1 <= h, w <= S is the top-left corner of a zero [4][S][S] array; mask / lu uint8 [h][w] are padded the same way.
 * mask NULL: all zeros.  lu NULL: ones everywhere, the padded area included.  The array is cut into n = (S / t)^2 sub-tiles
 * of t x t, sub-tile i = by * (S / t) + bx at (by * t, bx * t); t % 32 == 0, S % t == 0, S <= 32768.  Source pointers may
 * have any byte alignment.
 * census (may be NULL) int64 [n][DT_CENSUS_COLS], overwritten, one row per sub-tile of the PADDED array: DT_CENSUS_DEAD the
 *   non-zero mask pixels; VMIN / VMAX over the four bands; B0MIN / B0MAX of band 0; MID the image bytes not in {0, 255};
 *   SUM + c / SUMSQ + c the sum and the sum of squares of the bytes of band c; the remaining columns are zero.
 * slot (may be NULL: census only) int32 [n] on the device: sub-tile i is written into row slot[i] of a pool of pool_rows
 *   rows in dt_pool_gather_batch's layout: images [.][t][t][4] interleaved, masks / lu_out [.][t][t] (all three 4-byte
 *   aligned), sums[.] = SUM + 0 .. SUM + 3 added up.  slot[i] < 0 or >= pool_rows writes nothing for sub-tile i; rows that no
 *   slot names are not touched; two sub-tiles must not name one row.  slot and census must not both be NULL.
 * Two launches (the preset of census and sums[], then the pass), integers only: exact and independent of how the work is
 * split; no floating point, no scratch memory, no synchronisation. */
#define DT_CENSUS_COLS 16
#define DT_CENSUS_DEAD 0
#define DT_CENSUS_VMIN 1
#define DT_CENSUS_VMAX 2
#define DT_CENSUS_B0MIN 3
#define DT_CENSUS_B0MAX 4
#define DT_CENSUS_MID 5
#define DT_CENSUS_SUM 6
#define DT_CENSUS_SUMSQ 10
int dt_raster_cut_u8(const uint8_t* rgbn_chw, const uint8_t* mask, const uint8_t* lu, int h, int w, int S, int t,
                     const int32_t* slot, int64_t pool_rows, uint8_t* images, uint8_t* masks, uint8_t* lu_out,
                     uint64_t* sums, int64_t* census, void* stream);

/* Masks and zones from polygons (data/polygons.py states the contract): exact all-touched rasterisation of polygons on a
 * fixed-point pixel grid of 1/256 pixel into out uint8 [h][w], every byte written; h, w in 1..16384; `out` may have any
 * byte alignment (a view into a larger buffer).  Pixel (i, j) is the square (256 j, 256 j + 256) x (256 i, 256 i + 256).
 * edges int32 [n_edges][4] = (ax, ay, bx, by), |coordinate| <= 2^23: every ring closed, every edge taken upwards (ay < by,
 *   or ay == by and ax < bx), zero-length segments left out; n_edges <= 0x7fff0000.
 * polys int32 [n_polys][8] = (minx, miny, maxx, maxy, e0, e1, value, 0): the bounding box of the polygon's vertices, its
 *   edges e0 .. e1 (all its rings: even-odd parity) and its value in 1..255.  Both tables 16-byte aligned.
 * A polygon burns a pixel iff the pixel's centre is inside it (crossing number of the ray to +x, half-open rule ay <= cy <
 * by, side from the sign of the exact cross product) or, with all_touched != 0, one of its edges meets the pixel's open
 * square (bounding boxes strictly overlap in x and y, and the four corners' cross products against the edge have min < 0 <
 * max).  A pixel gets the minimum value among the polygons that burn it, 0 if none does.
 * One launch, integers only, no atomics, no scratch memory, no capacity limit (polygons per tile and edges per polygon
 * stream through LDS in chunks), no synchronisation: the map is a pure function of the tables. */
int dt_rasterize_polygons_u8(const int32_t* edges, int64_t n_edges, const int32_t* polys, int n_polys, int h, int w,
                             int all_touched, uint8_t* out, void* stream);

/* Signed Euclidean distance maps of the boundary loss, computed on the device in place of the
 * loader's scipy pass: data/deadtreedata.py:182-185 -> loss/losses.py:159-178 one_hot2dist(resolution=[1,1]).
 * labels int64 [B,H,W] -> dist fp32 [B,K,H,W]; per class: floor(edt to the class) outside it, 1 - floor(edt to the
 * outside) inside it, all zero when the class is absent (the int32 truncation of the reference included).
 * Exact integer arithmetic: bit-identical to the reference.  workspace: dt_signed_distmap_workspace() BYTES.
 * Labels outside [0,K) set err_flag[0] (the assert of losses.py:129). */
int64_t dt_signed_distmap_workspace(int B, int K, int H, int W);
int dt_signed_distmap(const int64_t* labels, float* dist, void* workspace, int32_t* err_flag, int B, int K, int H,
                      int W, void* stream);

/* ------------------------------------------------------------------ bf16 storage / fp32 accumulate (inference leg)
 * BASELINE configs[2] precision: activations NHWC bf16, weights [tap][Cout][Cin] bf16 (dt_pack_weights_bf16),
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulators, one rounding at the store.  Same descriptor semantics as
 * dt_conv2d (mode0 0/1/2, concat, split outputs, accumulate, BatchNorm partial statistics from the fp32
 * accumulators, fused input BatchNorm-apply + ReLU). */
int dt_conv2d_bf16_stat_rows(const dt_conv_desc* d);
/* The kernel dt_conv2d_bf16 runs for `d`.  row_tiles names the family:
 *    2  register-staged tiles of 256 pixels x tile_n channels, tile_w wide, chunk_k channels per chunk (and the stem);
 *    4  register-staged tiles of 512 pixels (tile_w 32, tile_n 64, chunk_k 16);
 *    8  the LDS-DMA staged kernel (512 pixels x 64 channels): reads the CHUNKED weight images, see dt_weight_images;
 *   16  the lean persistent kernel of the narrow full-resolution layers (Cin, Cout in {16, 32}).
 * For 8 and 16 the other three values describe that kernel's fixed tile and select nothing. */
int dt_conv2d_bf16_config(const dt_conv_desc* d, int* tile_w, int* tile_n, int* chunk_k, int* row_tiles);  /* conv_fwd_bf16_kernel<k,s,tw,tn,tf> */
int dt_conv2d_bf16(const dt_conv_desc* d, const void* src0, const void* src1, const void* w_bf16, void* out,
                   void* out1, float* stats, const float* in_scale, const float* in_shift, void* stream);
int dt_pack_weights_bf16(const float* w_hwio, void* out_bf16, int ksize, int Cin, int Cout, void* stream);
/* weights of the bf16 data-gradient convolution ([tap'][Cin][Cout] = HWIO with the taps reversed) */
int dt_pack_dgrad_weights_bf16(const float* w_hwio, void* out_bf16, int ksize, int Cin, int Cout, void* stream);
/* fp32 dW[kh][kw][ci][co] from bf16 x (same virtual-input modes as dt_conv2d_wgrad) and bf16 dy; operands are
 * transposed out of the pixel-major LDS tiles by ds_read_b64_tr_b16; split-K slabs reduced in fixed order. */
size_t dt_conv2d_wgrad_bf16_workspace(const dt_conv_desc* d);
int dt_conv2d_wgrad_bf16(const dt_conv_desc* d, const void* src0, const void* src1, const void* dy, float* dw_hwio,
                         float* workspace, size_t workspace_bytes, const float* in_scale, const float* in_shift,
                         void* stream);
/* out(bf16) = act(y*scale+shift + res'), y fp32 (y_is_f32) or bf16, res bf16 (optional affine); relu: 0 none, 1 ReLU after
 * the sum, 2 ReLU on the main branch only — relu(y*scale+shift) + res' (ResUnet decoder block, like dt_bn_act) */
int dt_bn_act_bf16(const void* y, int y_is_f32, const float* scale, const float* shift, const void* res,
                   const float* rscale, const float* rshift, void* out, int64_t n_pix, int C, int relu, void* stream);
int dt_maxpool3x3s2_bf16(const void* x, void* out, int B, int H, int W, int C, void* stream);
/* fp32 conv (dt_conv2d semantics, no split/accumulate/concat) storing its output as bf16 — the 7x7 stem of the
 * bf16 path keeps fp32 operands (K = 147) but feeds bf16 activations; statistics from the fp32 accumulators. */
int dt_conv2d_out_bf16(const dt_conv_desc* d, const float* src0, const float* w_hwio, void* out_bf16, float* stats,
                       void* stream);
/* stem weight gradient with the bf16 dy of the bf16 path (x fp32 image, dW fp32) */
int dt_conv2d_wgrad_stem_dy_bf16(const dt_conv_desc* d, const float* src0, const void* dy_bf16, float* dw_hwio,
                                 float* workspace, size_t workspace_bytes, void* stream);
/* head with bf16 decoder activations in (forward) / bf16 activation gradient out (backward); weights, logits,
 * dlogits and parameter gradients stay fp32 */
int dt_head_fwd_bf16(const void* x_bf16, const float* w_ohwi, const float* bias, float* logits_nchw,
                     int64_t* argmax_i64, uint8_t* argmax_u8, int B, int H, int W, int Cin, int K, void* stream);
int dt_head_bwd_bf16(const void* x_bf16, const float* w_ohwi, const float* dlogits_nchw, void* dx_bf16, float* red,
                     int B, int H, int W, int Cin, int K, void* stream);
int dt_bf16_to_f32(const void* x, float* out, int64_t n, void* stream);
int dt_f32_to_bf16(const float* x, void* out, int64_t n, void* stream);
/* bf16 training passes: same contracts as their fp32 namesakes, tensors bf16, sums fp32/fp64.  `red` holds
 * dt_bn_stats_floats(dt_bn_bwd_rows_bf16(n_pix), C) floats. */
int dt_bn_bwd_rows_bf16(int64_t n_pix);
int dt_bn_bwd_reduce_bf16(const void* dout, const void* out_act, const void* y, const float* mean,
                          const float* invstd, const float* act_scale, const float* act_shift, float* red,
                          int64_t n_pix, int C, void* stream);
int dt_bn_bwd_apply_bf16(const void* dout, const void* out_act, const void* y, const float* mean, const float* invstd,
                         const float* gamma, const float* act_scale, const float* act_shift, float* red, int P,
                         float* dgamma, float* dbeta, void* dy, void* dres, int dres_accumulate, int64_t n_pix, int C,
                         void* stream);
int dt_maxpool3x3s2_bf16_amax(const void* x, void* out, uint8_t* argmax, int B, int H, int W, int C, void* stream);
int dt_maxpool3x3s2_bwd_bf16(const void* dout, const uint8_t* argmax, void* dx, int accumulate, int B, int H, int W,
                             int C, void* stream);
int dt_upsample2x_bwd_bf16(const void* dup, void* dx, int B, int H, int W, int C, void* stream);
/* the same with accumulate != 0: dx = bf16(dx + sums) — a node of the Unet++ dense decoder collects several consumers */
int dt_upsample2x_bwd_acc_bf16(const void* dup, void* dx, int accumulate, int B, int H, int W, int C, void* stream);
/* bf16 twin of dt_channel_slice (channel counts and offset multiples of 8): torch.cat of the dense skip connections of
 * smp UnetPlusPlusDecoder.forward under AMP and its backward; the accumulating form adds in fp32 and rounds once */
int dt_channel_slice_bf16(const void* src, void* dst, int64_t n_pix, int C_narrow, int C_wide, int offset, int to_wide,
                          int accumulate, void* stream);

/* Every weight image of a network in one launch, table-driven over the flat parameter buffer: table int32
 * [n_layers][5] = (w_off, taps, Cin, Cout, first_tile) on the DEVICE, first_tile = running sum of
 * taps*ceil(Cin/32)*ceil(Cout/32); total_tiles = that sum over all layers.  The image of layer l lands at out + w_off
 * (in elements of the output type).  mode 0 = dt_weight_flip_transpose (fp32), 1 = dt_pack_weights_bf16,
 * 2 = dt_pack_dgrad_weights_bf16; 3 / 4 = the forward / data-gradient bf16 images in the chunked layout
 * [tap][K/32][N][32] that the LDS-DMA staged kernels read (dt_conv2d_bf16_config reports them with
 * row_tiles 8: pass THAT image to such a launch); layers with K or N not a multiple of 32 are skipped. */
int dt_weight_images(const float* params, void* out, const int32_t* table, int n_layers, int total_tiles, int mode,
                     void* stream);
/* modes 1 - 4 (the four bf16 images of a bf16 training step: forward / data-gradient, plain / chunked for the LDS-DMA
 * kernels) from one read of the parameters, each into its own n_params-element buffer */
int dt_weight_images_bf16_all(const float* params, void* fwd, void* dgrad, void* fwd_chunked, void* dgrad_chunked,
                              const int32_t* table, int n_layers, int total_tiles, void* stream);

/* The 7x7 / stride-2 stem on the bf16 convolution kernels (smp encoder conv1, reached from network/segmodel.py:214):
 * dt_stem_s2d_bf16 turns the fp32 NHWC image [B,H,W,Cin<=4] into its 2x2 space-to-depth form [B,H/2,W/2,16] bf16
 * (channel (a*2+b)*4 + c, unused channels zero), dt_stem_pack_weights_bf16 the HWIO 7x7 weights into the matching
 * [16 taps][Cout][16] image; dt_conv2d_bf16 with ksize = 4, stride 1, pad = 2 (C0 = 16, Ho = Hin, Wo = Win,
 * Cout %% 64 == 0) is then exactly the 7x7/2 convolution on bf16-rounded operands. */
int dt_stem_s2d_bf16(const float* x_nhwc, void* out_bf16, int B, int H, int W, int Cin, void* stream);
int dt_stem_pack_weights_bf16(const float* w_hwio_7x7, void* out_bf16, int Cin, int Cout, void* stream);
/* weight gradient of the stem in that form: dt_conv2d_wgrad_bf16 with ksize = 4 (C0 = 16, pad 2) gives
 * dw4 fp32 [16 taps][16][Cout]; dt_stem_unpack_wgrad gathers it into the HWIO 7x7 gradient [7][7][Cin][Cout]. */
int dt_stem_unpack_wgrad(const float* dw4, float* dw_hwio_7x7, int Cin, int Cout, void* stream);

/* bf16 twin of dt_conv2d_bn_bwd: fuse->y points at the bf16 raw output of the BatchNorm layer (cast to const
 * float*); the sums use the rounded bf16 gradient and the mask of bf16(y*scale+shift), like dt_bn_bwd_reduce_bf16.
 * P = dt_conv2d_bf16_stat_rows(desc). */
int dt_conv2d_bf16_bn_bwd(const dt_conv_desc* desc, const void* src0, const void* w_bf16, void* out, float* red,
                          const dt_bn_bwd_fuse* fuse, void* stream);

/* bf16: data gradient of y = conv3x3(nearest_upsample_x2(x)) for the narrow decoder layer in ONE launch: `desc`, dy and
 * w_bf16 as for dt_conv2d_bf16_bn_bwd (the full-resolution data-gradient form, plain store); the 2x2 sums of the
 * up-sampling's backward are taken on the fp32 accumulators, gx [B, Ho/2, Wo/2, Cout] (bf16) is stored and red
 * [2][P][Cout], P = dt_conv2d_bf16_stat_rows(desc), receives the BatchNorm-backward sums of the layer that produced x
 * (fuse: its bf16 raw output at gx's resolution, mean, invstd, act_scale / act_shift) like dt_upsample2x_bwd_bn_bf16
 * — which it replaces together with the full-resolution dt_conv2d_bf16 launch (reference: autograd of
 * F.interpolate(nearest, x2) + Conv2d under AMP, smp unet/decoder.py DecoderBlock.forward via segmodel.py:30-57). */
int dt_conv2d_bf16_upsampled_dgrad_supported(const dt_conv_desc* desc);
int dt_conv2d_bf16_upsampled_dgrad(const dt_conv_desc* desc, const void* dy, const void* w_bf16, void* gx, float* red,
                                   const dt_bn_bwd_fuse* fuse, void* stream);

/* Max-pool 3x3 / 2 backward (dt_maxpool3x3s2_bwd / _bf16) with the BatchNorm-backward sums of the layer whose (virtual)
 * activation was pooled — the stem — taken from the gradient the pass writes (after the optional join with the skip
 * gradient already in dx): red[2][P][C], P = dt_maxpool3x3s2_bwd_bn[_bf16]_rows(...) (0: odd map or channel count not
 * covered — use the plain pass + dt_bn_bwd_reduce), -> dt_bn_bwd_apply.  bf16: sums from the rounded gradient and the mask
 * of bf16(y * scale + shift), like dt_bn_bwd_reduce_bf16. */
int dt_maxpool3x3s2_bwd_bn_rows(int B, int H, int W, int C);
int dt_maxpool3x3s2_bwd_bn(const float* dout, const uint8_t* argmax, float* dx, int accumulate, const dt_bn_bwd_fuse* fuse,
                           float* red, int B, int H, int W, int C, void* stream);
int dt_maxpool3x3s2_bwd_bn_bf16_rows(int B, int H, int W, int C);
int dt_maxpool3x3s2_bwd_bn_bf16(const void* dout, const uint8_t* argmax, void* dx, int accumulate, const dt_bn_bwd_fuse* fuse,
                                float* red, int B, int H, int W, int C, void* stream);

/* Nearest x2 upsample backward (2x2 sums, like dt_upsample2x_bwd) with the BatchNorm-backward reduction of the layer
 * whose (virtual) activation was upsampled fused in: dx[B,H,W,C] is that layer's output gradient, fuse->y its raw
 * output; red[2][P][C], P = dt_upsample2x_bwd_bn_rows(...), holds dt_bn_stats_floats(P, C) floats -> dt_bn_bwd_apply.
 * The _bf16 twins take bf16 tensors (fuse->y bf16) and follow dt_bn_bwd_reduce_bf16's arithmetic. */
int dt_upsample2x_bwd_bn_rows(int B, int H, int W, int C);
int dt_upsample2x_bwd_bn(const float* dup, float* dx, const dt_bn_bwd_fuse* fuse, float* red, int B, int H, int W, int C,
                         void* stream);
/* Data gradient of y = conv3x3(nearest_upsample_x2(x)) in ONE kernel (sub-pixel form: a 4x4 stride-2 convolution over
 * dY with 16 combined weight matrices, 16 tap products per source pixel instead of 36): replaces the chain
 * dt_conv2d (data-gradient form) -> dt_upsample2x_bwd(_bn) for the narrow decoder layer without a skip (reference:
 * autograd of F.interpolate(x, scale_factor=2, mode="nearest") + Conv2d, deadtrees/network/segmodel.py:30-57 via
 * segmentation_models_pytorch 0.2.1 unet/decoder.py DecoderBlock.forward).  `desc` describes the FORWARD convolution
 * (mode0 = 1, C0 = channels of x, Cout); w_hwio the forward weights; gx[B, Hin/2, Win/2, C0].  With `fuse` (y, mean,
 * invstd, act_scale, act_shift of the layer that produced x) red[2][P][C0], P = dt_conv2d_upsampled_dgrad_rows(desc),
 * receives the BatchNorm-backward sums like dt_upsample2x_bwd_bn; fuse = NULL: plain gradient. */
int dt_conv2d_upsampled_dgrad_supported(const dt_conv_desc* desc);
int dt_conv2d_upsampled_dgrad_rows(const dt_conv_desc* desc);
int dt_conv2d_upsampled_dgrad(const dt_conv_desc* desc, const float* dy, const float* w_hwio, float* gx, float* red,
                              const dt_bn_bwd_fuse* fuse, void* stream);
int dt_upsample2x_bwd_bn_bf16_rows(int B, int H, int W, int C);
int dt_upsample2x_bwd_bn_bf16(const void* dup, void* dx, const dt_bn_bwd_fuse* fuse, float* red, int B, int H, int W,
                              int C, void* stream);

/* ------------------------------------------------------------------ optimiser (K22) */
/* sum of squares of g[n] -> partial[rows]; rows = dt_sumsq_rows(n) */
int dt_sumsq_rows(int64_t n);
int dt_sumsq(const float* g, int64_t n, double* partial, void* stream);
/* norm[0] = sqrt(sum partial) ; clipcoef[0] = min(1, max_norm/(norm+1e-6)) * gscale  (clip_grad_norm_).
 * skip_flag (may be NULL): set to 1 when the norm is NaN/Inf — a non-finite gradient must not reach Adam's moments even
 * when the loss itself stayed finite (the reference's Lightning loop would have seen the NaN loss of the next step;
 * here the update is dropped like a non-finite loss, segmodel.py:220-222).  Never cleared here. */
int dt_clip_coef(const double* partial, int rows, float max_norm, float gscale, float* norm, float* clipcoef,
                 int32_t* skip_flag, void* stream);
/* torch.optim.Adam step on a flat buffer (segmodel.py:420-425): g' = g*clipcoef[0];
 * skipped entirely when skip_flag[0] != 0 (non-finite loss: segmodel.py:220-222). */
int dt_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                 float eps, float bias_c1, float bias_c2, const float* clipcoef, const int32_t* skip_flag,
                 void* stream);
/* skip_flag[0] = !isfinite(loss[0])  (segmodel.py:220-222: training_step returns None) */
int dt_skip_from_loss(const float* loss, int32_t* skip_flag, void* stream);
/* device-resident step count: t += (skip ? 0 : 1); hyper[3] = (lr_dev[0], 1 - beta1^t, 1 - beta2^t) for
 * dt_adam_step_dev — a skipped step does not advance the bias correction (torch.optim.Adam is not called then).
 * The betas travel as doubles: torch computes 1 - beta^t in Python doubles ((double)(float)0.999 is off by 1.3e-8). */
int dt_adam_advance(double* t_dev, const int32_t* skip_flag, const double* lr_dev, double beta1, double beta2,
                    float* hyper, void* stream);
/* the same step with the per-step scalars on the device: hyper fp32 [3] = (lr, 1 - beta1^t, 1 - beta2^t), so a
 * training step captured in a HIP graph replays with the current learning rate and bias corrections. */
int dt_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, double beta1,
                     double beta2, float eps, const float* clipcoef, const int32_t* skip_flag, void* stream);
/* The same over the TRAINABLE ranges of the flat buffer only (frozen encoder; torch.optim.Adam skips a parameter whose
 * .grad is None and clip_grad_norm_ sees only parameters with a gradient).  table: device int64 [4 * nranges] of
 * (lo, hi, first partial row, segment); lo and hi multiples of 4; the rows of range r are
 * dt_sumsq_rows(hi - lo) starting at its first row, `rows` their total (dt_clip_coef reads partial[rows]).  Each range
 * carries its own step count t_seg[segment] and bias corrections hyper_seg[3 * segment ..]; frozen ranges are neither
 * read nor written.  Everything stays on the device (capturable); the skip flag keeps its global meaning. */
int dt_sumsq_ranges(const float* g, const int64_t* table, int nranges, int rows, double* partial, void* stream);
int dt_adam_advance_ranges(double* t_seg, const int64_t* table, int nranges, const int32_t* skip_flag,
                           const double* lr_dev, double beta1, double beta2, float* hyper_seg, void* stream);
int dt_adam_step_ranges(float* p, const float* g, float* m, float* v, const int64_t* table, int nranges, int64_t max_len,
                        const float* hyper_seg, double beta1, double beta2, float eps, const float* clipcoef,
                        const int32_t* skip_flag, void* stream);

/* Averaged copy of the flat parameter buffer (torch.optim.swa_utils.AveragedModel).  count_dev (int64[1], device) is
 * the number of models averaged so far; it is advanced ON the device and the pass that follows reads it:
 *   DT_AVG_SWA: avg = (count == 0) ? p : avg + (p - avg) / (count + 1)           (get_swa_multi_avg_fn)
 *   DT_AVG_EMA: avg = (count == 0) ? p : avg + (p - avg) * (1 - decay)           (get_ema_multi_avg_fn)
 * A set skip_flag (int32[1], as written by dt_clip_coef / dt_skip_from_loss; may be NULL) leaves avg AND the count
 * untouched.  No host-side value changes between calls: capturable in a HIP graph.  avg, p: 16-byte aligned, n floats. */
#define DT_AVG_SWA 0
#define DT_AVG_EMA 1
int dt_weight_average(float* avg, const float* p, int64_t n, int64_t* count_dev, const int32_t* skip_flag, int mode,
                      double decay, void* stream);
/* Cumulative moving average of BatchNorm statistics (torch: momentum=None): n_dev += 1, momentum_dev = 1 / n_dev.
 * dt_bn_finalize_dev reads that momentum from the device. */
int dt_cma_advance(int64_t* n_dev, float* momentum_dev, void* stream);

/* ------------------------------------------------------------------ inverted-residual block (EfficientUnet++ decoder), inference
 * Reference: network/extra/efficientunetplusplus/decoder.py InvertedResidual — ATen chain conv2d(1x1) -> batch_norm(eval)
 * -> hardswish_ -> conv2d(3x3, groups=C) -> batch_norm -> hardswish_ -> scSE (adaptive_avg_pool2d, two 1x1 conv2d, relu_,
 * sigmoid; 1x1 conv2d C -> 1, sigmoid; x * cSE + x * sSE) -> conv2d(1x1) -> batch_norm, plus x or batch_norm(conv2d(1x1, x)).
 * Everything NHWC fp32.  A block is pwconv -> dwconv -> gates -> [pwconv: skip projection] -> pwconv(gate, res).
 *
 * Pointwise convolution as a GEMM over pixels:  out[p,n] = act(sum_k a[p,k] w[k,n] * scale[n] + shift[n]) + res[p,n]
 *   a = the virtual input cat(src0', src1) of [B,H,W,C0+C1]: src0' = src0 [B,H,W,C0] (up0 = 0) or the nearest x2
 *       up-sampling of src0 [B,(H+1)/2,(W+1)/2,C0] (up0 = 1); src1 [B,H,W,C1] or NULL with C1 = 0;
 *       with gates (both or neither): a[p,k] *= gate_c[b,k] + sigmoid(gate_s[p]), gate_c [B,C0+C1], gate_s [B,H,W]
 *   w_io [C0+C1][Cout]; scale / shift [Cout]: eval BatchNorm with the convolution's bias folded in
 *   act 0 none, 1 Hardswish; res optional, layout of out, may alias out.  C0, C1, Cout multiples of 16.
 * One fixed-order sum per output element: a pixel's result does not depend on the batch it arrives in. */
int dt_pwconv_affine(const float* src0, const float* src1, const float* w_io, float* out, const float* scale,
                     const float* shift, const float* gate_c, const float* gate_s, const float* res, int B, int H, int W,
                     int C0, int C1, int up0, int Cout, int act, void* stream);
/* Depthwise 3x3, stride 1, pad 1:  out = hardswish(dw(x) * scale[c] + shift[c]), x / out [B,H,W,C], w_tc [9][C].  The same
 * pass writes the sSE logits s[p] = sse_w . out[p,:] + sse_b[0] ([B,H,W]) and, per workgroup, one row of channel sums of out:
 * part [B][P][C], P = dt_dwconv3x3_rows(H, W) — fixed order, no float atomics.  C a multiple of 16, at most 1536. */
int dt_dwconv3x3_rows(int H, int W);
int dt_dwconv3x3_affine(const float* x, const float* w_tc, const float* scale, const float* shift, const float* sse_w,
                        const float* sse_b, float* out, float* s, float* part, int B, int H, int W, int C, void* stream);
/* cSE gate: mean[b,c] = (sum of the P rows of image b, in one order) / HW;
 * gc [B,C] = sigmoid(W2 relu(W1 mean + b1) + b2), w1_io [C][Ch], w2_io [Ch][C], Ch = C / squeeze_ratio.  One launch. */
int dt_scse_gates(const float* part, const float* w1_io, const float* b1, const float* w2_io, const float* b2, float* gc,
                  int B, int P, int C, int Ch, int HW, void* stream);
/* dt_bn_eval_affine behind a convolution WITH bias: shift = beta - mean * scale + scale * bias */
int dt_bn_eval_affine_bias(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                           const float* bias, float eps, int C, float* scale, float* shift, void* stream);

/* ------------------------------------------------------------------ library options */
/* Kernel-selection switches (host side, process wide; every choice computes the same values):
 *   "bf16_dma": 0 = register-staged bf16 convolutions only, 1 (default) = the LDS-DMA staged 512-pixel kernel where
 *               its tiles fill the chip, 2 = wherever its shape conditions hold.  Also read from the environment
 *               variable DT_BF16_DMA at first use. */
int dt_set_option(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* DEADTREES_HIP_H */
