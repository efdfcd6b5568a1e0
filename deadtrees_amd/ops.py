"""Thin tensor-level wrappers over the C ABI (one python function per ``dt_*`` entry point).

Every function takes/returns torch HIP tensors, validates nothing beyond what the C side validates,
and raises RuntimeError when the library reports an error.  Used by the engine-independent callers
(tiled inference, optimiser) and by the parity tests, which therefore exercise the C ABI itself.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import ptr as _p, stream as _st


def _gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("deadtrees_amd ops need HIP device tensors (no CPU fallback)")


def conv_desc(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad, split=0, acc=0):
    Ho = (Hin + 2 * pad - k) // stride + 1
    Wo = (Win + 2 * pad - k) // stride + 1
    return _lib.ConvDesc(B, Hin, Win, C0, C1, mode0, Ho, Wo, Cout, k, stride, pad, split, acc)


# ---- what the convolution wrappers of the three families (fp32 direct, Winograd, bf16) share
def _src_desc(src0, src1, mode0, Cout, k, stride, pad, split=0, accumulate=False):
    """descriptor of a convolution over the virtual input (src0 up-sampled x2 / zero-inserted for mode0 1 / 2) | src1"""
    B, H, W, C0 = src0.shape
    if mode0 != 0:
        H, W = 2 * H, 2 * W
    C1 = 0 if src1 is None else src1.shape[-1]
    return conv_desc(B, H, W, C0, C1, mode0, Cout, k, stride, pad, split, 1 if accumulate else 0)


def _split_outputs(d, split, out0, out1, dtype, device):
    """the outputs the caller did not bring: out0 (the first `split` channels, or all), out1 (the rest of a split)"""
    if out0 is None:
        out0 = torch.empty((d.B, d.Ho, d.Wo, split if split else d.Cout), dtype=dtype, device=device)
    if split and out1 is None:
        out1 = torch.empty((d.B, d.Ho, d.Wo, d.Cout - split), dtype=dtype, device=device)
    return out0, out1


def _rows_buffer(P, Cc, device):
    """BatchNorm partial-sum buffer (statistics or `red`) for the answer P of a rows query -> (the buffer the ABI takes,
    its [2, P, Cc] view); a refused query (P <= 0) raises the library's message"""
    lib = _lib.load()
    if P <= 0:
        raise RuntimeError(lib.dt_last_error().decode())
    buf = torch.empty(lib.dt_bn_stats_floats(P, Cc), dtype=torch.float32, device=device)
    return buf, buf[:2 * P * Cc].view(2, P, Cc)


def _wgrad(entry, d, src0, src1, dy, dw, in_scale=None, in_shift=None, what=None):
    """weight gradient `entry` (the entry points share one signature) into dw, on a workspace of `<entry>_workspace`
    bytes; a refused workspace query (0) raises the library's message"""
    lib = _lib.load()
    nbytes = getattr(lib, entry + "_workspace")(C.byref(d))
    if nbytes <= 0:
        raise RuntimeError(lib.dt_last_error().decode())
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device)
    _lib.check(getattr(lib, entry)(C.byref(d), _p(src0), _p(src1), _p(dy.contiguous()), _p(dw), _p(ws), nbytes,
                                   _p(in_scale), _p(in_shift), _st()), what or entry)
    return dw


def _bn_bwd_setup(rows_query, src0, Cout, dtype, y, mean, invstd, act_scale, act_shift, act, join_into):
    """what the *_bn_bwd wrappers prepare: descriptor of the plain 3x3 data gradient (a join when join_into is given),
    output, `red` buffer and its view, fuse block"""
    B, H, W, C0 = src0.shape
    d = conv_desc(B, H, W, C0, 0, 0, Cout, 3, 1, 1, 0, 1 if join_into is not None else 0)
    red, red_view = _rows_buffer(rows_query(C.byref(d)), Cout, src0.device)
    out = join_into if join_into is not None else torch.empty((B, H, W, Cout), dtype=dtype, device=src0.device)
    fuse = _lib.BnBwdFuse(_p(y.contiguous()), _p(mean), _p(invstd), _p(act_scale), _p(act_shift), _p(act))
    return d, out, red, red_view, fuse


def conv2d(src0, w_hwio, k, stride, pad, src1=None, mode0=0, split=0, out0=None, out1=None, accumulate=False,
           want_stats=False, in_scale=None, in_shift=None):
    """NHWC conv through dt_conv2d.  Returns (out0, out1, stats[2,P,Cout] or None)."""
    _gpu(src0, src1, w_hwio)
    lib = _lib.load()
    Cout = w_hwio.shape[-1]
    d = _src_desc(src0, src1, mode0, Cout, k, stride, pad, split, accumulate)
    out0, out1 = _split_outputs(d, split, out0, out1, torch.float32, src0.device)
    buf, stats = _rows_buffer(lib.dt_conv2d_stat_rows(C.byref(d)), Cout, src0.device) if want_stats else (None, None)
    _lib.check(lib.dt_conv2d(C.byref(d), _p(src0), _p(src1), _p(w_hwio.contiguous()), _p(out0), _p(out1), _p(buf),
                             _p(in_scale), _p(in_shift), _st()), "dt_conv2d")
    return out0, out1, stats


def conv2d_affine(src0, w_hwio, k, stride, pad, scale, shift, relu=True, src1=None, mode0=0):
    """inference form through dt_conv2d_affine: [relu](conv(x) * scale + shift) in one launch (eval-mode BatchNorm folded
    into per-channel scale / shift) -> NHWC activation"""
    _gpu(src0, src1, w_hwio, scale, shift)
    d = _src_desc(src0, src1, mode0, w_hwio.shape[-1], k, stride, pad)
    out = torch.empty((d.B, d.Ho, d.Wo, d.Cout), dtype=torch.float32, device=src0.device)
    _lib.check(_lib.load().dt_conv2d_affine(C.byref(d), _p(src0), _p(src1), _p(w_hwio.contiguous()), _p(out), _p(scale),
                                            _p(shift), 1 if relu else 0, _st()), "dt_conv2d_affine")
    return out


def conv2d_wgrad_winograd(src0, dy, src1=None, mode0=0, in_scale=None, in_shift=None):
    """3x3 stride-1 pad-1 weight gradient through dt_conv2d_wgrad_winograd -> dw HWIO"""
    _gpu(src0, src1, dy)
    d = _src_desc(src0, src1, mode0, dy.shape[-1], 3, 1, 1)
    if not _lib.load().dt_conv2d_wgrad_winograd_supported(C.byref(d)):
        raise ValueError("layer shape not supported by the Winograd weight-gradient kernel")
    dw = torch.empty((3, 3, d.C0 + d.C1, d.Cout), dtype=torch.float32, device=dy.device)
    return _wgrad("dt_conv2d_wgrad_winograd", d, src0, src1, dy, dw, in_scale, in_shift)


def winograd_weights(w_hwio):
    """U = G g G^T of a 3x3 HWIO weight in the Winograd kernel's image order [16][Cin/8][2][Cout][4]."""
    _gpu(w_hwio)
    k, _, cin, cout = w_hwio.shape
    assert k == 3
    u = torch.empty((16, cin // 8, 2, cout, 4), dtype=torch.float32, device=w_hwio.device)
    _lib.check(_lib.load().dt_winograd_weights(_p(w_hwio.contiguous()), _p(u), cin, cout, _st()), "dt_winograd_weights")
    return u


def conv2d_winograd(src0, u, src1=None, mode0=0, split=0, out0=None, out1=None, accumulate=False, want_stats=False,
                    in_scale=None, in_shift=None):
    """3x3 stride-1 pad-1 NHWC conv through dt_conv2d_winograd.  Returns (out0, out1, stats[2,P,Cout] or None)."""
    _gpu(src0, src1, u)
    lib = _lib.load()
    Cout = u.shape[3]
    d = _src_desc(src0, src1, mode0, Cout, 3, 1, 1, split, accumulate)
    if not lib.dt_conv2d_winograd_supported(C.byref(d)):
        raise ValueError("layer shape not supported by the Winograd kernel")
    out0, out1 = _split_outputs(d, split, out0, out1, torch.float32, src0.device)
    buf, stats = _rows_buffer(lib.dt_conv2d_winograd_stat_rows(C.byref(d)), Cout, src0.device) if want_stats else (None, None)
    _lib.check(lib.dt_conv2d_winograd(C.byref(d), _p(src0), _p(src1), _p(u), _p(out0), _p(out1), _p(buf),
                                      _p(in_scale), _p(in_shift), _st()), "dt_conv2d_winograd")
    return out0, out1, stats


def weight_flip_transpose(w_hwio):
    _gpu(w_hwio)
    k, _, cin, cout = w_hwio.shape
    wd = torch.empty((k, k, cout, cin), dtype=torch.float32, device=w_hwio.device)
    _lib.check(_lib.load().dt_weight_flip_transpose(_p(w_hwio.contiguous()), _p(wd), k, cin, cout, _st()),
               "dt_weight_flip_transpose")
    return wd


def conv2d_wgrad(src0, dy, k, stride, pad, src1=None, mode0=0, in_scale=None, in_shift=None):
    _gpu(src0, src1, dy)
    d = _src_desc(src0, src1, mode0, dy.shape[-1], k, stride, pad)
    assert (d.Ho, d.Wo) == (dy.shape[1], dy.shape[2]), ((d.Ho, d.Wo), dy.shape)
    dw = torch.empty((k, k, d.C0 + d.C1, d.Cout), dtype=torch.float32, device=dy.device)
    return _wgrad("dt_conv2d_wgrad", d, src0, src1, dy, dw, in_scale, in_shift)


def bn_finalize(stats, count, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    _gpu(stats, gamma, beta)
    _, P, Cc = stats.shape
    dev = stats.device
    full = torch.empty(_lib.load().dt_bn_stats_floats(P, Cc), dtype=torch.float32, device=dev)
    full[:2 * P * Cc] = stats.reshape(-1)
    stats = full
    mean, invstd, scale, shift = (torch.empty(Cc, dtype=torch.float32, device=dev) for _ in range(4))
    _lib.check(_lib.load().dt_bn_finalize(_p(stats), P, Cc, float(count), _p(gamma), _p(beta), eps, momentum,
                                          _p(running_mean), _p(running_var), _p(mean), _p(invstd), _p(scale),
                                          _p(shift), _st()), "dt_bn_finalize")
    return mean, invstd, scale, shift


def bn_finalize_dev(stats, count, gamma, beta, running_mean, running_var, momentum_dev, eps=1e-5):
    """``bn_finalize`` with the momentum read from the device tensor float32[1] when the kernel runs"""
    _gpu(stats, gamma, beta, running_mean, running_var, momentum_dev)
    if momentum_dev.dtype != torch.float32:
        raise RuntimeError("bn_finalize_dev: the momentum is a float32 device tensor")
    _, P, Cc = stats.shape
    dev = stats.device
    full = torch.empty(_lib.load().dt_bn_stats_floats(P, Cc), dtype=torch.float32, device=dev)
    full[:2 * P * Cc] = stats.reshape(-1)
    mean, invstd, scale, shift = (torch.empty(Cc, dtype=torch.float32, device=dev) for _ in range(4))
    _lib.check(_lib.load().dt_bn_finalize_dev(_p(full), P, Cc, float(count), _p(gamma), _p(beta), eps, _p(momentum_dev),
                                              _p(running_mean), _p(running_var), _p(mean), _p(invstd), _p(scale),
                                              _p(shift), _st()), "dt_bn_finalize_dev")
    return mean, invstd, scale, shift


def cma_advance(n_dev, momentum_dev):
    """n_dev (int64[1]) += 1; momentum_dev (float32[1]) = 1 / n_dev — the cumulative-average momentum of BatchNorm"""
    _gpu(n_dev, momentum_dev)
    if n_dev.dtype != torch.int64 or momentum_dev.dtype != torch.float32:
        raise RuntimeError("cma_advance: int64 count and float32 momentum")
    _lib.check(_lib.load().dt_cma_advance(_p(n_dev), _p(momentum_dev), _st()), "dt_cma_advance")


AVG_MODES = {"swa": 0, "ema": 1}      # DT_AVG_SWA / DT_AVG_EMA


def weight_average(avg, p, count_dev, mode="swa", decay=0.0, skip_flag=None):
    """one ``dt_weight_average`` update of ``avg`` (fp32, contiguous, 16-byte aligned) with the parameters ``p``;
    ``count_dev`` int64[1] is advanced on the device unless ``skip_flag`` (int32[1]) is set"""
    _gpu(avg, p, count_dev, skip_flag)
    if avg.dtype != torch.float32 or p.dtype != torch.float32 or count_dev.dtype != torch.int64:
        raise RuntimeError("weight_average: float32 buffers and an int64 count")
    if avg.numel() != p.numel() or not (avg.is_contiguous() and p.is_contiguous()):
        raise RuntimeError("weight_average: avg and p must be contiguous and of one size")
    if avg.device != p.device or count_dev.device != p.device or (skip_flag is not None and skip_flag.device != p.device):
        raise RuntimeError(f"weight_average: avg on {avg.device}, parameters on {p.device}")
    if skip_flag is not None and skip_flag.dtype != torch.int32:
        raise RuntimeError("weight_average: the skip flag is an int32 device tensor")
    _lib.check(_lib.load().dt_weight_average(_p(avg), _p(p), p.numel(), _p(count_dev), _p(skip_flag), AVG_MODES[mode],
                                             float(decay), _st()), "dt_weight_average")
    return avg


def bn_act(y, scale, shift, res=None, rscale=None, rshift=None, relu=True):
    _gpu(y, scale, shift, res)
    out = torch.empty_like(y)
    n_pix = y.numel() // y.shape[-1]
    _lib.check(_lib.load().dt_bn_act(_p(y), _p(scale), _p(shift), _p(res), _p(rscale), _p(rshift), _p(out), n_pix,
                                     y.shape[-1], 1 if relu else 0, _st()), "dt_bn_act")
    return out


def bn_backward(dout, out_act, y, mean, invstd, gamma, want_dres=False, act_scale=None, act_shift=None):
    _gpu(dout, y)
    lib = _lib.load()
    Cc = y.shape[-1]
    n_pix = y.numel() // Cc
    P = lib.dt_bn_bwd_rows(n_pix, Cc)
    red = torch.empty(lib.dt_bn_bwd_red_floats(n_pix, Cc), dtype=torch.float32, device=y.device)
    _lib.check(lib.dt_bn_bwd_reduce(_p(dout), _p(out_act), _p(y), _p(mean), _p(invstd), _p(act_scale), _p(act_shift),
                                    _p(red), n_pix, Cc, _st()), "dt_bn_bwd_reduce")
    dgamma = torch.empty(Cc, dtype=torch.float32, device=y.device)
    dbeta = torch.empty_like(dgamma)
    dy = torch.empty_like(y)
    dres = torch.empty_like(y) if want_dres else None
    _lib.check(lib.dt_bn_bwd_apply(_p(dout), _p(out_act), _p(y), _p(mean), _p(invstd), _p(gamma), _p(act_scale),
                                   _p(act_shift), _p(red), P, _p(dgamma), _p(dbeta), _p(dy), _p(dres), 0, n_pix, Cc,
                                   _st()), "dt_bn_bwd_apply")
    return dy, dgamma, dbeta, dres


def maxpool3x3s2(x, want_argmax=True):
    _gpu(x)
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    out = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    am = torch.empty((B, Ho, Wo, Cc), dtype=torch.uint8, device=x.device) if want_argmax else None
    _lib.check(_lib.load().dt_maxpool3x3s2(_p(x), _p(out), _p(am), B, H, W, Cc, _st()), "dt_maxpool3x3s2")
    return out, am


def maxpool3x3s2_bwd(dout, argmax, H, W, dx=None):
    _gpu(dout, argmax)
    B, _, _, Cc = dout.shape
    acc = dx is not None
    if dx is None:
        dx = torch.empty((B, H, W, Cc), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.load().dt_maxpool3x3s2_bwd(_p(dout), _p(argmax), _p(dx), 1 if acc else 0, B, H, W, Cc, _st()),
               "dt_maxpool3x3s2_bwd")
    return dx


def upsample2x_bwd(dup):
    _gpu(dup)
    B, H2, W2, Cc = dup.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, Cc), dtype=torch.float32, device=dup.device)
    _lib.check(_lib.load().dt_upsample2x_bwd(_p(dup), _p(dx), 0, B, H2 // 2, W2 // 2, Cc, _st()), "dt_upsample2x_bwd")
    return dx


def nchw_to_nhwc(x):
    _gpu(x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dt_nchw_to_nhwc(_p(x.contiguous()), _p(out), B, Cc, H, W, _st()), "dt_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x):
    _gpu(x)
    B, H, W, Cc = x.shape
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dt_nhwc_to_nchw(_p(x.contiguous()), _p(out), B, Cc, H, W, _st()), "dt_nhwc_to_nchw")
    return out


def normalize_u8(src_u8_nhwc, mean, std, c_dst):
    """uint8 [..., Csrc] -> f32 [..., c_dst] with (x - 255*mean) / (255*std)  (deadtreedata.py:148-154)."""
    _gpu(src_u8_nhwc)
    cs = src_u8_nhwc.shape[-1]
    n_pix = src_u8_nhwc.numel() // cs
    out = torch.empty(tuple(src_u8_nhwc.shape[:-1]) + (c_dst,), dtype=torch.float32, device=src_u8_nhwc.device)
    m = (C.c_float * c_dst)(*[float(v) for v in mean[:c_dst]])
    s = (C.c_float * c_dst)(*[float(v) for v in std[:c_dst]])
    _lib.check(_lib.load().dt_normalize_u8(_p(src_u8_nhwc.contiguous()), _p(out), n_pix, cs, c_dst, m, s, _st()),
               "dt_normalize_u8")
    return out


def head_fwd(x, w_ohwi, bias, argmax: Optional[str] = None):
    _gpu(x, w_ohwi, bias)
    B, H, W, Cin = x.shape
    K = w_ohwi.shape[0]
    logits = torch.empty((B, K, H, W), dtype=torch.float32, device=x.device)
    a64 = torch.empty((B, H, W), dtype=torch.int64, device=x.device) if argmax == "int64" else None
    a8 = torch.empty((B, H, W), dtype=torch.uint8, device=x.device) if argmax == "uint8" else None
    _lib.check(_lib.load().dt_head_fwd(_p(x), _p(w_ohwi.contiguous()), _p(bias), _p(logits), _p(a64), _p(a8), B, H, W,
                                       Cin, K, _st()), "dt_head_fwd")
    return logits, (a64 if a64 is not None else a8)


def head_eval(x, w_ohwi, bias, labels, lu=None, dist=None, gamma: float = 2.0, counts=None, err=None,
              want_argmax: bool = False):
    """fused evaluation head (dt_head_eval / dt_head_eval_bf16 by the dtype of x): head convolution, softmax, the loss
    and F-score sums, arg-max and the confusion counts in one pass over the decoder output x [B,H,W,16].
    -> (acc f64 [B,K,10] with slots 8, 9 zero, counts int64 [2,K,K] (+= when given), uint8 arg-max map or None,
    err int32[1] (set, never cleared, when given)).  labels / lu int64 [B,H,W]; dist fp32 [B,K,H,W] or None."""
    _gpu(x, w_ohwi, bias, labels, lu, dist)
    lib = _lib.load()
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"head_eval: x must be fp32 or bf16 [B,H,W,C], got {x.dtype} {tuple(x.shape)}")
    B, H, W, Cin = x.shape
    K = w_ohwi.shape[0]
    dev = x.device

    def i64(t, what):
        if tuple(t.shape) != (B, H, W):
            raise RuntimeError(f"head_eval: {what} {tuple(t.shape)} must be [{B},{H},{W}]")
        return (t if t.dtype == torch.int64 else t.long()).contiguous()

    labels = i64(labels, "labels")
    lu = None if lu is None else i64(lu, "lu")
    if dist is not None:
        if tuple(dist.shape) != (B, K, H, W):
            raise RuntimeError(f"head_eval: dist {tuple(dist.shape)} must be [{B},{K},{H},{W}]")
        dist = dist.contiguous().float()
    if counts is None:
        counts = torch.zeros((2, K, K), dtype=torch.int64, device=dev)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (2, K, K) or counts.device != dev or not counts.is_contiguous():
        raise RuntimeError(f"head_eval: counts must be a contiguous int64 [2,{K},{K}] on {dev}")
    err = _err_flag("head_eval", err, dev)
    n = lib.dt_head_eval_acc_doubles(B, K, H, W)
    if n <= 0:
        raise RuntimeError(f"head_eval: bad sizes B={B} K={K} H={H} W={W}")
    acc = torch.empty(n, dtype=torch.float64, device=dev)
    am = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_argmax else None
    fn, name = (lib.dt_head_eval_bf16, "dt_head_eval_bf16") if x.dtype == torch.bfloat16 else (lib.dt_head_eval, "dt_head_eval")
    _lib.check(fn(_p(x.contiguous()), _p(w_ohwi.contiguous().float()), _p(bias.contiguous().float()), _p(labels), _p(lu),
                  _p(dist), float(gamma), _p(acc), _p(counts), _p(am), _p(err), B, H, W, Cin, K, _st()), name)
    return acc[:B * K * 10].view(B, K, 10), counts, am, err


def eval_accumulate(parts, weight: float, epoch):
    """epoch f64[9] on the device: epoch[i] += weight * parts[i] (i < 8), epoch[8] += weight (dt_eval_accumulate)"""
    _gpu(parts, epoch)
    if parts.dtype != torch.float32 or parts.numel() < 8 or not parts.is_contiguous():
        raise RuntimeError("eval_accumulate: parts must be a contiguous fp32 [8]")
    if epoch.dtype != torch.float64 or epoch.numel() < 9 or not epoch.is_contiguous():
        raise RuntimeError("eval_accumulate: epoch must be a contiguous fp64 [9]")
    _lib.check(_lib.load().dt_eval_accumulate(_p(parts), float(weight), _p(epoch), _st()), "dt_eval_accumulate")
    return epoch


# ---------------------------------------------------------------------- inverted-residual block (csrc/mbconv.hip), inference
def _f32c(what, t, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous float32 tensor, got {t.dtype} {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what} {tuple(t.shape)} must be {list(shape)}")
    return t


def pwconv_affine(src0, w_io, scale, shift, src1=None, up0=False, gate=None, act=False, res=None, out=None, hw=None):
    """pointwise convolution through dt_pwconv_affine: out = act(a @ w_io * scale + shift) [+ res], a = the virtual input
    cat(src0 or its nearest x2 up-sampling, src1) [B,H,W,C0+C1], optionally gated: a[p,k] *= gc[b,k] + sigmoid(s[p]) with
    gate = (gc [B,K], s [B,H,W]).  act: Hardswish.  res [B,H,W,Cout] may be `out` itself.  hw: (H, W) of the output when
    src0 is up-sampled to an odd size (src0 then is [B,(H+1)//2,(W+1)//2,C0]; default: twice its size)."""
    _gpu(src0, src1, w_io, scale, shift, res, out)
    if src0.dim() != 4:
        raise RuntimeError(f"pwconv_affine: src0 must be [B,H,W,C], got {tuple(src0.shape)}")
    B, Hs, Ws, C0 = src0.shape
    H, W = (hw if hw is not None else (2 * Hs, 2 * Ws)) if up0 else (Hs, Ws)
    if up0 and ((H + 1) // 2 != Hs or (W + 1) // 2 != Ws):
        raise RuntimeError(f"pwconv_affine: src0 {Hs}x{Ws} is not the half-size source of a {H}x{W} output")
    _f32c("pwconv_affine: src0", src0)
    C1 = 0
    if src1 is not None:
        C1 = src1.shape[-1]
        _f32c("pwconv_affine: src1", src1, (B, H, W, C1))
    K = C0 + C1
    if w_io.dim() != 2 or w_io.shape[0] != K:
        raise RuntimeError(f"pwconv_affine: w_io {tuple(w_io.shape)} must be [{K}, Cout]")
    N = w_io.shape[1]
    _f32c("pwconv_affine: w_io", w_io)
    _f32c("pwconv_affine: scale", scale, (N,))
    _f32c("pwconv_affine: shift", shift, (N,))
    gc = gs = None
    if gate is not None:
        gc, gs = gate
        _gpu(gc, gs)
        _f32c("pwconv_affine: channel gate", gc, (B, K))
        _f32c("pwconv_affine: spatial gate", gs, (B, H, W))
    if out is None:
        out = torch.empty((B, H, W, N), dtype=torch.float32, device=src0.device)
    _f32c("pwconv_affine: out", out, (B, H, W, N))
    if res is not None:
        _f32c("pwconv_affine: res", res, (B, H, W, N))
    _lib.check(_lib.load().dt_pwconv_affine(_p(src0), _p(src1), _p(w_io), _p(out), _p(scale), _p(shift), _p(gc), _p(gs),
                                            _p(res), B, H, W, C0, C1, 1 if up0 else 0, N, 1 if act else 0, _st()),
               "dt_pwconv_affine")
    return out


def dwconv3x3_affine(x, w_tc, scale, shift, sse_w, sse_b):
    """depthwise 3x3 (stride 1, pad 1) through dt_dwconv3x3_affine: b = hardswish(dw(x) * scale + shift) plus the two side
    outputs of the same pass -> (b [B,H,W,C], s [B,H,W] = sse_w . b + sse_b, pool): pool is one buffer, the [B,C] channel
    gates ``scse_gates`` writes in front and the [B,P,C] per-workgroup channel sums of b behind them (``pool_rows``)."""
    _gpu(x, w_tc, scale, shift, sse_w, sse_b)
    lib = _lib.load()
    if x.dim() != 4:
        raise RuntimeError(f"dwconv3x3_affine: x must be [B,H,W,C], got {tuple(x.shape)}")
    B, H, W, Cc = x.shape
    _f32c("dwconv3x3_affine: x", x)
    _f32c("dwconv3x3_affine: w_tc", w_tc, (9, Cc))
    for what, t in (("scale", scale), ("shift", shift), ("sse_w", sse_w)):
        _f32c(f"dwconv3x3_affine: {what}", t, (Cc,))
    _f32c("dwconv3x3_affine: sse_b", sse_b, (1,))
    P = lib.dt_dwconv3x3_rows(H, W)
    if P <= 0:
        raise RuntimeError(f"dt_dwconv3x3_rows: {lib.dt_last_error().decode()}")
    out = torch.empty_like(x)
    s = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    pool = torch.empty(B * Cc * (1 + P), dtype=torch.float32, device=x.device)
    _lib.check(lib.dt_dwconv3x3_affine(_p(x), _p(w_tc), _p(scale), _p(shift), _p(sse_w), _p(sse_b), _p(out), _p(s),
                                       _p(pool[B * Cc:]), B, H, W, Cc, _st()), "dt_dwconv3x3_affine")
    return out, s, pool


def pool_rows(pool, B, Cc):
    """the [B,P,C] partial channel sums of a ``dwconv3x3_affine`` pool buffer"""
    return pool[B * Cc:].view(B, -1, Cc)


def scse_gates(pool, B, Cc, HW, w1_io, b1, w2_io, b2):
    """cSE gate through dt_scse_gates: the rows of `pool` (``dwconv3x3_affine``) reduced per image in a fixed order to the
    mean over HW pixels, then gc = sigmoid(W2 relu(W1 mean + b1) + b2) -> [B,C], written into the front of `pool`"""
    _gpu(pool, w1_io, b1, w2_io, b2)
    _f32c("scse_gates: pool", pool)
    if pool.numel() % (B * Cc) or pool.numel() < 2 * B * Cc:
        raise RuntimeError(f"scse_gates: pool of {pool.numel()} floats is not [B*C + B*P*C] for B={B}, C={Cc}")
    P = pool.numel() // (B * Cc) - 1
    if w1_io.dim() != 2 or w1_io.shape[0] != Cc:
        raise RuntimeError(f"scse_gates: w1_io {tuple(w1_io.shape)} must be [{Cc}, hidden]")
    Ch = w1_io.shape[1]
    _f32c("scse_gates: w1_io", w1_io)
    _f32c("scse_gates: b1", b1, (Ch,))
    _f32c("scse_gates: w2_io", w2_io, (Ch, Cc))
    _f32c("scse_gates: b2", b2, (Cc,))
    _lib.check(_lib.load().dt_scse_gates(_p(pool[B * Cc:]), _p(w1_io), _p(b1), _p(w2_io), _p(b2), _p(pool), B, P, Cc, Ch,
                                         HW, _st()), "dt_scse_gates")
    return pool[:B * Cc].view(B, Cc)


def bn_eval_affine_bias(gamma, beta, running_mean, running_var, bias, eps=1e-5):
    """eval BatchNorm behind a biased convolution as per-channel (scale, shift): dt_bn_eval_affine_bias"""
    _gpu(gamma, beta, running_mean, running_var, bias)
    n = gamma.numel()
    scale, shift = torch.empty_like(gamma), torch.empty_like(gamma)
    _lib.check(_lib.load().dt_bn_eval_affine_bias(_p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(bias),
                                                  float(eps), n, _p(scale), _p(shift), _st()), "dt_bn_eval_affine_bias")
    return scale, shift


def head_bwd(x, w_ohwi, dlogits):
    _gpu(x, w_ohwi, dlogits)
    lib = _lib.load()
    B, H, W, Cin = x.shape
    K = w_ohwi.shape[0]
    P = lib.dt_head_bwd_rows(B, H, W)
    red = torch.empty(lib.dt_head_bwd_red_floats(B, H, W, Cin, K), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    _lib.check(lib.dt_head_bwd(_p(x), _p(w_ohwi.contiguous()), _p(dlogits.contiguous()), _p(dx), _p(red), B, H, W, Cin,
                               K, _st()), "dt_head_bwd")
    dw = torch.empty_like(w_ohwi)
    db = torch.empty(K, dtype=torch.float32, device=x.device)
    _lib.check(lib.dt_head_bwd_finalize(_p(red), P, _p(dw), _p(db), Cin, K, _st()), "dt_head_bwd_finalize")
    return dx, dw, db


def conv2d_bf16(src0, w_packed, k, stride, pad, cout, src1=None, mode0=0, split=0, out0=None, out1=None,
                accumulate=False, want_stats=False, in_scale=None, in_shift=None):
    """bf16 NHWC conv (fp32 accumulate) through dt_conv2d_bf16; w_packed = [k*k, cout, cin] bf16."""
    _gpu(src0, src1, w_packed)
    lib = _lib.load()
    d = _src_desc(src0, src1, mode0, cout, k, stride, pad, split, accumulate)
    out0, out1 = _split_outputs(d, split, out0, out1, torch.bfloat16, src0.device)
    buf, stats = _rows_buffer(lib.dt_conv2d_bf16_stat_rows(C.byref(d)), cout, src0.device) if want_stats else (None, None)
    w_packed = _dma_image(d, w_packed)
    _lib.check(lib.dt_conv2d_bf16(C.byref(d), _p(src0), _p(src1), _p(w_packed), _p(out0), _p(out1), _p(buf),
                                  _p(in_scale), _p(in_shift), _st()), "dt_conv2d_bf16")
    return out0, out1, stats


def _dma_image(d, w_packed):
    """the LDS-DMA staged kernels (_lib.BF16_MT_DMA) read the weights in the chunked layout [tap][Cin/32][Cout][32]
    (dt_weight_images modes 3 / 4); this test-level wrapper re-arranges a [tap][Cout][Cin] image"""
    cfg = _lib.bf16_config(d)
    if cfg is None or cfg[3] != _lib.BF16_MT_DMA:
        return w_packed
    return w_packed.view(d.ksize * d.ksize, d.Cout, (d.C0 + d.C1) // 32, 32).permute(0, 2, 1, 3).contiguous()


def pack_weights_bf16(w_hwio, dgrad=False):
    """fp32 HWIO -> bf16 [taps][Cout][Cin] (forward) or the data-gradient image [taps][Cin][Cout] (taps reversed)"""
    _gpu(w_hwio)
    k, _, cin, cout = w_hwio.shape
    lib = _lib.load()
    if dgrad:
        out = torch.empty((k * k, cin, cout), dtype=torch.bfloat16, device=w_hwio.device)
        _lib.check(lib.dt_pack_dgrad_weights_bf16(_p(w_hwio.contiguous()), _p(out), k, cin, cout, _st()),
                   "dt_pack_dgrad_weights_bf16")
    else:
        out = torch.empty((k * k, cout, cin), dtype=torch.bfloat16, device=w_hwio.device)
        _lib.check(lib.dt_pack_weights_bf16(_p(w_hwio.contiguous()), _p(out), k, cin, cout, _st()),
                   "dt_pack_weights_bf16")
    return out


def conv2d_wgrad_bf16(src0, dy, k, stride, pad, src1=None, mode0=0, in_scale=None, in_shift=None):
    _gpu(src0, src1, dy)
    d = _src_desc(src0, src1, mode0, dy.shape[-1], k, stride, pad)
    assert (d.Ho, d.Wo) == (dy.shape[1], dy.shape[2])
    dw = torch.empty((k, k, d.C0 + d.C1, d.Cout), dtype=torch.float32, device=dy.device)
    return _wgrad("dt_conv2d_wgrad_bf16", d, src0, src1, dy, dw, in_scale, in_shift)


def confusion_matrix(pred, target, lu=None, K=2, counts=None):
    """counts int64 [2,K,K] (+=): [0] all pixels, [1] pixels with lu == 1; rows target, cols prediction."""
    _gpu(pred, target, lu)
    # the kernel reads target / lu as int64 for pred.numel() elements: anything else would run past the allocation
    if target.numel() != pred.numel() or (lu is not None and lu.numel() != pred.numel()):
        raise RuntimeError(f"confusion_matrix: prediction {tuple(pred.shape)}, target {tuple(target.shape)}" +
                           (f", lu {tuple(lu.shape)}" if lu is not None else "") + " must have the same number of pixels")
    if target.dtype != torch.int64:
        target = target.long()
    if lu is not None and lu.dtype != torch.int64:
        lu = lu.long()
    if counts is None:
        counts = torch.zeros((2, K, K), dtype=torch.int64, device=pred.device)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (2, K, K) or counts.device != pred.device:
        raise RuntimeError(f"confusion_matrix: counts must be int64 [2,{K},{K}] on {pred.device}")
    err = torch.zeros(1, dtype=torch.int32, device=pred.device)
    pred = pred.contiguous()
    p64 = pred if pred.dtype == torch.int64 else None
    p8 = pred if pred.dtype == torch.uint8 else None
    if p64 is None and p8 is None:
        raise RuntimeError("confusion_matrix: prediction must be int64 or uint8")
    _lib.check(_lib.load().dt_confusion_matrix(_p(p64), _p(p8), _p(target.contiguous()),
                                               _p(lu.contiguous()) if lu is not None else None, K, pred.numel(),
                                               _p(counts), _p(err), _st()), "dt_confusion_matrix")
    return counts, err


def prob_histogram(src, labels, lu=None, hist=None, err=None, logits: bool = False, want_q: bool = False):
    """probability histogram of ``loss/curves.py`` through dt_prob_histogram: ``src`` fp32 [B,K,H,W] probabilities (``logits``:
    logits, through the loss kernels' softmax), ``labels`` / ``lu`` [B,H,W].  ``hist`` int64 [2,K,2,256] is added to (+=;
    allocated zeroed when None), ``err`` int32 [1] likewise.  -> ``(hist, err)``, with ``want_q`` ``(hist, err, q)``: the
    quantised probabilities uint16 [B,K,H,W]."""
    _gpu(src, labels, lu, hist, err)
    if src.dtype != torch.float32 or src.dim() != 4:
        raise RuntimeError(f"prob_histogram: src must be float32 [B,K,H,W], got {src.dtype} {tuple(src.shape)}")
    B, K, H, W = src.shape
    n = B * H * W
    # the kernel reads labels / lu as int64 for B * H * W elements: anything else would run past the allocation
    if n == 0 or labels.numel() != n or (lu is not None and lu.numel() != n):
        raise RuntimeError(f"prob_histogram: src {tuple(src.shape)}, labels {tuple(labels.shape)}" +
                           (f", lu {tuple(lu.shape)}" if lu is not None else "") + " must have the same number of pixels (> 0)")
    if labels.dtype != torch.int64:
        labels = labels.long()
    if lu is not None and lu.dtype != torch.int64:
        lu = lu.long()
    if hist is None:
        hist = torch.zeros((2, K, 2, 256), dtype=torch.int64, device=src.device)
    elif hist.dtype != torch.int64 or tuple(hist.shape) != (2, K, 2, 256) or hist.device != src.device \
            or not hist.is_contiguous():
        raise RuntimeError(f"prob_histogram: hist must be contiguous int64 [2,{K},2,256] on {src.device}")
    err = _err_flag("prob_histogram", err, src.device)
    q = torch.empty((B, K, H, W), dtype=torch.uint16, device=src.device) if want_q else None
    _lib.check(_lib.load().dt_prob_histogram(_p(src.contiguous()), _p(labels.contiguous()),
                                             _p(lu.contiguous()) if lu is not None else None, _p(hist), _p(err), _p(q),
                                             B, K, H, W, 1 if logits else 0, _st()), "dt_prob_histogram")
    return (hist, err, q) if want_q else (hist, err)


def decide_classes(probs, decision_or_thresholds, out=None):
    """the decision of ``loss/curves.py`` through dt_decide_classes_u8: ``probs`` fp32 [K, ...] -> uint8 class map [...]
    (``out``: written in place).  ``decision_or_thresholds``: a ``Decision`` for K classes, or its K integer thresholds on
    the q axis (entry 0 is not read)."""
    from .loss.curves import Decision
    _gpu(probs, out)
    if probs.dtype != torch.float32 or probs.dim() < 2 or not probs.is_contiguous() or probs.numel() == 0:
        raise RuntimeError("decide_classes: probs must be non-empty contiguous float32 [K, ...]")
    K = probs.shape[0]
    if isinstance(decision_or_thresholds, Decision):
        thr = [int(v) for v in decision_or_thresholds.thresholds_u16(K)]
    else:
        thr = [int(v) for v in decision_or_thresholds]
        if len(thr) != K or any(not 1 <= v <= 65535 for v in thr[1:]):
            raise ValueError(f"decide_classes: {K} thresholds, those of the classes 1..{K - 1} in 1..65535; got {thr}")
        thr[0] = 0
    if out is None:
        out = torch.empty(tuple(probs.shape[1:]), dtype=torch.uint8, device=probs.device)
    elif out.dtype != torch.uint8 or out.numel() * K != probs.numel() or out.device != probs.device or not out.is_contiguous():
        raise RuntimeError(f"decide_classes: out must be contiguous uint8 {tuple(probs.shape[1:])} on {probs.device}")
    _lib.check(_lib.load().dt_decide_classes_u8(_p(probs), (C.c_uint16 * K)(*thr), _p(out), K, out.numel(), _st()),
               "dt_decide_classes_u8")
    return out


def decide_patchwise(probs, decision, out=None, return_support: bool = False):
    """the patch-wise decision of ``loss/curves.py`` (hysteresis and confidence filter): ``probs`` contiguous fp32 [K, h, w]
    -> uint8 class map [h, w] (``out``: written in place).  Four steps on the stream, no host synchronisation and no scalar
    read back: candidates at the low thresholds with their own q (``dt_decide_candidates_u8``), their label plane
    (``label_patches`` with the decision's connectivity), the per-root maximum / sum / count of q (``dt_patch_support``;
    sum and count only with a confidence filter) and the rejection in place (``dt_reject_patches_u8``).  Workspace next to
    the map: 2 + 4 + 4 bytes per pixel, 12 more with a confidence filter.  A decision that is not ``patchwise`` goes
    through ``decide_classes``.  ``return_support=True`` -> ``(classes, labels, qmax, qsum | None, area | None)``: the label
    plane int32 [h, w] of the CANDIDATES and the planes int32 / int64 / int32 [h * w], indexed by root, as the support pass
    left them."""
    from .loss.curves import Decision
    _gpu(probs, out)
    if probs.dtype != torch.float32 or probs.dim() != 3 or not probs.is_contiguous() or probs.numel() == 0:
        raise RuntimeError("decide_patchwise: probs must be non-empty contiguous float32 [K, h, w]")
    if not isinstance(decision, Decision):
        raise ValueError(f"decide_patchwise: decision must be a Decision, got {decision!r}")
    K, h, w = probs.shape
    high, low, conf = (a(K) for a in (decision.thresholds_u16, decision.low_u16, decision.min_confidence_u16))
    if max(h, w) > 16384 or h * w > 2 ** 31 - 2:
        raise RuntimeError(f"decide_patchwise: raster {h}x{w}: sides must be <= 16384 and h * w <= 2^31 - 2")
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or out.device != probs.device
                            or not out.is_contiguous()):
        raise RuntimeError(f"decide_patchwise: out must be contiguous uint8 {(h, w)} on {probs.device}")
    if not decision.patchwise and not return_support:
        return decide_classes(probs, decision, out=out)
    dev, lib = probs.device, _lib.load()
    if out is None:
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    u16 = C.c_uint16 * K
    q_own = torch.empty((h, w), dtype=torch.uint16, device=dev)
    _lib.check(lib.dt_decide_candidates_u8(_p(probs), u16(*low.tolist()), _p(out), _p(q_own), K, h * w, _st()),
               "dt_decide_candidates_u8")
    labels, _ = label_patches(out, K, decision.connectivity)
    filtered = bool(conf.any())
    qmax = torch.zeros(h * w, dtype=torch.int32, device=dev)
    qsum = torch.zeros(h * w, dtype=torch.int64, device=dev) if filtered else None
    area = torch.zeros(h * w, dtype=torch.int32, device=dev) if filtered else None
    _lib.check(lib.dt_patch_support(_p(labels), _p(q_own), h, w, _p(qmax), _p(qsum), _p(area), _st()), "dt_patch_support")
    _lib.check(lib.dt_reject_patches_u8(_p(out), _p(labels), _p(qmax), _p(qsum), _p(area), u16(*high.tolist()),
                                        u16(*conf.tolist()), K, h, w, _st()), "dt_reject_patches_u8")
    return (out, labels, qmax, qsum, area) if return_support else out


def object_plane_shape(B: int, H: int, W: int):
    """``(cols, ph, pw)``: the batch plane of ``object_histogram`` — ``ceil(sqrt(B))`` cells of ``(H + 1) x (W + 1)`` per row,
    the width rounded up to 4 pixels where that still fits a side of 16384 (packed stores).  Not part of the contract"""
    cols = math.isqrt(B - 1) + 1 if B > 1 else 1
    ph, pw = -(-B // cols) * (H + 1), cols * (W + 1)
    return cols, ph, (pw + 3) // 4 * 4 if (pw + 3) // 4 * 4 <= 16384 else pw


def object_histogram(q, target, sweep, hist=None, targets=None, err=None, _timed=None):
    """the crown-level histogram of ``loss/objects.py`` on the device: ``q`` contiguous uint16 [B,K,H,W] (what
    ``prob_histogram(..., want_q=True)`` returns), ``target`` int64 [B,H,W], ``sweep`` an ``ObjectSweep`` for K classes.
    ``hist`` int64 [K,2,256,256] and ``targets`` int64 [K] are added to (+=; allocated zeroed when None), ``err`` int32 [1]
    likewise (a target label outside [0, K)).  -> ``(hist, targets, err)``.  Launches only — no host synchronisation, no
    scalar read back, no sort: the images are laid out in one plane with background gutters (``dt_object_planes``),
    ``label_patches`` twice, ``patch_areas`` on the target, ``dt_patch_support`` on the candidates, then ``dt_object_vote``,
    ``dt_object_inter``, ``dt_object_targets`` and ``dt_object_histogram``.  Workspace: 45 bytes per plane pixel.  A plane
    beyond the labeller's limits (sides <= 16384, at most 2^31 - 2 pixels) is a ``RuntimeError`` before any launch.
    ``_timed(name, fn)``, for ``scripts/bench_objects.py`` alone, is called in place of every step and must return ``fn()``."""
    from .loss.objects import ObjectSweep
    _gpu(q, target, hist, targets, err)
    if not isinstance(sweep, ObjectSweep):
        raise ValueError(f"object_histogram: sweep must be an ObjectSweep, got {sweep!r}")
    if q.dtype != torch.uint16 or q.dim() != 4 or q.numel() == 0 or not q.is_contiguous():
        raise RuntimeError(f"object_histogram: q must be non-empty contiguous uint16 [B,K,H,W], got {q.dtype} {tuple(q.shape)}")
    B, K, H, W = q.shape
    dev = q.device
    if target.dtype != torch.int64 or tuple(target.shape) != (B, H, W) or target.device != dev or not target.is_contiguous():
        raise RuntimeError(f"object_histogram: target must be contiguous int64 {(B, H, W)} on {dev}, got {target.dtype} "
                           f"{tuple(target.shape)}")
    if not 2 <= K <= 8:
        raise RuntimeError(f"object_histogram: K={K} unsupported (2..8)")
    low = sweep.low_u16(K)
    cols, ph, pw = object_plane_shape(B, H, W)
    if max(ph, pw) > 16384 or ph * pw > 2 ** 31 - 2:
        raise RuntimeError(f"object_histogram: {B} images of {H}x{W} need a plane of {ph}x{pw}: sides must be <= 16384 and "
                           "h * w <= 2^31 - 2")
    if hist is None:
        hist = torch.zeros((K, 2, 256, 256), dtype=torch.int64, device=dev)
    elif hist.dtype != torch.int64 or tuple(hist.shape) != (K, 2, 256, 256) or hist.device != dev or not hist.is_contiguous():
        raise RuntimeError(f"object_histogram: hist must be contiguous int64 [{K},2,256,256] on {dev}")
    if targets is None:
        targets = torch.zeros(K, dtype=torch.int64, device=dev)
    elif targets.dtype != torch.int64 or tuple(targets.shape) != (K,) or targets.device != dev or not targets.is_contiguous():
        raise RuntimeError(f"object_histogram: targets must be contiguous int64 [{K}] on {dev}")
    err = _err_flag("object_histogram", err, dev)
    lib, n = _lib.load(), ph * pw
    step = _timed if _timed is not None else (lambda name, fn: fn())
    cand = torch.empty((ph, pw), dtype=torch.uint8, device=dev)
    tcls = torch.empty((ph, pw), dtype=torch.uint8, device=dev)
    q_own = torch.empty((ph, pw), dtype=torch.uint16, device=dev)
    step("planes", lambda: _lib.check(lib.dt_object_planes(_p(q), _p(target), (C.c_uint16 * K)(*low.tolist()), B, K, H, W, cols,
                                                            ph, pw, _p(cand), _p(q_own), _p(tcls), _p(err), _st()),
                                      "dt_object_planes"))
    labels_p = step("label_pred", lambda: label_patches(cand, K, sweep.connectivity, err=err)[0])
    labels_t = step("label_target", lambda: label_patches(tcls, K, sweep.connectivity, err=err)[0])
    area_t = step("areas_target", lambda: patch_areas(labels_t))
    # one zeroed workspace, carved by element size: vote and qsum int64, inter, qmax and area int32, matched uint8
    ws = step("zero", lambda: torch.zeros(29 * n + 8, dtype=torch.uint8, device=dev))
    wide, mid = ws[:16 * n].view(torch.int64), ws[16 * n:28 * n].view(torch.int32)
    vote, qsum = wide[:n], wide[n:]
    inter, qmax, area = mid[:n], mid[n:2 * n], mid[2 * n:]
    matched = ws[28 * n:29 * n]
    step("support", lambda: _lib.check(lib.dt_patch_support(_p(labels_p), _p(q_own), ph, pw, _p(qmax), _p(qsum), _p(area), _st()),
                                       "dt_patch_support"))
    step("vote", lambda: _lib.check(lib.dt_object_vote(_p(labels_t), _p(labels_p), ph, pw, _p(vote), _st()), "dt_object_vote"))
    step("inter", lambda: _lib.check(lib.dt_object_inter(_p(labels_t), _p(labels_p), _p(vote), ph, pw, _p(inter), _st()),
                                     "dt_object_inter"))
    step("targets", lambda: _lib.check(lib.dt_object_targets(_p(labels_t), _p(tcls), _p(cand), _p(vote), _p(inter), _p(area_t),
                                                             _p(area), K, ph, pw, sweep.min_pixels, sweep.iou_p, sweep.iou_q,
                                                             _p(targets), _p(matched), _st()), "dt_object_targets"))
    step("histogram", lambda: _lib.check(lib.dt_object_histogram(_p(labels_p), _p(cand), _p(qmax), _p(qsum), _p(area),
                                                                 _p(matched), K, ph, pw, sweep.min_pixels, _p(hist), _st()),
                                         "dt_object_histogram"))
    return hist, targets, err


def conv2d_bn_bwd(src0, w_hwio, y, mean, invstd, act_scale=None, act_shift=None, act=None, join_into=None):
    """3x3 stride-1 conv (a data gradient) whose epilogue also produces the BatchNorm-backward partial sums of the
    layer with raw output `y` (same shape as the result).  Virtual activation: give act_scale/act_shift; block
    output: give the stored activation `act` and the tensor `join_into` the gradient is ADDED to.
    -> (out [B,H,W,Cout], red [2,P,Cout])"""
    _gpu(src0, w_hwio, y, mean, invstd, act_scale, act_shift, act, join_into)
    lib = _lib.load()
    d, out, red, red_view, fuse = _bn_bwd_setup(lib.dt_conv2d_stat_rows, src0, w_hwio.shape[-1], torch.float32, y, mean,
                                                invstd, act_scale, act_shift, act, join_into)
    _lib.check(lib.dt_conv2d_bn_bwd(C.byref(d), _p(src0), _p(w_hwio.contiguous()), _p(out), _p(red), C.byref(fuse),
                                    _st()), "dt_conv2d_bn_bwd")
    return out, red_view


def conv2d_winograd_bn_bwd(src0, u, y, mean, invstd, act_scale=None, act_shift=None, act=None, join_into=None):
    """Winograd form of conv2d_bn_bwd (u = winograd_weights of the data-gradient HWIO image) -> (out, red [2,P,Cout])"""
    _gpu(src0, u, y, mean, invstd, act_scale, act_shift, act, join_into)
    lib = _lib.load()
    d, out, red, red_view, fuse = _bn_bwd_setup(lib.dt_conv2d_winograd_stat_rows, src0, u.shape[3], torch.float32, y, mean,
                                                invstd, act_scale, act_shift, act, join_into)
    _lib.check(lib.dt_conv2d_winograd_bn_bwd(C.byref(d), _p(src0), _p(u), _p(out), _p(red), C.byref(fuse), _st()),
               "dt_conv2d_winograd_bn_bwd")
    return out, red_view


def conv2d_bf16_bn_bwd(src0, w_packed, cout, y, mean, invstd, act_scale=None, act_shift=None, act=None,
                       join_into=None):
    """bf16 twin of conv2d_bn_bwd (src0, y, act, join_into bf16 NHWC; w_packed from pack_weights_bf16)
    -> (out bf16, red [2,P,Cout])"""
    _gpu(src0, w_packed, y, mean, invstd, act_scale, act_shift, act, join_into)
    lib = _lib.load()
    d, out, red, red_view, fuse = _bn_bwd_setup(lib.dt_conv2d_bf16_stat_rows, src0, cout, torch.bfloat16, y, mean, invstd,
                                                act_scale, act_shift, act, join_into)
    _lib.check(lib.dt_conv2d_bf16_bn_bwd(C.byref(d), _p(src0), _p(_dma_image(d, w_packed)), _p(out), _p(red), C.byref(fuse),
                                         _st()), "dt_conv2d_bf16_bn_bwd")
    return out, red_view


def conv2d_bf16_upsampled_dgrad(dy, w_packed_dgrad, cin, y, mean, invstd, act_scale, act_shift):
    """bf16 gradient of x for out = conv3x3(nearest_upsample_x2(x)) from dy [B,2h,2w,cout] (bf16) and the data-gradient
    weight image (pack_weights_bf16(..., dgrad=True)), the narrow layers only: the 2x2 sums are taken on the fp32
    accumulators -> (gx [B,h,w,cin] bf16, red [2,P,cin] = BatchNorm-backward partial sums of the layer with raw output y)"""
    _gpu(dy, w_packed_dgrad, y, mean, invstd, act_scale, act_shift)
    lib = _lib.load()
    B, H, W, cout = dy.shape
    d = conv_desc(B, H, W, cout, 0, 0, cin, 3, 1, 1)
    if not lib.dt_conv2d_bf16_upsampled_dgrad_supported(C.byref(d)):
        raise ValueError("conv2d_bf16_upsampled_dgrad: layer shape not covered by the narrow kernel")
    red, red_view = _rows_buffer(lib.dt_conv2d_bf16_stat_rows(C.byref(d)), cin, dy.device)
    gx = torch.empty((B, H // 2, W // 2, cin), dtype=torch.bfloat16, device=dy.device)
    fuse = _lib.BnBwdFuse(_p(y.contiguous()), _p(mean), _p(invstd), _p(act_scale), _p(act_shift))
    _lib.check(lib.dt_conv2d_bf16_upsampled_dgrad(C.byref(d), _p(dy.contiguous()), _p(w_packed_dgrad), _p(gx), _p(red),
                                                  C.byref(fuse), _st()), "dt_conv2d_bf16_upsampled_dgrad")
    return gx, red_view


def upsample2x_bwd_bn(dup, y, mean, invstd, act_scale, act_shift):
    """2x2-sum backward of a nearest x2 upsample + the BatchNorm-backward partial sums of the layer with raw output
    `y` ([B,H,W,C], fp32 or bf16 like dup) -> (dx, red [2,P,C])"""
    _gpu(dup, y, mean, invstd, act_scale, act_shift)
    lib = _lib.load()
    B, H2, W2, Cc = dup.shape
    H, W = H2 // 2, W2 // 2
    bf = dup.dtype == torch.bfloat16
    P = (lib.dt_upsample2x_bwd_bn_bf16_rows if bf else lib.dt_upsample2x_bwd_bn_rows)(B, H, W, Cc)
    red = torch.empty(lib.dt_bn_stats_floats(P, Cc), dtype=torch.float32, device=dup.device)
    dx = torch.empty((B, H, W, Cc), dtype=dup.dtype, device=dup.device)
    fuse = _lib.BnBwdFuse(_p(y.contiguous()), _p(mean), _p(invstd), _p(act_scale), _p(act_shift))
    fn = lib.dt_upsample2x_bwd_bn_bf16 if bf else lib.dt_upsample2x_bwd_bn
    _lib.check(fn(_p(dup.contiguous()), _p(dx), C.byref(fuse), _p(red), B, H, W, Cc, _st()), "dt_upsample2x_bwd_bn")
    return dx, red[:2 * P * Cc].view(2, P, Cc)


def conv2d_upsampled_dgrad(dy, w_hwio, cin, y=None, mean=None, invstd=None, act_scale=None, act_shift=None):
    """gradient of x for out = conv3x3(nearest_upsample_x2(x)) (pad 1) from dy [B,2h,2w,cout] and the forward weights
    [3,3,cin,cout] in one sub-pixel kernel -> (gx [B,h,w,cin], red [2,P,cin] or None).  With y/mean/invstd/act_*: the
    BatchNorm-backward partial sums of the layer with raw output y (x = relu(y*act_scale+act_shift)) come along."""
    _gpu(dy, w_hwio)
    lib = _lib.load()
    B, H, W, cout = dy.shape
    d = _lib.ConvDesc(B, H, W, cin, 0, 1, H, W, cout, 3, 1, 1, 0, 0)
    if not lib.dt_conv2d_upsampled_dgrad_supported(C.byref(d)):
        raise ValueError("conv2d_upsampled_dgrad: layer shape not covered by the sub-pixel kernel")
    gx = torch.empty((B, H // 2, W // 2, cin), dtype=torch.float32, device=dy.device)
    red, red_view, fuse = None, None, None
    if y is not None:
        _gpu(y, mean, invstd, act_scale, act_shift)
        red, red_view = _rows_buffer(lib.dt_conv2d_upsampled_dgrad_rows(C.byref(d)), cin, dy.device)
        fuse = _lib.BnBwdFuse(_p(y.contiguous()), _p(mean), _p(invstd), _p(act_scale), _p(act_shift))
    _lib.check(lib.dt_conv2d_upsampled_dgrad(C.byref(d), _p(dy.contiguous()), _p(w_hwio.contiguous()), _p(gx), _p(red),
                                             C.byref(fuse) if fuse is not None else None, _st()), "dt_conv2d_upsampled_dgrad")
    return gx, red_view


def stem_conv_bf16(x_nhwc_f32, w_hwio_7x7, want_stats=False):
    """the 7x7 / stride-2 / pad-3 stem on the bf16 MFMA kernels: fp32 NHWC image [B,H,W,Cin<=4] -> bf16
    [B,H/2,W/2,Cout] (+ fp32 BatchNorm partial statistics), via the 2x2 space-to-depth image and a 4x4 window"""
    _gpu(x_nhwc_f32, w_hwio_7x7)
    lib = _lib.load()
    B, H, W, Cin = x_nhwc_f32.shape
    Cout = w_hwio_7x7.shape[-1]
    st = _st()
    s2d = torch.empty((B, H // 2, W // 2, 16), dtype=torch.bfloat16, device=x_nhwc_f32.device)
    _lib.check(lib.dt_stem_s2d_bf16(_p(x_nhwc_f32.contiguous()), _p(s2d), B, H, W, Cin, st), "dt_stem_s2d_bf16")
    wp = torch.empty(16 * Cout * 16, dtype=torch.bfloat16, device=x_nhwc_f32.device)
    _lib.check(lib.dt_stem_pack_weights_bf16(_p(w_hwio_7x7.contiguous()), _p(wp), Cin, Cout, st),
               "dt_stem_pack_weights_bf16")
    d = _lib.ConvDesc(B, H // 2, W // 2, 16, 0, 0, H // 2, W // 2, Cout, 4, 1, 2, 0, 0)
    out = torch.empty((B, H // 2, W // 2, Cout), dtype=torch.bfloat16, device=x_nhwc_f32.device)
    buf, stats = _rows_buffer(lib.dt_conv2d_bf16_stat_rows(C.byref(d)), Cout, out.device) if want_stats else (None, None)
    _lib.check(lib.dt_conv2d_bf16(C.byref(d), _p(s2d), None, _p(wp), _p(out), None, _p(buf), None, None, st),
               "dt_conv2d_bf16(stem)")
    return out, stats


def stem_wgrad_bf16(x_nhwc_f32, dy_bf16):
    """weight gradient of the 7x7 / stride-2 stem on the bf16 MFMA kernels (space-to-depth form) -> fp32 HWIO
    [7,7,Cin,Cout]; dy bf16 [B,H/2,W/2,Cout]"""
    _gpu(x_nhwc_f32, dy_bf16)
    lib = _lib.load()
    B, H, W, Cin = x_nhwc_f32.shape
    Cout = dy_bf16.shape[-1]
    st = _st()
    s2d = torch.empty((B, H // 2, W // 2, 16), dtype=torch.bfloat16, device=x_nhwc_f32.device)
    _lib.check(lib.dt_stem_s2d_bf16(_p(x_nhwc_f32.contiguous()), _p(s2d), B, H, W, Cin, st), "dt_stem_s2d_bf16")
    d = _lib.ConvDesc(B, H // 2, W // 2, 16, 0, 0, H // 2, W // 2, Cout, 4, 1, 2, 0, 0)
    dw4 = torch.empty(16 * 16 * Cout, dtype=torch.float32, device=s2d.device)
    _wgrad("dt_conv2d_wgrad_bf16", d, s2d, None, dy_bf16, dw4, what="dt_conv2d_wgrad_bf16(stem)")
    dw7 = torch.empty((7, 7, Cin, Cout), dtype=torch.float32, device=s2d.device)
    _lib.check(lib.dt_stem_unpack_wgrad(_p(dw4), _p(dw7), Cin, Cout, st), "dt_stem_unpack_wgrad")
    return dw7


# ---- bf16 elementwise kernels (thin wrappers; the engine calls the C ABI directly with its own buffers)
def bn_act_bf16(y, scale, shift, res=None, rscale=None, rshift=None, relu=True):
    """bf16 (or fp32) y [.., C] -> bf16 act(y*scale+shift + (res*rscale+rshift))"""
    _gpu(y, scale, shift, res)
    Cq = y.shape[-1]
    out = torch.empty(y.shape, dtype=torch.bfloat16, device=y.device)
    _lib.check(_lib.load().dt_bn_act_bf16(_p(y), 1 if y.dtype == torch.float32 else 0, _p(scale), _p(shift), _p(res),
                                          _p(rscale), _p(rshift), _p(out), y.numel() // Cq, Cq, 1 if relu else 0,
                                          _st()), "dt_bn_act_bf16")
    return out


def bn_backward_bf16(dout, out_act, y, mean, invstd, gamma, want_dres=False, act_scale=None, act_shift=None,
                     dres=None):
    """-> (dy bf16, dgamma f32, dbeta f32, dres bf16 or None); same contract as bn_backward, bf16 activations.
    `dres` given: the masked gradient is ADDED to it (gradient join)."""
    _gpu(dout, y, mean, invstd, gamma)
    lib = _lib.load()
    Cq = y.shape[-1]
    n_pix = y.numel() // Cq
    P = lib.dt_bn_bwd_rows_bf16(n_pix)
    red = torch.empty(lib.dt_bn_stats_floats(P, Cq), dtype=torch.float32, device=y.device)
    _lib.check(lib.dt_bn_bwd_reduce_bf16(_p(dout), _p(out_act), _p(y), _p(mean), _p(invstd), _p(act_scale),
                                         _p(act_shift), _p(red), n_pix, Cq, _st()), "dt_bn_bwd_reduce_bf16")
    dy = torch.empty(y.shape, dtype=torch.bfloat16, device=y.device)
    dgamma = torch.empty(Cq, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(Cq, dtype=torch.float32, device=y.device)
    acc = dres is not None
    if want_dres and dres is None:
        dres = torch.empty(y.shape, dtype=torch.bfloat16, device=y.device)
    _lib.check(lib.dt_bn_bwd_apply_bf16(_p(dout), _p(out_act), _p(y), _p(mean), _p(invstd), _p(gamma), _p(act_scale),
                                        _p(act_shift), _p(red), P, _p(dgamma), _p(dbeta), _p(dy), _p(dres),
                                        1 if acc else 0, n_pix, Cq, _st()), "dt_bn_bwd_apply_bf16")
    return dy, dgamma, dbeta, dres


def maxpool3x3s2_bf16(x):
    """bf16 NHWC -> (pooled bf16, argmax bytes [B,Ho,Wo,C] uint8: window position kh*3+kw of the first maximum)"""
    _gpu(x)
    B, H, W, Cq = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((B, Ho, Wo, Cq), dtype=torch.bfloat16, device=x.device)
    am = torch.empty((B, Ho, Wo, Cq), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().dt_maxpool3x3s2_bf16_amax(_p(x), _p(out), _p(am), B, H, W, Cq, _st()),
               "dt_maxpool3x3s2_bf16_amax")
    return out, am


def maxpool3x3s2_bwd_bf16(dout, argmax, H, W, dx=None):
    """gradient of maxpool3x3s2_bf16 wrt its [B,H,W,C] input; `dx` given: accumulate into it"""
    _gpu(dout, argmax)
    B, _, _, Cq = dout.shape
    acc = dx is not None
    if dx is None:
        dx = torch.empty((B, H, W, Cq), dtype=torch.bfloat16, device=dout.device)
    _lib.check(_lib.load().dt_maxpool3x3s2_bwd_bf16(_p(dout), _p(argmax), _p(dx), 1 if acc else 0, B, H, W, Cq, _st()),
               "dt_maxpool3x3s2_bwd_bf16")
    return dx


def upsample2x_bwd_bf16(dup):
    """[B,2H,2W,C] bf16 gradient of a nearest x2 upsample -> [B,H,W,C] (2x2 sums, one rounding)"""
    _gpu(dup)
    B, H2, W2, Cq = dup.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, Cq), dtype=torch.bfloat16, device=dup.device)
    _lib.check(_lib.load().dt_upsample2x_bwd_bf16(_p(dup), _p(dx), B, H2 // 2, W2 // 2, Cq, _st()),
               "dt_upsample2x_bwd_bf16")
    return dx


def split_normalize_u8(raster_chw_u8, d: int, first: int, count: int, mean, std, c_dst: int):
    """band-major uint8 raster [C,h,w] on the device -> the fp32 NHWC sub-tiles [count,d,d,c_dst] ``first`` .. of the
    row-major d x d block grid of the zero-padded raster (tiler.py:121-134 + make_blocks_vectorized + Normalize, fused)"""
    _gpu(raster_chw_u8)
    if raster_chw_u8.dtype != torch.uint8 or raster_chw_u8.dim() != 3:
        raise RuntimeError("split_normalize_u8: raster must be uint8 [C,h,w]")
    cs, h, w = raster_chw_u8.shape
    nbx = -(-w // d)
    nby = -(-h // d)
    if first < 0 or count <= 0 or first + count > nbx * nby:
        raise RuntimeError(f"split_normalize_u8: blocks {first}..{first + count - 1} outside the {nby} x {nbx} grid")
    out = torch.empty((count, d, d, c_dst), dtype=torch.float32, device=raster_chw_u8.device)
    m = (C.c_float * c_dst)(*[float(v) for v in mean[:c_dst]])
    s = (C.c_float * c_dst)(*[float(v) for v in std[:c_dst]])
    _lib.check(_lib.load().dt_split_normalize_u8(_p(raster_chw_u8.contiguous()), _p(out), cs, h, w, d, nbx, first, count,
                                                 c_dst, m, s, _st()), "dt_split_normalize_u8")
    return out


def _stitch_grid(h: int, w: int, d: int, overlap: int, what: str):
    """(ny, nx) of the overlap-stitch window grid, from the library's own count (the kernels' definition)"""
    lib = _lib.load()
    ny, nx = lib.dt_stitch_window_count(h, d, overlap), lib.dt_stitch_window_count(w, d, overlap)
    _lib.check(min(ny, nx, 0), what)
    return ny, nx


def _views_array(views):
    """a sequence of (flip, rot) pairs -> (ctypes int array (flip_0, rot_0, ...), T); the library validates the values.
    ``None`` (the plain window: the one identity view) -> (None, 0), the library's NULL form"""
    if views is None:
        return None, 0
    flat = [int(v) for pair in views for v in pair]
    if len(flat) != 2 * len(views):
        raise RuntimeError("views must be a sequence of (flip, rot) pairs")
    return (C.c_int * max(1, len(flat)))(*flat), len(views)


def window_normalize_u8(raster_chw_u8, d: int, overlap: int, first: int, count: int, mean, std, c_dst: int, views=None):
    """``split_normalize_u8`` with window origins ``d - overlap`` apart: band-major uint8 raster [C,h,w] on the device -> the
    fp32 NHWC windows [count,d,d,c_dst] ``first`` .. of the row-major overlap-stitch grid (``tiler.window_grid``); overlap 0
    is the block grid, bit-identical to ``split_normalize_u8``.  ``views`` (T pairs (flip, rot), ``tiler.tta_views``): T
    tiles per window, [count*T,d,d,c_dst], tile k*T + v = rot90^rot(flip(window first + k)) bit for bit."""
    _gpu(raster_chw_u8)
    if raster_chw_u8.dtype != torch.uint8 or raster_chw_u8.dim() != 3:
        raise RuntimeError("window_normalize_u8: raster must be uint8 [C,h,w]")
    cs, h, w = raster_chw_u8.shape
    ny, nx = _stitch_grid(h, w, d, overlap, "window_normalize_u8")
    if first < 0 or count <= 0 or first + count > ny * nx:
        raise RuntimeError(f"window_normalize_u8: windows {first}..{first + count - 1} outside the {ny} x {nx} grid")
    m = (C.c_float * c_dst)(*[float(v) for v in mean[:c_dst]])
    s = (C.c_float * c_dst)(*[float(v) for v in std[:c_dst]])
    arr, T = _views_array(views)
    out = torch.empty((count * max(T, 1), d, d, c_dst), dtype=torch.float32, device=raster_chw_u8.device)
    _lib.check(_lib.load().dt_window_normalize_u8(_p(raster_chw_u8.contiguous()), _p(out), cs, h, w, d, d - overlap, nx,
                                                  first, count, c_dst, m, s, arr, T, _st()), "dt_window_normalize_u8")
    return out


STITCH_WEIGHTS = {"ramp": 0, "keep": 1}      # DT_STITCH_WEIGHT_* of include/deadtrees_hip.h


def stitch_accumulate(logits, acc, overlap: int, first: int, views=None, weight: str = "ramp"):
    """average-mode blend: fp32 NCHW logits [count,K,d,d] of the windows ``first`` .. -> ``acc`` fp32 [K,h,w] (zeroed before
    the first call) += weight * softmax, in place.  Calls in ascending window order give a bit-identical accumulator
    for every split of the windows into calls.  Returns ``acc``.

    ``views`` (T pairs (flip, rot)): logits are [count,T,K,d,d], tile [k, v] the network's answer to view v of window
    ``first + k``; the T softmax vectors are mapped back, averaged (view order, times 1/T) and then weighted; without views
    the window is its own identity view.  ``weight="ramp"``: the blend ramp (``tiler.blend_ramp``); ``weight="keep"``: 1
    inside the window's crop-mode region (``tiler.window_keep``), 0 outside.  Several models may add into one ``acc``,
    each in ascending window order."""
    _gpu(logits, acc)
    if weight not in STITCH_WEIGHTS:
        raise RuntimeError(f"stitch_accumulate: weight {weight!r}: use 'ramp' or 'keep'")
    arr, T = _views_array(views)
    shape = ("count", "K", "d", "d") if views is None else ("count", T, "K", "d", "d")
    if (logits.dtype != torch.float32 or logits.dim() != len(shape) or logits.shape[-1] != logits.shape[-2]
            or (views is not None and logits.shape[1] != T)):
        raise RuntimeError(f"stitch_accumulate: logits must be float32 [{','.join(map(str, shape))}]")
    count, (K, d) = logits.shape[0], logits.shape[-3:-1]
    if acc.dtype != torch.float32 or acc.dim() != 3 or acc.shape[0] != K or not acc.is_contiguous():
        raise RuntimeError(f"stitch_accumulate: acc must be contiguous float32 [{K},h,w]")
    _lib.check(_lib.load().dt_stitch_accumulate(_p(logits.contiguous()), _p(acc), K, acc.shape[1], acc.shape[2], d, overlap,
                                                first, count, arr, T, STITCH_WEIGHTS[weight], _st()),
               "dt_stitch_accumulate")
    return acc


def stitch_finalize(acc, want_probs: bool = False):
    """accumulator fp32 [K,h,w] -> uint8 class map [h,w] (argmax, ties -> lowest class); with ``want_probs`` also the
    normalised probabilities fp32 [K,h,w]: returns ``classes`` or ``(classes, probs)``"""
    _gpu(acc)
    if acc.dtype != torch.float32 or acc.dim() != 3 or not acc.is_contiguous():
        raise RuntimeError("stitch_finalize: acc must be contiguous float32 [K,h,w]")
    K, h, w = acc.shape
    classes = torch.empty((h, w), dtype=torch.uint8, device=acc.device)
    probs = torch.empty_like(acc) if want_probs else None
    _lib.check(_lib.load().dt_stitch_finalize(_p(acc), _p(classes), _p(probs), K, h, w, _st()), "dt_stitch_finalize")
    return (classes, probs) if want_probs else classes


def stitch_classes(maps_u8, out_hw_u8, overlap: int, first: int):
    """crop-mode merge: uint8 class maps [count,d,d] of the windows ``first`` .. -> their kept regions written into the
    uint8 raster map ``out_hw_u8`` [h,w] in place (regions are disjoint).  Returns ``out_hw_u8``."""
    _gpu(maps_u8, out_hw_u8)
    if maps_u8.dtype != torch.uint8 or maps_u8.dim() != 3 or maps_u8.shape[1] != maps_u8.shape[2]:
        raise RuntimeError("stitch_classes: maps must be uint8 [count,d,d]")
    if out_hw_u8.dtype != torch.uint8 or out_hw_u8.dim() != 2 or not out_hw_u8.is_contiguous():
        raise RuntimeError("stitch_classes: the raster map must be contiguous uint8 [h,w]")
    count, d, _ = maps_u8.shape
    _lib.check(_lib.load().dt_stitch_classes_u8(_p(maps_u8.contiguous()), _p(out_hw_u8), out_hw_u8.shape[0],
                                                out_hw_u8.shape[1], d, overlap, first, count, _st()), "dt_stitch_classes_u8")
    return out_hw_u8


def band_has_data(band_u8) -> torch.Tensor:
    """int32[1] device flag: 1 iff some byte is neither 0 nor 255 (scripts/inference.py:60-62 is_valid_tile, no host pass)"""
    _gpu(band_u8)
    if band_u8.dtype != torch.uint8:
        raise RuntimeError("band_has_data: uint8 band expected")
    flag = torch.zeros(1, dtype=torch.int32, device=band_u8.device)
    _lib.check(_lib.load().dt_band_has_data(_p(band_u8.contiguous()), band_u8.numel(), _p(flag), _st()), "dt_band_has_data")
    return flag


def augment_normalize_u8(src_u8_nhwc, geo, bc, mean, std, c_dst):
    """uint8 [B,H,W,Csrc] -> fp32 [B,H,W,c_dst]: flip / rot90 / brightness-contrast LUT / normalise in one pass
    (data/deadtreedata.py:128-146).  geo int32 [B,2] = (flip, rot k), bc fp32 [B,2] = (alpha, beta)."""
    _gpu(src_u8_nhwc, geo, bc)
    B, H, W, cs = src_u8_nhwc.shape
    if geo.dtype != torch.int32 or bc.dtype != torch.float32 or tuple(geo.shape) != (B, 2) or tuple(bc.shape) != (B, 2):
        raise RuntimeError("augment_normalize_u8: geo must be int32 [B,2] and bc float32 [B,2]")
    if H != W and bool((geo[:, 1] % 2 == 1).any()):
        raise RuntimeError("augment_normalize_u8: odd rot90 counts need square tiles")
    out = torch.empty((B, H, W, c_dst), dtype=torch.float32, device=src_u8_nhwc.device)
    sums = torch.empty(B, dtype=torch.int64, device=src_u8_nhwc.device)
    m = (C.c_float * c_dst)(*[float(v) for v in mean[:c_dst]])
    s = (C.c_float * c_dst)(*[float(v) for v in std[:c_dst]])
    _lib.check(_lib.load().dt_augment_normalize_u8(_p(src_u8_nhwc.contiguous()), _p(out), _p(geo.contiguous()),
                                                   _p(bc.contiguous()), _p(sums), B, H, W, cs, c_dst, m, s, _st()),
               "dt_augment_normalize_u8")
    return out


def augment_labels(labels, geo):
    """int64 [B,H,W] masks / land-use maps through the same flip + rot90 as the image batch"""
    _gpu(labels, geo)
    if labels.dtype != torch.int64 or labels.dim() != 3:
        raise RuntimeError("augment_labels: labels must be int64 [B,H,W]")
    B, H, W = labels.shape
    out = torch.empty_like(labels)
    _lib.check(_lib.load().dt_augment_labels(_p(labels.contiguous()), _p(out), _p(geo.contiguous()), B, H, W, _st()),
               "dt_augment_labels")
    return out


def _pool_gather(who, sources, src, idx, geo, bc, mean, std, c_dst, merge_above, out, err):
    """the one validator and launch behind ``pool_gather_batch`` (one source, ``src`` None) and ``pool_gather_combined``;
    who: the caller's name, for the messages"""
    if not 1 <= len(sources) <= _lib.POOL_MAX_SOURCES:
        raise RuntimeError(f"{who}: 1 .. {_lib.POOL_MAX_SOURCES} sources, not {len(sources)}")
    sources = [tuple(t) for t in sources]
    if any(len(t) != 4 for t in sources):
        raise RuntimeError(f"{who}: a source is (images, masks, lu, sums)")
    if src is None and len(sources) != 1:
        raise RuntimeError(f"{who}: src may be None with one source only, not with {len(sources)} sources")
    with_lu = sources[0][2] is not None
    _gpu(src, idx, geo, bc, *(x for t in sources for x in t))
    dev = sources[0][0].device
    H, W = sources[0][0].shape[1:3] if sources[0][0].dim() == 4 else (0, 0)
    table = (_lib.PoolSource * len(sources))()
    for j, (images, masks, lu, sums) in enumerate(sources):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 4 or not images.is_contiguous():
            raise RuntimeError(f"{who}: source {j}: images must be contiguous uint8 [N,H,W,4]")
        N = images.shape[0]
        if tuple(images.shape[1:3]) != (H, W):
            raise RuntimeError(f"{who}: source {j} holds {images.shape[1]}x{images.shape[2]} tiles, source 0 {H}x{W}")
        if (lu is not None) != with_lu:
            raise RuntimeError(f"{who}: lu in every source or in none")
        for name, t in (("masks", masks), ("lu", lu)):
            if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != (N, H, W) or not t.is_contiguous()):
                raise RuntimeError(f"{who}: source {j}: {name} must be contiguous uint8 [N,H,W]")
        if sums.dtype != torch.int64 or tuple(sums.shape) != (N,) or not sums.is_contiguous():
            raise RuntimeError(f"{who}: source {j}: sums must be contiguous int64 [N]")
        if any(t is not None and t.device != dev for t in (images, masks, lu, sums)):
            raise RuntimeError(f"{who}: source {j} is not on {dev}")
        table[j] = _lib.PoolSource(_p(images), _p(masks), _p(lu), _p(sums), N)
    B = idx.shape[0]
    if (idx.dtype != torch.int32 or idx.dim() != 1 or geo.dtype != torch.int32 or tuple(geo.shape) != (B, 2)
            or bc.dtype != torch.float32 or tuple(bc.shape) != (B, 2)
            or (src is not None and (src.dtype != torch.int32 or tuple(src.shape) != (B,) or not src.is_contiguous()))
            or not (idx.is_contiguous() and geo.is_contiguous() and bc.is_contiguous())):
        raise RuntimeError(f"{who}: src (if given) and idx must be int32 [B], geo int32 [B,2] and bc float32 [B,2], "
                           "contiguous")
    if any(t is not None and t.device != dev for t in (src, idx, geo, bc)):
        raise RuntimeError(f"{who}: src, idx, geo and bc must be on {dev}")
    if out is None:
        out = (torch.empty((B, c_dst, H, W), dtype=torch.float32, device=dev),
               torch.empty((B, H, W), dtype=torch.int64, device=dev),
               torch.empty((B, H, W), dtype=torch.int64, device=dev) if with_lu else None)
    img, mask, lu_out = out
    for name, t, shape, dt in (("img", img, (B, c_dst, H, W), torch.float32), ("mask", mask, (B, H, W), torch.int64),
                               ("lu", lu_out, (B, H, W), torch.int64)):
        if (t is None) != (name == "lu" and not with_lu):
            raise RuntimeError(f"{who}: out needs img and mask, and lu exactly when the pools have one")
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev):
            raise RuntimeError(f"{who}: out {name} must be contiguous {dt} {list(shape)} on {dev}")
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    m = (C.c_float * c_dst)(*[float(v) for v in mean[:c_dst]])
    s = (C.c_float * c_dst)(*[float(v) for v in std[:c_dst]])
    _lib.check(_lib.load().dt_pool_gather_combined(table, len(sources), _p(src), _p(idx), _p(geo), _p(bc), _p(img),
                                                   _p(mask), _p(lu_out), _p(err), B, H, W, c_dst,
                                                   int(bool(merge_above)), m, s, _st()), "dt_pool_gather_combined")
    return img, mask, lu_out, err


def pool_gather_batch(images, masks, lu, sums, idx, geo, bc, mean, std, c_dst, merge_above=False, out=None, err=None):
    """One batch out of a device-resident pool in one launch (csrc/pool.hip): images uint8 [N,H,W,4], masks / lu uint8
    [N,H,W] (lu may be None), sums int64 [N] (the exact byte sum of every image; the bits of the ABI's uint64), idx int32
    [B], geo int32 [B,2], bc fp32 [B,2] -> (img fp32 [B,c_dst,H,W] contiguous, mask int64 [B,H,W], lu int64 [B,H,W] or
    None, err int32 [1]).  The arithmetic is that of ``augment_normalize_u8`` / ``augment_labels`` on ``images[idx]``.
    out: (img, mask, lu) tensors to write into (e.g. ``HipTrainer.static_batch()``'s); err: a flag to OR into.  No host
    synchronisation: a bad index or an odd turn of a non-square tile zeroes that sample and sets a bit of ``err``.
    This is ``pool_gather_combined`` with one source and no ``src``."""
    return _pool_gather("pool_gather_batch", [(images, masks, lu, sums)], None, idx, geo, bc, mean, std, c_dst,
                        merge_above, out, err)


def pool_gather_combined(sources, src, idx, geo, bc, mean, std, c_dst, merge_above=False, out=None, err=None):
    """One batch out of several device-resident pools in one launch (``dt_pool_gather_combined``, csrc/pool.hip).
    sources: a list of ``(images, masks, lu, sums)`` tensor tuples as ``pool_gather_batch`` takes them, all of one tile
    size (lu: None in every source or in none); slot b is sample ``idx[b]`` of ``sources[src[b]]``: src, idx int32 [B], geo
    int32 [B,2], bc fp32 [B,2]; with one source src may be None.  Returns what ``pool_gather_batch`` returns.  A source
    number outside the list sets bit 4 of ``err``, an index outside its source bit 1, an odd turn of a non-square tile bit
    2; those slots are zeros."""
    return _pool_gather("pool_gather_combined", sources, src, idx, geo, bc, mean, std, c_dst, merge_above, out, err)


def ensemble_vote(maps_u8: torch.Tensor, K: int, dtype: str = "int64"):
    """uint8 class maps [M, ...] of M models -> per-pixel mode [...] (ties -> smallest class, torch.mode);
    returns (map, err flag).  deployment/inference.py:65-116."""
    _gpu(maps_u8)
    if maps_u8.dtype != torch.uint8:
        raise RuntimeError("ensemble_vote: class maps must be uint8")
    M = maps_u8.shape[0]
    n = maps_u8[0].numel()
    out8 = torch.empty(maps_u8.shape[1:], dtype=torch.uint8, device=maps_u8.device) if dtype == "uint8" else None
    out64 = torch.empty(maps_u8.shape[1:], dtype=torch.int64, device=maps_u8.device) if dtype == "int64" else None
    err = torch.zeros(1, dtype=torch.int32, device=maps_u8.device)
    _lib.check(_lib.load().dt_ensemble_vote(_p(maps_u8.contiguous()), M, n, K, _p(out8), _p(out64), _p(err), _st()),
               "dt_ensemble_vote")
    return (out64 if out64 is not None else out8), err


def zonal_counts(classes_u8: torch.Tensor, zones_u8: torch.Tensor = None, K: int = 3, Z: int = 1, counts=None, err=None):
    """class counts per zone of a uint8 class map on the device (``dt_zonal_counts_u8``): counts int64 [Z,K] (+=),
    ``counts[z, c]`` = pixels with zone z and class c; ``zones_u8`` None: every pixel is zone 0 and Z must be 1.  Any shape
    (``zones_u8`` the same one); a non-contiguous view is made contiguous, a contiguous one is read where it lies, whatever
    its storage offset.  ``counts`` / ``err`` (int32 [1]) are allocated zeroed when not given and accumulated into
    otherwise.  No host synchronisation: a class >= K ORs 1 into ``err``, a zone >= Z ORs 2, and such a pixel enters no
    count.  Returns (counts, err)."""
    _gpu(classes_u8, zones_u8, counts, err)
    if classes_u8.dtype != torch.uint8 or (zones_u8 is not None and zones_u8.dtype != torch.uint8):
        raise RuntimeError("zonal_counts: classes and zones must be uint8")
    if zones_u8 is not None and (tuple(zones_u8.shape) != tuple(classes_u8.shape) or zones_u8.device != classes_u8.device):
        raise RuntimeError(f"zonal_counts: classes {tuple(classes_u8.shape)} and zones {tuple(zones_u8.shape)} must have "
                           "the same shape and device")
    K, Z = int(K), int(Z)
    dev = classes_u8.device
    if counts is None:
        counts = torch.zeros((max(Z, 0), max(K, 0)), dtype=torch.int64, device=dev)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (Z, K) or counts.device != dev or not counts.is_contiguous():
        raise RuntimeError(f"zonal_counts: counts must be contiguous int64 [{Z},{K}] on {dev}")
    err = _err_flag("zonal_counts", err, dev)
    classes_u8 = classes_u8.contiguous()
    zones_u8 = None if zones_u8 is None else zones_u8.contiguous()
    _lib.check(_lib.load().dt_zonal_counts_u8(_p(classes_u8), _p(zones_u8), classes_u8.numel(), K, Z, _p(counts), _p(err),
                                              _st()), "dt_zonal_counts_u8")
    return counts, err


def cover_grid(classes_u8: torch.Tensor, zones_u8: torch.Tensor = None, K: int = 3, Z: int = 1, yq=None, xq=None, sums=None,
               err=None):
    """area-weighted class counts per zone and per cell of a coarser grid, of a uint8 [h, w] class map on the device
    (``dt_cover_grid_u8``; the contract is ``deployment/cover.py``): sums int64 [gy, gx, Z, K] (+=) in 1/65536 pixel.  ``yq`` /
    ``xq``: the edge tables in 1/256 pixel as HOST integer arrays (checked here — ``ValueError`` before any launch — and
    uploaded as int32).  ``zones_u8`` None: every pixel is zone 0 and Z must be 1.  A non-contiguous view is made
    contiguous, a contiguous one (a crop of full rows, a member of a stacked tensor) is read where it lies.  ``sums`` /
    ``err`` (int32 [1]) are allocated zeroed when not given and accumulated into otherwise.  No host synchronisation: a
    class >= K ORs 1 into ``err``, a zone >= Z ORs 2, and such a pixel enters no sum.  Returns (sums, err)."""
    from .deployment.cover import check_cover
    _gpu(classes_u8, zones_u8, sums, err)
    yq, xq = (q.numpy() if isinstance(q, torch.Tensor) and not q.is_cuda else q for q in (yq, xq))
    if isinstance(yq, torch.Tensor) or isinstance(xq, torch.Tensor):
        raise ValueError("cover_grid: the edge tables are host arrays (they are checked before the launch)")
    K, Z, yq, xq = check_cover(classes_u8, zones_u8, K, Z, yq, xq)
    dev = classes_u8.device
    if zones_u8 is not None and zones_u8.device != dev:
        raise ValueError("cover_grid: the map and zones must be on the same device")
    gy, gx = len(yq) - 1, len(xq) - 1
    if sums is None:
        sums = torch.zeros((gy, gx, Z, K), dtype=torch.int64, device=dev)
    elif sums.dtype != torch.int64 or tuple(sums.shape) != (gy, gx, Z, K) or sums.device != dev or not sums.is_contiguous():
        raise ValueError(f"cover_grid: sums must be contiguous int64 [{gy},{gx},{Z},{K}] on {dev}")
    err = _err_flag("cover_grid", err, dev)
    tables = torch.cat([torch.from_numpy(yq), torch.from_numpy(xq)]).to(torch.int32).to(dev, non_blocking=True)
    classes_u8 = classes_u8.contiguous()
    zones_u8 = None if zones_u8 is None else zones_u8.contiguous()
    h, w = classes_u8.shape
    _lib.check(_lib.load().dt_cover_grid_u8(_p(classes_u8), _p(zones_u8), h, w, K, Z, _p(tables), gy, _p(tables[gy + 1:]), gx,
                                            _p(sums), _p(err), _st()), "dt_cover_grid_u8")
    return sums, err


def raster_cut(rgbn: torch.Tensor, mask: Optional[torch.Tensor] = None, lu: Optional[torch.Tensor] = None,
               source_dim: int = 2048, tile_size: int = 256, slot: Optional[torch.Tensor] = None, out=None, census=True):
    """Sub-tile cut and census of one raster on the device (``dt_raster_cut_u8``, csrc/raster_cut.hip; the contract is
    ``data.rasters.cut_raster_host``).  rgbn uint8 [4,h,w], mask / lu uint8 [h,w] or None (zeros / ones), each contiguous
    at any storage offset.  ``slot`` int32 [n] on the device, n = (source_dim // tile_size)^2, with ``out = (images
    [R,t,t,4], masks [R,t,t], lu [R,t,t], sums int64 [R])`` contiguous pool tensors: sub-tile i goes into row ``slot[i]``;
    a negative entry (or one >= R) writes nothing, rows no entry names are not touched, and no two entries may name one
    row.  ``census``: True allocates the int64 [n,16] table (columns ``_lib.CENSUS_*``), a tensor is overwritten, False /
    None leaves it out (``slot`` is then required).  No host synchronisation.  Returns the census tensor or None."""
    _gpu(rgbn, mask, lu, slot)
    S, t = int(source_dim), int(tile_size)
    if rgbn.dtype != torch.uint8 or rgbn.dim() != 3 or rgbn.shape[0] != 4:
        raise RuntimeError(f"raster_cut: rgbn must be uint8 [4,h,w], not {rgbn.dtype} {tuple(rgbn.shape)}")
    h, w = int(rgbn.shape[1]), int(rgbn.shape[2])
    dev = rgbn.device
    for name, m in (("mask", mask), ("lu", lu)):
        if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != (h, w) or m.device != dev):
            raise RuntimeError(f"raster_cut: {name} must be uint8 [{h},{w}] on {dev}")
    n = (S // t) ** 2 if t > 0 else 0
    rows = 0
    images = masks = lu_out = sums = None
    if slot is not None:
        if slot.dtype != torch.int32 or tuple(slot.shape) != (n,) or slot.device != dev or not slot.is_contiguous():
            raise RuntimeError(f"raster_cut: slot must be contiguous int32 [{n}] on {dev}")
        if out is None or len(out) != 4:
            raise RuntimeError("raster_cut: slot needs out = (images, masks, lu, sums)")
        images, masks, lu_out, sums = out
        _gpu(images, masks, lu_out, sums)
        rows = int(images.shape[0])
        want = ((images, torch.uint8, (rows, t, t, 4)), (masks, torch.uint8, (rows, t, t)),
                (lu_out, torch.uint8, (rows, t, t)), (sums, torch.int64, (rows,)))
        for x, dtype, shape in want:
            if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
                raise RuntimeError(f"raster_cut: out must be contiguous (images u8 [R,{t},{t},4], masks u8 [R,{t},{t}], "
                                   f"lu u8 [R,{t},{t}], sums i64 [R]) on {dev}; got {x.dtype} {tuple(x.shape)}")
    elif out is not None:
        raise RuntimeError("raster_cut: out without slot")
    if census is True:
        census = torch.empty((n, _lib.CENSUS_COLS), dtype=torch.int64, device=dev)
    elif census is False:
        census = None
    if census is not None and (census.dtype != torch.int64 or tuple(census.shape) != (n, _lib.CENSUS_COLS)
                               or census.device != dev or not census.is_contiguous()):
        raise RuntimeError(f"raster_cut: census must be contiguous int64 [{n},{_lib.CENSUS_COLS}] on {dev}")
    rgbn = rgbn.contiguous()
    mask = None if mask is None else mask.contiguous()
    lu = None if lu is None else lu.contiguous()
    _lib.check(_lib.load().dt_raster_cut_u8(_p(rgbn), _p(mask), _p(lu), h, w, S, t, _p(slot), rows, _p(images), _p(masks),
                                            _p(lu_out), _p(sums), _p(census), _st()), "dt_raster_cut_u8")
    return census


def rasterize_polygons(edges: torch.Tensor, polys: torch.Tensor, shape, all_touched: bool = True,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Polygons burnt into a uint8 [h, w] map on the device (``dt_rasterize_polygons_u8``, csrc/polygons.hip; the contract
    is ``data.polygons.rasterize_host``).  ``edges`` int32 [E, 4] and ``polys`` int32 [P, 8] are ``PolygonSet.tables()`` on
    the device, contiguous; P = 0 gives zeros.  ``out``: a contiguous uint8 [h, w] tensor at any storage offset (a view
    into a larger buffer: only its own bytes are written), allocated when not given; every byte of it is written.  One
    launch, no host synchronisation.  Returns ``out``."""
    _gpu(edges, polys, out)
    h, w = int(shape[0]), int(shape[1])
    dev = edges.device
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 4 or not edges.is_contiguous():
        raise RuntimeError(f"rasterize_polygons: edges must be contiguous int32 [E,4], not {edges.dtype} {tuple(edges.shape)}")
    if (polys.dtype != torch.int32 or polys.dim() != 2 or polys.shape[1] != 8 or not polys.is_contiguous()
            or polys.device != dev):
        raise RuntimeError(f"rasterize_polygons: polys must be contiguous int32 [P,8] on {dev}, not {polys.dtype} "
                           f"{tuple(polys.shape)}")
    if out is None:
        if h < 1 or w < 1:
            raise RuntimeError(f"rasterize_polygons: raster {h}x{w} must be at least 1x1")
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (h, w) or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"rasterize_polygons: out must be contiguous uint8 [{h},{w}] on {dev}")
    E, P = int(edges.shape[0]), int(polys.shape[0])
    _lib.check(_lib.load().dt_rasterize_polygons_u8(_p(edges) if E else None, E, _p(polys) if P else None, P, h, w,
                                                    1 if all_touched else 0, _p(out), _st()), "dt_rasterize_polygons_u8")
    return out


# constants asked of the library on first use -> (getter, count).  PATCH_TILE = (th, tw): the tile of dt_label_patches_u8's
# local launch; OUTLINE_CHUNK / OVERLAP_CHUNK: the consecutive pixels one workgroup of dt_outline_count / dt_overlap_count takes;
# PROXIMITY_SEGMENT: the rows of one column segment of dt_proximity_columns; PROXIMITY_WINDOW: the pixels of one row that a
# workgroup of dt_proximity_query takes; ATTRIBUTE_SPAN: the consecutive 64-pixel chunks a wave of dt_patch_attributes_u8 takes;
# CURVE_CHUNK: the consecutive pixels of the B * H * W axis one workgroup of dt_prob_histogram takes
_LIB_CONSTANTS = {"PATCH_TILE": ("dt_patch_tile", 2), "OUTLINE_CHUNK": ("dt_outline_chunk", 1),
                  "CURVE_CHUNK": ("dt_curve_chunk", 1),
                  "OVERLAP_CHUNK": ("dt_overlap_chunk", 1), "PROXIMITY_SEGMENT": ("dt_proximity_segment", 1),
                  "PROXIMITY_WINDOW": ("dt_proximity_window", 1), "ATTRIBUTE_SPAN": ("dt_attribute_span", 1),
                  "SUPPORT_SPAN": ("dt_support_span", 1), "CROWN_SEGMENT": ("dt_crown_segment", 1)}
# growth rounds of ``split_patches`` enqueued back to back before the host reads their flags
CROWN_ROUND_GROUP = 8


def _constant(name: str):
    if name not in globals():
        entry, n = _LIB_CONSTANTS[name]
        vals = [C.c_int(0) for _ in range(n)]
        _lib.check(getattr(_lib.load(), entry)(*map(C.byref, vals)), entry)
        globals()[name] = vals[0].value if n == 1 else tuple(v.value for v in vals)
    return globals()[name]


def __getattr__(name):
    if name in _LIB_CONSTANTS:
        return _constant(name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _err_flag(what: str, err, device):
    """the ``err`` argument of a wrapper: int32 [1] on ``device``, allocated zeroed when not given"""
    if err is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    if err.dtype != torch.int32 or tuple(err.shape) != (1,) or err.device != device:
        raise RuntimeError(f"{what}: err must be int32 [1] on {device}")
    return err


def _chunk_scan(counts):
    """int32 [chunks, 2] counts per chunk, scanned: (the two totals as Python ints — ONE read-back —, int32 [chunks]: the
    exclusive scan of column 0, the first slot of every chunk)"""
    scan = torch.cumsum(counts, 0, dtype=torch.int32)
    first, second = (int(v) for v in scan[-1].tolist())
    return first, second, (scan[:, 0] - counts[:, 0]).contiguous()


def _patch_planes(what, classes_u8=None, **planes):
    """the argument checks of the patch wrappers: a uint8 [h, w] class map and int32 planes of its shape on its device;
    returns them contiguous (a contiguous view is read where it lies, whatever its storage offset)"""
    first = classes_u8 if classes_u8 is not None else next(iter(planes.values()))
    _gpu(classes_u8, *planes.values())
    if classes_u8 is not None and classes_u8.dtype != torch.uint8:
        raise RuntimeError(f"{what}: classes must be uint8")
    if first.dim() != 2 or first.numel() == 0:
        raise RuntimeError(f"{what}: expected a non-empty [h, w] map, got shape {tuple(first.shape)}")
    for name, t in planes.items():
        if t.dtype != torch.int32 or tuple(t.shape) != tuple(first.shape) or t.device != first.device:
            raise RuntimeError(f"{what}: {name} must be int32 {list(first.shape)} on {first.device}")
    return first.shape[0], first.shape[1]


def label_patches(classes_u8: torch.Tensor, K: int, connectivity: int = 8, err=None):
    """patch labels of a uint8 class map [h, w] on the device (``dt_label_patches_u8``, contract in
    ``deployment/patches.py``): int32 [h, w], 0 on background, elsewhere 1 + the row-major index of the first pixel of the
    pixel's patch (same class 1 <= c < K, 4- or 8-connected).  A non-contiguous view is made contiguous, a contiguous one
    is read where it lies.  No host synchronisation: a class >= K ORs 1 into ``err`` (int32 [1], allocated zeroed when not
    given) and is background.  Returns (labels, err)."""
    h, w = _patch_planes("label_patches", classes_u8)
    dev = classes_u8.device
    err = _err_flag("label_patches", err, dev)
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().dt_label_patches_u8(_p(classes_u8.contiguous()), h, w, int(K), int(connectivity), _p(labels),
                                               _p(err), _st()), "dt_label_patches_u8")
    return labels, err


def patch_areas(labels: torch.Tensor) -> torch.Tensor:
    """int32 [h * w]: the pixel count of every patch at its root's index (label - 1), 0 elsewhere (``dt_patch_areas``)"""
    h, w = _patch_planes("patch_areas", labels=labels)
    area = torch.zeros(h * w, dtype=torch.int32, device=labels.device)
    _lib.check(_lib.load().dt_patch_areas(_p(labels.contiguous()), h, w, _p(area), _st()), "dt_patch_areas")
    return area


def sieve_patches(classes_u8: torch.Tensor, labels: torch.Tensor, area_plane: torch.Tensor, min_pixels: int) -> None:
    """IN PLACE (``dt_sieve_patches_u8``): the pixels of every patch with fewer than ``min_pixels`` pixels become class 0 /
    label 0 and the root's entry of ``area_plane`` becomes 0; a removed patch is not filled from its neighbours.  The three
    tensors are written where they lie, so they must be contiguous; ``min_pixels <= 1`` changes nothing"""
    h, w = _patch_planes("sieve_patches", classes_u8, labels=labels)
    _gpu(area_plane)
    if (area_plane.dtype != torch.int32 or area_plane.numel() != h * w or area_plane.device != labels.device
            or not area_plane.is_contiguous()):
        raise RuntimeError(f"sieve_patches: area_plane must be contiguous int32 [{h * w}] on {labels.device}")
    if not (classes_u8.is_contiguous() and labels.is_contiguous()):
        raise RuntimeError("sieve_patches: works in place and needs a contiguous class map and label plane")
    _lib.check(_lib.load().dt_sieve_patches_u8(_p(classes_u8), _p(labels), _p(area_plane), h, w, int(min_pixels), _st()),
               "dt_sieve_patches_u8")


def patch_table(labels: torch.Tensor, classes_u8: torch.Tensor, area_plane: torch.Tensor = None,
                reuse_area_plane: bool = False):
    """the ``PatchTable`` (host arrays) of a label plane and its class map, sieved or not.  ``area_plane``
    (``patch_areas``; computed here when not given) names the surviving roots — its non-zero entries, which
    ``torch.nonzero`` compacts in ascending order — and gives the area column; ``dt_patch_measure`` fills class, bounding
    box and coordinate sums.  The row count is the ONE scalar read back before the table itself.  ``reuse_area_plane=True``
    turns the caller's ``area_plane`` into the root -> row plane instead of allocating one (its content is lost)."""
    from .deployment.patches import PatchTable
    h, w = _patch_planes("patch_table", classes_u8, labels=labels)
    dev = labels.device
    if area_plane is None:
        area_plane, reuse_area_plane = patch_areas(labels), True
    elif (area_plane.dtype != torch.int32 or area_plane.numel() != h * w or area_plane.device != dev
          or not area_plane.is_contiguous()):
        raise RuntimeError(f"patch_table: area_plane must be contiguous int32 [{h * w}] on {dev}")
    area_plane = area_plane.view(-1)
    root = torch.nonzero(area_plane).view(-1)                  # int64, ascending; synchronises: n is read here
    n = int(root.numel())
    area = area_plane[root].to(torch.int64)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    sum_y = torch.empty(n, dtype=torch.int64, device=dev)
    sum_x = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        dense = area_plane if reuse_area_plane else torch.empty(h * w, dtype=torch.int32, device=dev)
        dense[root] = torch.arange(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().dt_patch_measure(_p(labels.contiguous()), _p(classes_u8.contiguous()), h, w, _p(dense), n,
                                                _p(cls), _p(bbox), _p(sum_y), _p(sum_x), _st()), "dt_patch_measure")
    return PatchTable(*(t.cpu().numpy() for t in (root, cls, area, bbox, sum_y, sum_x)), shape=(h, w))


def patch_outlines(labels: torch.Tensor, classes_u8: torch.Tensor, connectivity: int = 8):
    """the outlines of the patches of a label plane int32 [h, w] (``label_patches``, sieved or not) and its class map, as a
    ``PolygonSet`` of host arrays (csrc/outlines.hip; the contract is ``deployment.outlines.polygonize_host``): one
    polygon per patch in ascending root — polygon ``k`` is row ``k`` of ``patch_table`` —, the exterior ring first, one
    vertex per corner, ``xy`` in 1/256 pixel.  ``connectivity`` must be the labelling's.  Neither tensor is written; a
    non-contiguous view is made contiguous.  Sides <= 16384.

    All per-edge work runs in the ``dt_outline_*`` kernels: count -> (scan; E and V are read back: the first of two
    read-backs) -> edges -> ceil(log2 E) pointer-jumping rounds -> (the ring heads are compacted: R is read back) ->
    rings -> (a stable sort by label and a scan over the R rings) -> scatter.  Only the four ``PolygonSet`` arrays are
    downloaded.  Workspace: 4 bytes per pixel and about 40 bytes per boundary edge (two 16-byte states, the edge word,
    head flag and ring row), next to the label plane."""
    from .data.polygons import PolygonSet
    from .deployment.outlines import empty_outlines
    h, w = _patch_planes("patch_outlines", classes_u8, labels=labels)
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise RuntimeError(f"patch_outlines: connectivity must be 4 or 8, got {connectivity!r}")
    lib, dev = _lib.load(), labels.device
    labels, classes_u8 = labels.contiguous(), classes_u8.contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    counts = torch.empty((-(-h * w // _constant("OUTLINE_CHUNK")), 2), **i32)
    _lib.check(lib.dt_outline_count(_p(labels), h, w, _p(counts), _st()), "dt_outline_count")
    E, V, chunk_first = _chunk_scan(counts)                    # read-back 1: edges and vertices
    if E == 0:
        return empty_outlines()
    first = torch.empty(h * w, **i32)
    edges = torch.empty(E, **i32)
    state = torch.empty((2, E, 4), **i32)
    head = torch.empty(E, dtype=torch.uint8, device=dev)
    _lib.check(lib.dt_outline_edges(_p(labels), h, w, int(connectivity), _p(chunk_first), E, _p(first), _p(edges),
                                    _p(state[0]), _st()), "dt_outline_edges")
    _lib.check(lib.dt_outline_jump(_p(state[0]), _p(state[1]), E, _p(head), _st()), "dt_outline_jump")
    final = state[lib.dt_outline_rounds(E) & 1]
    heads = torch.nonzero(head).view(-1)                       # int64, ascending ring id; read-back 2: the ring count
    R = int(heads.numel())
    corners = torch.empty(R, **i32)
    ring_label = torch.empty(R, **i32)
    _lib.check(lib.dt_outline_rings(_p(labels), h, w, int(connectivity), _p(first), _p(edges), _p(final), E, _p(heads), R,
                                    _p(corners), _p(ring_label), _st()), "dt_outline_rings")
    # (label, ring id): ids ascend already, so a stable sort by label; the exterior 4 * root + 0 is a patch's smallest key
    ring_label, order = torch.sort(ring_label, stable=True)
    ring_offsets = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    ring_offsets[1:] = torch.cumsum(corners[order], 0, dtype=torch.int64)
    row_of = torch.empty(E, **i32)
    row_of[heads[order]] = torch.arange(R, **i32)
    new_polygon = torch.ones(R, dtype=torch.bool, device=dev)
    new_polygon[1:] = ring_label[1:] != ring_label[:-1]
    ring_polygon = torch.cumsum(new_polygon, 0, dtype=torch.int32) - 1
    values = torch.zeros(R, dtype=torch.uint8, device=dev)      # one per polygon, P <= R of them: cut on the host
    values[ring_polygon.long()] = classes_u8.view(-1)[(ring_label.long() - 1).clamp_(0, h * w - 1)]
    xy = torch.zeros((V, 2), **i32)
    _lib.check(lib.dt_outline_scatter(_p(edges), _p(final), E, w, _p(row_of), _p(ring_offsets), R, V, _p(xy), _st()),
               "dt_outline_scatter")
    xy, ring_offsets, ring_polygon, values = (t.cpu().numpy() for t in (xy, ring_offsets, ring_polygon, values))
    return PolygonSet(xy, ring_offsets, ring_polygon, values[:int(ring_polygon[-1]) + 1])


def _overlap_planes(labels_a: torch.Tensor, labels_b: torch.Tensor, what: str = "patch_overlaps"):
    """the argument checks of ``patch_overlaps``: (h, w, a, b) with both planes contiguous and 16-byte aligned"""
    h, w = _patch_planes(what, labels_a=labels_a, labels_b=labels_b)
    if h * w > 2 ** 31 - 2:
        raise RuntimeError(f"{what}: {h * w} pixels do not fit int32 labels (h * w <= {2 ** 31 - 2})")
    planes = []
    for t in (labels_a, labels_b):
        t = t.contiguous()
        planes.append(t if t.data_ptr() % 16 == 0 else t.clone())       # a view at an odd storage offset: 16-byte loads
    return h, w, planes[0], planes[1]


def patch_overlaps(labels_a: torch.Tensor, labels_b: torch.Tensor):
    """the overlap table of two label planes int32 [h, w] on one HIP device (``label_patches``, sieved or not; contract in
    ``deployment/overlaps.py``, csrc/overlaps.hip): host int64 arrays ``(a, b, n)``, one row per pair of patches that
    share a pixel — ``a`` / ``b`` the roots (label - 1) in the two planes, ``n`` the shared pixels — ascending in
    ``(a, b)``.  Neither plane is written; a non-contiguous view is made contiguous.  ``h * w <= 2**31 - 2``.

    All per-pixel work runs in two kernels over the runs of equal pair keys in flat row-major order: ``dt_overlap_count``
    -> (a scan over the chunks; the run count R and the runs with a key are read back: read-back 1) ->
    ``dt_overlap_runs`` (key and start of every run) -> on the R runs only: lengths by difference, ``torch.sort`` by key,
    segment ids where the sorted key changes (the pair count P is read back: read-back 2), a segmented int64 sum of the
    lengths, the key-0 segment dropped.  Only the three result arrays are downloaded; without any overlap neither
    ``dt_overlap_runs`` nor the sort is launched.  Workspace: 8 bytes per chunk of ``OVERLAP_CHUNK`` = 1024 pixels (the second
    count is what lets a pair of maps without overlap stop after the scan) and 12 bytes per run, plus the sort's own."""
    h, w, a, b = _overlap_planes(labels_a, labels_b)
    lib, dev = _lib.load(), a.device
    empty = tuple(torch.zeros(0, dtype=torch.int64).numpy() for _ in range(3))
    counts = torch.empty((-(-h * w // _constant("OVERLAP_CHUNK")), 2), dtype=torch.int32, device=dev)
    _lib.check(lib.dt_overlap_count(_p(a), _p(b), h, w, _p(counts), _st()), "dt_overlap_count")
    R, live, chunk_first = _chunk_scan(counts)                 # read-back 1: runs, and runs whose key is not 0
    if live == 0:
        return empty
    key = torch.empty(R, dtype=torch.int64, device=dev)
    start = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.check(lib.dt_overlap_runs(_p(a), _p(b), h, w, _p(chunk_first), R, _p(key), _p(start), _st()), "dt_overlap_runs")
    length = torch.empty(R, dtype=torch.int64, device=dev)
    length[:-1] = start[1:] - start[:-1]
    length[-1] = h * w - start[-1]
    key, order = torch.sort(key)
    segment = torch.zeros(R, dtype=torch.int64, device=dev)
    segment[1:] = torch.cumsum(key[1:] != key[:-1], 0)
    S = int(segment[-1]) + 1                                   # read-back 2: the segments; P = S - (one of key 0, if any)
    n = torch.zeros(S, dtype=torch.int64, device=dev).index_add_(0, segment, length[order])
    pair = torch.empty(S, dtype=torch.int64, device=dev)
    pair[segment] = key                                        # every run of a segment writes the same value
    first = 1 if live < R else 0                               # keys are >= 0 and sorted: the key-0 segment comes first
    pair, n = pair[first:], n[first:]
    return tuple(t.cpu().numpy() for t in ((pair >> 32) - 1, (pair & 0xffffffff) - 1, n))


def proximity_tables(labels_src: torch.Tensor, second: bool = False):
    """the column tables of a source label plane int32 [h, w] (``dt_proximity_columns``; contiguous and 16-byte aligned, as
    ``_overlap_planes`` returns it): ``(dist uint16 [P, h, w], nearest int32 [P, h, w], flag int32 [1])``, P = 2, or 4 with
    ``second`` (what ``exclude_own`` needs).  12 bytes per pixel, 24 with ``second``, and 32 bytes per column and segment of
    ``PROXIMITY_SEGMENT`` rows for the carried states.  No synchronisation"""
    h, w = labels_src.shape
    if max(h, w) > 16384:
        raise RuntimeError(f"patch_proximity: raster {h}x{w}: sides must be <= 16384 (column distances are uint16)")
    dev, P = labels_src.device, 4 if second else 2
    dist = torch.empty((P, h, w), dtype=torch.int16, device=dev)                   # read as uint16 by the kernels
    nearest = torch.empty((P, h, w), dtype=torch.int32, device=dev)
    carry = torch.empty((2, -(-h // _constant("PROXIMITY_SEGMENT")), w, 4), dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().dt_proximity_columns(_p(labels_src), h, w, 1 if second else 0, _p(dist), _p(nearest), _p(carry),
                                                _p(flag), _st()), "dt_proximity_columns")
    return dist, nearest, flag


def proximity_query(tables, labels_qry: torch.Tensor, roots_qry: torch.Tensor, exclude_own: bool = False, limit2: int = -1):
    """``dt_proximity_query`` over the tables of ``proximity_tables``: int64 [n] on the device, ``d2 << 32 | root`` per query
    root (``roots_qry`` int64 [n] on the device, n >= 1), -1 (all ones) for none.  No synchronisation"""
    dist, nearest, flag = tables
    h, w = labels_qry.shape
    dev, n = labels_qry.device, int(roots_qry.numel())
    dense = torch.full((h * w + 1,), -1, dtype=torch.int32, device=dev)      # the last entry takes the roots off the raster
    on_grid = (roots_qry >= 0) & (roots_qry < h * w)
    dense[torch.where(on_grid, roots_qry, h * w)] = torch.arange(n, dtype=torch.int32, device=dev)
    best = torch.full((n,), -1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().dt_proximity_query(_p(dist), _p(nearest), _p(flag), _p(labels_qry), h, w, _p(dense), n,
                                              1 if exclude_own else 0, 1 if dist.shape[0] == 4 else 0, int(limit2), _p(best),
                                              _st()), "dt_proximity_query")
    return best


def patch_proximity(labels_src: torch.Tensor, labels_qry: torch.Tensor, roots_qry, exclude_own: bool = False, limit2=None):
    """nearest-patch distances between two label planes int32 [h, w] on one HIP device (``label_patches``, sieved or not;
    contract in ``deployment/proximity.py``, csrc/proximity.hip): host int64 arrays ``(d2, nearest_root)`` with one entry per
    element of ``roots_qry`` (the ascending roots of the query plane's table, a host array or a device tensor) — the smallest
    squared distance between a pixel of the query patch and a labelled pixel of ``labels_src``, and the smallest root among
    the source patches that reach it; ``-1, -1`` when there is none.  ``exclude_own``: source pixels that carry the query
    pixel's own label do not count (``labels_src`` is ``labels_qry``: the gap to the nearest OTHER patch).  ``limit2`` (an
    int >= 0, None: no limit): pairs with ``d2 > limit2`` do not count.  Neither plane is written; a non-contiguous view is
    made contiguous.  Sides <= 16384, ``h * w <= 2**31 - 2``.

    ``dt_proximity_columns`` (three launches: the column tables of ``labels_src``) -> ``dt_proximity_query`` (one launch:
    outward search along the rows, 64-bit ``atomicMin`` per patch).  No scalar is read back — n is the length of
    ``roots_qry`` — and the only download is the result; with n == 0 nothing is launched.  Workspace: the tables of
    ``proximity_tables`` and 4 bytes per pixel for the root -> row plane"""
    h, w, src, qry = _overlap_planes(labels_src, labels_qry, "patch_proximity")
    if limit2 is not None and (isinstance(limit2, bool) or int(limit2) != limit2 or limit2 < 0):
        raise RuntimeError(f"patch_proximity: limit2 must be an int >= 0 or None, got {limit2!r}")
    if max(h, w) > 16384:
        raise RuntimeError(f"patch_proximity: raster {h}x{w}: sides must be <= 16384 (column distances are uint16)")
    roots = roots_qry if isinstance(roots_qry, torch.Tensor) else torch.tensor(roots_qry)     # a copy: the table's is read-only
    if roots.dim() != 1 or roots.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"patch_proximity: roots_qry must be a one-dimensional integer array, got {roots.dtype} "
                           f"{tuple(roots.shape)}")
    n = int(roots.numel())
    if n == 0:
        return torch.zeros(0, dtype=torch.int64).numpy(), torch.zeros(0, dtype=torch.int64).numpy()
    if n > h * w:
        raise RuntimeError(f"patch_proximity: {n} roots for {h * w} pixels")
    roots = roots.to(src.device, torch.int64, non_blocking=True)
    tables = proximity_tables(src, second=bool(exclude_own))
    best = proximity_query(tables, qry, roots, bool(exclude_own), -1 if limit2 is None else int(limit2))
    none = best < 0
    out = torch.stack((torch.where(none, best, best >> 32), torch.where(none, best, best & 0xffffffff))).cpu().numpy()
    return out[0], out[1]


def patch_attributes(labels: torch.Tensor, roots, raster_u8: torch.Tensor, classes_u8: torch.Tensor = None,
                     probs: torch.Tensor = None, indices=()):
    """the attribute tables of the patches of a label plane int32 [h, w] on a HIP device (``label_patches``, sieved or not)
    over a planar raster uint8 [C, h, w] on its grid, 1 <= C <= 8 (contract in ``deployment/attributes.py``,
    csrc/attributes.hip): host arrays ``(sums int64 [n, Q], extremes int32 [n, M])`` in the layout of
    ``attributes.table_columns``, one row per element of ``roots`` (the ascending roots of the plane's table, a host array or a
    device tensor).  ``indices``: up to 4 band pairs ``(a, b)``, bands < C.  ``classes_u8`` uint8 [h, w] and ``probs`` fp32
    [K, h, w]: both or neither; with them the sum and the minimum of the quantised probability of every pixel's own class.
    No input is written; a non-contiguous view is made contiguous, a contiguous one is read where it lies.  Sides <= 16384,
    ``h * w <= 2**31 - 2``.

    ``dt_patch_attributes_u8``: one init launch, one pass over the pixels with one integer atomic per quantity and run of
    equal labels.  No scalar is read back — n is the length of ``roots`` — and the two tables are the only downloads; with
    n == 0 nothing is launched.  Workspace: 4 bytes per pixel for the root -> row plane"""
    h, w = _patch_planes("patch_attributes", labels=labels)
    dev = labels.device
    if max(h, w) > 16384 or h * w > 2 ** 31 - 2:
        raise RuntimeError(f"patch_attributes: raster {h}x{w}: sides must be <= 16384 and h * w <= {2 ** 31 - 2}")
    _gpu(raster_u8)
    if (raster_u8.dtype != torch.uint8 or raster_u8.dim() != 3 or tuple(raster_u8.shape[1:]) != (h, w)
            or not 1 <= raster_u8.shape[0] <= 8 or raster_u8.device != dev):
        raise RuntimeError(f"patch_attributes: raster must be uint8 [C, {h}, {w}] with 1 <= C <= 8 on {dev}, got "
                           f"{raster_u8.dtype} {tuple(raster_u8.shape)}")
    C_ = int(raster_u8.shape[0])
    pairs = [(int(a), int(b)) for a, b in indices]
    if len(pairs) > 4 or any(not (0 <= a < C_ and 0 <= b < C_) for a, b in pairs):
        raise RuntimeError(f"patch_attributes: indices must be at most 4 pairs of bands below {C_}, got {pairs}")
    if (classes_u8 is None) != (probs is None):
        raise RuntimeError("patch_attributes: probabilities come with their class map (classes_u8 and probs: both or neither)")
    K = 0
    if probs is not None:
        _patch_planes("patch_attributes", classes_u8, labels=labels)
        _gpu(probs)
        if (probs.dtype != torch.float32 or probs.dim() != 3 or tuple(probs.shape[1:]) != (h, w)
                or not 2 <= probs.shape[0] <= 8 or probs.device != dev):
            raise RuntimeError(f"patch_attributes: probs must be float32 [K, {h}, {w}] with 2 <= K <= 8 on {dev}, got "
                               f"{probs.dtype} {tuple(probs.shape)}")
        K = int(probs.shape[0])
        classes_u8, probs = classes_u8.contiguous(), probs.contiguous()
    roots = roots if isinstance(roots, torch.Tensor) else torch.tensor(roots)          # a copy: the table's is read-only
    if roots.dim() != 1 or roots.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"patch_attributes: roots must be a one-dimensional integer array, got {roots.dtype} "
                           f"{tuple(roots.shape)}")
    n = int(roots.numel())
    if n > h * w:
        raise RuntimeError(f"patch_attributes: {n} roots for {h * w} pixels")
    conf = probs is not None
    Q, M = 2 * C_ + len(pairs) + conf, 2 * C_ + conf
    if n == 0:
        return torch.zeros((0, Q), dtype=torch.int64).numpy(), torch.zeros((0, M), dtype=torch.int32).numpy()
    roots = roots.to(dev, torch.int64, non_blocking=True)
    dense = torch.full((h * w + 1,), -1, dtype=torch.int32, device=dev)      # the last entry takes the roots off the raster
    on_grid = (roots >= 0) & (roots < h * w)
    dense[torch.where(on_grid, roots, h * w)] = torch.arange(n, dtype=torch.int32, device=dev)
    sums = torch.empty((n, Q), dtype=torch.int64, device=dev)
    extremes = torch.empty((n, M), dtype=torch.int32, device=dev)
    flat = (C.c_int * max(1, 2 * len(pairs)))(*[v for pair in pairs for v in pair])
    _lib.check(_lib.load().dt_patch_attributes_u8(_p(labels.contiguous()), _p(raster_u8.contiguous()), C_, h, w, _p(dense), n,
                                                  _p(classes_u8), _p(probs), K, flat, len(pairs), _p(sums), _p(extremes),
                                                  _st()), "dt_patch_attributes_u8")
    return sums.cpu().numpy(), extremes.cpu().numpy()


def _aligned(t: torch.Tensor, to: int = 16) -> torch.Tensor:
    """``t`` contiguous at an address that is a multiple of ``to`` (a view at an odd storage offset is copied)"""
    t = t.contiguous()
    return t if t.data_ptr() % to == 0 else t.clone()


def _crown_limits(what: str, h: int, w: int):
    if max(h, w) > 16384 or h * w > 2 ** 31 - 2:
        raise RuntimeError(f"{what}: raster {h}x{w}: sides must be <= 16384 and h * w <= {2 ** 31 - 2}")


def patch_depth2(classes_u8: torch.Tensor, K: int, cap2: int = 65535, err=None, core2=None):
    """the depth plane of a uint8 class map [h, w] on the device (``dt_patch_depth2_u8``; step 1 of the contract in
    ``deployment/crowns.py``): int32 [h, w], 0 on class 0, elsewhere ``min(cap2, squared distance to the nearest pixel inside
    the raster of another class)``.  Returns ``(depth2, err)``; with ``core2`` (E) ``(depth2, core, err)``, ``core`` uint8
    [h, w] the class where ``depth2 >= core2``, written in the same pass.  No host synchronisation: a class >= K ORs 1 into
    ``err`` and has depth 0.  The map is not written.  Four launches; workspace 2 bytes per pixel (the column distances) and
    16 bytes per column and segment of ``CROWN_SEGMENT`` rows"""
    h, w = _patch_planes("patch_depth2", classes_u8)
    _crown_limits("patch_depth2", h, w)
    for name, v in (("cap2", cap2),) + ((("core2", core2),) if core2 is not None else ()):
        if isinstance(v, bool) or int(v) != v or not 1 <= v <= 2 ** 30:
            raise RuntimeError(f"patch_depth2: {name} must be an integer in 1..2**30, got {v!r}")
    if core2 is not None and core2 > cap2:
        raise RuntimeError(f"patch_depth2: core2={core2} above cap2={cap2}")
    dev = classes_u8.device
    err = _err_flag("patch_depth2", err, dev)
    column = torch.empty((h, w), dtype=torch.int16, device=dev)                     # read as uint16 by the kernels
    carry = torch.empty((-(-h // _constant("CROWN_SEGMENT")), w, 4), dtype=torch.int32, device=dev)
    depth2 = torch.empty((h, w), dtype=torch.int32, device=dev)
    core = None if core2 is None else torch.empty((h, w), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().dt_patch_depth2_u8(_p(classes_u8.contiguous()), h, w, int(K), int(cap2),
                                              int(core2 if core2 is not None else 1), _p(column), _p(carry), _p(depth2),
                                              _p(core), _p(err), _st()), "dt_patch_depth2_u8")
    return (depth2, err) if core2 is None else (depth2, core, err)


def split_patches(classes_u8: torch.Tensor, labels: torch.Tensor, K: int, connectivity: int, config, err=None):
    """the crown plane of a uint8 class map [h, w] and its label plane on the device (csrc/crowns.hip; contract in
    ``deployment/crowns.py``): ``(crowns int32 [h, w], depth2 int32 [h, w], crown_depth int32 [h * w], flags int32 [3])`` —
    ``crowns`` keeps the label contract (a crown's label names its first pixel), ``crown_depth`` holds at every crown's root
    the largest ``depth2`` of its pixels (``crowns.crown_depths_host``), ``flags`` = (1 if a class >= K was met, 1 if the
    growth has NOT converged, the growth rounds that labelled a pixel).  ``labels`` is the plane ``label_patches`` gave for
    ``classes_u8`` (after the sieve); neither input is written.

    ``patch_depth2`` (depth and cores in one pass) -> ``label_patches`` on the cores -> ``dt_crown_grow`` once per round, in
    groups of ``CROWN_ROUND_GROUP`` with no synchronisation inside a group; after a group the host reads the group's flag
    slots (ONE small read-back per group) and stops when the last round of the group labelled nothing: later rounds would be
    no-ops -> ``dt_crown_remainder`` -> ``label_patches`` on the remainder -> ``dt_crown_merge`` -> ``dt_crown_relabel``.
    Workspace per pixel while it runs: 24 bytes of int32 planes (depth2, the two growth planes — one ends as ``crowns``,
    the other as the merge's first-pixel plane —, the remainder's labels, the per-seg depth and ``crown_depth``) and 4 bytes
    of narrow ones (column distances, cores, remainder); 12 bytes per pixel are returned"""
    from .deployment.crowns import CrownConfig
    h, w = _patch_planes("split_patches", classes_u8, labels=labels)
    _crown_limits("split_patches", h, w)
    if not isinstance(config, CrownConfig):
        raise RuntimeError(f"split_patches: config must be a CrownConfig, got {config!r}")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise RuntimeError(f"split_patches: connectivity must be 4 or 8, got {connectivity!r}")
    lib, dev = _lib.load(), classes_u8.device
    i32 = dict(dtype=torch.int32, device=dev)
    classes_u8 = _aligned(classes_u8, 4)
    flags = torch.zeros(3, **i32)
    depth2, core, _ = patch_depth2(classes_u8, K, config.depth_cap2, err=flags[0:1], core2=config.min_core2)
    src, _ = label_patches(core, K, connectivity, err=flags[0:1])
    src = _aligned(src)
    dst = torch.empty((h, w), **i32)
    rounds = done = 0
    stream = _st()
    while done < config.max_rounds:
        group = min(CROWN_ROUND_GROUP, config.max_rounds - done)
        slots = torch.zeros(group, **i32)
        for k in range(group):                                 # slot k of the group: 4 bytes each
            _lib.check(lib.dt_crown_grow(_p(classes_u8), _p(src), _p(dst), h, w, int(connectivity), _p(slots) + 4 * k, stream),
                       "dt_crown_grow")
            src, dst = dst, src
        done += group
        took = slots.tolist()                                  # the group's one read-back
        rounds += sum(1 for v in took if v)
        if took[-1] == 0:
            break
    flags[2] = rounds
    remainder = torch.empty((h, w), dtype=torch.uint8, device=dev)
    _lib.check(lib.dt_crown_remainder(_p(classes_u8), _p(src), h, w, int(connectivity), _p(remainder), _p(flags[1:2]), _st()),
               "dt_crown_remainder")
    seg, _ = label_patches(remainder, K, connectivity, err=flags[0:1])
    first = dst.view(-1).fill_(2 ** 31 - 1)
    depth = torch.zeros(h * w, **i32)
    crown_depth = torch.zeros(h * w, **i32)
    _lib.check(lib.dt_crown_merge(_p(src), _p(seg), _p(depth2), h, w, _p(first), _p(depth), _st()), "dt_crown_merge")
    _lib.check(lib.dt_crown_relabel(_p(seg), _p(first), _p(depth), h, w, _p(src), _p(crown_depth), _st()), "dt_crown_relabel")
    if err is not None:
        _err_flag("split_patches", err, dev).bitwise_or_(flags[0:1])
    return src, depth2, crown_depth, flags


def signed_distmap(labels: torch.Tensor, K: int):
    """int64 labels [B,H,W] -> (fp32 distance maps [B,K,H,W], err flag) — the boundary-loss maps of
    loss/losses.py:159-178 as attached by data/deadtreedata.py:182-185, computed exactly on the device."""
    _gpu(labels)
    if labels.dtype != torch.int64 or labels.dim() != 3:
        raise RuntimeError("signed_distmap: labels must be int64 [B,H,W]")
    B, H, W = labels.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.dt_signed_distmap_workspace(B, K, H, W)), dtype=torch.uint8, device=labels.device)
    dist = torch.empty((B, K, H, W), dtype=torch.float32, device=labels.device)
    err = torch.zeros(1, dtype=torch.int32, device=labels.device)
    _lib.check(lib.dt_signed_distmap(_p(labels.contiguous()), _p(dist), _p(ws), _p(err), B, K, H, W, _st()),
               "dt_signed_distmap")
    return dist, err


MAX_TRAINABLE_SEGMENTS = 64      # dt_adam_advance_ranges: one thread per trainable segment, one wave


class FlatAdam:
    """clip_grad_norm_(max_norm) + torch.optim.Adam on one flat buffer, two fused HIP passes
    (reference: configs/trainer/default.yaml:18 + segmodel.py:420-425).

    Every per-step scalar lives on the device: the step count ``t_dev`` (advanced by ``dt_adam_advance`` only when the
    step is not skipped — Lightning does not call ``optimizer.step`` when ``training_step`` returns None, so the bias
    correction must not move either), the learning rate ``lr_dev`` (refreshed by a stream-ordered fill when ``lr``
    changes) and the bias corrections.  The launch sequence is therefore identical for every step: no ATen algebra,
    no host synchronisation, capturable in a HIP graph."""

    def __init__(self, params: torch.Tensor, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_norm: float = 0.5):
        _gpu(params)
        self.p = params
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.lr, self.betas, self.eps, self.max_norm = lr, betas, eps, max_norm
        self.t = 0          # host mirror: number of step() calls (skipped steps included; the device count is t_dev)
        lib = _lib.load()
        dev = params.device
        self.rows = lib.dt_sumsq_rows(params.numel())
        self.partial = torch.empty(self.rows, dtype=torch.float64, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.coef = torch.ones(1, dtype=torch.float32, device=dev)
        self.t_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float64, device=dev)
        self._lr_on_dev = float(lr)
        self.hyper = torch.ones(3, dtype=torch.float32, device=dev)
        self.skip = torch.zeros(1, dtype=torch.int32, device=dev)
        # trainable ranges (set_trainable): None = the whole buffer with the one step count t_dev (the default launches).
        # Otherwise the buffer is partitioned into segments at every range boundary seen so far, each with its own device
        # step count (t_seg) and bias corrections (hyper_seg); the range table lists the trainable segments
        self._segments = None       # [(lo, hi)] partition of [0, n)
        self._trainable = None      # [bool] per segment
        self.t_seg = self.hyper_seg = self.table = None
        self._table_rows = self._table_n = self._max_len = 0

    def set_trainable(self, ranges=None):
        """Only the given [(lo, hi)] ranges of the flat buffer are clipped and updated (None = all).  torch.optim.Adam
        semantics for a parameter without a gradient: its m, v and step count stay — every range keeps its own device
        step count, so a range unfrozen after k steps starts with the step-1 bias correction.  Call outside graph
        capture; calling it again with the same ranges changes nothing (no new device tensors)."""
        n = self.p.numel()
        rng = [(0, n)] if ranges is None else sorted((int(lo), int(hi)) for lo, hi in ranges if int(hi) > int(lo))
        for lo, hi in rng:
            if lo < 0 or hi > n or lo % 4 or hi % 4 and hi != n:
                raise ValueError(f"trainable range [{lo}, {hi}) of a {n}-float buffer: ends must be multiples of 4")
        if self._segments is None and rng == [(0, n)]:
            return                      # all trainable, never partitioned: the default launches
        old = self._segments or [(0, n)]
        cuts = sorted({b for seg in old for b in seg} | {b for r in rng for b in r})
        segs = list(zip(cuts[:-1], cuts[1:]))
        trainable = [any(lo <= a and b <= hi for lo, hi in rng) for a, b in segs]
        # checked before any state changes: after the error the last ranges stay in force
        if not any(trainable):
            raise ValueError("set_trainable: no trainable range")
        if sum(trainable) > MAX_TRAINABLE_SEGMENTS:
            raise ValueError(f"set_trainable: {sum(trainable)} trainable segments (cut at every range end seen so far), "
                             f"at most {MAX_TRAINABLE_SEGMENTS}")
        if self._segments is None:
            self._segments = [(0, n)]
            self.t_seg = self.t_dev.clone()
            self.hyper_seg = self.hyper.clone()
        if segs == self._segments and trainable == self._trainable:
            return
        dev = self.p.device
        if segs != self._segments:      # a split segment hands its step count to both parts
            src = [next(i for i, (a, b) in enumerate(self._segments) if a <= lo and hi <= b) for lo, hi in segs]
            idx = torch.tensor(src, dtype=torch.int64, device=dev)
            self.t_seg = self.t_seg.index_select(0, idx)
            self.hyper_seg = self.hyper_seg.view(-1, 3).index_select(0, idx).reshape(-1).contiguous()
        self._set_partition(segs, trainable)

    def _set_partition(self, segs, trainable):
        """the range table of a partition: what the ranged kernels read (``table``, its rows, the longest range, the
        partial-sum buffer) is derived here from ``segs`` / ``trainable`` and from nothing else"""
        dev = self.p.device
        self._segments, self._trainable = segs, trainable
        table, row = [], 0
        lib = _lib.load()
        for si, ((lo, hi), tr) in enumerate(zip(segs, trainable)):
            if tr:
                table += [lo, hi, row, si]
                row += lib.dt_sumsq_rows(hi - lo)
        self.table = torch.tensor(table, dtype=torch.int64, device=dev)
        self._table_n = len(table) // 4
        self._table_rows = row
        self._max_len = max(hi - lo for (lo, hi), tr in zip(segs, trainable) if tr)
        if row > self.partial.numel():
            self.partial = torch.empty(row, dtype=torch.float64, device=dev)

    def reset_state(self, lr: Optional[float] = None):
        """a fresh torch.optim.Adam on the same parameters (the reference MultiStage's LR-reduce stage): moments and step
        counts back to zero, trainable ranges kept"""
        self.m.zero_()
        self.v.zero_()
        self.t_dev.zero_()
        if self.t_seg is not None:
            self.t_seg.zero_()
        self.t = 0
        if lr is not None:
            self.lr = float(lr)

    def state_dict(self) -> dict:
        """everything a continued run needs, on the host: the moments, the device step counts and bias corrections (per
        range too once ranges exist), the device learning rate, and the host fields.  The range table, its rows and the
        partial-sum buffer are not stored: ``load_state_dict`` derives them from the partition (host sync)."""
        sd = {name: getattr(self, name).detach().cpu() for name in ("m", "v", "t_dev", "hyper", "lr_dev")}
        if self._segments is not None:
            sd["t_seg"], sd["hyper_seg"] = self.t_seg.detach().cpu(), self.hyper_seg.detach().cpu()
        sd.update(t=int(self.t), lr=float(self.lr), betas=[float(b) for b in self.betas], eps=float(self.eps),
                  max_norm=None if self.max_norm is None else float(self.max_norm),
                  _segments=None if self._segments is None else [[int(a), int(b)] for a, b in self._segments],
                  _trainable=None if self._trainable is None else [bool(t) for t in self._trainable])
        return sd

    def check_state_dict(self, sd):
        """RuntimeError unless ``sd`` fits this buffer; reads only"""
        n = self.p.numel()
        want = {"m": n, "v": n, "t_dev": 1, "hyper": 3, "lr_dev": 1}
        segs = sd.get("_segments")
        if segs is not None:
            want.update(t_seg=len(segs), hyper_seg=3 * len(segs))
        for name, numel in want.items():
            if name not in sd:
                raise RuntimeError(f"FlatAdam: the state has no {name!r}")
            if sd[name].numel() != numel:
                raise RuntimeError(f"FlatAdam: state {name!r} of {sd[name].numel()} elements, this optimiser's has {numel}")
        if segs is not None:
            flags = sd.get("_trainable")
            cuts = [int(a) for a, _ in segs] + [int(segs[-1][1])] if segs else []
            if (not segs or cuts[0] != 0 or cuts[-1] != n or any(int(b) != c for (_, b), c in zip(segs, cuts[1:]))
                    or any(a >= b for a, b in zip(cuts[:-1], cuts[1:])) or flags is None or len(flags) != len(segs)
                    or not any(flags)):
                raise RuntimeError(f"FlatAdam: the saved ranges {segs} / {flags} do not partition a {n}-float buffer")
            if sum(bool(f) for f in flags) > MAX_TRAINABLE_SEGMENTS:
                raise RuntimeError(f"FlatAdam: {sum(bool(f) for f in flags)} trainable ranges, at most {MAX_TRAINABLE_SEGMENTS}")

    @torch.no_grad()
    def load_state_dict(self, sd):
        """continue where ``state_dict()`` was taken.  Every length is checked first (RuntimeError, nothing written).  The
        saved partition goes through ``set_trainable``'s table builder; then the values are copied INTO the existing device
        tensors — ``m``, ``v``, ``t_dev``, ``hyper`` and ``lr_dev`` are never rebound, so whoever holds them (a captured
        graph, a view) keeps seeing the optimiser's state.  The per-range tensors are rebound where their length changes,
        as ``set_trainable`` does: call outside graph capture and drop graphs captured on another partition."""
        self.check_state_dict(sd)
        dev = self.p.device
        segs = sd.get("_segments")
        if segs is None:
            self._segments = self._trainable = None
            self.t_seg = self.hyper_seg = self.table = None
            self._table_rows = self._table_n = self._max_len = 0
        else:
            segs = [(int(a), int(b)) for a, b in segs]
            for name, numel, like in (("t_seg", len(segs), self.t_dev), ("hyper_seg", 3 * len(segs), self.hyper)):
                if getattr(self, name) is None or getattr(self, name).numel() != numel:
                    setattr(self, name, torch.zeros(numel, dtype=like.dtype, device=dev))
            self._set_partition(segs, [bool(t) for t in sd["_trainable"]])
            self.t_seg.copy_(sd["t_seg"].to(dev, self.t_seg.dtype).view(-1))
            self.hyper_seg.copy_(sd["hyper_seg"].to(dev, self.hyper_seg.dtype).view(-1))
        for name in ("m", "v", "t_dev", "hyper", "lr_dev"):
            t = getattr(self, name)
            t.copy_(sd[name].to(dev, t.dtype).view(-1))
        self.t, self.lr = int(sd["t"]), float(sd["lr"])
        self.betas, self.eps = tuple(float(b) for b in sd["betas"]), float(sd["eps"])
        self.max_norm = None if sd["max_norm"] is None else float(sd["max_norm"])
        # what the device holds is the saved run's: sync_lr fills again exactly when that run's next step would have
        self._lr_on_dev = float(sd["lr_dev"].double().view(-1)[0])

    def sync_lr(self):
        """push a changed learning rate to the device (stream-ordered fill: the value travels as a kernel argument).
        Call OUTSIDE graph capture / before a replay."""
        if self._lr_on_dev != float(self.lr):
            self.lr_dev.fill_(float(self.lr))
            self._lr_on_dev = float(self.lr)

    def skip_from_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """device flag int32[1] = loss is NaN/Inf (segmodel.py:220-222); `loss` fp32 device scalar"""
        _gpu(loss)
        if loss.dtype != torch.float32:
            loss = loss.float()
        _lib.check(_lib.load().dt_skip_from_loss(_p(loss), _p(self.skip), _st()), "dt_skip_from_loss")
        return self.skip

    def steps_applied(self) -> int:
        """optimiser steps that were not skipped (host sync; with trainable ranges: the largest per-range count)"""
        if self.t_seg is not None:
            return int(self.t_seg.max().item())
        return int(self.t_dev.item())

    def step(self, grads: torch.Tensor, grad_scale: float = 1.0, skip_flag: Optional[torch.Tensor] = None,
             lr: Optional[float] = None, capturing: bool = False):
        lib = _lib.load()
        if lr is not None:
            self.lr = lr
        if not capturing:
            self.sync_lr()
        n = self.p.numel()
        st = _st()
        if skip_flag is None:          # stand-alone use: the non-finite-gradient guard of dt_clip_coef still applies
            skip_flag = self.skip.zero_()
        if self._segments is not None:  # trainable ranges: frozen parts are neither read nor written
            b1, b2 = self.betas
            _lib.check(lib.dt_sumsq_ranges(_p(grads), _p(self.table), self._table_n, self._table_rows, _p(self.partial), st),
                       "dt_sumsq_ranges")
            _lib.check(lib.dt_clip_coef(_p(self.partial), self._table_rows, float(self.max_norm or 0.0), float(grad_scale),
                                        _p(self.norm), _p(self.coef), _p(skip_flag), st), "dt_clip_coef")
            _lib.check(lib.dt_adam_advance_ranges(_p(self.t_seg), _p(self.table), self._table_n, _p(skip_flag),
                                                  _p(self.lr_dev), b1, b2, _p(self.hyper_seg), st), "dt_adam_advance_ranges")
            _lib.check(lib.dt_adam_step_ranges(_p(self.p), _p(grads), _p(self.m), _p(self.v), _p(self.table), self._table_n,
                                               self._max_len, _p(self.hyper_seg), b1, b2, self.eps, _p(self.coef),
                                               _p(skip_flag), st), "dt_adam_step_ranges")
            self.t += 1
            return self.norm
        _lib.check(lib.dt_sumsq(_p(grads), n, _p(self.partial), st), "dt_sumsq")
        _lib.check(lib.dt_clip_coef(_p(self.partial), self.rows, float(self.max_norm or 0.0), float(grad_scale),
                                    _p(self.norm), _p(self.coef), _p(skip_flag), st), "dt_clip_coef")
        b1, b2 = self.betas
        _lib.check(lib.dt_adam_advance(_p(self.t_dev), _p(skip_flag), _p(self.lr_dev), b1, b2, _p(self.hyper), st),
                   "dt_adam_advance")
        _lib.check(lib.dt_adam_step_dev(_p(self.p), _p(grads), _p(self.m), _p(self.v), n, _p(self.hyper), b1, b2,
                                        self.eps, _p(self.coef), _p(skip_flag), st), "dt_adam_step_dev")
        self.t += 1
        return self.norm


def parse_average(mode):
    """"swa" | "ema" | ("ema", decay) | ("swa",) -> (name, decay); ValueError otherwise"""
    name, decay = (mode, None) if isinstance(mode, str) else (tuple(mode) + (None,))[:2]
    if name == "swa" and not decay:
        return "swa", 0.0
    if name == "ema":
        decay = 0.999 if decay is None else float(decay)      # torch's get_ema_multi_avg_fn default
        if 0.0 <= decay <= 1.0:
            return "ema", decay
    raise ValueError(f"average {mode!r}: use 'swa' or ('ema', decay) with 0 <= decay <= 1")


class WeightAverager:
    """An averaged copy of a flat fp32 parameter buffer (``torch.optim.swa_utils.AveragedModel`` with
    ``get_swa_multi_avg_fn`` / ``get_ema_multi_avg_fn``, parameters only — BatchNorm buffers are not averaged).

    ``avg`` and the number of averaged models ``n_dev`` live on the parameters' device; ``update`` is one
    ``dt_weight_average`` call with nothing that changes on the host, so it can sit inside a captured step."""

    def __init__(self, params: torch.Tensor, mode="swa"):
        _gpu(params)
        if params.dtype != torch.float32 or params.dim() != 1 or not params.is_contiguous():
            raise RuntimeError("WeightAverager: a contiguous flat float32 parameter buffer")
        self.mode, self.decay = parse_average(mode)
        self.p = params
        self.avg = torch.zeros_like(params)
        self.n_dev = torch.zeros(1, dtype=torch.int64, device=params.device)

    def to(self, params: torch.Tensor) -> "WeightAverager":
        """follow the parameters after ``model.to(device)``: rebind to the new buffer, moving ``avg`` and the count"""
        _gpu(params)
        if params.numel() != self.avg.numel():
            raise RuntimeError(f"WeightAverager: {params.numel()} parameters, average of {self.avg.numel()}")
        self.p = params
        self.avg = self.avg.to(params.device)
        self.n_dev = self.n_dev.to(params.device)
        return self

    def update(self, skip_flag: Optional[torch.Tensor] = None, capturing: bool = False):
        """fold the current parameters into ``avg``; a set ``skip_flag`` leaves ``avg`` and the count alone.
        capturing: inside a HIP-graph capture (nothing differs: there is no host-side state to refresh)"""
        if self.p.device != self.avg.device:
            raise RuntimeError(f"WeightAverager: average on {self.avg.device}, parameters on {self.p.device}: "
                               "call averager.to(model.flat_params.data)")
        weight_average(self.avg, self.p, self.n_dev, self.mode, self.decay, skip_flag)

    @property
    def n_averaged(self) -> int:
        """number of models averaged so far (host sync)"""
        return int(self.n_dev.item())

    def copy_to(self, params: torch.Tensor):
        if params.device != self.avg.device:
            raise RuntimeError(f"WeightAverager: average on {self.avg.device}, target on {params.device}")
        if params.numel() != self.avg.numel():
            raise RuntimeError(f"WeightAverager: {params.numel()} parameters, average of {self.avg.numel()}")
        params.detach().view(-1).copy_(self.avg)

    def state_dict(self):
        return {"mode": self.mode, "decay": self.decay, "avg": self.avg.detach().cpu().clone(),
                "n_averaged": self.n_averaged}

    def load_state_dict(self, sd):
        if sd["avg"].numel() != self.avg.numel():
            raise RuntimeError(f"WeightAverager: state of {sd['avg'].numel()} floats, buffer of {self.avg.numel()}")
        self.mode, self.decay = parse_average((sd["mode"], sd["decay"]))
        self.avg.copy_(sd["avg"].to(self.avg.device, torch.float32).view(-1))
        self.n_dev.fill_(int(sd["n_averaged"]))
