"""The whole-tiles form of the Winograd fp32 kernel (conv_wino.hip, template parameter FULL: maps whose sides are multiples
of 16 carry no per-output validity in the epilogue) against the general (ragged) form of the same kernel, bit for bit.

There is no switch between the two forms, so they are compared by zero extension: a map of H x W (both multiples of 16) runs
the whole-tiles form; the same operands extended by one row and one column run the ragged form with the same tile origins,
and the extra pixels contribute exactly what the padding contributed before.  The outputs on [0:H, 0:W] must be equal
(`torch.equal`).  What "extended by one zero pixel" means per operand:
  * a nearest-x2 source (mode0 = 1) is extended by one SOURCE pixel, so the map and every full-resolution operand grow by 2;
  * with the fused input BatchNorm + ReLU a real pixel of value 0 would become relu(shift) — the extension value is -1e4 with
    positive scales, which the transform maps to exactly 0 (the value a padded pixel has);
  * the data gradient with the fused up-sampling backward (form 6) needs even maps: the gradient grows by 2, the
    half-resolution operands and outputs by 1, and the outputs are compared on the common region.
The first k-step of a tile starts its accumulators from the MFMA's zero operand (no clear after the epilogue); Cin = 16 makes
that peeled chunk pair the whole channel loop, Cin = 32 leaves one pair after it; B = 3 at 32 x 48 gives tiles_x != tiles_y
and, with 128 output channels, two channel blocks per spatial tile.

Statistics rows differ between the two runs (the extended map has more outputs), so they are checked against fp64 sums of the
whole-tiles output at the tolerances tests/test_winograd_gpu.py uses for the same quantities (1e-4 relative for the BatchNorm
sums and the BatchNorm-backward sums of forms 1 / 3, 1e-5 for form 6)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = -1.0e4     # relu(NEG * scale + shift) == 0 for the scales (>= 0.5) and shifts (|.| < 2) used here


def _ops():
    from deadtrees_amd import ops
    return ops


def ext(t, n=1, value=0.0):
    """NHWC tensor with n more rows and columns (at the bottom / right) filled with `value`"""
    return None if t is None else F.pad(t, (0, 0, 0, n, 0, n), value=value).contiguous()


def crop(t, H, W):
    return t[:, :H, :W, :]


def _layer(g, B, H, W, C0, C1, mode0, Cout, tf):
    """operands of one layer; H x W = the map (= 2 x the stored size of an up-sampled source 0)"""
    hs, ws = (H // 2, W // 2) if mode0 else (H, W)
    x = torch.randn((B, hs, ws, C0), generator=g).to(DEV)
    s1 = torch.randn((B, H, W, C1), generator=g).to(DEV) if C1 else None
    w = (torch.randn((3, 3, C0 + C1, Cout), generator=g) * (2.0 / (9 * (C0 + C1))) ** 0.5).to(DEV)
    sc = (0.5 + torch.rand(C0, generator=g)).to(DEV) if tf else None
    sh = (0.3 * torch.randn(C0, generator=g).clamp(-3, 3) + 0.2).to(DEV) if tf else None
    return x, s1, w, sc, sh


FWD_CASES = [  # B, H, W (the map), C0, C1, mode0, Cout, split, transform, join
    (2, 16, 16, 16, 0, 0, 64, 0, False, False),      # one tile, all four borders; the peel is the whole channel loop
    (3, 32, 48, 32, 0, 0, 128, 0, True, False),      # tiles_x != tiles_y, one pair after the peel, two channel blocks
    (2, 16, 16, 32, 32, 1, 64, 0, True, False),      # up-sampled source + second source, input transform
    (3, 32, 48, 256, 0, 0, 64, 0, False, False),     # 32 chunks
    (2, 32, 48, 64, 64, 1, 128, 64, False, False),   # split outputs (64 + 64), up-sampled source + skip
    (2, 16, 16, 64, 0, 0, 64, 0, True, False),       # Cin = 64 with the input transform
    (5, 64, 64, 16, 0, 0, 256, 0, True, False),      # 320 tiles on 256 workgroups: a second, partial round
    # form 2: gradient joins (out0 += ...)
    (2, 16, 16, 16, 0, 0, 64, 0, False, True),
    (3, 32, 48, 64, 0, 0, 128, 64, True, True),      # join into out0, plain store into out1, input transform
    (2, 32, 48, 256, 0, 0, 128, 0, False, True),
]


@pytest.mark.parametrize("B,H,W,C0,C1,mode0,Cout,split,tf,join", FWD_CASES)
def test_whole_tiles_forms_0_and_2_equal_the_ragged_form_bit_for_bit(B, H, W, C0, C1, mode0, Cout, split, tf, join):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + H + C0 + Cout + 7 * join)
    x, s1, w, sc, sh = _layer(g, B, H, W, C0, C1, mode0, Cout, tf)
    u = ops.winograd_weights(w)
    n = 2 if mode0 else 1                    # growth of the map and of every full-resolution operand
    base = torch.randn((B, H, W, split if split else Cout), generator=g).to(DEV) if join else None
    kw = dict(mode0=mode0, split=split, accumulate=join, want_stats=not join, in_scale=sc, in_shift=sh)
    o0, o1, st = ops.conv2d_winograd(x, u, src1=s1, out0=base.clone() if join else None, **kw)
    e0, e1, _ = ops.conv2d_winograd(ext(x, 1, NEG if tf else 0.0), u, src1=ext(s1, n),
                                    out0=ext(base, n) if join else None, **kw)
    assert e0.shape[1:3] == (H + n, W + n)
    assert torch.equal(o0, crop(e0, H, W))
    if split:
        assert torch.equal(o1, crop(e1, H, W))
    if join:
        return
    out = (torch.cat([o0, o1], -1) if split else o0).double().cpu()
    want1, want2 = out.sum(dim=(0, 1, 2)), (out * out).sum(dim=(0, 1, 2))
    np.testing.assert_allclose(st[0].double().sum(0).cpu(), want1, rtol=1e-4,
                               atol=1e-4 * float(out.abs().sum(dim=(0, 1, 2)).max()))
    np.testing.assert_allclose(st[1].double().sum(0).cpu(), want2, rtol=1e-4)


BNB_CASES = [  # join (form 3: stored activation + gradient join; else form 1: virtual activation), B, H, W, Cin, Cout
    (False, 2, 16, 16, 64, 64), (False, 3, 32, 48, 32, 128), (False, 2, 32, 48, 256, 64),
    (True, 3, 32, 48, 16, 64), (True, 2, 16, 16, 256, 128), (True, 2, 16, 16, 64, 64)]


@pytest.mark.parametrize("join,B,H,W,Cin,Cout", BNB_CASES)
def test_whole_tiles_forms_1_and_3_equal_the_ragged_form_bit_for_bit(join, B, H, W, Cin, Cout):
    ops = _ops()
    g = torch.Generator().manual_seed(11 + join + B * 100 + Cin + Cout)
    dy = torch.randn((B, H, W, Cin), generator=g).to(DEV)
    u = ops.winograd_weights((torch.randn((3, 3, Cin, Cout), generator=g) * 0.05).to(DEV))
    y = (torch.randn((B, H, W, Cout), generator=g) * 1.5 + 0.2).to(DEV)
    mean = y.mean(dim=(0, 1, 2)).contiguous()
    invstd = (1.0 / torch.sqrt(y.var(dim=(0, 1, 2), unbiased=False) + 1e-5)).contiguous()
    sc = (1 + 0.2 * torch.randn(Cout, generator=g)).to(DEV)
    sh = (0.2 * torch.randn(Cout, generator=g)).to(DEV)
    act = torch.relu(y * sc + sh) if join else None
    base = torch.randn((B, H, W, Cout), generator=g).to(DEV) if join else None

    def run(e):
        f = (lambda t: ext(t, 1)) if e else (lambda t: t)
        kw = dict(act=f(act), join_into=f(base).clone()) if join else dict(act_scale=sc, act_shift=sh)
        return ops.conv2d_winograd_bn_bwd(f(dy), u, f(y), mean, invstd, **kw)

    out, red = run(False)
    out_e, _ = run(True)
    assert torch.equal(out, crop(out_e, H, W))
    mask = (act > 0) if join else ((y * sc + sh) > 0)
    gm = torch.where(mask, out, torch.zeros_like(out)).double()
    want = torch.stack([gm.sum(dim=(0, 1, 2)),
                        (gm * ((y.double() - mean.double()) * invstd.double())).sum(dim=(0, 1, 2))]).cpu()
    got = red.double().sum(1).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-4 * float(want.abs().max()))


UP_CASES = [  # B, H, W (the gradient's map), Cy, cx (up-sampled part), sk (skip), x_only
    (2, 16, 16, 64, 64, 64, False), (3, 32, 48, 32, 128, 0, False), (2, 32, 48, 16, 64, 64, False),
    (3, 32, 48, 256, 64, 64, True)]


@pytest.mark.parametrize("B,H,W,Cy,cx,sk,x_only", UP_CASES)
def test_whole_tiles_form_6_equals_the_ragged_form_bit_for_bit(B, H, W, Cy, cx, sk, x_only):
    from deadtrees_amd import _lib
    ops = _ops()
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * 7 + H + cx + Cy)
    st = torch.cuda.current_stream().cuda_stream
    dy = torch.randn((B, H, W, Cy), generator=g).to(DEV)
    wd = ops.weight_flip_transpose((torch.randn((3, 3, cx + sk, Cy), generator=g) * 0.05).to(DEV))
    u = ops.winograd_weights(wd)
    yl = torch.randn((B, H // 2, W // 2, cx), generator=g).to(DEV)
    mu, istd = (0.1 * torch.randn(cx, generator=g)).to(DEV), (1 + 0.2 * torch.rand(cx, generator=g)).to(DEV)
    sc, sh = (1 + 0.3 * torch.randn(cx, generator=g)).to(DEV), (0.2 * torch.randn(cx, generator=g)).to(DEV)

    def run(dy_, yl_):
        Hh, Ww = dy_.shape[1], dy_.shape[2]
        d = _lib.ConvDesc(B, Hh, Ww, Cy, 0, 0, Hh, Ww, cx + sk, 3, 1, 1, cx, 0)
        assert lib.dt_conv2d_winograd_upsampled_dgrad_supported(C.byref(d))
        rows = lib.dt_conv2d_winograd_upsampled_dgrad_x_rows if x_only else lib.dt_conv2d_winograd_upsampled_dgrad_rows
        P = rows(C.byref(d))
        red = torch.empty(lib.dt_bn_stats_floats(P, cx), dtype=torch.float32, device=DEV)
        gx = torch.empty((B, Hh // 2, Ww // 2, cx), dtype=torch.float32, device=DEV)
        dskip = torch.empty((B, Hh, Ww, sk), dtype=torch.float32, device=DEV) if sk and not x_only else None
        fuse = _lib.BnBwdFuse(yl_.data_ptr(), mu.data_ptr(), istd.data_ptr(), sc.data_ptr(), sh.data_ptr())
        if x_only:
            rc = lib.dt_conv2d_winograd_upsampled_dgrad_x(C.byref(d), dy_.data_ptr(), u.data_ptr(), gx.data_ptr(),
                                                          red.data_ptr(), C.byref(fuse), st)
        else:
            rc = lib.dt_conv2d_winograd_upsampled_dgrad(C.byref(d), dy_.data_ptr(), u.data_ptr(), gx.data_ptr(),
                                                        dskip.data_ptr() if dskip is not None else None, red.data_ptr(),
                                                        C.byref(fuse), 1, st)
        _lib.check(rc, "dt_conv2d_winograd_upsampled_dgrad")
        torch.cuda.synchronize()
        return gx, dskip, red[:2 * P * cx].view(2, P, cx)

    gx, dskip, red = run(dy, yl)
    gx_e, dskip_e, _ = run(ext(dy, 2), ext(yl, 1))
    assert torch.equal(gx, crop(gx_e, H // 2, W // 2))
    if dskip is not None:
        assert torch.equal(dskip, crop(dskip_e, H, W))
    gm = torch.where((yl * sc + sh) > 0, gx, torch.zeros_like(gx)).double()
    want = torch.stack([gm.sum(dim=(0, 1, 2)),
                        (gm * ((yl.double() - mu.double()) * istd.double())).sum(dim=(0, 1, 2))]).cpu()
    got = red.double().sum(1).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * float(want.abs().max()))
