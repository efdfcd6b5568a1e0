"""Every capped launch of tests/grid_cap_cases.py past its cap, against a plain reference of the same operation.

Almost every non-convolution kernel runs on a capped grid with a grid-stride loop behind the cap, and the benchmark workload
is deep in that regime, while the other kernel tests stay below or exactly on the caps.  Here every kernel runs at
``cap * 256 + r`` items (some threads take two turns, some one) and at ``2 * cap * 256 + r'`` (a third turn), compared with
the fp64 composition (and at the bound) of its small-shape test; exact kernels must be bit-equal to numpy / torch.

Per-channel sums add 10 to 100 times more terms here than in the small-shape tests.  Their bound is the small-shape floor plus
the yardstick rule of tests/test_loss_kernels_gpu.py: 4 x the distance of the same formula, evaluated in fp32 on the CPU,
from fp64 (``_sum_bound``; measured error, floor and bound go to the parity report).

Every output lies in front of a guard band (NaN, or a byte pattern for integers) that is checked after the launches, and an
output a wrapper allocates starts out as that pattern as well: a write past the end, or an element no thread wrote, fails an
assertion.  Needs an MI355X."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grid_cap_cases as gcc
from test_bf16_gpu import close_bf16
from test_finetune_kernels_gpu import GUARD
from test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PATTERN = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


# ------------------------------------------------------------------------------------------------ guard bands
class _Guards:
    """Allocates device tensors in front of a guard band and checks the bands afterwards.  As the ``torch`` name of
    deadtrees_amd.ops it hands such tensors to the wrappers for the outputs they allocate (empty / empty_like / zeros /
    zeros_like); everything else is torch's."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def new(self, shape, dtype=torch.float32, zero=False, what="output"):
        shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
        n = math.prod(shape)
        fill = float("nan") if dtype.is_floating_point else PATTERN[dtype]
        buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        if zero:
            buf[:n] = 0
        self.made.append((buf, n, what))
        return buf[:n].view(shape)

    def empty(self, *size, dtype=torch.float32, device=None):
        return self.new(size[0] if len(size) == 1 else size, dtype)

    def zeros(self, *size, dtype=torch.float32, device=None):
        return self.new(size[0] if len(size) == 1 else size, dtype, zero=True)

    def empty_like(self, t):
        return self.new(t.shape, t.dtype)

    def zeros_like(self, t):
        return self.new(t.shape, t.dtype, zero=True)

    def check(self):
        torch.cuda.synchronize()
        for buf, n, what in self.made:
            band = buf[n:]
            ok = band.isnan() if buf.dtype.is_floating_point else band == PATTERN[buf.dtype]
            assert bool(ok.all()), f"{what} {tuple(buf.shape)} {buf.dtype}: {int((~ok).sum())} writes behind the used region"


@contextlib.contextmanager
def guarded():
    from deadtrees_amd import ops
    g = _Guards()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = torch
    g.check()


def _lib():
    from deadtrees_amd import _lib as L
    return L, L.load(), torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _report(line):
    from conftest import parity_report
    parity_report("[above cap] " + line)


def _sum_bound(tag, got, want64, want32, floor):
    """per-channel sums: |got - fp64| <= floor + 4 x |fp32-CPU - fp64| (max over channels); reports the figures"""
    err = float((got.double().cpu() - want64).abs().max())
    e32 = float((want32.double() - want64).abs().max())
    bound = floor + 4 * e32
    _report(f"{tag}: max abs err {err:.3e}, fp32-CPU {e32:.3e}, floor {floor:.3e}, bound {bound:.3e}, err/floor {err / floor:.3f}")
    assert err <= bound, (tag, err, floor, e32)


def _ratio(tag, err, bound):
    _report(f"{tag}: {err:.3e} (bound {bound:.1e})")
    assert err < bound, (tag, err, bound)


# ------------------------------------------------------------------------------------------------ dt_bn_act
@pytest.mark.parametrize("C,n_pix", gcc.BN_ACT_BELOW + gcc.BN_ACT)
def test_bn_act(C, n_pix):
    """relu 0 / 1 / 2, without, with a plain and with a scaled residual: C = 64 keeps one channel quad per thread, C = 48
    re-reads its coefficients in every turn (12 quads divide no grid stride used here).  Bound: the 1e-5 of
    test_batchnorm_train_forward_backward"""
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(C + n_pix)
    stride = min(-(-(n_pix * C // 4) // 256), gcc.EW_CAP) * 256
    assert (stride % (C // 4) == 0) == (C == 64)
    y = torch.randn((n_pix, C), generator=g) * 1.5 + 0.3
    res = torch.randn((n_pix, C), generator=g)
    sc, sh, rsc, rsh = (1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g),
                        1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g))
    main = y.double() * sc.double() + sh.double()
    side = {"none": None, "plain": res.double(), "scaled": res.double() * rsc.double() + rsh.double()}
    yd, rd, scd, shd, rscd, rshd = (t.to(DEV) for t in (y, res, sc, sh, rsc, rsh))
    worst = 0.0
    with guarded() as G:
        for relu in (0, 1, 2):
            for kind, r64 in side.items():
                out = G.new((n_pix, C), what=f"bn_act relu={relu} res={kind}")
                L.check(lib.dt_bn_act(_p(yd), _p(scd), _p(shd), _p(rd) if r64 is not None else None,
                                      _p(rscd) if kind == "scaled" else None, _p(rshd) if kind == "scaled" else None,
                                      _p(out), n_pix, C, relu, st), "dt_bn_act")
                want = torch.relu(main) if relu == 2 else main
                if r64 is not None:
                    want = want + r64
                if relu == 1:
                    want = torch.relu(want)
                e = rel_err(out.cpu(), want)
                worst = max(worst, e)
                assert e < 1e-5, (relu, kind, e)
    _ratio(f"bn_act C={C} n_pix={n_pix}: worst rel err of 9 forms", worst, 1e-5)


# ------------------------------------------------------------------------------------------------ BatchNorm backward, fp32
def _bn_backward_dev(G, dout, act, y, mean, invstd, gamma, asc, ash, want_dres, frozen):
    """ops.bn_backward on guarded buffers, with the frozen-statistics apply pass on request"""
    L, lib, st = _lib()
    n_pix, Cc = y.shape
    P = lib.dt_bn_bwd_rows(n_pix, Cc)
    red = G.new(lib.dt_bn_bwd_red_floats(n_pix, Cc), what="red")
    L.check(lib.dt_bn_bwd_reduce(_p(dout), _p(act), _p(y), _p(mean), _p(invstd), _p(asc), _p(ash), _p(red), n_pix, Cc, st),
            "dt_bn_bwd_reduce")
    dgamma, dbeta, dy = G.new(Cc, what="dgamma"), G.new(Cc, what="dbeta"), G.new((n_pix, Cc), what="dy")
    dres = G.new((n_pix, Cc), what="dres") if want_dres else None
    apply = lib.dt_bn_bwd_apply_frozen if frozen else lib.dt_bn_bwd_apply
    L.check(apply(_p(dout), _p(act), _p(y), _p(mean), _p(invstd), _p(gamma), _p(asc), _p(ash), _p(red), P, _p(dgamma),
                  _p(dbeta), _p(dy), _p(dres), 0, n_pix, Cc, st), "dt_bn_bwd_apply")
    return dy, dgamma, dbeta, dres


@pytest.mark.parametrize("C,n_pix", gcc.BN_BWD)
def test_bn_backward(C, n_pix):
    """dt_bn_act, dt_bn_bwd_reduce with grown row blocks and dt_bn_bwd_apply(_frozen) past the cap against the fp64 formulas
    of test_batchnorm_train_forward_backward (bounds 1e-5 / 2e-5 / 1e-6), statistics handed over from fp64 as in the
    partial-row-extremes tests; stored, virtual and no activation.  The ReLU masks are those of the fp32 arithmetic the
    kernels define (z = relu(y * scale + shift + res) as torch computes it in fp32): at 10^6 .. 10^7 elements an fp64 mask
    differs from it in a few elements, which is a property of the data, not of the kernels"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(C * 7 + n_pix % 1000)
    y = torch.randn((n_pix, C), generator=g) * 1.5 + 0.3
    res = torch.randn((n_pix, C), generator=g)
    dout = torch.randn((n_pix, C), generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    y64, d64, g64 = y.double(), dout.double(), gamma.double()
    mean = y64.mean(0)
    invstd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)
    sc64, sh64 = g64 * invstd, beta.double() - mean * g64 * invstd
    sc, sh = sc64.float(), sh64.float()
    xh = (y64 - mean) * invstd
    xh32 = (y - mean.float()) * invstd.float()
    virt = y * sc + sh                                  # fp32, the kernels' arithmetic
    z = torch.relu(virt + res)
    yd, dd, zd = y.to(DEV), dout.to(DEV), z.to(DEV)
    mu_d, is_d, ga_d, sc_d, sh_d = (t.float().to(DEV) for t in (mean, invstd, gamma, sc, sh))
    with guarded() as G:
        zg = ops.bn_act(yd, sc_d, sh_d, res=res.to(DEV), relu=True)
        _ratio(f"bn_backward C={C} n_pix={n_pix}: bn_act rel err", rel_err(zg.cpu(), torch.relu(y64 * sc64 + sh64 + res.double())),
               1e-5)
        for mode, mask in (("stored", z > 0), ("virtual", virt > 0), ("linear", None)):
            tag = f"bn_backward C={C} n_pix={n_pix} {mode}"
            gm = d64 if mask is None else torch.where(mask, d64, torch.zeros((), dtype=torch.float64))
            gm32 = gm.float()
            dbeta, dgamma = gm.sum(0), (gm * xh).sum(0)
            dy = g64 * invstd * (gm - dbeta / n_pix - xh * dgamma / n_pix)
            args = (dd, zd if mode == "stored" else None, yd, mu_d, is_d, ga_d, sc_d if mode == "virtual" else None,
                    sh_d if mode == "virtual" else None)
            got_dy, got_dg, got_db, got_res = _bn_backward_dev(G, *args, want_dres=True, frozen=False)
            _ratio(tag + ": dy rel err", rel_err(got_dy.cpu(), dy), 2e-5)
            _sum_bound(tag + " dbeta", got_db, dbeta, gm32.sum(0), 2e-5 * float(dbeta.abs().max()))
            _sum_bound(tag + " dgamma", got_dg, dgamma, (gm32 * xh32).sum(0), 2e-5 * float(dgamma.abs().max()))
            assert rel_err(got_res.cpu(), gm) < 1e-6
            del got_dy, got_res, dy
            if mode == "virtual":       # frozen statistics: dy = g * gamma * invstd, the sums as before
                fr_dy, fr_dg, fr_db, _ = _bn_backward_dev(G, *args, want_dres=False, frozen=True)
                _ratio(tag + ": frozen dy rel err", rel_err(fr_dy.cpu(), g64 * invstd * gm), 2e-5)
                assert torch.equal(fr_dg, got_dg) and torch.equal(fr_db, got_db)
                del fr_dy
            G.check()
            G.made.clear()


# ------------------------------------------------------------------------------------------------ BatchNorm backward, bf16
@pytest.mark.parametrize("C,n_pix", gcc.BN_BWD_BF16)
def test_bn_backward_bf16(C, n_pix):
    """dt_bn_bwd_reduce_bf16 with grown row blocks and dt_bn_bwd_apply_bf16 past the cap: the formulas and bounds of
    tests/test_bf16_gpu.py::_bn_backward_bf16 on the same bf16 operands, the three mask modes, the gradient join"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(n_pix % 97 + C)
    y = (torch.randn((n_pix, C), generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g)).to(BF)
    dout = torch.randn((n_pix, C), generator=g).to(BF)
    prev = torch.randn((n_pix, C), generator=g).to(BF)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    y64, d64 = y.double(), dout.double()
    mean = y64.mean(0)
    invstd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)
    sc, sh = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    z = torch.relu(y.float() * sc.float() + sh.float()).to(BF)          # what the forward stored / consumers saw
    xh = (y64 - mean) * invstd
    xh32 = (y.float() - mean.float()) * invstd.float()
    yd, dd, zd, prev_d = y.to(DEV), dout.to(DEV), z.to(DEV), prev.to(DEV)
    mu_d, is_d, ga_d, sc_d, sh_d = (t.float().to(DEV) for t in (mean, invstd, gamma, sc, sh))
    for mode in ("stored_act", "virtual_act", "linear"):
        tag = f"bn_backward_bf16 C={C} n_pix={n_pix} {mode}"
        gm = d64 if mode == "linear" else torch.where(z > 0, d64, torch.zeros((), dtype=torch.float64))
        gm32 = gm.float()
        dbeta, dgamma = gm.sum(0), (gm * xh).sum(0)
        dy = gamma.double() * invstd * (gm - dbeta / n_pix - xh * dgamma / n_pix)
        with guarded() as G:
            dres = G.new((n_pix, C), BF, what="dres")
            dres.copy_(prev_d)
            got_dy, got_dg, got_db, got_res = ops.bn_backward_bf16(
                dd, zd if mode == "stored_act" else None, yd, mu_d, is_d, ga_d,
                act_scale=sc_d if mode == "virtual_act" else None, act_shift=sh_d if mode == "virtual_act" else None, dres=dres)
        tol = 3e-5 * float(gm.abs().sum(0).max()) + 1e-4
        _sum_bound(tag + " dbeta", got_db, dbeta, gm32.sum(0), tol)
        _sum_bound(tag + " dgamma", got_dg, dgamma, (gm32 * xh32).sum(0), 4 * tol)
        close_bf16(got_dy.cpu().double(), dy, extra=1e-4)
        close_bf16(got_res.cpu().double(), prev.double() + gm)
        del got_dy, got_res, dy, dres


# ------------------------------------------------------------------------------------------------ max-pool
def _pool_reference(x, dtype=torch.float64):
    """NCHW relu'd values (many exact zeros: ties) -> (x as a leaf of `dtype`, its pooled map, a gradient for that map)"""
    g = torch.Generator().manual_seed(x.shape[1] + x.shape[2])
    leaf = x.to(dtype).requires_grad_(True)
    out = F.max_pool2d(leaf, 3, 2, 1)
    dout = torch.randn(out.shape, generator=g)
    return leaf, out, dout


def _nhwc(t, dtype=torch.float32):
    return t.detach().permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("C,H,W", gcc.MAXPOOL)
def test_maxpool(C, H, W):
    """dt_maxpool3x3s2 bit-equal to F.max_pool2d with the tie rule on many exact zeros (the argmax bytes are checked through
    the backward: autograd routes a tie to the first maximum); dt_maxpool3x3s2_bwd at the 1e-6 of
    test_maxpool_forward_backward_with_ties: the 2 x 2 kernel on even maps, the per-pixel kernel on odd ones, and the join"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = F.relu(torch.randn((1, C, H, W), generator=g))
    leaf, out, dout = _pool_reference(x)
    out.backward(dout.double())
    with guarded() as G:
        o, am = ops.maxpool3x3s2(_nhwc(x))
        assert torch.equal(_nchw(o), out.detach().float())
        assert float((o == 0).float().mean()) > 0.001                     # windows of zeros only: every tap ties
        dx = ops.maxpool3x3s2_bwd(_nhwc(dout), am, H, W)
        _ratio(f"maxpool C={C} {H}x{W}: backward rel err", rel_err(_nchw(dx), leaf.grad), 1e-6)
        if C == 4:
            prev = torch.randn((1, H, W, C), generator=g)
            acc = G.new((1, H, W, C), what="joined dx")
            acc.copy_(prev)
            ops.maxpool3x3s2_bwd(_nhwc(dout), am, H, W, dx=acc)
            assert rel_err(_nchw(acc), leaf.grad + prev.permute(0, 3, 1, 2).double()) < 1e-6


@pytest.mark.parametrize("C,H,W", gcc.MAXPOOL_BF16)
def test_maxpool_bf16(C, H, W):
    """dt_maxpool3x3s2_bf16_amax and dt_maxpool3x3s2_bf16 bit-equal to F.max_pool2d on the bf16 values (with ties);
    dt_maxpool3x3s2_bwd_bf16 within one bf16 rounding (close_bf16, as test_maxpool_and_upsample_backward_bf16) of autograd.
    The reference runs in fp32: max-pooling is exact in any format, and a gradient pixel sums at most four bf16 values"""
    from deadtrees_amd import ops
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(C + W)
    x = F.relu(torch.randn((1, C, H, W), generator=g)).to(BF)
    leaf, out, dout = _pool_reference(x.float(), torch.float32)
    dout = dout.to(BF)
    out.backward(dout.float())
    xg = _nhwc(x, BF)
    with guarded() as G:
        pooled, am = ops.maxpool3x3s2_bf16(xg)
        assert torch.equal(_nchw(pooled).float(), out.detach())
        plain = G.new(pooled.shape, BF, what="pooled (no argmax)")
        L.check(lib.dt_maxpool3x3s2_bf16(_p(xg), _p(plain), 1, H, W, C, st), "dt_maxpool3x3s2_bf16")
        assert torch.equal(plain, pooled)
        dg = _nhwc(dout, BF)
        dx = ops.maxpool3x3s2_bwd_bf16(dg, am, H, W)
        close_bf16(_nchw(dx).float(), leaf.grad)
        if C == 8:
            prev = torch.randn((1, H, W, C), generator=g).to(BF)
            acc = G.new((1, H, W, C), BF, what="joined dx")
            acc.copy_(prev)
            ops.maxpool3x3s2_bwd_bf16(dg, am, H, W, dx=acc)
            close_bf16(_nchw(acc).float(), leaf.grad + prev.permute(0, 3, 1, 2).float())


def _masked_sums(act, grad, y, mean, invstd):
    """fp64 BatchNorm-backward sums over the pixels with act > 0, [n, C] operands in blocks of 2^20 pixels:
    (sum g, sum g * xhat, the largest per-channel sum |g|)"""
    Cc = y.shape[-1]
    act, grad, y = act.reshape(-1, Cc), grad.reshape(-1, Cc), y.reshape(-1, Cc)
    s0, s1, sa = (torch.zeros(Cc, dtype=torch.float64) for _ in range(3))
    for lo in range(0, y.shape[0], 1 << 20):
        hi = lo + (1 << 20)
        gm = torch.where(act[lo:hi] > 0, grad[lo:hi].double(), torch.zeros((), dtype=torch.float64))
        s0 += gm.sum(0)
        s1 += (gm * ((y[lo:hi].double() - mean.double()) * invstd.double())).sum(0)
        sa += gm.abs().sum(0)
    return s0, s1, float(sa.max())


# the join (acc) once per precision: the third-turn shapes hold 34 and 67 million elements
@pytest.mark.parametrize("bf,C,H,W,acc", [(False,) + gcc.MAXPOOL_BN[0] + (False,), (False,) + gcc.MAXPOOL_BN[0] + (True,),
                                          (False,) + gcc.MAXPOOL_BN[1] + (False,), (True,) + gcc.MAXPOOL_BN_BF16[0] + (False,),
                                          (True,) + gcc.MAXPOOL_BN_BF16[0] + (True,), (True,) + gcc.MAXPOOL_BN_BF16[1] + (False,)])
def test_maxpool_backward_bn(bf, C, H, W, acc):
    """dt_maxpool3x3s2_bwd_bn(_bf16) with exactly `cap` partial rows: the composition and the bounds of
    tests/test_kernels_gpu.py::_maxpool_backward_with_fused_batchnorm_sums — the gradient bit-identical to
    dt_maxpool3x3s2_bwd(_bf16) (compared with autograd above), the rows summed in fp64 equal to the BatchNorm-backward
    reduction of the pooled layer over that gradient"""
    from deadtrees_amd import ops
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(C + H * W % 1000 + acc)
    dt = BF if bf else torch.float32
    yraw = torch.randn((1, H, W, C), generator=g)
    sc, sh = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    mu, istd = 0.1 * torch.randn(C, generator=g), 1 + 0.2 * torch.rand(C, generator=g)
    xd = F.relu(yraw * sc + sh).to(dt).to(DEV)
    yd = yraw.to(dt).to(DEV)
    coef = [t.to(DEV) for t in (mu, istd, sc, sh)]
    with guarded() as G:
        pooled, am = ops.maxpool3x3s2_bf16(xd) if bf else ops.maxpool3x3s2(xd)
        del xd
        dout = torch.randn(pooled.shape, generator=g).to(dt).to(DEV)
        want = G.new((1, H, W, C), dt, what="dx of the plain kernel")
        dx = G.new((1, H, W, C), dt, what="dx of the fused kernel")
        if acc:
            prev = torch.randn((1, H, W, C), generator=g).to(dt).to(DEV)
            want.copy_(prev)
            dx.copy_(prev)
        L.check((lib.dt_maxpool3x3s2_bwd_bf16 if bf else lib.dt_maxpool3x3s2_bwd)(_p(dout), _p(am), _p(want), 1 if acc else 0, 1,
                                                                               H, W, C, st), "maxpool_bwd")
        rows = (lib.dt_maxpool3x3s2_bwd_bn_bf16_rows if bf else lib.dt_maxpool3x3s2_bwd_bn_rows)(1, H, W, C)
        assert rows == gcc.EW_CAP
        red = G.new(lib.dt_bn_stats_floats(rows, C), what="red")
        fuse = L.BnBwdFuse(_p(yd), *(_p(t) for t in coef))
        L.check((lib.dt_maxpool3x3s2_bwd_bn_bf16 if bf else lib.dt_maxpool3x3s2_bwd_bn)(
            _p(dout), _p(am), _p(dx), 1 if acc else 0, ctypes.byref(fuse), _p(red), 1, H, W, C, st), "maxpool_bwd_bn")
        assert torch.equal(dx, want)
        r = red[:2 * rows * C].view(2, rows, C).double().sum(1).cpu()
        grad = dx.cpu()
    assert not bool(r.isnan().any())
    yq = yraw.to(dt)
    act = yq.float() * sc + sh
    s0, s1, scale = _masked_sums(act.to(BF).float() if bf else act, grad, yq, mu, istd)
    tol = 1e-4 * scale
    _report(f"maxpool_backward_bn {'bf16' if bf else 'fp32'} C={C} {H}x{W} acc={acc}: sum g err "
            f"{float((r[0] - s0).abs().max()):.3e} (atol {tol:.3e}), sum g xhat err {float((r[1] - s1).abs().max()):.3e} "
            f"(atol {3 * tol:.3e})")
    np.testing.assert_allclose(r[0], s0, rtol=1e-4, atol=tol)
    np.testing.assert_allclose(r[1], s1, rtol=1e-4, atol=3 * tol)


# ------------------------------------------------------------------------------------------------ up-sampling backward
def _upsample_fused_sums(tag, dx, red, y, mean, invstd, sc, sh, bf):
    """the reduction check of tests/test_kernels_gpu.py::_upsample_backward_with_fused_bn_reduction, bounds unchanged"""
    act = (y.float() * sc + sh).to(BF).float() if bf else y * sc + sh
    s0, s1, scale = _masked_sums(act, dx.cpu(), y, mean, invstd)
    sums = red.double().sum(dim=1).cpu()
    assert not bool(sums.isnan().any())
    scale += 1.0
    e0, e1 = float((sums[0] - s0).abs().max()), float((sums[1] - s1).abs().max())
    _report(f"{tag}: sum g err {e0:.3e} (bound {3e-5 * scale:.3e}), sum g xhat err {e1:.3e} (bound {1e-4 * scale:.3e})")
    assert e0 <= 3e-5 * scale and e1 <= 1e-4 * scale


def _upsample_inputs(C, H, W, dtype):
    g = torch.Generator().manual_seed(H + W + C)
    dup = torch.randn((1, 2 * H, 2 * W, C), generator=g).to(dtype)
    y = (torch.randn((1, H, W, C), generator=g) * 1.3 + 0.1).to(dtype)
    mean = y.float().mean(dim=(0, 1, 2))
    invstd = 1.0 / torch.sqrt(y.float().var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    return g, dup, y, mean, invstd, gamma * invstd, beta - mean * gamma * invstd


@pytest.mark.parametrize("C,H,W", gcc.UPSAMPLE)
def test_upsample_backward(C, H, W):
    """dt_upsample2x_bwd against the fp64 2 x 2 sums at the 1e-6 of test_upsample_bwd_and_layout; dt_upsample2x_bwd_bn
    (`cap` partial rows) bit-identical to it, its sums as in test_upsample_backward_with_fused_bn_reduction"""
    from deadtrees_amd import ops
    _, dup, y, mean, invstd, sc, sh = _upsample_inputs(C, H, W, torch.float32)
    want = dup.double().reshape(1, H, 2, W, 2, C).sum(dim=(2, 4))
    with guarded():
        dx = ops.upsample2x_bwd(dup.to(DEV))
        _ratio(f"upsample_backward C={C} {H}x{W}: rel err", rel_err(dx.cpu(), want), 1e-6)
        fused, red = ops.upsample2x_bwd_bn(dup.to(DEV), y.to(DEV), mean.to(DEV), invstd.to(DEV), sc.to(DEV), sh.to(DEV))
        assert red.shape[1] == gcc.EW_CAP and torch.equal(fused, dx)
    _upsample_fused_sums(f"upsample_backward_bn C={C} {H}x{W}", fused, red, y, mean, invstd, sc, sh, False)


@pytest.mark.parametrize("C,H,W", gcc.UPSAMPLE_BF16)
def test_upsample_backward_bf16(C, H, W):
    """dt_upsample2x_bwd_bf16, its joining form dt_upsample2x_bwd_acc_bf16 (one launcher) and dt_upsample2x_bwd_bn_bf16"""
    from deadtrees_amd import ops
    L, lib, st = _lib()
    g, dup, y, mean, invstd, sc, sh = _upsample_inputs(C, H, W, BF)
    want = dup.double().reshape(1, H, 2, W, 2, C).sum(dim=(2, 4))
    dd = dup.to(DEV)
    with guarded() as G:
        dx = ops.upsample2x_bwd_bf16(dd)
        close_bf16(dx.cpu().double(), want)
        prev = torch.randn((1, H, W, C), generator=g).to(BF)
        acc = G.new((1, H, W, C), BF, what="joined dx")
        acc.copy_(prev)
        L.check(lib.dt_upsample2x_bwd_acc_bf16(_p(dd), _p(acc), 1, 1, H, W, C, st), "dt_upsample2x_bwd_acc_bf16")
        close_bf16(acc.cpu().double(), want + prev.double())
        fused, red = ops.upsample2x_bwd_bn(dd, y.to(DEV), mean.to(DEV), invstd.to(DEV), sc.to(DEV), sh.to(DEV))
        assert red.shape[1] == gcc.EW_CAP and torch.equal(fused, dx)
    _upsample_fused_sums(f"upsample_backward_bn_bf16 C={C} {H}x{W}", fused, red, y, mean, invstd, sc, sh, True)


# ------------------------------------------------------------------------------------------------ exact element-wise kernels
@pytest.mark.parametrize("B,C,H,W", gcc.LAYOUT)
def test_layout_shuttles(B, C, H, W):
    from deadtrees_amd import ops
    x = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(B))
    with guarded():
        nhwc = ops.nchw_to_nhwc(x.to(DEV))
        assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous())
        assert torch.equal(ops.nhwc_to_nchw(nhwc).cpu(), x)


@pytest.mark.parametrize("n_pix", gcc.NORMALIZE)
def test_normalize_u8(n_pix):
    """bit-equal to (x - 255 mean) * (1 / (255 std)) in fp32, the formula of oracle/augment_ref.py"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    src = np.random.default_rng(n_pix).integers(0, 256, (n_pix, 4), dtype=np.uint8)
    m = np.asarray(MEAN[:3], np.float32) * np.float32(255.0)
    inv = np.float32(1.0) / (np.asarray(STD[:3], np.float32) * np.float32(255.0))
    with guarded():
        got = ops.normalize_u8(torch.from_numpy(src).to(DEV), MEAN, STD, 3)
        assert np.array_equal(got.cpu().numpy(), (src[:, :3].astype(np.float32) - m) * inv)


@pytest.mark.parametrize("n", gcc.BAND)
def test_band_has_data(n):
    """blank bands of 0 / 255 with one informative byte: nowhere, the very last byte, one byte of the wrapped part only
    (between cap * 256 and n), and the first byte"""
    from deadtrees_amd import ops
    cap = gcc.EW_CAP * 256
    blank = torch.from_numpy(np.where(np.random.default_rng(n).random(n) < 0.5, 0, 255).astype(np.uint8)).to(DEV)
    with guarded():
        assert int(ops.band_has_data(blank)) == 0
        for at in (n - 1, cap * (n // cap) + 13, 0):
            band = blank.clone()
            band[at] = 7
            assert int(ops.band_has_data(band)) == 1, at
            assert int(ops.band_has_data(band[:at])) == 0 if at else True


def _slice_case(lib_fn, G, Cn, Cw, off, n_pix, dtype):
    """to the wide tensor, back, and back accumulating; the joins add in fp32 and round once"""
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(Cn + n_pix % 1000)
    narrow = torch.randn((n_pix, Cn), generator=g).to(dtype)
    base = torch.randn((n_pix, Cw), generator=g).to(dtype)
    prev = torch.randn((n_pix, Cn), generator=g).to(dtype)
    fn = getattr(lib, lib_fn)
    wide = G.new((n_pix, Cw), dtype, what="wide")
    wide.copy_(base)
    L.check(fn(_p(narrow.to(DEV)), _p(wide), n_pix, Cn, Cw, off, 1, 0, st), lib_fn)
    want = base.clone()
    want[:, off:off + Cn] = narrow
    assert torch.equal(wide.cpu(), want)
    back = G.new((n_pix, Cn), dtype, what="narrow")
    L.check(fn(_p(wide), _p(back), n_pix, Cn, Cw, off, 0, 0, st), lib_fn)
    assert torch.equal(back.cpu(), narrow)
    acc = G.new((n_pix, Cn), dtype, what="narrow, joined")
    acc.copy_(prev)
    L.check(fn(_p(wide), _p(acc), n_pix, Cn, Cw, off, 0, 1, st), lib_fn)
    assert torch.equal(acc.cpu(), (prev.float() + narrow.float()).to(dtype))


@pytest.mark.parametrize("Cn,Cw,off,n_pix", gcc.SLICE)
def test_channel_slice(Cn, Cw, off, n_pix):
    with guarded() as G:
        _slice_case("dt_channel_slice", G, Cn, Cw, off, n_pix, torch.float32)


@pytest.mark.parametrize("Cn,Cw,off,n_pix", gcc.SLICE_BF16)
def test_channel_slice_bf16(Cn, Cw, off, n_pix):
    with guarded() as G:
        _slice_case("dt_channel_slice_bf16", G, Cn, Cw, off, n_pix, BF)


@pytest.mark.parametrize("n", gcc.F32_BF16)
def test_precision_converters(n):
    """dt_f32_to_bf16 bit-equal to torch's round-to-nearest-even, dt_bf16_to_f32 to the exact widening"""
    L, lib, st = _lib()
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)) * 100.0
    with guarded() as G:
        down = G.new(n, BF, what="bf16")
        L.check(lib.dt_f32_to_bf16(_p(x.to(DEV)), _p(down), n, st), "dt_f32_to_bf16")
        assert torch.equal(down.cpu(), x.to(BF))
        up = G.new(n, what="f32")
        L.check(lib.dt_bf16_to_f32(_p(down), _p(up), n, st), "dt_bf16_to_f32")
        assert torch.equal(up.cpu(), x.to(BF).float())


@pytest.mark.parametrize("C,n_pix", gcc.BN_ACT_BF16)
def test_bn_act_bf16(C, n_pix):
    """the two forms and the bound (close_bf16) of tests/test_bf16_gpu.py::test_bn_act_bf16"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(C + n_pix % 1000)
    y = torch.randn((n_pix, C), generator=g)
    res = torch.randn((n_pix, C), generator=g).to(BF)
    sc, sh = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rsc, rsh = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    yb = y.to(BF)
    want = torch.relu(yb.double() * sc.double() + sh.double() + res.double() * rsc.double() + rsh.double())
    with guarded():
        got = ops.bn_act_bf16(yb.to(DEV), sc.to(DEV), sh.to(DEV), res.to(DEV), rsc.to(DEV), rsh.to(DEV))
        close_bf16(got.cpu().double(), want)
        got32 = ops.bn_act_bf16(y.to(DEV), sc.to(DEV), sh.to(DEV), relu=False)          # fp32 input (stem), no residual
        close_bf16(got32.cpu().double(), y.double() * sc.double() + sh.double())


@pytest.mark.parametrize("k,Cin,Cout", gcc.PACK_DGRAD)
def test_pack_dgrad_weights_bf16(k, Cin, Cout):
    """the data-gradient weight image: the HWIO tensor rounded to bf16 with the taps reversed, bit for bit"""
    from deadtrees_amd import ops
    w = torch.randn((k, k, Cin, Cout), generator=torch.Generator().manual_seed(Cin)) * 0.05
    with guarded():
        got = ops.pack_weights_bf16(w.to(DEV), dgrad=True)
        assert torch.equal(got.cpu(), w.reshape(k * k, Cin, Cout).flip(0).to(BF))


@pytest.mark.parametrize("B,H,W,Cin", gcc.STEM_S2D)
def test_stem_space_to_depth_bf16(B, H, W, Cin):
    """dt_stem_s2d_bf16: channel (a * 2 + b) * 4 + c of pixel (u, v) is bf16(x[2u + a, 2v + b, c]), zero for c >= Cin"""
    L, lib, st = _lib()
    x = torch.randn((B, H, W, Cin), generator=torch.Generator().manual_seed(B + Cin))
    with guarded() as G:
        out = G.new((B, H // 2, W // 2, 16), BF, what="space-to-depth image")
        L.check(lib.dt_stem_s2d_bf16(_p(x.to(DEV)), _p(out), B, H, W, Cin, st), "dt_stem_s2d_bf16")
        want = torch.zeros((B, H // 2, W // 2, 2, 2, 4), dtype=BF)
        want[..., :Cin] = x.to(BF).view(B, H // 2, 2, W // 2, 2, Cin).permute(0, 1, 3, 2, 4, 5)
        assert torch.equal(out.cpu(), want.view(B, H // 2, W // 2, 16))


# ------------------------------------------------------------------------------------------------ augmentation, pool gather
def _views(H, W):
    return [(f, r) for f in (0, 1, 2) for r in ((0, 1, 2, 3) if H == W else (0, 2))]


def _draws(rng, B):
    return np.array([[1.0, 0.0] if b % 2 == 0 else [1 + rng.uniform(-.15, .15), rng.uniform(-.2, .2)] for b in range(B)],
                    np.float32)


def _check_transformed(got, tile, f, r, al, be, c_dst, what):
    """exact where the brightness / contrast draw is (1, 0); elsewhere the cap of tests/test_surface_gpu.py (<= 1 grey level,
    < 1 % of the entries off by more than 1e-3 grey level) — a miscounted byte sum moves the LUT by whole grey levels"""
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    want = A.train_transform(tile, f, r, al, be, MEAN, STD, c_dst)
    if al == 1.0 and be == 0.0:
        assert np.array_equal(got, want), what
    else:
        diff = np.abs(got - want) * (np.asarray(STD[:c_dst], np.float32) * 255.0)
        assert float(diff.max()) <= 1.0 + 1e-3 and float((diff > 1e-3).mean()) < 1e-2, what


@pytest.mark.parametrize("H,W", gcc.AUGMENT)
def test_augment(H, W):
    """dt_augment_normalize_u8 (byte sums and gather, both past their per-image caps) and dt_augment_labels against
    oracle/augment_ref.py for every flip x turn the tile shape allows: all twelve on square tiles, flips and half turns on
    520 x 516 and 740 x 712 (a quarter turn of a non-square tile is refused by the wrapper)"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    rng = np.random.default_rng(H + W)
    views = _views(H, W)
    B = len(views)
    tiles = rng.integers(0, 256, (B, H, W, 4), dtype=np.uint8)
    tiles[1] = np.clip(tiles[1].astype(np.int32) + 150, 0, 255)          # drives the LUT into the upper clip
    mask = rng.integers(0, 3, (B, H, W)).astype(np.int64)
    geo = torch.tensor(views, dtype=torch.int32, device=DEV)
    bc = _draws(rng, B)
    with guarded():
        got = ops.augment_normalize_u8(torch.from_numpy(tiles).to(DEV), geo, torch.from_numpy(bc).to(DEV), MEAN, STD, 3)
        gm = ops.augment_labels(torch.from_numpy(mask).to(DEV), geo)
    got, gm = got.cpu().numpy(), gm.cpu().numpy()
    for b, (f, r) in enumerate(views):
        _check_transformed(got[b], tiles[b], f, r, float(bc[b, 0]), float(bc[b, 1]), 3, (b, f, r))
        assert np.array_equal(gm[b], A.geometric(mask[b], f, r)), (b, f, r)


@pytest.mark.parametrize("H,W", gcc.POOL)
def test_pool_gather(H, W):
    """dt_pool_gather_batch / _combined (one launcher) with more than 1024 workgroups of pixel quads per image: image, mask
    and land-use map against oracle/augment_ref.py, as tests/test_pool_gpu.py::test_gather_matches_the_numpy_oracle"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from oracle import augment_ref as A
    rng = np.random.default_rng(H * 3 + W)
    N = 3
    images = rng.integers(0, 256, (N, H, W, 4), dtype=np.uint8)
    masks = rng.integers(0, 3, (N, H, W)).astype(np.uint8)
    lu = rng.integers(0, 6, (N, H, W)).astype(np.uint8)
    sums = images.reshape(N, -1).astype(np.int64).sum(axis=1)
    views = (_views(H, W)[1::2] + [(1, 0)])[:4]
    idx = np.array([2, 0, 2, 1], np.int32)
    bc = _draws(rng, len(views))
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (images, masks, lu, sums, idx, np.array(views, np.int32), bc)]
    with guarded():
        img, mask, lu_out, err = ops.pool_gather_batch(*dev, MEAN, STD, 4, 1)
        assert int(err) == 0
    img, mask, lu_out = img.cpu().numpy(), mask.cpu().numpy(), lu_out.cpu().numpy()
    for b, (f, r) in enumerate(views):
        s = int(idx[b])
        _check_transformed(img[b].transpose(1, 2, 0), images[s], f, r, float(bc[b, 0]), float(bc[b, 1]), 4, (b, f, r))
        assert np.array_equal(mask[b], A.geometric(np.minimum(masks[s], 1).astype(np.int64), f, r))
        assert np.array_equal(lu_out[b], A.geometric(lu[s].astype(np.int64), f, r))


# ------------------------------------------------------------------------------------------------ weight gradient, bf16 conv
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s,p", gcc.WGRAD)
def test_weight_gradient_tail(B, H, W, Cin, Cout, k, s, p):
    """the final wgrad_reduce_kernel of dt_conv2d_wgrad with more than 2048 x 256 weights (every 128 -> 512 .. 512 -> 512 layer):
    fp64 autograd and the 3e-6 of test_conv_wgrad"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(B + H + Cin * 7 + Cout)
    x = torch.randn((B, Cin, H, W), generator=g, dtype=torch.float64)
    wt = (torch.randn((Cout, Cin, k, k), generator=g, dtype=torch.float64) * 0.05).requires_grad_(True)
    y = F.conv2d(x, wt, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    with guarded():
        dw = ops.conv2d_wgrad(_nhwc(x), _nhwc(dy), k, s, p)
    _ratio(f"weight_gradient_tail {Cin}->{Cout} k{k} s{s}: rel err", rel_err(dw.cpu().permute(3, 2, 0, 1), wt.grad), 3e-6)


def test_conv_bf16_wide_layer_after_packing():
    """pack + convolution 512 -> 512 on a 4 x 4 map against the rounding reference of test_conv_bf16_forward_and_stats"""
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(512)
    x = torch.randn((1, 512, 4, 4), generator=g)
    w = torch.randn((512, 512, 3, 3), generator=g) * (2.0 / (512 * 9)) ** 0.5
    ref = F.conv2d(x.to(BF).double(), w.to(BF).double(), padding=1)
    with guarded():
        wp = ops.pack_weights_bf16(w.permute(2, 3, 1, 0).contiguous().to(DEV))
        assert torch.equal(wp.cpu(), w.to(BF).permute(2, 3, 0, 1).reshape(9, 512, 512))
        y, _, _ = ops.conv2d_bf16(_nhwc(x, BF), wp, 3, 1, 1, 512)
    close_bf16(_nchw(y.float()).double(), ref)


# ------------------------------------------------------------------------------------------------ optimiser
def _clip_fp64(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ with the total norm taken in fp64.  torch's own fp32 norm of 4 .. 8 million elements is
    8e-5 .. 2e-4 off (the kernels' is within 1e-7: double partial sums), and the first Adam steps turn a relative error d of
    the clipped gradient into up to d / 4 of the update where |g| is near eps — more than the update-size bound allows"""
    norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
    coef = min(1.0, float(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))
    for g in grads:
        g.mul_(coef)
    return norm


@pytest.mark.parametrize("n", gcc.ADAM)
def test_flat_adam(n):
    """FlatAdam (dt_adam_step_dev) against torch.optim.Adam at the sizes of a network's flat buffer: (a) three steps with
    clip_grad_norm_(0.5) and the bounds of test_flat_adam_matches_torch (norm 1e-5, against the fp64 norm; parameters 1e-6);
    (b) the update p - p0 without clipping at the 2e-6 of the update-size test, and dt_adam_step with the same scalars from
    the host bit-identical to it"""
    from deadtrees_amd import ops
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=3e-4)
    with guarded() as G:
        pg = G.new(n, what="parameters")
        pg.copy_(p0)
        fa = ops.FlatAdam(pg, lr=3e-4, max_norm=0.5)
        for step in range(3):
            grad = torch.randn(n, generator=g) * (1e-4 if step == 1 else 1.0)   # step 1: below the clip norm
            ref_p.grad = grad.clone()
            torch.nn.utils.clip_grad_norm_([ref_p], 0.5)
            opt.step()
            norm = fa.step(grad.to(DEV))
            assert float(norm) == pytest.approx(float(grad.double().norm()), rel=1e-5)
        _ratio(f"flat_adam n={n}: parameters rel err after 3 clipped steps", rel_err(pg.cpu(), ref_p.detach()), 1e-6)
    p0 = 1e-3 * torch.randn(n, generator=g)     # small parameters: the update (3e-4) is far above the fp32 grid of p
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=3e-4)
    with guarded() as G:
        pg = G.new(n, what="parameters")
        pg.copy_(p0)
        host = [G.new(n, zero=z, what=w) for z, w in ((False, "parameters (host scalars)"), (True, "m"), (True, "v"))]
        host[0].copy_(p0)
        fa = ops.FlatAdam(pg, lr=3e-4, max_norm=0.0)
        for t in (1, 2):
            grad = torch.randn(n, generator=g)
            ref_p.grad = grad.clone()
            opt.step()
            gd = grad.to(DEV)
            fa.step(gd)
            L.check(lib.dt_adam_step(_p(host[0]), _p(gd), _p(host[1]), _p(host[2]), n, 3e-4, 0.9, 0.999, 1e-8,
                                     float(np.float32(1.0 - 0.9 ** t)), float(np.float32(1.0 - 0.999 ** t)), None, None, st),
                    "dt_adam_step")
            upd, upd_ref = (pg.cpu() - p0).double(), (ref_p.detach() - p0).double()
            _ratio(f"flat_adam n={n} step {t}: update err / largest update",
                   float((upd - upd_ref).abs().max()) / float(upd_ref.abs().max()), 2e-6)
        assert torch.equal(host[0], pg) and torch.equal(host[1], fa.m) and torch.equal(host[2], fa.v)


def test_flat_adam_trainable_ranges():
    """dt_adam_step_ranges: two trainable ranges share the 4096 workgroups, so each wraps beyond 2048 x 256 quads (1.3 and
    2.1 turns); the frozen middle keeps parameters and moments bit for bit.  torch.optim.Adam over the two slices, clipped
    by their joint norm (_clip_fp64), at the 2e-6 of the update-size test"""
    from deadtrees_amd import ops
    n, ranges = gcc.ADAM_RANGES
    g = torch.Generator().manual_seed(10)
    p0 = 1e-3 * torch.randn(n, generator=g)
    refs = [p0[lo:hi].clone().requires_grad_(True) for lo, hi in ranges]
    opt = torch.optim.Adam(refs, lr=3e-4)
    with guarded() as G:
        pg = G.new(n, what="parameters")
        pg.copy_(p0)
        fa = ops.FlatAdam(pg, lr=3e-4, max_norm=0.5)
        fa.set_trainable(ranges)
        for step in range(2):
            grad = torch.randn(n, generator=g)
            for r, (lo, hi) in zip(refs, ranges):
                r.grad = grad[lo:hi].clone()
            want_norm = _clip_fp64([r.grad for r in refs], 0.5)
            opt.step()
            assert float(fa.step(grad.to(DEV))) == pytest.approx(want_norm, rel=1e-5)
        got = pg.cpu()
        for r, (lo, hi) in zip(refs, ranges):
            upd, upd_ref = (got[lo:hi] - p0[lo:hi]).double(), (r.detach() - p0[lo:hi]).double()
            _ratio(f"flat_adam ranges [{lo}, {hi}): update err / largest update",
                   float((upd - upd_ref).abs().max()) / float(upd_ref.abs().max()), 2e-6)
        lo, hi = ranges[0][1], ranges[1][0]
        assert torch.equal(got[lo:hi], p0[lo:hi]) and not bool(fa.m[lo:hi].any()) and not bool(fa.v[lo:hi].any())


@pytest.mark.parametrize("mode,decay", [("swa", 0.0), ("ema", 0.99)])
def test_weight_average(mode, decay):
    """five updates at the optimiser's n against the fp64 recurrence, with the bound of tests/test_swa_gpu.py"""
    from deadtrees_amd import ops
    from test_swa_gpu import _assert_avg_close, _torch_avg
    n = gcc.ADAM[1]
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + (mode == "ema"))
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = torch.randn(n, generator=g, device=DEV)
    a64 = a32 = None
    with guarded() as G:
        avg = G.new(n, what="avg")
        for t in range(5):
            ops.weight_average(avg, p, count, mode, decay)
            a64, a32 = _torch_avg(a64, p.double(), t, mode, decay), _torch_avg(a32, p, t, mode, decay)
            p = p + 0.05 * torch.randn(n, generator=g, device=DEV)
        assert int(count) == 5
        _assert_avg_close(avg, a64, a32, f"above cap {mode} n={n}")


# ------------------------------------------------------------------------------------------------ votes, counts, sieve
@pytest.mark.parametrize("n", gcc.VOTE)
def test_ensemble_vote(n):
    """four models, three classes: 2 : 2 and 2 : 1 : 1 ties all over the map go to the smaller class"""
    from deadtrees_amd import ops
    from test_loss_kernels_gpu import _vote_ref
    maps = torch.from_numpy(np.random.default_rng(n).integers(0, 3, (4, n), dtype=np.uint8))
    maps[:2, -1], maps[2:, -1] = 2, 1                       # a planted tie in the very last pixel
    want = _vote_ref(maps, 3)
    assert int(want[-1]) == 1
    with guarded():
        got, err = ops.ensemble_vote(maps.to(DEV), 3, dtype="int64")
        assert int(err) == 0 and torch.equal(got.cpu(), want)
        got8, err = ops.ensemble_vote(maps.to(DEV), 3, dtype="uint8")
        assert int(err) == 0 and torch.equal(got8.cpu().long(), want)


@pytest.mark.parametrize("n", gcc.ZONAL)
def test_zonal_counts(n):
    """exact counts per zone and class, for maps at an aligned and at an odd address (head, vectors, tail; the zone map
    three bytes off the class map's alignment)"""
    from deadtrees_amd import ops
    rng = np.random.default_rng(n)
    classes, zones = rng.integers(0, 3, n + 8, dtype=np.uint8), rng.integers(0, 4, n + 8, dtype=np.uint8)
    dc, dz = torch.from_numpy(classes).to(DEV), torch.from_numpy(zones).to(DEV)
    for co, zo in ((0, 0), (5, 8), (0, 3)):
        c, z = classes[co:co + n], zones[zo:zo + n]
        want = np.bincount(z.astype(np.int64) * 3 + c, minlength=12).reshape(4, 3)
        with guarded():
            counts, err = ops.zonal_counts(dc[co:co + n], dz[zo:zo + n], 3, 4)
            assert int(err) == 0 and np.array_equal(counts.cpu().numpy(), want), (co, zo)
    with guarded():
        counts, err = ops.zonal_counts(dc[:n], None, 3, 1)
        assert int(err) == 0 and np.array_equal(counts.cpu().numpy()[0], np.bincount(classes[:n], minlength=3))


@pytest.mark.parametrize("h,w", gcc.SIEVE)
def test_sieve(h, w):
    """dt_sieve_patches_u8 on the labels and areas of ops.label_patches / ops.patch_areas (pinned to the host labelling in
    tests/test_patches_gpu.py; the host's union-find takes too long at 10^6 pixels) against numpy on those planes"""
    from deadtrees_amd import ops
    rng = np.random.default_rng(h + w)
    c = (rng.random((h, w)) < 0.45) * rng.integers(1, 3, (h, w))
    dc = torch.from_numpy(c.astype(np.uint8)).to(DEV)
    labels, err = ops.label_patches(dc, 3, 8)
    area = ops.patch_areas(labels)
    assert int(err) == 0
    l0, a0 = labels.cpu().numpy(), area.cpu().numpy()
    for m in (3, 40):
        small = (l0 > 0) & (a0[np.maximum(l0, 1) - 1] < m)
        assert 0 < small.sum() < (l0 > 0).sum()
        with guarded() as G:
            bufs = [G.new(t.shape, t.dtype, what=wt) for t, wt in ((dc, "classes"), (labels, "labels"), (area, "areas"))]
            for b, t in zip(bufs, (dc, labels, area)):
                b.copy_(t)
            ops.sieve_patches(*bufs, m)
            assert np.array_equal(bufs[0].cpu().numpy(), np.where(small, 0, c))
            assert np.array_equal(bufs[1].cpu().numpy(), np.where(small, 0, l0))
            assert np.array_equal(bufs[2].cpu().numpy(), np.where(a0 < m, 0, a0))


# ------------------------------------------------------------------------------------------------ stitching
@pytest.mark.parametrize("h,w,d,o,ny,nx", gcc.GATHER)
def test_window_gather(h, w, d, o, ny, nx):
    """dt_window_normalize_u8 (and dt_split_normalize_u8 through it): every window the slice of the zero-padded raster
    through the fp32 normalisation, bit for bit; three views are exact permutations of the plain window"""
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment.tiler import window_grid
    from test_tta_stitch_gpu import np_view
    assert window_grid(h, w, d, o)[:2] == (ny, nx)
    raster = np.random.default_rng(h + w + o).integers(0, 256, (4, h, w), dtype=np.uint8)
    dev_r = torch.from_numpy(raster).to(DEV)
    m = (np.asarray(MEAN[:3], np.float32) * np.float32(255.0))[:, None, None]
    inv = (np.float32(1.0) / (np.asarray(STD[:3], np.float32) * np.float32(255.0)))[:, None, None]

    def windows(s, my, mx):
        padded = np.zeros((3, (my - 1) * s + d, (mx - 1) * s + d), np.uint8)
        padded[:, :h, :w] = raster[:3]
        norm = (padded.astype(np.float32) - m) * inv
        return np.stack([norm[:, i * s:i * s + d, j * s:j * s + d] for i in range(my) for j in range(mx)])

    with guarded():
        got = ops.window_normalize_u8(dev_r, d, o, 0, ny * nx, MEAN, STD, 3).cpu().numpy().transpose(0, 3, 1, 2)
        want = windows(d - o, ny, nx)
        assert np.array_equal(got, want)
        by, bx, _ = window_grid(h, w, d, 0)
        blocks = ops.split_normalize_u8(dev_r, d, 0, by * bx, MEAN, STD, 3).cpu().numpy().transpose(0, 3, 1, 2)
        assert np.array_equal(blocks, windows(d, by, bx))
        views = [(0, 1), (1, 2), (2, 3)]
        tta = ops.window_normalize_u8(dev_r, d, o, 1, ny * nx - 2, MEAN, STD, 3, views=views).cpu().numpy()
        tta = tta.reshape(ny * nx - 2, 3, d, d, 3)
        for v, (f, r) in enumerate(views):
            assert np.array_equal(tta[:, v].transpose(0, 3, 1, 2), np_view(want[1:-1], f, r)), (f, r)


@pytest.mark.parametrize("h,w,d,o,K", gcc.STITCH)
def test_stitch_accumulate_and_finalize(h, w, d, o, K):
    """dt_stitch_accumulate and dt_stitch_finalize on rasters of more than ST_CAP * 256 pixels against the host oracle of
    tests/test_overlap_stitch_gpu.py, with its ACC_TOL, MARGIN and MAX_EXCLUDED; two batchings agree bit for bit"""
    from deadtrees_amd import ops
    from test_overlap_stitch_gpu import ACC_TOL, MARGIN, MAX_EXCLUDED, _logits, _oracle_acc
    logits = _logits(h, w, d, o, K)
    want = _oracle_acc(logits, h, w, d, o)
    top = np.sort(want, axis=0)
    decided = (top[-1] - top[-2]) > MARGIN
    excluded = 1.0 - float(decided.mean())
    assert excluded <= MAX_EXCLUDED, excluded              # the oracle alone (checked on the host for these seeds)
    dev = logits.to(DEV)
    with guarded() as G:
        acc, acc7 = G.new((K, h, w), zero=True, what="accumulator"), G.new((K, h, w), zero=True, what="accumulator, batches of 7")
        ops.stitch_accumulate(dev, acc, o, 0)
        for j in range(0, dev.shape[0], 7):
            ops.stitch_accumulate(dev[j:j + 7], acc7, o, j)
        assert torch.equal(acc, acc7)
        err = float(np.abs(acc.cpu().numpy().astype(np.float64) - want).max())
        classes, probs = ops.stitch_finalize(acc, want_probs=True)
        assert float((probs.sum(dim=0) - 1.0).abs().max()) <= 1e-6
        classes = classes.cpu().numpy()
    flips = int((classes != want.argmax(axis=0))[decided].sum())
    _report(f"stitch h{h} w{w} d{d} o{o} K{K}: accumulator max abs err vs fp64 {err:.3e} (bound {ACC_TOL:.0e}); class map: {flips} "
            f"flips on decided pixels, excluded share {excluded:.3e} (bound {MAX_EXCLUDED:.0e})")
    assert err <= ACC_TOL, err
    assert classes.dtype == np.uint8 and classes.shape == (h, w)
    assert flips == 0, flips


@pytest.mark.parametrize("h,w,d,o,K", gcc.STITCH[1:])
def test_stitch_classes(h, w, d, o, K):
    """dt_stitch_classes_u8: every raster pixel gets the byte of the one window whose kept region holds it, as
    test_crop_scatter_writes_each_kept_region_once, for two splits of the windows into calls"""
    from deadtrees_amd import ops
    from deadtrees_amd.deployment.tiler import window_grid, window_keep
    ny, nx, s = window_grid(h, w, d, o)
    n = ny * nx
    maps = torch.randint(0, 256, (n, d, d), generator=torch.Generator().manual_seed(h + w + o), dtype=torch.uint8)
    want = np.zeros(((ny - 1) * s + d, (nx - 1) * s + d), np.uint8)
    for k in range(n):
        i, j = divmod(k, nx)
        (y0, y1), (x0, x1) = window_keep(i, ny, d, o), window_keep(j, nx, d, o)
        want[y0:y1, x0:x1] = maps[k].numpy()[y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s]
    dev_maps = maps.to(DEV)
    for batch in (n, 3):
        with guarded() as G:
            out = G.new((h, w), torch.uint8, what="class map")
            for j in range(0, n, batch):
                ops.stitch_classes(dev_maps[j:j + batch], out, o, j)
            assert np.array_equal(out.cpu().numpy(), want[:h, :w]), batch
