"""Device code of the fine-tuning modes, kernel by kernel, against fp64 references and against the full launches they
narrow: the Winograd data gradient restricted to the up-sampled channels (frozen encoder, decoder blocks 1-3), the
eval-mode BatchNorm backward and statistics (encoder on running statistics) and the range optimiser (FlatAdam with
trainable ranges) against torch.optim.Adam.

Wide running statistics throughout (running_var log-uniform over [1e-2, 1e2]): eval-mode BatchNorm far from the identity,
so a mix-up of mean and variance, of layers or of eps moves every result."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
GUARD = 4096          # NaN floats behind every output buffer: an out-of-range write shows up as a finite value there


def _lib():
    from deadtrees_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n):
    """(view of n floats, the whole NaN-filled buffer): the caller checks buf[n:] after the launch"""
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf[:n], buf


def _band_untouched(buf, n, what):
    band = buf[n:]
    assert bool(band.isnan().all()), f"{what}: {int((~band.isnan()).sum())} writes behind the used region"


def _log_uniform(n, lo, hi, g):
    return torch.exp(torch.empty(n).uniform_(float(np.log(lo)), float(np.log(hi)), generator=g))


# ---------------------------------------------------------------- 1a. dt_conv2d_winograd_upsampled_dgrad_x
UPX_CASES = [   # B, H, W (the up-sampled input's resolution = dy's), Cy, cx, sk; x-only tiles = B * ceil(H/16) * ceil(W/16) * cx/64
    (1, 36, 20, 64, 128, 64),        # 12: B = 1, one round, ragged
    (2, 16, 16, 128, 256, 128),      # 8: one round
    (4, 64, 64, 128, 256, 128),      # 256: exactly one full round of the persistent grid
    (5, 64, 64, 128, 256, 128),      # 320: two rounds, the last one partial
    (4, 100, 84, 64, 128, 64),       # 336: maps not multiples of 16, partial last round
    (3, 130, 258, 32, 64, 64),       # 459: block 3's geometry, ragged, one channel block
    (32, 64, 64, 128, 256, 128),     # 2048: decoder block 1 of the benchmark (8 tiles per workgroup)
    (32, 128, 128, 64, 128, 64),     # 4096: decoder block 2 of the benchmark (16 tiles per workgroup)
    (32, 256, 256, 32, 64, 64),      # 8192: decoder block 3 of the benchmark (32 tiles per workgroup)
]
FP64_MAX_GFLOP = 13.0   # fp64 CPU reference of the data gradient only up to this size (the B=32 cases: full launch only)


def _upx_inputs(B, H, W, Cy, cx, sk, seed):
    from deadtrees_amd import ops
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn((B, H, W, Cy), generator=g)
    wt = torch.randn((3, 3, cx + sk, Cy), generator=g) * 0.05            # forward HWIO: (cx + sk) -> Cy
    u = ops.winograd_weights(ops.weight_flip_transpose(wt.to(DEV)))      # data-gradient image: Cy -> (cx + sk)
    # the layer below (raw output y at half resolution) on running statistics far from the identity
    rv = _log_uniform(cx, 1e-2, 1e2, g)
    rm = torch.randn(cx, generator=g) * rv.sqrt()
    yl = rm + rv.sqrt() * torch.randn((B, H // 2, W // 2, cx), generator=g)
    gamma = 1 + 0.5 * torch.randn(cx, generator=g)
    beta = 0.5 * torch.randn(cx, generator=g)
    istd = (1.0 / torch.sqrt(rv.double() + EPS)).float()
    sc = gamma * istd
    sh = beta - rm * sc
    return dy, wt, u, yl, rm, istd, sc, sh


def _upx_launch(d, dy, u, yl, mu, istd, sc, sh, x_only, sk):
    L, lib = _lib()
    B, H, W, cx = d.B, d.Hin, d.Win, d.cout_split
    P = (lib.dt_conv2d_winograd_upsampled_dgrad_x_rows if x_only else lib.dt_conv2d_winograd_upsampled_dgrad_rows)(C.byref(d))
    assert P > 0
    n_red = int(lib.dt_bn_stats_floats(P, cx))
    n_gx = B * (H // 2) * (W // 2) * cx
    red, red_buf = _guarded(n_red)
    gx, gx_buf = _guarded(n_gx)
    fuse = L.BnBwdFuse(yl.data_ptr(), mu.data_ptr(), istd.data_ptr(), sc.data_ptr(), sh.data_ptr())
    if x_only:
        L.check(lib.dt_conv2d_winograd_upsampled_dgrad_x(C.byref(d), dy.data_ptr(), u.data_ptr(), gx.data_ptr(),
                                                         red.data_ptr(), C.byref(fuse), _st()),
                "dt_conv2d_winograd_upsampled_dgrad_x")
        dskip = None
    else:
        dskip = torch.empty((B, H, W, sk), dtype=torch.float32, device=DEV)
        L.check(lib.dt_conv2d_winograd_upsampled_dgrad(C.byref(d), dy.data_ptr(), u.data_ptr(), gx.data_ptr(),
                                                       dskip.data_ptr(), red.data_ptr(), C.byref(fuse), 1, _st()),
                "dt_conv2d_winograd_upsampled_dgrad")
    torch.cuda.synchronize()
    what = "x-only" if x_only else "full"
    _band_untouched(gx_buf, n_gx, f"{what} gx")
    _band_untouched(red_buf, 2 * P * cx, f"{what} BatchNorm-backward rows")   # (the finalize scratch tail: not this kernel's)
    assert not bool(gx.isnan().any()), f"{what}: gx not fully written"
    rows = red[:2 * P * cx].view(2, P, cx)
    assert not bool(rows.isnan().any()), f"{what}: a partial row not written"
    return gx.view(B, H // 2, W // 2, cx), rows.double().sum(1), P


@pytest.mark.parametrize("B,H,W,Cy,cx,sk", UPX_CASES)
def test_upsampled_dgrad_x_matches_full_launch_and_fp64(B, H, W, Cy, cx, sk):
    """the frozen-encoder form of the decoder's fused data gradient: gx bit-identical to the full launch's, the
    BatchNorm-backward sums of the block below equal to the full launch's and to fp64 sums of g * mask and g * mask * xhat
    (mask y * scale + shift > 0 in fp32, no fma: the kernel's), gx within the Winograd bound of an fp64 data gradient,
    no write behind either output (NaN guard bands)"""
    L, lib = _lib()
    dy, wt, u, yl, mu, istd, sc, sh = _upx_inputs(B, H, W, Cy, cx, sk, seed=B * 7919 + H * 31 + W + cx)
    dy_d, yl_d = dy.to(DEV), yl.to(DEV)
    mu_d, istd_d, sc_d, sh_d = (t.to(DEV) for t in (mu, istd, sc, sh))
    d = L.ConvDesc(B, H, W, Cy, 0, 0, H, W, cx + sk, 3, 1, 1, cx, 0)
    assert lib.dt_conv2d_winograd_upsampled_dgrad_supported(C.byref(d))
    gx, sums, P = _upx_launch(d, dy_d, u, yl_d, mu_d, istd_d, sc_d, sh_d, True, sk)
    gx_full, sums_full, P_full = _upx_launch(d, dy_d, u, yl_d, mu_d, istd_d, sc_d, sh_d, False, sk)
    assert torch.equal(gx, gx_full)
    tol = 1e-5 * float(sums_full.abs().max())
    np.testing.assert_allclose(sums.cpu().numpy(), sums_full.cpu().numpy(), rtol=1e-5, atol=tol)
    # fp64 sums of the kernel's own gradient under the kernel's mask; an element within rounding distance of the mask's
    # tie may go either way: its |term| is added to the bound
    z32 = yl_d * sc_d + sh_d                     # two roundings, like the kernel (built with -ffp-contract=off)
    mask = (z32 > 0).double()
    near = ((yl_d.double() * sc_d.double() + sh_d.double()).abs()
            <= 4 * torch.finfo(torch.float32).eps * ((yl_d * sc_d).abs() + sh_d.abs()).double()).double()
    g64 = gx.double()
    xhat = ((yl_d - mu_d) * istd_d).double()
    ref = torch.stack([(g64 * mask).sum((0, 1, 2)), (g64 * mask * xhat).sum((0, 1, 2))])
    slack = torch.stack([(g64.abs() * near).sum((0, 1, 2)), (g64 * xhat).abs().mul(near).sum((0, 1, 2))])
    mag = torch.stack([(g64 * mask).abs().sum((0, 1, 2)), (g64 * mask * xhat).abs().sum((0, 1, 2))])
    err = (sums - ref).abs()
    bound = 1e-6 * mag + slack + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, ("BatchNorm-backward sums vs fp64", worst, float(err.max()))
    gflop = 2.0 * B * H * W * Cy * cx * 9 / 1e9
    rel = float("nan")
    if gflop <= FP64_MAX_GFLOP:
        w64 = wt.permute(3, 2, 0, 1)[:, :cx].double()                     # OIHW, the up-sampled input's channels
        dup = torch.nn.grad.conv2d_input((B, cx, H, W), w64, dy.permute(0, 3, 1, 2).double(), padding=1)
        gx64 = dup.view(B, cx, H // 2, 2, W // 2, 2).sum((3, 5)).permute(0, 2, 3, 1)
        amax = float(gx64.abs().max())
        rel = float((gx.cpu().double() - gx64).abs().max()) / amax
        assert rel <= 1e-5, ("gx vs fp64", rel)
    from conftest import parity_report
    parity_report(f"upsampled_dgrad_x B={B} {H}x{W} Cy={Cy} cx={cx}: rows {P} (full {P_full}), gx vs fp64 max/max|ref| "
                  f"{rel:.2e}, sums vs fp64 worst err/bound {worst:.3f}")


# ---------------------------------------------------------------- 1b. eval-mode BatchNorm backward
BN_SHAPES = [(16, 37), (32, 1000), (64, 4099), (256, 777), (512, 2500), (16, 600001)]   # (C, pixels): none a multiple of
# the 256-row block; the last one grows the row block (more than 2048 blocks of 256)


def _bn_inputs(Cc, n, seed):
    g = torch.Generator().manual_seed(seed)
    rv = _log_uniform(Cc, 1e-2, 1e2, g)
    rm = torch.randn(Cc, generator=g) * 3
    gamma = 1 + 0.5 * torch.randn(Cc, generator=g)
    beta = 0.5 * torch.randn(Cc, generator=g)
    y = rm + rv.sqrt() * torch.randn((n, Cc), generator=g)
    dout = torch.randn((n, Cc), generator=g)
    res = torch.randn((n, Cc), generator=g)
    dres0 = torch.randn((n, Cc), generator=g)
    return y, dout, res, dres0, rm, rv, gamma, beta


BN_FORMS = [("stored", None), ("stored", "write"), ("stored", "acc"), ("virtual", None), ("linear", None),
            ("linear", "write"), ("linear", "acc")]     # (a virtual activation is relu(y * scale + shift): no residual)


@pytest.mark.parametrize("Cc,n", BN_SHAPES)
@pytest.mark.parametrize("form,res", BN_FORMS)
def test_bn_bwd_apply_frozen_matches_fp64_autograd(Cc, n, form, res):
    """dt_bn_bwd_reduce + dt_bn_bwd_apply_frozen against fp64 autograd of F.batch_norm(training=False) (+ residual)
    (+ ReLU): the ReLU mask from a stored activation, from a virtual one (y * act_scale + act_shift) or none (linear);
    the residual branch's gradient written or added to.  Elements within rounding distance of the ReLU's tie get a zero
    output gradient (either mask decision is right there)."""
    L, lib = _lib()
    y, dout, resid, dres0, rm, rv, gamma, beta = _bn_inputs(Cc, n, seed=Cc * 1009 + n + len(form))
    istd = (1.0 / torch.sqrt(rv.double() + EPS)).float()
    y64 = y.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    r64 = resid.double().requires_grad_(True)
    z = F.batch_norm(y64, rm.double(), rv.double(), g64, b64, training=False, eps=EPS)
    if res is not None:
        z = z + r64
    act = None
    if form != "linear":
        zz = z.detach()
        if form == "virtual":           # the kernel recomputes the activation from y in fp32
            sc, sh = gamma * istd, beta - rm * gamma * istd
            scale = (y.double() * sc.double()).abs() + sh.double().abs()
            act_scale, act_shift = sc.to(DEV), sh.to(DEV)
        else:
            scale = zz.abs() + 1.0
            act = F.relu(zz).float()    # the stored activation: sign of the fp64 value (no fp32 tie)
        dout = torch.where(zz.abs() <= 1e-5 * scale, torch.zeros_like(dout), dout)
        z = F.relu(z)
    z.backward(dout.double())
    dev = [t.to(DEV).contiguous() for t in (dout, y, rm, istd, gamma)]
    dout_d, y_d, mu_d, istd_d, gamma_d = dev
    act_d = act.to(DEV) if act is not None else None
    asc = act_scale if form == "virtual" else None
    ash = act_shift if form == "virtual" else None
    P = lib.dt_bn_bwd_rows(n, Cc)
    red = torch.empty(int(lib.dt_bn_bwd_red_floats(n, Cc)), dtype=torch.float32, device=DEV)
    pp = lambda t: None if t is None else t.data_ptr()       # noqa: E731
    L.check(lib.dt_bn_bwd_reduce(dout_d.data_ptr(), pp(act_d), y_d.data_ptr(), mu_d.data_ptr(), istd_d.data_ptr(),
                                 pp(asc), pp(ash), red.data_ptr(), n, Cc, _st()), "dt_bn_bwd_reduce")
    dgamma = torch.empty(Cc, dtype=torch.float32, device=DEV)
    dbeta = torch.empty_like(dgamma)
    dy, dy_buf = _guarded(n * Cc)
    dres = None
    if res == "acc":
        dres_buf = torch.full((n * Cc + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        dres_buf[:n * Cc] = dres0.to(DEV).view(-1)
        dres = dres_buf[:n * Cc]
    elif res == "write":
        dres, dres_buf = _guarded(n * Cc)
    L.check(lib.dt_bn_bwd_apply_frozen(dout_d.data_ptr(), pp(act_d), y_d.data_ptr(), mu_d.data_ptr(), istd_d.data_ptr(),
                                       gamma_d.data_ptr(), pp(asc), pp(ash), red.data_ptr(), P, dgamma.data_ptr(),
                                       dbeta.data_ptr(), dy.data_ptr(), pp(dres), 1 if res == "acc" else 0, n, Cc, _st()),
            "dt_bn_bwd_apply_frozen")
    torch.cuda.synchronize()
    _band_untouched(dy_buf, n * Cc, "dy")
    if dres is not None:
        _band_untouched(dres_buf, n * Cc, "dres")
    # dy = g * gamma * invstd elementwise (two fp32 products): a few ulp of the element, a floor far below any batch-mean term
    dy_ref = y64.grad
    np.testing.assert_allclose(dy.view(n, Cc).cpu().double().numpy(), dy_ref.numpy(), rtol=1e-6,
                               atol=1e-7 * float(dy_ref.abs().max()))
    # dgamma / dbeta: fp32 partial rows, fp64 finalize; bounded by the magnitude of the summed terms
    xhat = (y.double() - rm.double()) / torch.sqrt(rv.double() + EPS)
    gm = dout.double() if form == "linear" else dout.double() * (z.detach() > 0).double()
    for got, want, mag, what in ((dbeta, b64.grad, gm.abs().sum(0), "dbeta"),
                                 (dgamma, g64.grad, (gm * xhat).abs().sum(0), "dgamma")):
        err = (got.cpu().double() - want).abs()
        assert bool((err <= 2e-6 * mag + 1e-30).all()), (what, float((err / mag).max()))
    if res is not None:
        want = r64.grad + (dres0.double() if res == "acc" else 0)
        np.testing.assert_allclose(dres.view(n, Cc).cpu().double().numpy(), want.numpy(), rtol=1e-7, atol=0)


# ---------------------------------------------------------------- 1c. eval-mode statistics and affine coefficients
def _ulps(got, want):
    """|got - want| in units of the fp32 spacing at want"""
    w32 = want.float().numpy()
    return (got.double().numpy() - want.numpy()).__abs__() / np.spacing(np.abs(w32)).astype(np.float64)


@pytest.mark.parametrize("Cc", [16, 64, 300, 512, 2048])
def test_bn_eval_stats_and_affine_match_fp64(Cc):
    """dt_bn_eval_stats (mean, invstd) and dt_bn_eval_affine (scale, shift) from running statistics: within 2 fp32 ulp
    of fp64 (shift: of the larger of its two terms, beta - mean * scale cancels, given the kernel's scale)"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(Cc)
    rv = _log_uniform(Cc, 1e-2, 1e2, g)
    rm = torch.randn(Cc, generator=g) * 3
    gamma = 1 + 0.5 * torch.randn(Cc, generator=g)
    beta = 0.5 * torch.randn(Cc, generator=g)
    rm_d, rv_d, ga_d, be_d = (t.to(DEV) for t in (rm, rv, gamma, beta))
    outs = [_guarded(Cc) for _ in range(4)]
    mean, invstd, scale, shift = (o[0] for o in outs)
    L.check(lib.dt_bn_eval_stats(rm_d.data_ptr(), rv_d.data_ptr(), EPS, Cc, mean.data_ptr(), invstd.data_ptr(), _st()),
            "dt_bn_eval_stats")
    L.check(lib.dt_bn_eval_affine(ga_d.data_ptr(), be_d.data_ptr(), rm_d.data_ptr(), rv_d.data_ptr(), EPS, Cc,
                                  scale.data_ptr(), shift.data_ptr(), _st()), "dt_bn_eval_affine")
    torch.cuda.synchronize()
    for (_, buf), what in zip(outs, ("mean", "invstd", "scale", "shift")):
        _band_untouched(buf, Cc, what)
    eps32 = float(np.float32(EPS))      # the kernels take eps as a float argument
    is64 = 1.0 / torch.sqrt(rv.double() + eps32)
    sc64 = gamma.double() * is64
    sh64 = beta.double() - rm.double() * sc64
    assert torch.equal(mean.cpu(), rm)
    assert _ulps(invstd.cpu(), is64).max() <= 2.0
    assert _ulps(scale.cpu(), sc64).max() <= 2.0
    # shift = beta - mean * scale: given the kernel's scale (pinned above), two roundings — within 2 ulp of the larger
    # term (the subtraction cancels; against sh64 the scale's own error would be multiplied by |mean|)
    sc = scale.cpu().double()
    sh_ref = beta.double() - rm.double() * sc
    big = torch.maximum(beta.double().abs(), (rm.double() * sc).abs())
    err = (shift.cpu().double() - sh_ref).abs().numpy()
    assert (err <= 2 * np.spacing(big.float().numpy()).astype(np.float64)).all(), float(err.max())
    # and the shift against fp64 throughout: the scale's error (<= 2 ulp) carried by |mean|
    err64 = (shift.cpu().double() - sh64).abs().numpy()
    carried = rm.double().abs().numpy() * 2 * np.spacing(np.abs(sc64.float().numpy())).astype(np.float64)
    assert (err64 <= carried + 2 * np.spacing(big.float().numpy()).astype(np.float64)).all(), float(err64.max())


# ---------------------------------------------------------------- 1d. FlatAdam.set_trainable against torch.optim.Adam
N_FLAT = 1202       # not a multiple of 4: the last segment ends in the scalar tail
CUTS = [0, 64, 68, 512, 768, 1000, N_FLAT]     # every range end used below; [64, 68) is a 4-element segment


def _torch_params(p0):
    return [torch.nn.Parameter(p0[a:b].clone()) for a, b in zip(CUTS[:-1], CUTS[1:])]


def test_flat_adam_trainable_ranges_match_torch_adam():
    """per-range clip + Adam against torch.optim.Adam with one parameter per segment (.grad None where frozen) over a
    schedule of range sets: disjoint, adjacent, a 4-element range, the scalar tail, a trained segment split in two (both
    parts keep its step count), freeze / unfreeze / freeze / unfreeze of one range, reset_state, a non-finite gradient in
    a trainable range (the step is skipped) and in a frozen one (ignored).  Frozen gradient slices are NaN every step;
    frozen parameters, m and v stay bit-unchanged"""
    from deadtrees_amd.ops import FlatAdam
    lr = 1e-2
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(N_FLAT, generator=g)
    params = _torch_params(p0)
    ref = torch.optim.Adam(params, lr=lr)
    flat = p0.clone().to(DEV)
    opt = FlatAdam(flat, lr=lr, max_norm=0.5)
    schedule = [   # (trainable ranges, event)
        ([(0, 64), (512, 1000)], None),                 # disjoint; [512, 1000) trains as one segment
        ([(0, 64), (512, 1000)], None),
        ([(0, 64), (64, 68), (68, 512)], None),         # adjacent ranges, a 4-element one
        ([(768, N_FLAT)], None),                        # [512, 1000) split at 768: the upper part keeps count 2
        ([(512, 768)], None),                           # ... and so does the lower part
        ([(64, 68)], None),                             # freeze / unfreeze / freeze / unfreeze of [64, 68)
        ([(0, 64)], None),
        ([(64, 68), (1000, N_FLAT)], None),
        ([(0, 64), (512, 768)], None),
        ([(64, 68), (768, 1000)], None),
        ([(0, 512), (768, N_FLAT)], "nan_trainable"),   # a NaN inside a trainable range: the whole step is skipped
        ([(0, 512), (768, N_FLAT)], "nan_frozen"),      # a NaN in the frozen [512, 768): never read
        ([(512, 1000)], "reset"),                       # a fresh optimiser (the LR-reduce stage), ranges kept
        (None, None),                                   # everything trainable again
        ([(1000, N_FLAT)], None),
    ]
    for step, (ranges, event) in enumerate(schedule):
        if event == "reset":
            ref = torch.optim.Adam(params, lr=lr / 3)
            opt.reset_state(lr=lr / 3)
        opt.set_trainable(ranges)
        rng = [(0, N_FLAT)] if ranges is None else ranges
        live = [any(lo <= a and b <= hi for lo, hi in rng) for a, b in zip(CUTS[:-1], CUTS[1:])]
        gr = torch.randn(N_FLAT, generator=g)
        gd = gr.clone()
        for (a, b), on in zip(zip(CUTS[:-1], CUTS[1:]), live):
            if not on:
                gd[a:b] = float("nan")                   # a frozen range is never read
        if event == "nan_trainable":
            gd[3] = float("nan")
        for prm, (a, b), on in zip(params, zip(CUTS[:-1], CUTS[1:]), live):
            prm.grad = gr[a:b].clone() if on else None
        before = [t.clone() for t in (flat, opt.m, opt.v)]
        norm = opt.step(gd.to(DEV))
        torch.cuda.synchronize()
        if event == "nan_trainable":
            assert not np.isfinite(float(norm)), step
            for t, t0 in zip((flat, opt.m, opt.v), before):
                assert torch.equal(t, t0), step                     # skipped: nothing moved
            continue
        gn = torch.nn.utils.clip_grad_norm_([prm for prm in params if prm.grad is not None], 0.5)
        ref.step()
        assert float(norm) == pytest.approx(float(gn), rel=1e-5), step
        got = flat.cpu()
        for prm, (a, b), on in zip(params, zip(CUTS[:-1], CUTS[1:]), live):
            torch.testing.assert_close(got[a:b], prm.detach(), rtol=0, atol=2e-6, msg=f"step {step} [{a}, {b})")
            if not on:
                for t, t0 in zip((flat, opt.m, opt.v), before):
                    assert torch.equal(t[a:b], t0[a:b]), (step, a, b)


def test_flat_adam_rejects_bad_ranges_without_changing_state():
    """a misaligned range, no trainable range and more than 64 trainable segments (the per-segment step-count launch's
    limit) raise in set_trainable, before anything changes: the optimiser then steps exactly as before the failed call"""
    from deadtrees_amd.ops import FlatAdam
    n = 4096
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=g)
    a, b = torch.nn.Parameter(p0[:1024].clone()), torch.nn.Parameter(p0[1024:].clone())
    ref = torch.optim.Adam([a, b], lr=1e-2)
    flat = p0.clone().to(DEV)
    opt = FlatAdam(flat, lr=1e-2, max_norm=0.5)
    opt.set_trainable([(1024, n)])
    for bad in ([(2, 64)], [(0, 62)], [(-4, 64)], [(0, n + 4)], [], [(64, 64)],
                [(8 * i, 8 * i + 4) for i in range(65)]):         # 65 trainable segments
        state = (list(opt._segments), list(opt._trainable), opt.t_seg.clone(), opt.table.clone())
        with pytest.raises(ValueError):
            opt.set_trainable(bad)
        assert opt._segments == state[0] and opt._trainable == state[1]
        assert torch.equal(opt.t_seg, state[2]) and torch.equal(opt.table, state[3])
    opt.set_trainable([(8 * i, 8 * i + 4) for i in range(64)])    # 64: the limit itself is fine
    opt.set_trainable([(1024, n)])
    for _ in range(2):
        gr = torch.randn(n, generator=g)
        a.grad, b.grad = None, gr[1024:].clone()
        gn = torch.nn.utils.clip_grad_norm_([b], 0.5)
        ref.step()
        gd = gr.to(DEV)
        gd[:1024] = float("nan")
        norm = opt.step(gd)
        assert float(norm) == pytest.approx(float(gn), rel=1e-5)
        torch.testing.assert_close(flat.cpu()[:1024], p0[:1024], rtol=0, atol=0)
        torch.testing.assert_close(flat.cpu()[1024:], b.detach(), rtol=0, atol=2e-6)
