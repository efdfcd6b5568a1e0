"""Every convolution variant the dispatch table names (tests/golden/dispatch_table.json, network rows) against float64 torch
on the CPU, one case per variant key and precision, at the ragged descriptor tests/conv_variant_cases.py finds for the key.
Each case first asserts, through the library's config query, that its descriptor still dispatches to the key.

Bounds.  fp32: |err| <= (K + 8) * 2^-24 * mag per element, K = ksize^2 (C0 + C1) products, mag the same convolution over
absolute values (+ |base| for a gradient join): the dot-product bound of fp32 accumulation, whatever the order.  bf16: the
operands are rounded to bf16 first and the reference runs on the rounded values; the kernels accumulate in fp32 and round
once: 2^-8 |want| + (K + 8) * 2^-24 * mag.  BatchNorm partial statistics (both precisions take them from the fp32
accumulators, so their element error e is the fp32 bound): sum within sum(e) + g(n) * sum(|want| + e), sum of squares within
sum(2 |want| e + e^2) + g(n + 1) * sum((|want| + e)^2), g(n) = (n + 8) 2^-24 / (1 - (n + 8) 2^-24) over the n pixels of a
channel.  With a fused input transform z = relu(x * scale + shift) the device's z is within 2 * 2^-24 (|x scale| + |shift|) of
the float64 one, so mag is taken over |x scale| + |shift| and K + 8 becomes K + 11.

Batch invariance of the 64-wide tiles: image B // 2 computed alone runs a 32-wide kernel and must equal its slice of the
batched result, bit for bit where both config queries report the same channels per K step (the same order of products
per output element), within the bound otherwise."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_variant_cases as cvc

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BF = torch.bfloat16

FP32_KEYS, BF16_KEYS = (sorted(s) for s in cvc.golden_keys())


def _nhwc(t, dtype):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _nchw64(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).double()


def _hwio(w):
    return w.permute(2, 3, 1, 0).contiguous().float().to(DEV)


def _set_dma(mode):
    from deadtrees_amd import _lib
    _lib.check(_lib.load().dt_set_option(b"bf16_dma", mode), "dt_set_option")


def _inputs(t, prec, seed, transform=False):
    """CPU fp32 NCHW operands of descriptor t (bf16: already rounded to bf16 values).  mode0 = 2: w is the OIHW weight of
    the stride-2 convolution whose data gradient the descriptor asks for (O = C0, the gradient's channels)"""
    d = dict(zip(cvc.FIELDS, t))
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda x: x.to(BF).float()) if prec == "bf16" else (lambda x: x)
    sh = 1 if d["mode0"] else 0
    k, cin = d["ksize"], d["C0"] + d["C1"]
    x0 = rnd(torch.randn((d["B"], d["C0"], d["Hin"] >> sh, d["Win"] >> sh), generator=g))
    x1 = rnd(torch.randn((d["B"], d["C1"], d["Hin"], d["Win"]), generator=g)) if d["C1"] else None
    wshape = (d["C0"], d["Cout"], k, k) if d["mode0"] == 2 else (d["Cout"], cin, k, k)
    w = rnd(torch.randn(wshape, generator=g) * (2.0 / (k * k * cin)) ** 0.5)
    base = rnd(torch.randn((d["B"], d["cout_split"] or d["Cout"], d["Ho"], d["Wo"]), generator=g)) if d["accumulate"] else None
    tf = None
    if transform:
        tf = (1 + 0.3 * torch.randn(d["C0"], generator=g), 0.3 * torch.randn(d["C0"], generator=g) + 0.4)
    return dict(x0=x0, x1=x1, w=w, base=base, tf=tf)


def _reference(t, inp):
    """(want, mag) in float64 NCHW, before the join"""
    d = dict(zip(cvc.FIELDS, t))
    a, w = inp["x0"].double(), inp["w"].double()
    a_abs = a.abs()
    if inp["tf"] is not None:
        sc, sh = (v.double()[None, :, None, None] for v in inp["tf"])
        a_abs = a_abs * sc.abs() + sh.abs()
        a = F.relu(a * sc + sh)
    if d["mode0"] == 2:
        size = (d["B"], d["Cout"], d["Hin"], d["Win"])
        pf = d["ksize"] - 1 - d["pad"]
        return (torch.nn.grad.conv2d_input(size, w, a, stride=2, padding=pf),
                torch.nn.grad.conv2d_input(size, w.abs(), a_abs, stride=2, padding=pf))
    if d["mode0"] == 1:
        a, a_abs = (F.interpolate(v, scale_factor=2, mode="nearest") for v in (a, a_abs))
    if inp["x1"] is not None:
        a, a_abs = torch.cat([a, inp["x1"].double()], dim=1), torch.cat([a_abs, inp["x1"].double().abs()], dim=1)
    return (F.conv2d(a, w, stride=d["stride"], padding=d["pad"]),
            F.conv2d(a_abs, w.abs(), stride=d["stride"], padding=d["pad"]))


def _device_weights(t, prec, inp):
    from deadtrees_amd import ops
    d = dict(zip(cvc.FIELDS, t))
    if prec == "fp32":
        return ops.weight_flip_transpose(_hwio(inp["w"])) if d["mode0"] == 2 else _hwio(inp["w"])
    return ops.pack_weights_bf16(_hwio(inp["w"]), dgrad=d["mode0"] == 2)


def _device(t, prec, inp, wdev, want_stats=False, image=None):
    """(out0, out1, stats) of ops.conv2d / ops.conv2d_bf16 on the whole batch or on image `image` alone"""
    from deadtrees_amd import ops
    d = dict(zip(cvc.FIELDS, t))
    dt = torch.float32 if prec == "fp32" else BF
    sl = (lambda v: v) if image is None else (lambda v: None if v is None else v[image:image + 1])
    base = _nhwc(sl(inp["base"]), dt)
    kw = dict(src1=_nhwc(sl(inp["x1"]), dt), mode0=d["mode0"], split=d["cout_split"], out0=base,
              accumulate=bool(d["accumulate"]), want_stats=want_stats,
              in_scale=None if inp["tf"] is None else inp["tf"][0].to(DEV),
              in_shift=None if inp["tf"] is None else inp["tf"][1].to(DEV))
    x0 = _nhwc(sl(inp["x0"]), dt)
    if prec == "fp32":
        out = ops.conv2d(x0, wdev, d["ksize"], d["stride"], d["pad"], **kw)
    else:
        out = ops.conv2d_bf16(x0, wdev, d["ksize"], d["stride"], d["pad"], d["Cout"], **kw)
    torch.cuda.synchronize()
    return out


def _parts(t, inp, want, mag):
    """[(want, mag)] per output tensor: the channel ranges of a split, the join folded in"""
    d = dict(zip(cvc.FIELDS, t))
    sp = d["cout_split"]
    parts = [(want[:, :sp], mag[:, :sp]), (want[:, sp:], mag[:, sp:])] if sp else [(want, mag)]
    if inp["base"] is not None:
        b = inp["base"].double()
        parts[0] = (parts[0][0] + b, parts[0][1] + b.abs())
    return parts


def _worst(r):
    """the largest ratio; inf as soon as one is not finite (a NaN would otherwise get lost in max() and in <=)"""
    return float(r.max()) if bool(torch.isfinite(r).all()) else math.inf


def _ratio(got, want, bound):
    err = (got - want).abs()     # NaN / inf where the device result is
    return _worst(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, err, torch.full_like(err, math.inf))))


def _bound(prec, K, want, mag, slack=8):
    e = (K + slack) * U * mag
    return e if prec == "fp32" else e + 2.0 ** -8 * want.abs()


def _check_outputs(t, prec, inp, outs, want, mag, slack=8, image=None):
    d = dict(zip(cvc.FIELDS, t))
    K = d["ksize"] ** 2 * (d["C0"] + d["C1"])
    worst = 0.0
    for got, (w_, m_) in zip(outs[:2], _parts(t, inp, want, mag)):
        if image is not None:
            w_, m_ = w_[image:image + 1], m_[image:image + 1]
        got = _nchw64(got)
        assert got.shape == w_.shape
        worst = max(worst, _ratio(got, w_, _bound(prec, K, w_, m_, slack)))
    return worst


def _rows_per_image(prec, t, P):
    """partial rows per image where the kernel writes one row per spatial tile, image after image (the register-staged
    tiled kernels, conv_fwd_n16_kernel, the packed stride-2 tiles: row = spatial tile index, b = row / tiles per image);
    0 for the persistent kernels (lean narrow layers, LDS-DMA), whose rows belong to workgroups that walk several images"""
    d = dict(zip(cvc.FIELDS, t))
    tw, tn, ck, last = _config(prec, t)
    if (prec == "fp32" and ck >= 1000) or (prec == "bf16" and last not in (2, 4)):
        return 0
    th = 256 // tw if prec == "fp32" else 128 * last // tw
    tiles = -(-d["Ho"] // th) * -(-d["Wo"] // tw)
    return tiles if P == d["B"] * tiles else 0


def _check_stats(prec, t, stats, want, mag, slack=8):
    """(worst ratio of the channel sums, of the sums of squares).  Where the rows can be told apart by image the sums are
    compared per image (n = Ho Wo terms: a bound B times tighter than that of the whole batch), else over the batch"""
    d = dict(zip(cvc.FIELDS, t))
    K = d["ksize"] ** 2 * (d["C0"] + d["C1"])
    e = (K + slack) * U * mag
    hi = want.abs() + e
    g = lambda m: (m + 8) * U / (1 - (m + 8) * U)   # noqa: E731
    P = stats.shape[1]
    per = _rows_per_image(prec, t, P)
    G = d["B"] if per else 1
    n = d["B"] * d["Ho"] * d["Wo"] // G
    s = stats.double().cpu().reshape(2, G, P // G, -1).sum(dim=2)     # the partial rows, added up on the host in float64
    tot = (lambda v: v.sum(dim=(2, 3))) if per else (lambda v: v.sum(dim=(0, 2, 3))[None])
    b1 = tot(e) + g(n) * tot(hi)
    b2 = tot(2 * want.abs() * e + e * e) + g(n + 1) * tot(hi * hi)
    return _worst((s[0] - tot(want)).abs() / b1), _worst((s[1] - tot(want * want)).abs() / b2)


def _config(prec, t):
    return cvc.fp32_config(t) if prec == "fp32" else cvc.bf16_config(t)


def _one_image(t):
    return (1,) + tuple(t[1:])


def _run_case(prec, key, t, transform=False):
    """the whole check of one case; returns the worst err / bound ratio over its outputs"""
    d = dict(zip(cvc.FIELDS, t))
    keyf = cvc.fp32_key if prec == "fp32" else cvc.bf16_key
    assert keyf(t) == key, (t, keyf(t), key)
    assert cvc.within_budget(t)
    name = cvc.case_id(prec, key) + (" +transform" if transform else "")
    slack = 11 if transform else 8
    inp = _inputs(t, prec, seed=sum(v * (i + 3) for i, v in enumerate(key)), transform=transform)
    want, mag = _reference(t, inp)
    wdev = _device_weights(t, prec, inp)
    forward = d["accumulate"] == 0 and d["cout_split"] == 0 and d["mode0"] in (0, 1)
    outs = _device(t, prec, inp, wdev, want_stats=forward)
    worst = _check_outputs(t, prec, inp, outs, want, mag, slack)
    line = f"conv variant {name} {t}: worst err / bound {worst:.4f}"
    ok = worst <= 1.0
    if forward:
        r1, r2 = _check_stats(prec, t, outs[2], want, mag, slack)
        line += f", channel sums {r1:.4f}, sums of squares {r2:.4f} ({'per image' if _rows_per_image(prec, t, outs[2].shape[1]) else 'whole batch'})"
        ok = ok and r1 <= 1.0 and r2 <= 1.0
    tn, ck = _config(prec, t)[1:3]
    if tn == 64 and d["B"] > 1:
        b = d["B"] // 2
        t1 = _one_image(t)
        tn1, ck1 = _config(prec, t1)[1:3]
        one = _device(t1, prec, inp, wdev, image=b)
        if ck1 == ck:
            same = all(torch.equal(o1, o[b:b + 1]) for o1, o in zip(one[:2], outs[:2]) if o1 is not None)
            line += f", image {b} alone (tn {tn1}, ck {ck1}) bit-identical: {same}"
            ok = ok and same
        else:
            rb = _check_outputs(t, prec, inp, one, want, mag, slack, image=b)
            line += f", image {b} alone (tn {tn1}, ck {ck1} != {ck}) worst err / bound {rb:.4f}"
            ok = ok and rb <= 1.0
    print(line)
    assert ok, line
    return worst, inp, want, mag, wdev


@pytest.mark.parametrize("key", FP32_KEYS, ids=[cvc.case_id("fp32", k) for k in FP32_KEYS])
def test_fp32_variant_against_float64(key):
    _run_case("fp32", key, cvc.cases()["fp32"][key])


TRANSFORM_KEYS = [k for k in FP32_KEYS if k[:2] == (3, 1) and k[2] != 2 and k[4] == 64 and k[6] == 0]


@pytest.mark.parametrize("key", TRANSFORM_KEYS, ids=[cvc.case_id("fp32", k) for k in TRANSFORM_KEYS])
def test_fp32_wide_variant_with_fused_input_transform(key):
    """the 3x3 stride-1 64-wide tiles once more with the producer's BatchNorm + ReLU applied while staging (the dispatch
    table has no column for it: conv_fwd_kernel<..., TF = true>)"""
    _run_case("fp32", key, cvc.cases()["fp32"][key], transform=True)


def _bf16_stem(key, t):
    """the space-to-depth stem (ksize 4): through ops.stem_conv_bf16, against the 7x7 / stride-2 convolution of the
    bf16-rounded image and weights; K = 16 taps x 16 channels of the packed form (its zero products are exact)"""
    from deadtrees_amd import ops
    assert cvc.bf16_key(t) == key and cvc.within_budget(t)
    d = dict(zip(cvc.FIELDS, t))
    g = torch.Generator().manual_seed(4)
    x = torch.randn((d["B"], 3, 2 * d["Hin"], 2 * d["Win"]), generator=g)
    w = torch.randn((d["Cout"], 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5
    x64, w64 = x.to(BF).double(), w.to(BF).double()
    want, mag = F.conv2d(x64, w64, stride=2, padding=3), F.conv2d(x64.abs(), w64.abs(), stride=2, padding=3)
    y, stats = ops.stem_conv_bf16(x.permute(0, 2, 3, 1).contiguous().to(DEV), _hwio(w), want_stats=True)
    torch.cuda.synchronize()
    worst = _ratio(_nchw64(y), want, _bound("bf16", 256, want, mag))
    r1, r2 = _check_stats("bf16", t, stats, want, mag)
    line = f"conv variant {cvc.case_id('bf16', key)} {t}: worst err / bound {worst:.4f}, channel sums {r1:.4f}, sums of squares {r2:.4f}"
    print(line)
    assert worst <= 1.0 and r1 <= 1.0 and r2 <= 1.0, line


def _bf16_case(key, t):
    if key[0] == 4:
        return _bf16_stem(key, t)
    _, inp, want, mag, wdev = _run_case("bf16", key, t)
    if key[6] == cvc._lib().BF16_MT_DMA:
        # the LDS-DMA kernel ran above; with it switched off the same batch takes the register-staged 64-wide tiles
        # (256-pixel ones, mt = 2, at these batches: the 512-pixel form has its own case off the table)
        try:
            _set_dma(0)
            tw, tn, ck, mt = cvc.bf16_config(t)
            assert (tw, tn) == (32, 64) and mt in (2, 4), (tw, tn, ck, mt)
            outs = _device(t, "bf16", inp, wdev)
        finally:
            _set_dma(cvc.dma_default())
        worst = _check_outputs(t, "bf16", inp, outs, want, mag)
        line = f"conv variant {cvc.case_id('bf16', key)} with bf16_dma 0 (ck {ck}, mt {mt}): worst err / bound {worst:.4f}"
        print(line)
        assert worst <= 1.0, line


@pytest.mark.parametrize("key", BF16_KEYS, ids=[cvc.case_id("bf16", k) for k in BF16_KEYS])
def test_bf16_variant_against_float64(key):
    _bf16_case(key, cvc.cases()["bf16"][key])


@pytest.mark.parametrize("key", cvc.EXTRA_BF16_KEYS, ids=[cvc.case_id("bf16", k) for k in cvc.EXTRA_BF16_KEYS])
def test_bf16_variant_off_the_table_against_float64(key):
    """the 512-pixel register-staged tiles (mt = 4): no network row reaches them while the LDS-DMA kernel is on, a layer
    with 16 (mod 32) input channels does"""
    _bf16_case(key, cvc.cases()["bf16_extra"][key])


@pytest.mark.parametrize("C0,Cout", [(16, 2), (2, 16), (40, 6)])
def test_fp32_tiled_kernels_refuse_channel_counts_that_are_no_multiple_of_4(C0, Cout):
    """conv_fwd_kernel stages channels in 16-byte quads guarded by their first channel: a count that is no multiple of 4
    would read past the tensor (the two-channel head rows of the dispatch table are such shapes; the engines run the head
    through its own kernels).  dt_conv2d refuses them instead of launching"""
    from deadtrees_amd import ops
    t = cvc.make(1, 8, 8, C0, 0, 0, Cout, 3, 1, 1)
    assert cvc.fp32_config(t)[1:3] in ((32, 8), (32, 16))        # a tiled instantiation, not the 16-wide or lean kernels
    x = torch.zeros((1, 8, 8, C0), device=DEV)
    w = torch.zeros((3, 3, C0, Cout), device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.conv2d(x, w, 3, 1, 1)
