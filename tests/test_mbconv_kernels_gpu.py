"""The three kernels of csrc/mbconv.hip (inverted-residual block of the EfficientUnet++ decoder) one by one against a float64
torch composition on the CPU, at the smallest shapes at which they can go wrong: 70 pixel rows (no multiple of any tile),
every output-tile count of the pointwise kernel, the channel-group paths of the depthwise kernel, both reduction forms of
the gate kernel.  Bounds: the standard dot-product bound of fp32 accumulation, (terms + 8) * 2^-24 * sum |products|, times
Hardswish's largest slope 1.5 where one follows.  And batch invariance: an image's result does not depend on its batch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _rand(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def _hswish64(t):
    return t * (t + 3).clamp(0, 6) / 6


def _virtual_input(src0, src1, up, H, W):
    a = src0.double()
    if up:
        a = a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]
    return a if src1 is None else torch.cat([a, src1.double()], dim=-1)


PW_CASES = {      # (K or (C0, C1), N, up, gate, act, res): res "alias" = the residual is the output tensor itself
    "16x16 act": (16, 16, False, False, True, None),
    "16x16 gate res": (16, 16, False, True, False, "res"),
    "48x16 up+cat act": ((32, 16), 16, True, False, True, None),
    "48x16 up+cat gate act res": ((32, 16), 16, True, True, True, "res"),
    "48x16 cat gate": ((16, 32), 16, False, True, False, None),
    "768x256 gate alias": (768, 256, False, True, False, "alias"),
    "768x256 act res": (768, 256, False, False, True, "res"),
    "16x32": (16, 32, False, False, False, None),            # the other output-tile counts of a workgroup: 2, 3, 4, 8 ...
    "16x48 act": (16, 48, False, False, True, None),
    "32x64 gate": (32, 64, False, True, False, None),
    "16x128 res": (16, 128, False, False, False, "res"),
    "32x272 gate act alias": (32, 272, False, True, True, "alias"),    # ... and a second workgroup column (256 + 16)
}


def _pw_inputs(case, B=2, H=5, W=7, seed=0):
    KK, N, up, gate, act, res = PW_CASES[case]
    C0, C1 = KK if isinstance(KK, tuple) else (KK, 0)
    g = torch.Generator().manual_seed(seed)
    src0 = _rand(g, B, (H + 1) // 2, (W + 1) // 2, C0) if up else _rand(g, B, H, W, C0)
    src1 = _rand(g, B, H, W, C1) if C1 else None
    w = _rand(g, C0 + C1, N, scale=(2.0 / (C0 + C1)) ** 0.5)
    scale, shift = 1.0 + 0.2 * _rand(g, N), _rand(g, N)
    gt = (torch.sigmoid(_rand(g, B, C0 + C1)), 2.0 * _rand(g, B, H, W)) if gate else None
    r = _rand(g, B, H, W, N) if res else None
    return dict(src0=src0, src1=src1, w=w, scale=scale, shift=shift, gate=gt, res=r, up=up, act=act, alias=res == "alias",
                hw=(H, W))


def _pw_run(d):
    from deadtrees_amd import ops
    t = lambda x: None if x is None else x.to(DEV)
    res = t(d["res"])
    out = ops.pwconv_affine(t(d["src0"]), t(d["w"]), t(d["scale"]), t(d["shift"]), src1=t(d["src1"]), up0=d["up"],
                            gate=None if d["gate"] is None else (t(d["gate"][0]), t(d["gate"][1])), act=d["act"], res=res,
                            out=res if d["alias"] else None, hw=d["hw"])
    assert not d["alias"] or out.data_ptr() == res.data_ptr()
    return out.cpu()


@pytest.mark.parametrize("case", list(PW_CASES))
def test_pwconv_affine_against_float64(case):
    d = _pw_inputs(case)
    H, W = d["hw"]
    a = _virtual_input(d["src0"], d["src1"], d["up"], H, W)
    K = a.shape[-1]
    if d["gate"] is not None:
        gc, s = d["gate"]
        a = a * (gc.double()[:, None, None, :] + torch.sigmoid(s.double())[..., None])
    w, sc, sh = d["w"].double(), d["scale"].double(), d["shift"].double()
    t = (a @ w) * sc + sh
    want = _hswish64(t) if d["act"] else t
    mag = (a.abs() @ w.abs()) * sc.abs() + sh.abs()
    if d["res"] is not None:
        want = want + d["res"].double()
        mag = mag + d["res"].double().abs()
    bound = 1.5 * (K + 8) * U * mag
    got = _pw_run(d).double()
    ratio = float(((got - want).abs() / bound).max())
    print(f"pwconv_affine {case}: max|err| {float((got - want).abs().max()):.3e}, worst err / bound {ratio:.4f}")
    assert ratio <= 1.0


DW_SHAPES = [(2, 5, 7, 16), (1, 1, 1, 48), (2, 9, 33, 768)]


def _dw_inputs(B, H, W, C, seed=1):
    g = torch.Generator().manual_seed(seed)
    return dict(x=_rand(g, B, H, W, C), w=_rand(g, 9, C, scale=(2.0 / 9) ** 0.5), scale=1.0 + 0.2 * _rand(g, C),
                shift=_rand(g, C), ws=_rand(g, C, scale=C ** -0.5), bs=_rand(g, 1))


def _dw_run(d):
    from deadtrees_amd import ops
    B, _, _, C = d["x"].shape
    b, s, pool = ops.dwconv3x3_affine(*(d[k].to(DEV) for k in ("x", "w", "scale", "shift", "ws", "bs")))
    return b.cpu(), s.cpu(), ops.pool_rows(pool, B, C).cpu()


@pytest.mark.parametrize("B,H,W,C", DW_SHAPES)
def test_dwconv3x3_affine_against_float64(B, H, W, C):
    d = _dw_inputs(B, H, W, C)
    x = d["x"].double().permute(0, 3, 1, 2)
    wk = d["w"].double().t().reshape(C, 1, 3, 3)
    sc, sh = d["scale"].double()[None, :, None, None], d["shift"].double()[None, :, None, None]
    want = _hswish64(F.conv2d(x, wk, padding=1, groups=C) * sc + sh).permute(0, 2, 3, 1)
    b_bound = (1.5 * (9 + 8) * U * (F.conv2d(x.abs(), wk.abs(), padding=1, groups=C) * sc.abs() + sh.abs())).permute(0, 2, 3, 1)
    b, s, rows = _dw_run(d)
    assert tuple(rows.shape) == (B, -(-H * W // 256), C)
    r_b = float(((b.double() - want).abs() / b_bound).max())
    ws, bs = d["ws"].double(), d["bs"].double()
    s_want = want @ ws + bs
    s_bound = b_bound @ ws.abs() + (C + 8) * U * (want.abs() @ ws.abs() + bs.abs())
    r_s = float(((s.double() - s_want).abs() / s_bound).max())
    sums = rows.double().sum(dim=1)                                 # the partial rows, added up on the host in float64
    sums_want = want.sum(dim=(1, 2))
    sums_bound = b_bound.sum(dim=(1, 2)) + (H * W + 8) * U * want.abs().sum(dim=(1, 2))
    r_p = float(((sums - sums_want).abs() / sums_bound).max())
    print(f"dwconv3x3_affine {B}x{H}x{W}x{C}: worst err / bound: b {r_b:.4f}, sSE logits {r_s:.4f}, channel sums {r_p:.4f}")
    assert r_b <= 1.0 and r_s <= 1.0 and r_p <= 1.0


GATE_SHAPES = [(16, 1, 5), (768, 1, 3), (64, 4, 2)]      # (C, squeeze ratio, rows): sliced and plain row reduction


def _gate_inputs(C, r, P, B=2, HW=500, seed=2):
    g = torch.Generator().manual_seed(seed)
    Ch = C // r
    return dict(rows=_rand(g, B, P, C, scale=HW / P * 0.5), HW=HW, w1=_rand(g, C, Ch, scale=(2.0 / C) ** 0.5), b1=_rand(g, Ch, scale=0.1),
                w2=_rand(g, Ch, C, scale=(2.0 / Ch) ** 0.5), b2=_rand(g, C, scale=0.1))


def _gate_formula(d, dtype):
    mean = d["rows"].to(dtype).sum(dim=1) / d["HW"]
    hid = torch.relu(mean @ d["w1"].to(dtype) + d["b1"].to(dtype))
    return torch.sigmoid(hid @ d["w2"].to(dtype) + d["b2"].to(dtype))


def _gate_run(d):
    from deadtrees_amd import ops
    B, P, C = d["rows"].shape
    pool = torch.cat([torch.zeros(B * C), d["rows"].reshape(-1)]).to(DEV)
    return ops.scse_gates(pool, B, C, d["HW"], d["w1"].to(DEV), d["b1"].to(DEV), d["w2"].to(DEV), d["b2"].to(DEV)).cpu()


@pytest.mark.parametrize("C,r,P", GATE_SHAPES)
def test_scse_gates_against_float64(C, r, P):
    d = _gate_inputs(C, r, P)
    want = _gate_formula(d, torch.float64)
    e32 = float((_gate_formula(d, torch.float32).double() - want).abs().max())      # the same formula in fp32 on the CPU
    got = _gate_run(d)
    assert tuple(got.shape) == (2, C)
    err = float((got.double() - want).abs().max())
    print(f"scse_gates C={C} r={r} P={P}: device max|err| {err:.3e}, fp32 CPU formula {e32:.3e}")
    assert err <= 4 * e32 + 4 * 2.0 ** -23


# ---------------------------------------------------------------------------------------------- batch invariance
def _middle(d, keys):
    return {k: (v[1:2].contiguous() if k in keys and v is not None else v) for k, v in d.items()}


@pytest.mark.parametrize("case", ["48x16 up+cat gate act res", "768x256 gate alias", "32x272 gate act alias"])
def test_pwconv_affine_is_batch_invariant(case):
    d = _pw_inputs(case, B=3, seed=5)
    one = _middle(d, ("src0", "src1", "res"))
    one["gate"] = (d["gate"][0][1:2].contiguous(), d["gate"][1][1:2].contiguous())
    assert torch.equal(_pw_run(d)[1:2], _pw_run(one))


@pytest.mark.parametrize("H,W,C", [(5, 7, 16), (9, 33, 768), (17, 19, 48)])
def test_dwconv3x3_affine_is_batch_invariant(H, W, C):
    d = _dw_inputs(3, H, W, C, seed=6)
    for a, b in zip(_dw_run(d), _dw_run(_middle(d, ("x",)))):
        assert torch.equal(a[1:2], b)


@pytest.mark.parametrize("C,r,P", GATE_SHAPES)
def test_scse_gates_is_batch_invariant(C, r, P):
    d = _gate_inputs(C, r, P, B=3, seed=7)
    assert torch.equal(_gate_run(d)[1:2], _gate_run(_middle(d, ("rows",))))
