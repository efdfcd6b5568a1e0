"""The case table of tests/test_unwritten_gpu.py: one or more cases per public wrapper of deadtrees_amd/ops.py that
allocates with torch.empty* (directly or through _split_outputs, _rows_buffer, _wgrad, _bn_bwd_setup, _pool_gather).

A case is ``Case(name, wrappers, make, call, cut, wide_u8)``: ``make()`` builds the inputs once on the device (a dict
of tensors / plain values; it also asserts, through the library's own queries, that the shape has the row / slab form
the case is there for), ``call(**inputs)`` runs the wrapper(s) and returns every tensor they return plus the caller
supplied tensors they write.  ``cut`` maps the result to its defined part; every cut is listed here with its reason.
``wide_u8`` names the functions whose uint8 workspace a kernel reads as wider integers.

Whether the values are right is the business of the fp64 / host-reference tests of each op; the inputs here are the
shapes of those tests (or smaller ones with the same bookkeeping), filled with finite random numbers.

``allocating_wrappers()`` is the ast scan tests/test_unwritten_cases_host.py holds against the table.  No test lives
here; importing needs neither a GPU nor the library."""
from __future__ import annotations

import ast
import collections
import ctypes as C
import os
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_PY = os.path.join(ROOT, "deadtrees_amd", "ops.py")
DEV = "cuda"
BF = torch.bfloat16
ALLOCATORS = ("empty", "empty_like", "empty_strided", "new_empty")
HELPERS = ("_split_outputs", "_rows_buffer", "_wgrad", "_bn_bwd_setup", "_pool_gather")

Case = collections.namedtuple("Case", "name wrappers make call cut wide_u8 ref")
CASES: list = []
# name of the case -> (what is cut away, why): the only results that are not compared whole
CUTS = {}
# (case name, check): what a case's shape must be by the library's own host queries; make() runs it, and so does the host test
FORMS: list = []


# generators that the cases of one family share (see _family_gen): a case reseeds them before it builds its inputs
_FAMILY_GENS: list = []


def case(name, wrappers, make, call, cut=None, wide_u8=(), ref=None):
    """``ref(inputs, {path: tensor})``: the comparison of the plain run with the existing reference of the op, at that
    reference test's own bound, for a case whose shape no fp64 / host-reference test has"""
    assert name not in {c.name for c in CASES}, name

    def seeded_make():
        for g in _FAMILY_GENS:          # the inputs depend on the case alone, not on the cases that ran before it
            g.manual_seed(zlib.crc32(name.encode()))
        return make()
    CASES.append(Case(name, (wrappers,) if isinstance(wrappers, str) else tuple(wrappers), seeded_make, call, cut, tuple(wide_u8), ref))


# ------------------------------------------------------------------------------------------------ the source scan
def allocation_sites(path):
    """[(line, qualified name of the innermost enclosing function, allocator)] of every ``torch.empty*`` / ``x.new_empty``
    call of a file (``np.empty`` is none)"""
    with open(path) as f:
        tree = ast.parse(f.read())
    out = []

    def walk(node, qual):
        for child in ast.iter_child_nodes(node):
            inner = qual
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                inner = f"{qual}.{child.name}" if qual else child.name
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in ALLOCATORS:
                owner = child.func.value
                if child.func.attr == "new_empty" or (isinstance(owner, ast.Name) and owner.id == "torch"):
                    out.append((child.lineno, qual or "<module>", child.func.attr))
            walk(child, inner)
    walk(tree, "")
    return sorted(out)


def allocating_wrappers(path=OPS_PY):
    """{public function or class of ops.py: sorted names of the allocators / helpers it calls}"""
    with open(path) as f:
        tree = ast.parse(f.read())
    found = {}
    for top in tree.body:
        if not isinstance(top, (ast.FunctionDef, ast.ClassDef)) or top.name.startswith("_"):
            continue
        used = set()
        for n in ast.walk(top):
            if isinstance(n, ast.Call):
                f = n.func
                if isinstance(f, ast.Attribute) and f.attr in ALLOCATORS and (
                        f.attr == "new_empty" or (isinstance(f.value, ast.Name) and f.value.id == "torch")):
                    used.add(f.attr)
                elif isinstance(f, ast.Name) and f.id in HELPERS:
                    used.add(f.id)
        if used:
            found[top.name] = sorted(used)
    return found


# ------------------------------------------------------------------------------------------------ input helpers
def _ops():
    from deadtrees_amd import ops
    return ops


def _lib():
    from deadtrees_amd import _lib
    return _lib.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _family_gen():
    """a generator for the make() closures of one family; ``case`` reseeds it from the case's name"""
    g = torch.Generator()
    _FAMILY_GENS.append(g)
    return g


def nchw64(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).double()


def oihw64(w_hwio):
    return w_hwio.detach().float().cpu().permute(3, 2, 0, 1).double()


def virtual_input(x, s1=None, mode0=0, sc=None, sh=None, round_bf16=False):
    """fp64 NCHW input of a convolution over (x transformed in fp32 by relu(x * sc + sh), up-sampled for mode0 1) | s1"""
    import torch.nn.functional as F
    z = x.detach().float().cpu().permute(0, 3, 1, 2)
    if sc is not None:
        z = F.relu(z * sc.cpu()[None, :, None, None] + sh.cpu()[None, :, None, None])
        if round_bf16:
            z = z.to(BF).float()
    z = z.double()
    if mode0 == 1:
        z = F.interpolate(z, scale_factor=2, mode="nearest")
    return z if s1 is None else torch.cat([z, nchw64(s1)], 1)


def _assert_rel(got, want, bound):
    err = float((got.double() - want.double()).abs().max() / (want.double().abs().max() + 1e-30))
    assert err < bound, err


def _assert_equal(*pairs):
    for got, want in zip(pairs[::2], pairs[1::2]):
        assert got.shape == want.shape and torch.equal(got, want)


def bn_bwd_sums(out, y, mean, invstd, sc, sh, act, bf16=False):
    """(sum g, sum g * xhat, scale) per channel in fp64 of the stored gradient ``out`` with the ReLU mask the kernels use:
    the stored activation, or y * sc + sh recomputed in fp32 (bf16: rounded to bf16) — the reference of
    test_conv_with_fused_bn_backward_reduction / test_conv_bf16_with_fused_bn_backward_reduction"""
    dz, y64 = nchw64(out), nchw64(y)
    if act is not None:
        mask = nchw64(act) > 0
    else:
        a = y64.float() * sc.cpu()[None, :, None, None] + sh.cpu()[None, :, None, None]
        mask = (a.to(BF).float() if bf16 else a) > 0
    gm = torch.where(mask, dz, torch.zeros_like(dz))
    xh = (y64 - mean.cpu().double()[None, :, None, None]) * invstd.cpu().double()[None, :, None, None]
    return gm.sum(dim=(0, 2, 3)), (gm * xh).sum(dim=(0, 2, 3)), float(gm.abs().sum(dim=(0, 2, 3)).max()) + 1.0


def R(g, *shape, scale=1.0, shift=0.0, dtype=torch.float32):
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).to(DEV)


def U8(g, *shape, high=256):
    return torch.randint(0, high, shape, generator=g, dtype=torch.int64).to(torch.uint8).to(DEV)


def bn_coef(g, Cc):
    """(mean, invstd, act_scale, act_shift) of a layer with Cc channels"""
    return (R(g, Cc, scale=0.1), R(g, Cc, scale=0.1, shift=1.1).abs(), R(g, Cc, scale=0.3, shift=1.0), R(g, Cc, scale=0.2))


def class_map(seed, h, w, K=3, cell=(5, 7)):
    """uint8 [h, w] on the device: random classes on a coarse grid (about 60 % background), blown up to blocks — patches
    that touch along edges and corners, reach the border and differ in class"""
    g = _gen(seed)
    gh, gw = -(-h // cell[0]), -(-w // cell[1])
    coarse = torch.randint(1, K, (gh, gw), generator=g) * (torch.rand((gh, gw), generator=g) > 0.6)
    fine = coarse.repeat_interleave(cell[0], 0).repeat_interleave(cell[1], 1)[:h, :w]
    speck = torch.rand((h, w), generator=g) > 0.97
    fine = torch.where(speck, torch.randint(0, K, (h, w), generator=g), fine)
    return fine.to(torch.uint8).contiguous().to(DEV)


def desc(B, Hin, Win, C0, C1, mode0, Cout, k=3, stride=1, pad=1, split=0, acc=0):
    return _ops().conv_desc(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad, split, acc)


# the constants of data/synthetic.py (deadtreedata.py:31-32): what val_transform and oracle/augment_ref.py normalise with
MEAN4 = [0.3661029729, 0.3875165941, 0.3501133538, 0.5797285859]
STD4 = [0.2388708549, 0.2103625723, 0.2050272174, 0.2025812523]


def _augment_ref():
    from oracle import augment_ref
    return augment_ref


def _np(t):
    return t.detach().cpu().numpy()


def _close_bf16(got, want, extra=0.0):
    """tests/test_bf16_gpu.py::close_bf16: half an ulp of bf16 on the element plus 2^-9 of the largest"""
    err = (got.double().cpu() - want).abs()
    tol = want.abs() * 2.0 ** -8 + want.abs().max() * (2.0 ** -9 + extra)
    assert bool((err <= tol).all()), float((err / tol).max())



# ------------------------------------------------------------------------------------------------ Winograd forward
def _wino_rows(d):
    """the statistics rows of a Winograd descriptor and the form they must have (restated from the wrapper's docstring of
    the rows: one per workgroup when 32 % n_tiles == 0 — at most 256 workgroups —, one per spatial tile otherwise)"""
    lib = _lib()
    assert lib.dt_conv2d_winograd_supported(C.byref(d))
    return lib.dt_conv2d_winograd_stat_rows(C.byref(d))


def _wino(name, B, H, W, C0, Cout, rows, C1=0, mode0=0, split=0, join=False, tf=False, stats=True):
    Hin, Win = (2 * H, 2 * W) if mode0 else (H, W)

    def form():
        d = desc(B, Hin, Win, C0, C1, mode0, Cout, split=split, acc=int(join))
        assert _wino_rows(d) == rows, (name, _wino_rows(d), rows)
    FORMS.append((f"conv2d_winograd {name}", form))

    def make():
        g = _gen(len(name) + B + H + Cout)
        form()
        w = R(g, 3, 3, C0 + C1, Cout, scale=(2.0 / (9 * (C0 + C1))) ** 0.5)
        return dict(x=R(g, B, H, W, C0), u=_ops().winograd_weights(w), w=w, s1=R(g, B, Hin, Win, C1) if C1 else None,
                    base=R(g, B, Hin, Win, split or Cout) if join else None,
                    sc=R(g, C0, scale=0.3, shift=1.0) if tf else None, sh=R(g, C0, scale=0.3, shift=0.2) if tf else None)

    def call(x, u, w, s1, base, sc, sh):
        return _ops().conv2d_winograd(x, u, src1=s1, mode0=mode0, split=split, out0=base, accumulate=join,
                                      want_stats=stats, in_scale=sc, in_shift=sh)

    def ref(inp, out):
        """fp64 convolution, the bounds of test_winograd_conv_matches_fp64_and_direct_kernel"""
        import torch.nn.functional as F
        want = F.conv2d(virtual_input(inp["x"], inp["s1"], mode0, inp["sc"], inp["sh"]), oihw64(inp["w"]), padding=1)
        got = nchw64(out["out[0]"])
        slack = 0.0
        if join:
            got, slack = got - nchw64(inp["base"]), 1e-6 * float(inp["base"].abs().max())
        if split:
            got = torch.cat([got, nchw64(out["out[1]"])], 1)
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-5 * scale + slack, (name, float((got - want).abs().max()) / scale)
        if stats and not split and not join:
            st = out["out[2]"].double().cpu()
            assert tuple(st.shape) == (2, rows, Cout), st.shape
            np.testing.assert_allclose(st[0].sum(0), want.sum(dim=(0, 2, 3)), rtol=1e-4,
                                       atol=1e-4 * float(want.abs().sum(dim=(0, 2, 3)).max()))
            np.testing.assert_allclose(st[1].sum(0), (want * want).sum(dim=(0, 2, 3)), rtol=1e-4)
    case(f"conv2d_winograd {name}", "conv2d_winograd", make, call, ref=ref)


_wino("Cout 64 ragged 17x33: a row per workgroup", 1, 17, 33, 64, 64, rows=6)
_wino("Cout 128 ragged 17x33: a row per workgroup", 1, 17, 33, 64, 128, rows=12)
_wino("Cout 192 ragged 17x33: a row per spatial tile", 1, 17, 33, 64, 192, rows=6)
_wino("Cout 64 whole tiles 32x48", 1, 32, 48, 64, 64, rows=6)
_wino("Cout 192 whole tiles 32x48", 1, 32, 48, 64, 192, rows=6)
_wino("packed small maps B=5 7x6", 5, 7, 6, 64, 128, rows=4)
_wino("300 tiles on 256 workgroups, partial last round", 3, 80, 80, 64, 256, rows=256)
_wino("split 64 | 64", 1, 17, 33, 64, 128, rows=12, split=64)
_wino("join", 1, 17, 33, 64, 64, rows=6, join=True)
_wino("up-sampled + skip", 2, 9, 17, 64, 64, rows=12, C1=64, mode0=1)
_wino("input transform", 1, 17, 33, 64, 64, rows=6, tf=True, stats=False)


def _bn_bwd(name, wrapper, B, H, W, C0, Cout, rows_query, rows=None, join=False, dtype=torch.float32, config=None):
    """config: what dt_conv2d_config (tw, tn, ck, uses_zi) / dt_conv2d_bf16_config (tw, tn, ck, mt) answer for the descriptor:
    the forward kernel the fused epilogue runs in (ck >= 1000: the lean narrow fp32 kernel; mt 16: the bf16 narrow one)"""
    def form():
        d = desc(B, H, W, C0, 0, 0, Cout, acc=int(join))
        got = getattr(_lib(), rows_query)(C.byref(d))
        assert got > 0 and (rows is None or got == rows), (name, got, rows)
        if config is not None:
            import conv_variant_cases as cvc
            t = cvc.make(B, H, W, C0, 0, 0, Cout, 3, 1, 1, 0, int(join))
            answer = cvc.bf16_config(t) if dtype == BF else cvc.fp32_config(t)
            assert tuple(answer) == config, (name, answer, config)
    FORMS.append((f"{wrapper} {name}", form))

    def make():
        g = _gen(B + H + C0 + Cout + int(join))
        form()
        w = R(g, 3, 3, C0, Cout, scale=(2.0 / (9 * C0)) ** 0.5)
        if wrapper == "conv2d_winograd_bn_bwd":
            weights = _ops().winograd_weights(w)
        elif wrapper == "conv2d_bf16_bn_bwd":
            weights = _ops().pack_weights_bf16(w)
        else:
            weights = w
        mean, invstd, sc, sh = bn_coef(g, Cout)
        y = R(g, B, H, W, Cout, dtype=dtype)
        inp = dict(x=R(g, B, H, W, C0, dtype=dtype), weights=weights, w=w, y=y, mean=mean, invstd=invstd)
        if join:      # block output: the stored activation and the tensor the gradient is added to
            inp.update(act=torch.relu(y.float() * sc + sh).to(dtype), join_into=R(g, B, H, W, Cout, dtype=dtype), sc=None, sh=None)
        else:
            inp.update(act=None, join_into=None, sc=sc, sh=sh)
        return inp

    def call(x, weights, w, y, mean, invstd, sc, sh, act, join_into):
        kw = dict(act_scale=sc, act_shift=sh, act=act, join_into=join_into)
        if wrapper == "conv2d_bf16_bn_bwd":
            return _ops().conv2d_bf16_bn_bwd(x, weights, Cout, y, mean, invstd, **kw)
        return getattr(_ops(), wrapper)(x, weights, y, mean, invstd, **kw)

    def ref(inp, out):
        """the references and bounds of test_conv_with_fused_bn_backward_reduction, its bf16 twin and
        test_winograd_fused_bn_backward_sums_match_the_direct_kernel: the output against the plain convolution (+ join),
        the rows summed against the BatchNorm-backward reduction of the stored gradient in fp64"""
        ops, bf = _ops(), dtype == BF
        base = None if inp["join_into"] is None else inp["join_into"].clone()
        if bf:
            plain, _, _ = ops.conv2d_bf16(inp["x"], inp["weights"], 3, 1, 1, Cout, out0=base, accumulate=join)
        else:
            plain, _, _ = ops.conv2d(inp["x"], inp["w"], 3, 1, 1, out0=base, accumulate=join)
        got, red = out["out[0]"], out["out[1]"].double().cpu()
        assert tuple(red.shape[::2]) == (2, Cout) and (rows is None or red.shape[1] == rows), red.shape
        if wrapper == "conv2d_winograd_bn_bwd":
            scale = float(plain.abs().max())
            assert float((got - plain).abs().max()) <= 1e-5 * scale, (name, float((got - plain).abs().max()) / scale)
        else:
            assert torch.equal(got, plain), name
        s0, s1, scale = bn_bwd_sums(got, inp["y"], inp["mean"], inp["invstd"], inp["sc"], inp["sh"], inp["act"], bf16=bf)
        b0, b1 = (3e-5, 1e-4) if bf else (2e-5, 6e-5)
        if wrapper == "conv2d_winograd_bn_bwd":          # that test's bound against the direct kernel's sums
            b0 = b1 = 1e-4
        assert float((red[0].sum(0) - s0).abs().max()) <= b0 * scale, (name, float((red[0].sum(0) - s0).abs().max()) / scale)
        assert float((red[1].sum(0) - s1).abs().max()) <= b1 * scale, (name, float((red[1].sum(0) - s1).abs().max()) / scale)
    case(f"{wrapper} {name}", wrapper, make, call, ref=ref)


def _wino_up_dgrad(B, H, W, Cy, cx, sk, x_only=False):
    """dt_conv2d_winograd_upsampled_dgrad / _x have no wrapper in ops.py (the engine calls them): the call of
    tests/test_winograd_gpu.py, with the outputs and the `red` buffer allocated here, under the poison"""
    from deadtrees_amd import _lib as L
    rows_query = "dt_conv2d_winograd_upsampled_dgrad_x_rows" if x_only else "dt_conv2d_winograd_upsampled_dgrad_rows"

    def descriptor():
        return L.ConvDesc(B, H, W, Cy, 0, 0, H, W, cx + sk, 3, 1, 1, cx, 0)

    def form():
        d = descriptor()
        assert _lib().dt_conv2d_winograd_upsampled_dgrad_supported(C.byref(d)) and getattr(_lib(), rows_query)(C.byref(d)) > 0
    name = f"dt_conv2d_winograd_upsampled_dgrad{'_x' if x_only else ''} {B} x {H}x{W}, {Cy} -> {cx}{f' + skip {sk}' if sk else ''}"
    FORMS.append((name, form))

    def make():
        g = _gen(B * 7 + H + cx)
        form()
        wd = _ops().weight_flip_transpose(R(g, 3, 3, cx + sk, Cy, scale=0.05))
        mean, invstd, sc, sh = bn_coef(g, cx)
        return dict(dy=R(g, B, H, W, Cy), u=_ops().winograd_weights(wd), y=R(g, B, H // 2, W // 2, cx), mean=mean, invstd=invstd, sc=sc, sh=sh)

    def call(dy, u, y, mean, invstd, sc, sh):
        lib, d = _lib(), descriptor()
        P = getattr(lib, rows_query)(C.byref(d))
        red = torch.empty(lib.dt_bn_stats_floats(P, cx), dtype=torch.float32, device=DEV)
        gx = torch.empty((B, H // 2, W // 2, cx), dtype=torch.float32, device=DEV)
        dskip = torch.empty((B, H, W, sk), dtype=torch.float32, device=DEV) if sk and not x_only else None
        fuse = L.BnBwdFuse(y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), sc.data_ptr(), sh.data_ptr())
        st = torch.cuda.current_stream().cuda_stream
        if x_only:
            L.check(lib.dt_conv2d_winograd_upsampled_dgrad_x(C.byref(d), dy.data_ptr(), u.data_ptr(), gx.data_ptr(), red.data_ptr(),
                                                             C.byref(fuse), st), name)
        else:
            L.check(lib.dt_conv2d_winograd_upsampled_dgrad(C.byref(d), dy.data_ptr(), u.data_ptr(), gx.data_ptr(),
                                                           dskip.data_ptr() if sk else None, red.data_ptr(), C.byref(fuse), 3, st), name)
        return gx, dskip, red[:2 * P * cx].view(2, P, cx)

    def ref(inp, out):
        """the chain it replaces, as test_winograd_data_gradient_with_fused_upsample_backward compares it: conv2d_winograd with
        split outputs, then upsample2x_bwd_bn; gx and the skip's gradient bit-identical, the sums at rtol 1e-5"""
        dup, dskip_ref, _ = _ops().conv2d_winograd(inp["dy"], inp["u"], split=cx if sk else 0)
        g_ref, red_ref = _ops().upsample2x_bwd_bn(dup, inp["y"], inp["mean"], inp["invstd"], inp["sc"], inp["sh"])
        assert torch.equal(out["out[0]"], g_ref), name
        if sk and not x_only:
            assert torch.equal(out["out[1]"], dskip_ref), name
        got = out["out[2]"].double().sum(1).cpu()
        want = red_ref.double().sum(1).cpu()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    case(name, (), make, call, ref=ref)


for _x_only in (False, True):
    _wino_up_dgrad(3, 18, 34, 64, 64, 0, _x_only)
    _wino_up_dgrad(1, 18, 34, 64, 64, 64, _x_only)
    _wino_up_dgrad(2, 32, 48, 64, 128, 64, _x_only)
    _wino_up_dgrad(2, 32, 48, 64, 64, 0, _x_only)

WQ = "dt_conv2d_winograd_stat_rows"
_bn_bwd("Cout 64 ragged 17x33, virtual activation", "conv2d_winograd_bn_bwd", 1, 17, 33, 64, 64, WQ, rows=6)
_bn_bwd("Cout 128 ragged 17x33, join", "conv2d_winograd_bn_bwd", 1, 17, 33, 64, 128, WQ, rows=12, join=True)
_bn_bwd("Cout 192 ragged 17x33: a row per spatial tile", "conv2d_winograd_bn_bwd", 1, 17, 33, 64, 192, WQ, rows=6)
_bn_bwd("Cout 64 whole tiles 32x48, join", "conv2d_winograd_bn_bwd", 1, 32, 48, 64, 64, WQ, rows=6, join=True)
_bn_bwd("packed small maps B=5 7x6", "conv2d_winograd_bn_bwd", 5, 7, 6, 64, 128, WQ, rows=4)
_bn_bwd("300 tiles on 256 workgroups", "conv2d_winograd_bn_bwd", 3, 80, 80, 64, 256, WQ, rows=256)
_bn_bwd("40 -> 48 ragged 17x33, virtual activation", "conv2d_bn_bwd", 1, 17, 33, 40, 48, "dt_conv2d_stat_rows", config=(32, 32, 16, 0))
_bn_bwd("40 -> 48 ragged 17x33, join", "conv2d_bn_bwd", 1, 17, 33, 40, 48, "dt_conv2d_stat_rows", join=True, config=(32, 32, 16, 0))
_bn_bwd("16 -> 16 narrow 17x33", "conv2d_bn_bwd", 2, 17, 33, 16, 16, "dt_conv2d_stat_rows", config=(32, 16, 1011, 0))
_bn_bwd("40 -> 48 ragged 17x33, virtual activation", "conv2d_bf16_bn_bwd", 1, 17, 33, 40, 48, "dt_conv2d_bf16_stat_rows", dtype=BF,
        config=(32, 32, 32, 2))
_bn_bwd("64 -> 128 ragged 17x33, join", "conv2d_bf16_bn_bwd", 2, 17, 33, 64, 128, "dt_conv2d_bf16_stat_rows", join=True, dtype=BF,
        config=(32, 32, 32, 2))
_bn_bwd("16 -> 16 narrow 17x33", "conv2d_bf16_bn_bwd", 2, 17, 33, 16, 16, "dt_conv2d_bf16_stat_rows", dtype=BF,
        config=(32, 16, 16, 16))


# ------------------------------------------------------------------------------------------------ direct / bf16 forward
def variant_descriptors(prec):
    """the descriptors of tests/conv_variant_cases.py this table takes for ``prec``: per kernel configuration (tn, ck and
    the lean / persistent flag: uses_zi or mt) the cheapest plain descriptor, and the cheapest split and join ones"""
    import conv_variant_cases as cvc
    found = cvc.cases()[prec]
    penalty = {sh: pen for pen, sh in cvc._shapes()}          # the raggedness rank conv_variant_cases puts first
    rank = lambda t: (penalty[t[1:6] + t[8:]], cvc.macs(t), t)      # noqa: E731  (t without B, Ho, Wo is the shape)
    best = {}
    for key, t in found.items():
        k = dict(zip(cvc.FP32_KEY if prec == "fp32" else cvc.BF16_KEY, key))
        if k["ksize"] == 4:
            continue                                    # the space-to-depth stem: the stem_conv_bf16 case
        kind = "split" if k["split"] else "join" if k["accumulate"] else ("plain", k["tn"], k["ck"], k.get("uses_zi", k.get("mt")))
        if kind not in best or rank(t) < rank(best[kind][1]):
            best[kind] = (cvc.case_id(prec, key), t)
    return sorted(best.values())


def _variant(prec, ident, t):
    import conv_variant_cases as cvc
    d = dict(zip(cvc.FIELDS, t))
    dtype = torch.float32 if prec == "fp32" else BF
    k, cin = d["ksize"], d["C0"] + d["C1"]
    key_of, config_of = (cvc.fp32_key, cvc.fp32_config) if prec == "fp32" else (cvc.bf16_key, cvc.bf16_config)

    def form():
        """the descriptor still dispatches to the configuration its name says, and has statistics rows"""
        assert cvc.case_id(prec, key_of(t)) == ident, (ident, cvc.case_id(prec, key_of(t)))
        rows = getattr(_lib(), "dt_conv2d_stat_rows" if prec == "fp32" else "dt_conv2d_bf16_stat_rows")(C.byref(cvc.descriptor(t)))
        assert rows > 0, (ident, rows)
    FORMS.append((f"conv2d {ident}", form))

    def make():
        g = _gen(sum(t))
        sh = 1 if d["mode0"] else 0
        form()
        w = R(g, k, k, cin, d["Cout"], scale=(2.0 / (k * k * cin)) ** 0.5)
        if prec == "bf16":
            w = R(g, k * k, d["Cout"], cin, scale=(2.0 / (k * k * cin)) ** 0.5, dtype=BF)
        return dict(x0=R(g, d["B"], d["Hin"] >> sh, d["Win"] >> sh, d["C0"], dtype=dtype),
                    x1=R(g, d["B"], d["Hin"], d["Win"], d["C1"], dtype=dtype) if d["C1"] else None, w=w,
                    base=R(g, d["B"], d["Ho"], d["Wo"], d["cout_split"] or d["Cout"], dtype=dtype) if d["accumulate"] else None,
                    )

    def call(x0, x1, w, base):
        kw = dict(src1=x1, mode0=d["mode0"], split=d["cout_split"], out0=base, accumulate=bool(d["accumulate"]), want_stats=True)
        if prec == "fp32":
            return _ops().conv2d(x0, w, k, d["stride"], d["pad"], **kw)
        return _ops().conv2d_bf16(x0, w, k, d["stride"], d["pad"], d["Cout"], **kw)
    case(f"{'conv2d' if prec == 'fp32' else 'conv2d_bf16'} {ident}", "conv2d" if prec == "fp32" else "conv2d_bf16", make, call)


def add_variant_cases():
    """the conv2d / conv2d_bf16 cases need the library's dispatch queries, so they join the table on first use (the
    host test and the GPU module call this; the queries run on the host)"""
    if any(c.name.startswith("conv2d fp32-") for c in CASES):
        return
    for prec in ("fp32", "bf16"):
        picked = variant_descriptors(prec)
        assert len(picked) >= 6, picked
        for ident, t in picked:
            _variant(prec, ident, t)


def _conv_affine():
    def make():
        g = _gen(5)
        return dict(x=R(g, 1, 17, 33, 40), w=R(g, 3, 3, 40, 48, scale=0.07), sc=R(g, 48, scale=0.2, shift=1.0), sh=R(g, 48, scale=0.2))
    def ref(inp, out):
        """bit-identical to dt_conv2d followed by dt_bn_act (test_kernels_gpu.py, the fused inference epilogue test)"""
        y, _, _ = _ops().conv2d(inp["x"], inp["w"], 3, 1, 1)
        _assert_equal(out["out"], _ops().bn_act(y, inp["sc"], inp["sh"], relu=True))
    case("conv2d_affine 40 -> 48 ragged 17x33", "conv2d_affine", make,
         lambda x, w, sc, sh: _ops().conv2d_affine(x, w, 3, 1, 1, sc, sh, relu=True), ref=ref)


_conv_affine()


# ------------------------------------------------------------------------------------------------ weight gradients
def _wgrad(name, wrapper, B, H, W, C0, Cout, k=3, stride=1, pad=1, C1=0, mode0=0, tf=False, parts=None, dtype=torch.float32,
           family=None):
    """H, W: the stored size of source 0.  parts: (parts, parts2) of wg_cfg, confirmed through the workspace query.
    family: (kernel family of dt_conv2d_wgrad_bf16, its partial slabs).  The ABI has no query that names the family, so the
    check restates the dispatch rule of csrc (LDS-DMA: 3x3 stride 1 with C0, C1 and Cout multiples of 64; narrow: Cin and
    Cout <= 32; register-staged: the rest) and pins the slab count of the workspace, which differs between the families and
    moves when the dispatch does (with the LDS-DMA kernel at its default, on)"""
    Hin, Win = (2 * H, 2 * W) if mode0 else (H, W)

    def form():
        d = desc(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad)
        E = k * k * (C0 + C1) * Cout
        got = getattr(_lib(), f"dt_{wrapper}_workspace")(C.byref(d))
        assert got > 0, (name, _lib().dt_last_error().decode())
        if parts is not None:
            want = (parts[0] + (parts[1] if parts[1] != parts[0] else 0)) * E * 4
            assert got == want, (name, got, want, got / (E * 4))
        if "n16" in name or "sub-pixel" in name:
            assert _lib().dt_conv2d_wgrad_n16_supported(C.byref(d)), name
        if wrapper == "conv2d_wgrad_winograd":
            assert _lib().dt_conv2d_wgrad_winograd_supported(C.byref(d)), name
        if family is not None:
            import conv_variant_cases as cvc
            dma_shape = k == 3 and stride == 1 and C0 % 64 == 0 and C1 % 64 == 0 and Cout % 64 == 0
            narrow_shape = C0 + C1 <= 32 and Cout <= 32
            assert {"LDS-DMA": dma_shape, "narrow": narrow_shape, "register-staged": not dma_shape and not narrow_shape}[family[0]], name
            if cvc.dma_default() == 1:
                assert got == family[1] * E * 4, (name, got / (E * 4), family)
    FORMS.append((f"{wrapper} {name}", form))

    def make():
        g = _gen(B * 100 + H + C0 + Cout + k)
        form()
        d = desc(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad)
        return dict(x=R(g, B, H, W, C0, dtype=dtype), dy=R(g, B, d.Ho, d.Wo, Cout, dtype=dtype),
                    s1=R(g, B, Hin, Win, C1, dtype=dtype) if C1 else None,
                    sc=R(g, C0, scale=0.3, shift=1.0) if tf else None, sh=R(g, C0, scale=0.3, shift=0.2) if tf else None)

    def call(x, dy, s1, sc, sh):
        kw = dict(src1=s1, mode0=mode0, in_scale=sc, in_shift=sh)
        if wrapper == "conv2d_wgrad_winograd":
            return _ops().conv2d_wgrad_winograd(x, dy, **kw)
        return getattr(_ops(), wrapper)(x, dy, k, stride, pad, **kw)

    def ref(inp, out):
        """fp64 weight gradient of the same (bf16: bf16-rounded) operands, HWIO; 2e-5 of the largest element, the bound of
        test_winograd_weight_gradient_matches_fp64_and_direct_kernel (both fp32 kernels) and of test_wgrad_bf16"""
        xin = virtual_input(inp["x"], inp["s1"], mode0, inp["sc"], inp["sh"], round_bf16=dtype == BF)
        want = torch.nn.grad.conv2d_weight(xin, (Cout, C0 + C1, k, k), nchw64(inp["dy"]), stride=stride, padding=pad)
        want = want.permute(2, 3, 1, 0)
        got = out["out"].double().cpu()
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 2e-5 * scale, (name, float((got - want).abs().max()) / scale)
    case(f"{wrapper} {name}", wrapper, make, call, ref=ref)


_wgrad("single stage: 4 parts", "conv2d_wgrad", 1, 16, 16, 64, 64, parts=(4, 4))
_wgrad("17 parts, rb 2, a short last block of 9", "conv2d_wgrad", 1, 68, 16, 64, 64, parts=(17, 9))
_wgrad("ksplit limited by T: a 4x4 map", "conv2d_wgrad", 1, 4, 4, 64, 64, parts=(1, 1))
_wgrad("two images of 17x33, 40 -> 48", "conv2d_wgrad", 2, 17, 33, 40, 48)
_wgrad("stem 7x7 stride 2", "conv2d_wgrad", 1, 17, 33, 3, 64, k=7, stride=2, pad=3)
_wgrad("3x3 stride 2", "conv2d_wgrad", 1, 18, 34, 64, 128, stride=2)
_wgrad("1x1 stride 2", "conv2d_wgrad", 1, 18, 34, 64, 128, k=1, stride=2, pad=0)
_wgrad("n16 16 -> 16", "conv2d_wgrad", 1, 9, 33, 16, 16)
_wgrad("n16 16 -> 32", "conv2d_wgrad", 1, 9, 33, 16, 32)
_wgrad("n16 32 -> 16 with the input transform", "conv2d_wgrad", 2, 9, 33, 32, 16, tf=True)
_wgrad("sub-pixel mode0 = 1, 32 -> 16, input transform", "conv2d_wgrad", 2, 9, 17, 32, 16, mode0=1, tf=True)
_wgrad("sub-pixel mode0 = 1, 16 -> 16", "conv2d_wgrad", 1, 5, 37, 16, 16, mode0=1)
_wgrad("up-sampled + skip (C1 > 0), input transform", "conv2d_wgrad", 1, 9, 17, 64, 64, C1=64, mode0=1, tf=True)
_wgrad("Cout 32 ragged 17x33", "conv2d_wgrad_winograd", 3, 17, 33, 64, 32)
_wgrad("Cout 64 ragged 17x33", "conv2d_wgrad_winograd", 1, 17, 33, 64, 64)
_wgrad("Cout 64 whole tiles 32x32", "conv2d_wgrad_winograd", 2, 32, 32, 64, 64)
_wgrad("mode0 = 1 with C1, Cout 32, input transform", "conv2d_wgrad_winograd", 2, 16, 20, 64, 32, C1=64, mode0=1, tf=True)
_wgrad("register-staged 64 -> 32, 8x8", "conv2d_wgrad_bf16", 2, 8, 8, 64, 32, dtype=BF, family=("register-staged", 2))
_wgrad("narrow 16 -> 16, 40x24", "conv2d_wgrad_bf16", 1, 40, 24, 16, 16, dtype=BF, family=("narrow", 10))
_wgrad("LDS-DMA 64 -> 64, 8x8", "conv2d_wgrad_bf16", 2, 8, 8, 64, 64, dtype=BF, family=("LDS-DMA", 2))
_wgrad("LDS-DMA ragged 5 x 13x11", "conv2d_wgrad_bf16", 5, 13, 11, 64, 64, dtype=BF, family=("LDS-DMA", 10))
_wgrad("LDS-DMA up-sampled + skip", "conv2d_wgrad_bf16", 1, 12, 10, 128, 64, C1=64, mode0=1, dtype=BF,
       family=("LDS-DMA", 6))
_wgrad("3x3 stride 2", "conv2d_wgrad_bf16", 2, 32, 32, 64, 128, stride=2, dtype=BF, family=("register-staged", 4))


def _weights():
    g = _family_gen()
    def wino_ref(inp, out):
        """U = G g G^T in fp64, 1e-6 of the largest element (test_winograd_weight_transform)"""
        w = inp["w"].double().cpu()
        G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
        want = torch.einsum("ia,abco,jb->ijco", G, w, G)
        cin, cout = w.shape[2:]
        got = out["out"].double().cpu().permute(0, 1, 2, 4, 3).reshape(16, cin, cout).reshape(4, 4, cin, cout)
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())

    def flip_ref(inp, out):
        """a permutation: the taps reversed, the channel axes exchanged (what the data-gradient tests feed to conv2d)"""
        _assert_equal(out["out"], inp["w"].flip(0, 1).permute(0, 1, 3, 2).contiguous())

    def pack_ref(inp, out):
        """permutations and one rounding to bf16: [tap][Cout][Cin], and [tap][Cin][Cout] with the taps reversed"""
        w = inp["w"]
        _assert_equal(out["out[0]"], w.permute(0, 1, 3, 2).reshape(9, w.shape[3], w.shape[2]).to(BF),
                      out["out[1]"], w.flip(0, 1).reshape(9, w.shape[2], w.shape[3]).to(BF))
    case("winograd_weights 64 -> 128", "winograd_weights", lambda: dict(w=R(g, 3, 3, 64, 128)), lambda w: _ops().winograd_weights(w),
         ref=wino_ref)
    case("weight_flip_transpose 3x3 40 -> 48", "weight_flip_transpose", lambda: dict(w=R(g, 3, 3, 40, 48)),
         lambda w: _ops().weight_flip_transpose(w), ref=flip_ref)
    case("pack_weights_bf16 forward and data-gradient images", "pack_weights_bf16", lambda: dict(w=R(g, 3, 3, 40, 48)),
         lambda w: (_ops().pack_weights_bf16(w), _ops().pack_weights_bf16(w, dgrad=True)), ref=pack_ref)


_weights()


def _stem():
    def make():
        g = _gen(9)
        return dict(x=R(g, 3, 34, 70, 3), w=R(g, 7, 7, 3, 64, scale=0.08), dy=R(g, 3, 17, 35, 64, dtype=BF))

    def conv_ref(inp, out):
        """fp64 convolution of the bf16-rounded image and weights, one bf16 rounding of the result (close_bf16)"""
        import torch.nn.functional as F
        x = inp["x"].to(BF).double().cpu().permute(0, 3, 1, 2)
        _close_bf16(nchw64(out["out[0]"]), F.conv2d(x, oihw64(inp["w"].to(BF)), stride=2, padding=3))

    def wgrad_ref(inp, out):
        """fp64 weight gradient on the bf16-rounded image and gradient, 3e-5 (test_stem_weight_gradient_on_bf16_kernels)"""
        x = inp["x"].to(BF).double().cpu().permute(0, 3, 1, 2)
        want = torch.nn.grad.conv2d_weight(x, (64, 3, 7, 7), nchw64(inp["dy"]), stride=2, padding=3).permute(2, 3, 1, 0)
        _assert_rel(out["out"].double().cpu(), want, 3e-5)
    # 3 x 34x70 x 3: a shape of test_stem_on_bf16_kernels_via_space_to_depth and test_stem_weight_gradient_on_bf16_kernels
    case("stem_conv_bf16 3 x 34x70 with statistics", "stem_conv_bf16", make, lambda x, w, dy: _ops().stem_conv_bf16(x, w, want_stats=True),
         ref=conv_ref)
    case("stem_wgrad_bf16 3 x 34x70", "stem_wgrad_bf16", make, lambda x, w, dy: _ops().stem_wgrad_bf16(x, dy), ref=wgrad_ref)


_stem()


def _up_dgrad(h, w_, cin, cout, fused=True):
    def make(dtype):
        g = _gen(h + w_ + cin)
        mean, invstd, sc, sh = bn_coef(g, cin)
        w = R(g, 3, 3, cin, cout, scale=0.08)
        return dict(dy=R(g, 2, 2 * h, 2 * w_, cout, dtype=dtype), w=w if dtype != BF else _ops().pack_weights_bf16(w, dgrad=True),
                    y=R(g, 2, h, w_, cin, dtype=dtype), mean=mean, invstd=invstd, sc=sc, sh=sh)
    if fused:
        case(f"conv2d_bf16_upsampled_dgrad {cin} -> {cout}, {h}x{w_}", "conv2d_bf16_upsampled_dgrad", lambda: make(BF),
             lambda dy, w, y, mean, invstd, sc, sh: _ops().conv2d_bf16_upsampled_dgrad(dy, w, cin, y, mean, invstd, sc, sh))
    case(f"conv2d_upsampled_dgrad {cin} -> {cout}, {h}x{w_}" + ("" if fused else " without the BatchNorm sums"),
         "conv2d_upsampled_dgrad", lambda: make(torch.float32),
         (lambda dy, w, y, mean, invstd, sc, sh: _ops().conv2d_upsampled_dgrad(dy, w, cin, y, mean, invstd, sc, sh)) if fused else
         (lambda dy, w, y, mean, invstd, sc, sh: _ops().conv2d_upsampled_dgrad(dy, w, cin)))


_up_dgrad(21, 19, 32, 16)
_up_dgrad(9, 40, 16, 32)
_up_dgrad(4, 16, 32, 16, fused=False)


# ------------------------------------------------------------------------------------------------ BatchNorm, element-wise
def _bn_stats(g, P, Cc, count):
    """[2, P, Cc] partial sums of a batch with per-channel mean m and variance v (v > 0.5: a finite invstd)"""
    m, v = torch.randn(Cc, generator=g) * 0.3, 0.5 + torch.rand(Cc, generator=g)
    share = torch.rand((P, 1), generator=g) + 0.5
    share = share / share.sum()
    return torch.stack((share * (m * count), share * ((v + m * m) * count))).float().to(DEV)


def _bn_finalize(P):
    def make():
        g = _gen(P)
        Cc = 64
        # two stages above 256 rows (BN_STAGE1_MIN_ROWS), 64-row blocks: 257 and 321 end in a block of one row
        assert _lib().dt_bn_stats_floats(P, Cc) == 2 * P * Cc + 2 * -(-P // 64) * Cc
        return dict(stats=_bn_stats(g, P, Cc, 4096.0), gamma=R(g, Cc, scale=0.2, shift=1.0), beta=R(g, Cc, scale=0.2),
                    rm=R(g, Cc, scale=0.1), rv=R(g, Cc, scale=0.1, shift=1.0).abs(), mom=torch.full((1,), 0.1, device=DEV))
    def ref(inp, out):
        """torch's training-mode BatchNorm bookkeeping in fp64 from the summed rows, at the tolerance
        test_kernels_gpu.py::_batchnorm_train_forward_backward holds the running statistics to (rtol 1e-5, atol 1e-6)"""
        n, eps, mom = 4096.0, 1e-5, 0.1
        S = inp["stats"].double().sum(1).cpu()
        mean = S[0] / n
        var = S[1] / n - mean * mean
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = inp["gamma"].double().cpu() * invstd
        want = {"out[0][0]": mean, "out[0][1]": invstd, "out[0][2]": scale, "out[0][3]": inp["beta"].double().cpu() - mean * scale,
                "out[1]": (1 - mom) * inp["rm"].double().cpu() + mom * mean,
                "out[2]": (1 - mom) * inp["rv"].double().cpu() + mom * var * n / (n - 1)}
        for path, w in want.items():
            np.testing.assert_allclose(out[path].double().cpu(), w, rtol=1e-5, atol=1e-6, err_msg=f"P = {P}: {path}")
    case(f"bn_finalize P = {P}", "bn_finalize", make,
         lambda stats, gamma, beta, rm, rv, mom: (_ops().bn_finalize(stats, 4096.0, gamma, beta, rm, rv), rm, rv), ref=ref)
    case(f"bn_finalize_dev P = {P}", "bn_finalize_dev", make,
         lambda stats, gamma, beta, rm, rv, mom: (_ops().bn_finalize_dev(stats, 4096.0, gamma, beta, rm, rv, mom), rm, rv), ref=ref)


for _P in (3, 256, 257, 321):
    _bn_finalize(_P)


def _bn_backward(Cc, n_pix, virtual, dtype=torch.float32, shape=None):
    shape = shape or (1, 1, n_pix, Cc)

    def make():
        g = _gen(Cc + n_pix)
        mean, invstd, sc, sh = bn_coef(g, Cc)
        y = R(g, *shape, dtype=dtype)
        return dict(dout=R(g, *shape, dtype=dtype), act=None if virtual else torch.relu(y.float() * sc + sh).to(dtype), y=y,
                    mean=mean, invstd=invstd, gamma=R(g, Cc, scale=0.2, shift=1.0), sc=sc if virtual else None,
                    sh=sh if virtual else None, dres=R(g, *shape, dtype=dtype) if dtype == BF and virtual else None)
    def ref(inp, out):
        """the fp64 BatchNorm backward of the masked gradient: test_kernels_gpu.py::_batchnorm_train_forward_backward (2e-5 of the
        largest element; the residual gradient 1e-6) and test_bf16_gpu.py::_bn_backward_bf16 (its sums and close_bf16 bounds)"""
        bf = dtype == BF
        flat = lambda t: t.double().cpu().reshape(-1, Cc)      # noqa: E731
        y, d = flat(inp["y"]), flat(inp["dout"])
        mean, invstd, gamma = (inp[k].double().cpu() for k in ("mean", "invstd", "gamma"))
        if virtual:
            a = flat(inp["y"]).float() * inp["sc"].cpu() + inp["sh"].cpu()
            mask = (a.to(BF).float() if bf else a) > 0
        else:
            mask = flat(inp["act"]) > 0
        gm = torch.where(mask, d, torch.zeros_like(d))
        n, xh = y.shape[0], (y - mean) * invstd
        dbeta, dgamma = gm.sum(0), (gm * xh).sum(0)
        dy = gamma * invstd * (gm - dbeta / n - xh * dgamma / n)
        dres = gm if inp["dres"] is None else flat(inp["dres"]) + gm
        got_dy, got_dg, got_db, got_res = (flat(out[f"out[{i}]"]) if i in (0, 3) else out[f"out[{i}]"].double().cpu() for i in range(4))
        if bf:
            tol = 3e-5 * float(gm.abs().sum(0).max()) + 1e-4
            assert float((got_db - dbeta).abs().max()) < tol and float((got_dg - dgamma).abs().max()) < 4 * tol
            _close_bf16(got_dy, dy, extra=1e-4)
            _close_bf16(got_res, dres)
        else:
            _assert_rel(got_dy, dy, 2e-5)
            _assert_rel(got_dg, dgamma, 2e-5)
            _assert_rel(got_db, dbeta, 2e-5)
            _assert_rel(got_res, dres, 1e-6)
    form = "virtual activation" if virtual else "stored activation"
    if dtype == BF:
        case(f"bn_backward_bf16 C = {Cc}, {n_pix} pixels, {form}", "bn_backward_bf16", make,
             lambda dout, act, y, mean, invstd, gamma, sc, sh, dres: _ops().bn_backward_bf16(
                 dout, act, y, mean, invstd, gamma, want_dres=True, act_scale=sc, act_shift=sh, dres=dres), ref=ref)
    else:
        case(f"bn_backward C = {Cc}, {n_pix} pixels, {form}", "bn_backward", make,
             lambda dout, act, y, mean, invstd, gamma, sc, sh, dres: _ops().bn_backward(
                 dout, act, y, mean, invstd, gamma, want_dres=True, act_scale=sc, act_shift=sh), ref=ref)


for _C in (4, 1024):
    for _n in (3, 257):
        for _virtual in (False, True):
            _bn_backward(_C, _n, virtual=_virtual)
            _bn_backward(2 * _C, _n, virtual=_virtual, dtype=BF)
_bn_backward(64, 2 * 17 * 33, False, shape=(2, 17, 33, 64))
_bn_backward(64, 2 * 17 * 33, True, dtype=BF, shape=(2, 17, 33, 64))


def _elementwise():
    g = _family_gen()

    def act_inputs(dtype):
        return lambda: dict(y=R(g, 2, 5, 7, 64, dtype=dtype), sc=R(g, 64, scale=0.2, shift=1.0), sh=R(g, 64, scale=0.2),
                            res=R(g, 2, 5, 7, 64, dtype=dtype), rsc=R(g, 64, scale=0.2, shift=1.0), rsh=R(g, 64, scale=0.2))
    def act_ref(bf):
        def ref(inp, out):
            """fp64 relu(y * sc + sh + res * rsc + rsh) and y * sc + sh: 1e-5 of the largest element in fp32
            (_batchnorm_train_forward_backward), close_bf16 in bf16 (test_bn_act_bf16)"""
            y, res = inp["y"].double().cpu(), inp["res"].double().cpu()
            sc, sh, rsc, rsh = (inp[k].double().cpu() for k in ("sc", "sh", "rsc", "rsh"))
            for path, want in (("out[0]", torch.relu(y * sc + sh + res * rsc + rsh)), ("out[1]", y * sc + sh)):
                if bf:
                    _close_bf16(out[path], want)
                else:
                    _assert_rel(out[path].cpu(), want, 1e-5)
        return ref
    case("bn_act 2 x 5x7 x 64 with a residual", "bn_act", act_inputs(torch.float32),
         lambda y, sc, sh, res, rsc, rsh: (_ops().bn_act(y, sc, sh, res=res, rscale=rsc, rshift=rsh), _ops().bn_act(y, sc, sh, relu=False)),
         ref=act_ref(False))
    case("bn_act_bf16 2 x 5x7 x 64 with a residual", "bn_act_bf16", act_inputs(BF),
         lambda y, sc, sh, res, rsc, rsh: (_ops().bn_act_bf16(y, sc, sh, res=res, rscale=rsc, rshift=rsh),
                                           _ops().bn_act_bf16(y.float(), sc, sh, relu=False)), ref=act_ref(True))
    for H, W in ((21, 27), (20, 28), (1, 1)):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1

        def pool_inputs(dtype, H=H, W=W, Ho=Ho, Wo=Wo):
            return lambda: dict(x=torch.relu(R(g, 2, H, W, 64)).to(dtype), dout=R(g, 2, Ho, Wo, 64, dtype=dtype),
                                dx=R(g, 2, H, W, 64, dtype=dtype))

        def pool_call(fwd, bwd, H=H, W=W):
            def call(x, dout, dx):
                out, am = getattr(_ops(), fwd)(x)
                return out, am, getattr(_ops(), bwd)(dout, am, H, W), getattr(_ops(), bwd)(dout, am, H, W, dx=dx)
            return call
        def pool_ref(inp, out, H=H, W=W):
            """fp64 max-pool and its autograd (test_maxpool_forward_backward_with_ties: the forward exact, the backward 1e-6)"""
            import torch.nn.functional as F
            x = nchw64(inp["x"]).requires_grad_(True)
            want = F.max_pool2d(x, 3, 2, 1)
            want.backward(nchw64(inp["dout"]))
            assert torch.equal(nchw64(out["out[0]"]), want.detach().float().double())
            err = float((nchw64(out["out[2]"]) - x.grad).abs().max() / (x.grad.abs().max() + 1e-30))
            assert err < 1e-6, err
            assert torch.equal(out["out[3]"], out["out[2]"] + inp["dx"])          # dx given: accumulated into
        case(f"maxpool3x3s2 forward and backward {H}x{W}", ("maxpool3x3s2", "maxpool3x3s2_bwd"), pool_inputs(torch.float32),
             pool_call("maxpool3x3s2", "maxpool3x3s2_bwd"), ref=pool_ref)
        def pool_ref_bf16(inp, out):
            """test_maxpool_and_upsample_backward_bf16: the forward exact, the gradient (and the accumulated one) close_bf16"""
            import torch.nn.functional as F
            x = nchw64(inp["x"]).requires_grad_(True)
            want = F.max_pool2d(x, 3, 2, 1)
            want.backward(nchw64(inp["dout"]))
            assert torch.equal(nchw64(out["out[0]"]), want.detach())
            _close_bf16(nchw64(out["out[2]"]), x.grad)
            _close_bf16(nchw64(out["out[3]"]), x.grad + nchw64(inp["dx"]))
        case(f"maxpool3x3s2_bf16 forward and backward {H}x{W}", ("maxpool3x3s2_bf16", "maxpool3x3s2_bwd_bf16"), pool_inputs(BF),
             pool_call("maxpool3x3s2_bf16", "maxpool3x3s2_bwd_bf16"), ref=pool_ref_bf16)
    for H, W, Cc in ((9, 17, 64), (1, 1, 4)):
        case(f"upsample2x_bwd {H}x{W} x {Cc}", "upsample2x_bwd", lambda H=H, W=W, Cc=Cc: dict(dup=R(g, 2, 2 * H, 2 * W, Cc)),
             lambda dup: _ops().upsample2x_bwd(dup),
             ref=lambda inp, out: _assert_rel(nchw64(out["out"]), torch.nn.functional.avg_pool2d(nchw64(inp["dup"]), 2) * 4, 1e-6))
        case(f"upsample2x_bwd_bf16 {H}x{W} x {2 * Cc}", "upsample2x_bwd_bf16",
             lambda H=H, W=W, Cc=Cc: dict(dup=R(g, 2, 2 * H, 2 * W, 2 * Cc, dtype=BF)), lambda dup: _ops().upsample2x_bwd_bf16(dup),
             ref=lambda inp, out: _close_bf16(nchw64(out["out"]), torch.nn.functional.avg_pool2d(nchw64(inp["dup"]), 2) * 4))
    def up_bn_ref(inp, out):
        """test_kernels_gpu.py::_upsample_backward_with_fused_bn_reduction: dx bit-identical to the plain 2x2-sum kernel, the rows
        summed against the fp64 BatchNorm-backward reduction of (dx, y) with the virtual-activation mask, 3e-5 / 1e-4"""
        bf = inp["dup"].dtype == BF
        plain = _ops().upsample2x_bwd_bf16(inp["dup"]) if bf else _ops().upsample2x_bwd(inp["dup"])
        _assert_equal(out["out[0]"], plain)
        s0, s1, scale = bn_bwd_sums(out["out[0]"], inp["y"], inp["mean"], inp["invstd"], inp["sc"], inp["sh"], None, bf16=bf)
        red = out["out[1]"].double().cpu().sum(1)
        assert float((red[0] - s0).abs().max()) <= 3e-5 * scale and float((red[1] - s1).abs().max()) <= 1e-4 * scale

    for dtype, B, H, W, Cc in ((torch.float32, 1, 2, 2, 4), (torch.float32, 1, 2, 2, 1024), (BF, 1, 2, 2, 8), (BF, 1, 2, 2, 2048),
                               (torch.float32, 2, 9, 17, 64), (BF, 2, 9, 17, 64)):
        def make(dtype=dtype, B=B, H=H, W=W, Cc=Cc):
            mean, invstd, sc, sh = bn_coef(g, Cc)
            return dict(dup=R(g, B, 2 * H, 2 * W, Cc, dtype=dtype), y=R(g, B, H, W, Cc, dtype=dtype), mean=mean, invstd=invstd, sc=sc, sh=sh)
        case(f"upsample2x_bwd_bn {'bf16' if dtype == BF else 'fp32'} {B} x {H}x{W} x {Cc}", "upsample2x_bwd_bn", make,
             lambda dup, y, mean, invstd, sc, sh: _ops().upsample2x_bwd_bn(dup, y, mean, invstd, sc, sh), ref=up_bn_ref)
    case("nchw_to_nhwc / nhwc_to_nchw 2 x 5 x 7x13", ("nchw_to_nhwc", "nhwc_to_nchw"), lambda: dict(x=R(g, 2, 5, 7, 13)),
         lambda x: (_ops().nchw_to_nhwc(x), _ops().nhwc_to_nchw(x)),
         ref=lambda inp, out: _assert_equal(out["out[0]"], inp["x"].permute(0, 2, 3, 1).contiguous(), out["out[1]"],
                                            inp["x"].permute(0, 3, 1, 2).contiguous()))
    case("normalize_u8 2 x 7x13 x 4 -> 3", "normalize_u8", lambda: dict(x=U8(g, 2, 7, 13, 4)),
         lambda x: _ops().normalize_u8(x, MEAN4, STD4, 3),
         ref=lambda inp, out: np.testing.assert_array_equal(
             _np(out["out"]), np.stack([_augment_ref().train_transform(t, 0, 0, 1.0, 0.0, MEAN4, STD4, 3) for t in _np(inp["x"])])))


_elementwise()


# ------------------------------------------------------------------------------------------------ head
def _head():
    g = _family_gen()

    def make(B, H, W, K, dtype=torch.float32):
        def f():
            labels = torch.randint(0, K, (B, H, W), generator=g).to(DEV)
            return dict(x=R(g, B, H, W, 16, dtype=dtype), w=R(g, K, 3, 3, 16, scale=0.1), bias=R(g, K, scale=0.1), labels=labels,
                        lu=torch.randint(0, 2, (B, H, W), generator=g).to(DEV), dist=R(g, B, K, H, W), dl=R(g, B, K, H, W))
        return f
    def logits64(inp):
        import torch.nn.functional as F
        return F.conv2d(nchw64(inp["x"]), inp["w"].double().cpu().permute(0, 3, 1, 2), inp["bias"].double().cpu(), padding=1)

    def fwd_ref(inp, out):
        """fp64 head convolution at 2e-6 of the largest logit, the arg-max maps those of the logits
        (test_kernels_gpu.py::test_head_forward_backward)"""
        logits = out["out[0][0]"].cpu()
        _assert_rel(logits, logits64(inp), 2e-6)
        _assert_equal(out["out[0][1]"].cpu(), logits.argmax(dim=1), out["out[1][1]"].cpu().long(), logits.argmax(dim=1), out["out[2][0]"].cpu(), logits)

    def eval_ref(inp, out):
        """test_head_eval_gpu.py::test_fused_head_against_the_unfused_chain_and_fp64: the integers against the unfused chain
        (head_fwd, loss_sums, confusion_matrix; fp32 input), the real-valued slots 1-5 against fp64 at rel 1e-5 / abs 1e-6"""
        from deadtrees_amd.loss.seg_loss import loss_sums
        acc, counts, am = out["out[0]"].cpu(), out["out[1]"], out["out[2]"]
        labels, n, K = inp["labels"], inp["labels"].numel(), inp["w"].shape[0]
        assert int(out["out[3]"]) == 0 and int(counts[0].sum()) == n and int(counts[1].sum()) == int((inp["lu"] == 1).sum())
        assert float(acc[..., 0].sum()) == n and float(acc[..., 8:].abs().max()) == 0.0
        if inp["x"].dtype == torch.float32:
            logits, am_u = _ops().head_fwd(inp["x"], inp["w"], inp["bias"], argmax="int64")
            acc_u, _, _ = loss_sums(logits, labels, inp["dist"], 2.0)
            counts_u, _ = _ops().confusion_matrix(am_u, labels, inp["lu"], K=K)
            _assert_equal(am.long(), am_u, counts, counts_u)
            for j in (0, 6, 7):
                _assert_equal(acc[..., j], acc_u.cpu()[..., j])
        p = logits64(inp).softmax(1)
        t = torch.stack([(labels.cpu() == k) for k in range(K)], 1).double()
        lp = torch.log(p + 1e-10)
        terms = [p * t, p, (1 - p) ** 2.0 * t * lp, t * lp, p * inp["dist"].double().cpu()]
        want = torch.stack([v.sum(dim=(2, 3)) for v in terms], -1)
        np.testing.assert_allclose(acc[..., 1:6].numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    # 3 x 21x17, K = 3 and 2 x 40x70, K = 2 in bf16: the "partial" and "bf16" shapes of test_head_eval_gpu.py
    for B, H, W, K in ((3, 21, 17, 3), (2, 40, 70, 2), (1, 1, 1, 3)):
        case(f"head_fwd {B} x {H}x{W}, K = {K}", "head_fwd", make(B, H, W, K),
             lambda x, w, bias, labels, lu, dist, dl: (_ops().head_fwd(x, w, bias, argmax="int64"), _ops().head_fwd(x, w, bias, argmax="uint8"),
                                                       _ops().head_fwd(x, w, bias)), ref=fwd_ref)
        for dtype in (torch.float32, BF):
            case(f"head_eval {'bf16' if dtype == BF else 'fp32'} {B} x {H}x{W}, K = {K}", "head_eval", make(B, H, W, K, dtype),
                 lambda x, w, bias, labels, lu, dist, dl: _ops().head_eval(x, w, bias, labels, lu=lu, dist=dist, want_argmax=True),
                 ref=eval_ref)

    def bwd_shape(two_stage):
        lib = _lib()
        W = 1024              # rows grow with the map: the last height with at most 256 rows, or the first with more
        H = next(h for h in range(8, 4096, 8) if lib.dt_head_bwd_rows(1, h + 8, W) > 256) + (8 if two_stage else 0)
        P = lib.dt_head_bwd_rows(1, H, W)
        assert (P > 256) == two_stage and 200 < P < 320, (H, P)           # dt_head_bwd_finalize: two stages above 256 rows
        return H, W, P

    def bwd(two_stage):
        def f():
            H, W, P = bwd_shape(two_stage)
            return dict(make(1, H, W, 2)(), P=P)
        return f
    FORMS.extend((f"head_bwd {'two' if t else 'single'}-stage", lambda t=t: bwd_shape(t)) for t in (False, True))
    def bwd_ref(inp, out):
        """fp64 autograd of the 3x3 head convolution, the bounds of test_kernels_gpu.py::test_head_forward_backward"""
        import torch.nn.functional as F
        x = nchw64(inp["x"]).requires_grad_(True)
        w = inp["w"].double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        b = inp["bias"].double().cpu().requires_grad_(True)
        F.conv2d(x, w, b, padding=1).backward(inp["dl"].double().cpu())
        rel = lambda a, r: float((a.double().cpu() - r).abs().max() / (r.abs().max() + 1e-30))       # noqa: E731
        assert rel(nchw64(out["out[0]"]), x.grad) < 2e-6, rel(nchw64(out["out[0]"]), x.grad)
        assert rel(out["out[1]"].permute(0, 3, 1, 2), w.grad) < 1e-5, rel(out["out[1]"].permute(0, 3, 1, 2), w.grad)
        assert rel(out["out[2]"], b.grad) < 1e-5, rel(out["out[2]"], b.grad)
    for two_stage in (False, True):
        case(f"head_bwd {'two-stage' if two_stage else 'single-stage'} reduction", "head_bwd", bwd(two_stage),
             lambda x, w, bias, labels, lu, dist, dl, P: _ops().head_bwd(x, w, dl), ref=bwd_ref)
    case("head_bwd 2 x 15x16, K = 3", "head_bwd", make(2, 15, 16, 3), lambda x, w, bias, labels, lu, dist, dl: _ops().head_bwd(x, w, dl),
         ref=bwd_ref)

    def with_counts():
        d = make(2, 15, 16, 2)()
        d.update(counts=torch.arange(8, dtype=torch.int64).view(2, 2, 2).to(DEV) + 5, err=torch.zeros(1, dtype=torch.int32, device=DEV))
        d["labels"][0, 0, 0] = 7              # a label outside [0, K): the flag the caller brought is set, never cleared
        return d

    def counts_ref(inp, out):
        """the caller's counts are added to (5 .. 12 were there), its err flag is set"""
        fresh = _ops().head_eval(inp["x"], inp["w"], inp["bias"], inp["labels"], lu=inp["lu"], dist=inp["dist"])
        assert torch.equal(out["out[1]"], fresh[1] + inp["counts"]) and int(fresh[1].sum()) > 0
        assert int(out["out[3]"]) != 0 and int(fresh[3]) == int(out["out[3]"])
    case("head_eval 2 x 15x16, K = 2, counts= and err= given", "head_eval", with_counts,
         lambda x, w, bias, labels, lu, dist, dl, counts, err: _ops().head_eval(x, w, bias, labels, lu=lu, dist=dist, counts=counts, err=err),
         ref=counts_ref)


_head()


# ------------------------------------------------------------------------------------------------ inverted-residual block
def _mbconv():
    g = _family_gen()

    def pw(C0, C1, N, up):
        B, H, W = 2, 5, 7

        def make():
            return dict(src0=R(g, B, (H + 1) // 2, (W + 1) // 2, C0) if up else R(g, B, H, W, C0), src1=R(g, B, H, W, C1) if C1 else None,
                        w=R(g, C0 + C1, N, scale=(2.0 / (C0 + C1)) ** 0.5), sc=R(g, N, scale=0.2, shift=1.0), sh=R(g, N),
                        gc=torch.sigmoid(R(g, B, C0 + C1)), gs=R(g, B, H, W, scale=2.0), res=R(g, B, H, W, N))
        def ref(inp, out):
            """test_mbconv_kernels_gpu.py::test_pwconv_affine_against_float64: fp64 with its bound 1.5 (K + 8) 2^-24 of the
            magnitude sum per element"""
            a = inp["src0"].double().cpu()
            if up:
                a = a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]
            if inp["src1"] is not None:
                a = torch.cat([a, inp["src1"].double().cpu()], dim=-1)
            a = a * (inp["gc"].double().cpu()[:, None, None, :] + torch.sigmoid(inp["gs"].double().cpu())[..., None])
            w, sc, sh, res = (inp[k].double().cpu() for k in ("w", "sc", "sh", "res"))
            t = (a @ w) * sc + sh
            want = t * (t + 3).clamp(0, 6) / 6 + res
            mag = (a.abs() @ w.abs()) * sc.abs() + sh.abs() + res.abs()
            ratio = float(((out["out"].double().cpu() - want).abs() / (1.5 * (C0 + C1 + 8) * 2.0 ** -24 * mag)).max())
            assert ratio <= 1.0, ratio
        case(f"pwconv_affine {C0}+{C1} -> {N}{' up-sampled' if up else ''}, gate, act, res", "pwconv_affine", make,
             lambda src0, src1, w, sc, sh, gc, gs, res: _ops().pwconv_affine(src0, w, sc, sh, src1=src1, up0=up, gate=(gc, gs), act=True,
                                                                             res=res, hw=(H, W) if up else None), ref=ref)
    pw(16, 0, 16, False)
    pw(32, 16, 16, True)
    pw(32, 0, 272, False)
    # the three shapes of DW_SHAPES in tests/test_mbconv_kernels_gpu.py (its fp64 reference pins b, s and the pool rows)
    for B, H, W, Cc in ((2, 5, 7, 16), (1, 1, 1, 48), (2, 9, 33, 768)):
        def make(B=B, H=H, W=W, Cc=Cc):
            Ch = max(Cc // 4, 4)
            return dict(x=R(g, B, H, W, Cc), w=R(g, 9, Cc, scale=0.47), sc=R(g, Cc, scale=0.2, shift=1.0), sh=R(g, Cc),
                        ws=R(g, Cc, scale=Cc ** -0.5), bs=R(g, 1), w1=R(g, Cc, Ch, scale=0.3), b1=R(g, Ch, scale=0.1),
                        w2=R(g, Ch, Cc, scale=0.3), b2=R(g, Cc, scale=0.1))

        def call(x, w, sc, sh, ws, bs, w1, b1, w2, b2):
            B, H, W, Cc = x.shape
            b, s, pool = _ops().dwconv3x3_affine(x, w, sc, sh, ws, bs)
            rows = _ops().pool_rows(pool, B, Cc).clone()
            gates = _ops().scse_gates(pool, B, Cc, H * W, w1, b1, w2, b2)       # fills the front of `pool`: now all of it is defined
            return b, s, rows, gates, pool
        case(f"dwconv3x3_affine + scse_gates {B} x {H}x{W} x {Cc}", "dwconv3x3_affine", make, call)
    def affine_ref(inp, out):
        """no test of its own: scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale in fp64.  The kernel does a
        sqrt, a division, a subtraction and a multiply-add in fp32: under 8 roundings of 2^-24, so 2e-6 relative and absolute"""
        gamma, beta, rm, rv, bias = (inp[k].double().cpu() for k in ("gamma", "beta", "rm", "rv", "bias"))
        scale = gamma / torch.sqrt(rv + 1e-5)
        np.testing.assert_allclose(out["out[0]"].double().cpu(), scale, rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(out["out[1]"].double().cpu(), beta + (bias - rm) * scale, rtol=2e-6, atol=2e-6)
    case("bn_eval_affine_bias 48 channels", "bn_eval_affine_bias",
         lambda: dict(gamma=R(g, 48, shift=1.0, scale=0.2), beta=R(g, 48), rm=R(g, 48), rv=R(g, 48, scale=0.1, shift=1.0).abs(), bias=R(g, 48)),
         lambda gamma, beta, rm, rv, bias: _ops().bn_eval_affine_bias(gamma, beta, rm, rv, bias), ref=affine_ref)


_mbconv()


# ------------------------------------------------------------------------------------------------ data: normalise, augment, pool
def _data():
    g = _family_gen()
    def window_ref(d, stride, first, views=None):
        def ref(inp, out):
            """every window is the [i*s : i*s+d, j*s : j*s+d] slice of the zero-padded raster through val_transform, bit for
            bit (test_split_normalize_gather_matches_tiler_blocks_and_val_transform and the window gather test); a view is
            rot90^rot(flip(window)) of oracle/augment_ref.py"""
            from deadtrees_amd.data.deadtreedata import val_transform
            raster = _np(inp["r"])
            _, h, w = raster.shape
            ny, nx = (-(-h // d), -(-w // d)) if stride == d else _ops()._stitch_grid(h, w, d, d - stride, "case")
            padded = np.zeros((4, (ny - 1) * stride + d, (nx - 1) * stride + d), np.uint8)
            padded[:, :h, :w] = raster
            got = _np(out["out"])
            T = len(views) if views else 1
            assert got.shape[0] % T == 0 and got.shape[0] // T <= ny * nx - first
            for k in range(got.shape[0] // T):
                i, j = divmod(first + k, nx)
                win = padded[:, i * stride:i * stride + d, j * stride:j * stride + d].transpose(1, 2, 0)
                want = val_transform(image=win)["image"][:got.shape[-1]].permute(1, 2, 0).numpy()
                for v, (flip, rot) in enumerate(views or ((0, 0),)):
                    np.testing.assert_array_equal(got[k * T + v], _augment_ref().geometric(want, flip, rot), err_msg=f"window {k} view {v}")
        return ref
    case("split_normalize_u8 4 x 70x149, 32-pixel blocks 1..14", "split_normalize_u8", lambda: dict(r=U8(g, 4, 70, 149)),
         lambda r: _ops().split_normalize_u8(r, 32, 1, 14, MEAN4, STD4, 3), ref=window_ref(32, 32, 1))

    def windows(views):
        def call(r):
            ny, nx = _ops()._stitch_grid(70, 149, 32, 8, "case")
            return _ops().window_normalize_u8(r, 32, 8, 1, ny * nx - 1, MEAN4, STD4, 3, views=views)
        return call
    case("window_normalize_u8 4 x 70x149, overlap 8", "window_normalize_u8", lambda: dict(r=U8(g, 4, 70, 149)), windows(None),
         ref=window_ref(32, 24, 1))
    case("window_normalize_u8 4 x 70x149, overlap 8, three views", "window_normalize_u8", lambda: dict(r=U8(g, 4, 70, 149)),
         windows(((0, 0), (1, 1), (0, 3))), ref=window_ref(32, 24, 1, ((0, 0), (1, 1), (0, 3))))
    case("window_normalize_u8 one-pixel raster", "window_normalize_u8", lambda: dict(r=U8(g, 4, 1, 1)),
         lambda r: _ops().window_normalize_u8(r, 32, 8, 0, 1, MEAN4, STD4, 4), ref=window_ref(32, 24, 0))
    def finalize_ref(inp, out):
        """test_finalize_probabilities_and_ties: the probabilities sum to one within 1e-6, the map does not depend on the probs
        pointer; the map is the arg-max of the accumulator and the probabilities its normalisation (one division: 1e-6)"""
        acc = inp["acc"]
        first = "out[0][0]" if "out[0][0]" in out else "out[0]"
        classes, probs = out[first], out["out[0][1]" if first == "out[0][0]" else "out[1]"]
        assert float((probs.sum(dim=0) - 1.0).abs().max()) <= 1e-6
        _assert_equal(classes.long(), acc.argmax(dim=0))
        if first == "out[0][0]":
            _assert_equal(out["out[1]"], classes)
        assert float((probs - acc / acc.sum(dim=0)).abs().max()) <= 1e-6
    case("stitch_finalize 3 x 70x149 with probabilities", "stitch_finalize", lambda: dict(acc=R(g, 3, 70, 149).abs() + 0.01),
         lambda acc: (_ops().stitch_finalize(acc, want_probs=True), _ops().stitch_finalize(acc)), ref=finalize_ref)
    case("stitch_finalize one pixel", "stitch_finalize", lambda: dict(acc=R(g, 2, 1, 1).abs() + 0.01),
         lambda acc: _ops().stitch_finalize(acc, want_probs=True), ref=finalize_ref)

    def augment_ref(inp, out):
        """oracle/augment_ref.py as test_device_train_transform_matches_numpy_restatement holds it: labels exact; the image
        within one grey level where a LUT entry lands on an integer, on fewer than 1 % of the pixels"""
        A = _augment_ref()
        x, labels, geo, bc = (_np(inp[k]) for k in ("x", "labels", "geo", "bc"))
        got, gm = _np(out["out[0]"]), _np(out["out[1]"])
        for b in range(x.shape[0]):
            f, r = int(geo[b, 0]), int(geo[b, 1])
            want = A.train_transform(x[b], f, r, float(bc[b, 0]), float(bc[b, 1]), MEAN4, STD4, 3)
            diff = np.abs(got[b] - want) * (np.asarray(STD4[:3], np.float32) * 255.0)
            assert float(diff.max()) <= 1.0 + 1e-3 and (diff.size < 100 or float((diff > 1e-3).mean()) < 1e-2), (b, float(diff.max()))
            np.testing.assert_array_equal(gm[b], A.geometric(labels[b], f, r))

    def aug(B, H, W):
        def make():
            rot = torch.randint(0, 4, (B,), generator=g) * (1 if H == W else 2) % 4
            geo = torch.stack((torch.randint(0, 2, (B,), generator=g), rot), 1).to(torch.int32).to(DEV)
            bc = torch.stack((0.8 + 0.4 * torch.rand(B, generator=g), 20 * torch.rand(B, generator=g) - 10), 1).float().to(DEV)
            return dict(x=U8(g, B, H, W, 4), labels=torch.randint(0, 3, (B, H, W), generator=g).to(DEV), geo=geo, bc=bc)
        case(f"augment_normalize_u8 / augment_labels {B} x {H}x{W}", ("augment_normalize_u8", "augment_labels"), make,
             lambda x, labels, geo, bc: (_ops().augment_normalize_u8(x, geo, bc, MEAN4, STD4, 3), _ops().augment_labels(labels, geo)),
             ref=augment_ref)
    aug(5, 13, 13)
    aug(3, 7, 19)
    aug(1, 1, 1)

    def pool(n_sources, with_lu, given_out):
        B, H, W, N = 5, 13, 13, 6

        def make():
            d = {}
            for j in range(n_sources):
                img = U8(g, N, H, W, 4)
                d[f"img{j}"], d[f"mask{j}"] = img, U8(g, N, H, W, high=3)
                d[f"lu{j}"] = U8(g, N, H, W, high=2) if with_lu else None
                d[f"sums{j}"] = img.to(torch.int64).sum(dim=(1, 2, 3))
            idx = torch.randint(0, N, (B,), generator=g).to(torch.int32)
            idx[2] = N + 3                                              # a bad index: the slot is zeroed, a bit of err is set
            d.update(src=torch.randint(0, n_sources, (B,), generator=g).to(torch.int32).to(DEV), idx=idx.to(DEV),
                     geo=torch.stack((torch.randint(0, 2, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)), 1).to(torch.int32).to(DEV),
                     bc=torch.stack((0.8 + 0.4 * torch.rand(B, generator=g), 20 * torch.rand(B, generator=g) - 10), 1).float().to(DEV))
            if given_out:
                d.update(o_img=R(g, B, 3, H, W), o_mask=torch.randint(0, 3, (B, H, W), generator=g).to(DEV),
                         o_lu=torch.randint(0, 2, (B, H, W), generator=g).to(DEV) if with_lu else None)
            return d

        def call(src, idx, geo, bc, o_img=None, o_mask=None, o_lu=None, **pools):
            sources = [(pools[f"img{j}"], pools[f"mask{j}"], pools[f"lu{j}"], pools[f"sums{j}"]) for j in range(n_sources)]
            out = (o_img, o_mask, o_lu) if given_out else None
            if n_sources == 1:
                return _ops().pool_gather_batch(*sources[0], idx, geo, bc, MEAN4, STD4, 3, merge_above=True, out=out)
            return _ops().pool_gather_combined(sources, src, idx, geo, bc, MEAN4, STD4, 3, out=out)
        def ref(inp, out):
            """tests/test_pool_gpu.py: every slot bit-identical to augment_normalize_u8 / augment_labels on its sample (labels
            above 1 merged by pool_gather_batch's merge_above); the slot with the bad index is zeros and sets err"""
            ops = _ops()
            merge = n_sources == 1
            assert int(out["out[3]"]) != 0
            for b in range(B):
                j, i = (int(inp["src"][b]) if n_sources > 1 else 0), int(inp["idx"][b])
                geo, bc = inp["geo"][b:b + 1], inp["bc"][b:b + 1]
                if i >= N:
                    assert b == 2 and all(int(out[k][b].abs().sum()) == 0 for k in ("out[0]", "out[1]") + (("out[2]",) if with_lu else ()))
                    continue
                want = ops.augment_normalize_u8(inp[f"img{j}"][i:i + 1], geo, bc, MEAN4, STD4, 3).permute(0, 3, 1, 2)
                m = inp[f"mask{j}"][i:i + 1].long()
                m = torch.where(m > 1, torch.ones_like(m), m) if merge else m
                _assert_equal(out["out[0]"][b:b + 1], want, out["out[1]"][b:b + 1], ops.augment_labels(m, geo))
                if with_lu:
                    _assert_equal(out["out[2]"][b:b + 1], ops.augment_labels(inp[f"lu{j}"][i:i + 1].long(), geo))
        name = "pool_gather_batch" if n_sources == 1 else "pool_gather_combined"
        case(f"{name} {n_sources} source(s){', lu' if with_lu else ''}{', out given' if given_out else ''}", name, make, call, ref=ref)
    pool(1, True, False)
    pool(1, False, True)
    pool(3, True, False)
    pool(2, False, True)
    case("ensemble_vote 5 maps of 70x150", "ensemble_vote", lambda: dict(m=U8(g, 5, 70, 150, high=3)),      # n % 4 == 0 is the ABI's
         lambda m: (_ops().ensemble_vote(m, 3), _ops().ensemble_vote(m, 3, dtype="uint8")),
         ref=lambda inp, out: _assert_equal(out["out[0][0]"].cpu(), torch.mode(inp["m"].cpu().long(), dim=0).values,
                                            out["out[1][0]"].cpu().long(), torch.mode(inp["m"].cpu().long(), dim=0).values))
    case("ensemble_vote one row of four pixels", "ensemble_vote", lambda: dict(m=U8(g, 3, 1, 4, high=3)), lambda m: _ops().ensemble_vote(m, 3),
         ref=lambda inp, out: _assert_equal(out["out[0]"].cpu(), torch.mode(inp["m"].cpu().long(), dim=0).values))

    def cut_inputs(h, w):
        def make():
            slot = torch.tensor([2, -1, 0, 3], dtype=torch.int32)        # row 1 of the pool is named by no entry: untouched
            return dict(rgbn=U8(g, 4, h, w), mask=U8(g, h, w, high=3), lu=U8(g, h, w, high=2), slot=slot.to(DEV),
                        images=U8(g, 4, 32, 32, 4), masks=U8(g, 4, 32, 32, high=3), lus=U8(g, 4, 32, 32, high=2),
                        sums=torch.randint(0, 9, (4,), generator=g).to(DEV))
        return make

    def cut_call(rgbn, mask, lu, slot, images, masks, lus, sums):
        census = _ops().raster_cut(rgbn, mask, lu, source_dim=64, tile_size=32, slot=slot, out=(images, masks, lus, sums))
        return census, images, masks, lus, sums, _ops().raster_cut(rgbn, None, None, source_dim=64, tile_size=32)
    def cut_ref(inp, out):
        """data.rasters.cut_raster_host, exact (tests/test_rasters_gpu.py): the census, the rows a slot names, and the row no
        slot names as it was; without mask and land-use map the host's defaults"""
        from deadtrees_amd.data.rasters import cut_raster_host
        want = cut_raster_host(_np(inp["rgbn"]), _np(inp["mask"]), _np(inp["lu"]), 64, 32)
        np.testing.assert_array_equal(_np(out["out[0]"]), want[4])
        named = set()
        for i, r in enumerate(inp["slot"].tolist()):
            if r < 0:
                continue
            named.add(r)
            for path, k in (("out[1]", 0), ("out[2]", 1), ("out[3]", 2)):
                np.testing.assert_array_equal(_np(out[path][r]), want[k][i])
            assert int(out["out[4]"][r]) == int(want[3][i])
        assert named == {0, 2, 3}
        for path, key in (("out[1]", "images"), ("out[2]", "masks"), ("out[3]", "lus"), ("out[4]", "sums")):
            _assert_equal(out[path][1], inp[key][1])
        np.testing.assert_array_equal(_np(out["out[5]"]), cut_raster_host(_np(inp["rgbn"]), None, None, 64, 32)[4])
    case("raster_cut 4 x 50x61 into a 64-pixel source, 32-pixel tiles", "raster_cut", cut_inputs(50, 61), cut_call, ref=cut_ref)
    case("raster_cut one-pixel raster", "raster_cut", cut_inputs(1, 1), cut_call, ref=cut_ref)


_data()


# ------------------------------------------------------------------------------------------------ maps: polygons, patches, ...
def _maps():
    def polygons(name, h, w):
        def make():
            from polygon_fixtures import fixture
            edges, polys = fixture(name, h, w).tables()
            return dict(edges=torch.from_numpy(np.array(edges)).to(DEV), polys=torch.from_numpy(np.array(polys)).to(DEV))
        def ref(inp, out):
            """data.polygons.rasterize_host, exact in both modes (tests/test_polygons_gpu.py::test_device_equals_host)"""
            from deadtrees_amd.data.polygons import rasterize_host
            from polygon_fixtures import fixture
            for path, mode in (("out[0]", True), ("out[1]", False)):
                np.testing.assert_array_equal(_np(out[path]), rasterize_host(fixture(name, h, w), h, w, mode))
        case(f"rasterize_polygons {name} on {h}x{w}", "rasterize_polygons", make,
             lambda edges, polys: (_ops().rasterize_polygons(edges, polys, (h, w)), _ops().rasterize_polygons(edges, polys, (h, w), all_touched=False)),
             ref=ref)
    polygons("stars", 70, 149)
    polygons("stars", 1, 1)

    for h, w in ((70, 149), (1, 67), (1, 1)):
        def make(h=h, w=w):
            cls = class_map(h + w, h, w)
            if h * w == 1:
                cls.fill_(1)
            g = _gen(h * w)
            return dict(cls=cls, other=class_map(h + w + 1, h, w, cell=(4, 9)) if h * w > 1 else cls.clone(), raster=U8(g, 4, h, w),
                        probs=torch.softmax(R(g, 3, h, w), 0).contiguous())

        def labelled(cls, other):
            ops = _ops()
            la, err = ops.label_patches(cls, 3, 8)
            lb, _ = ops.label_patches(other, 3, 4)
            return la, lb, err

        def patches(cls, other, raster, probs):
            ops = _ops()
            la, lb, err = labelled(cls, other)
            area = ops.patch_areas(la)
            return la, lb, err, area, ops.patch_table(la, cls), ops.patch_table(la, cls, area_plane=area.clone())
        def host_labels(inp):
            from deadtrees_amd.deployment.patches import label_patches_host
            return label_patches_host(_np(inp["cls"]), 3, 8), label_patches_host(_np(inp["other"]), 3, 4)

        def same_host(out, prefix, want):
            """every array of a host result against the device result under the same path"""
            import poison
            for path, t in poison.flatten(want, prefix):
                if not path.split(".")[-1].startswith("_t"):              # (a lazily built cache of the host object)
                    np.testing.assert_array_equal(_np(out[path]), _np(t), err_msg=path)

        def patches_ref(inp, out):
            """deployment.patches.label_patches_host / measure_patches_host, exact (tests/test_patches_gpu.py)"""
            from deadtrees_amd.deployment.patches import measure_patches_host
            la, lb = host_labels(inp)
            np.testing.assert_array_equal(_np(out["out[0]"]), la)
            np.testing.assert_array_equal(_np(out["out[1]"]), lb)
            assert int(out["out[2]"]) == 0
            np.testing.assert_array_equal(_np(out["out[3]"]), np.bincount(la[la > 0] - 1, minlength=la.size)[:la.size])
            for k in (4, 5):
                same_host(out, f"out[{k}]", measure_patches_host(la, _np(inp["cls"])))
        case(f"label_patches / patch_table {h}x{w}", ("label_patches", "patch_table"), make, patches, ref=patches_ref)

        def outlines(cls, other, raster, probs):
            la, lb, _ = labelled(cls, other)
            return _ops().patch_outlines(la, cls, 8), _ops().patch_outlines(lb, other, 4)
        def outlines_ref(inp, out):
            """deployment.outlines.polygonize_host, exact (tests/test_outlines_gpu.py)"""
            from deadtrees_amd.deployment.outlines import polygonize_host
            la, lb = host_labels(inp)
            same_host(out, "out[0]", polygonize_host(_np(inp["cls"]), 3, 8, labels=la))
            same_host(out, "out[1]", polygonize_host(_np(inp["other"]), 3, 4, labels=lb))
        case(f"patch_outlines {h}x{w}", "patch_outlines", make, outlines, ref=outlines_ref)

        def overlaps(cls, other, raster, probs):
            la, lb, _ = labelled(cls, other)
            return _ops().patch_overlaps(la, lb), _ops().patch_overlaps(la, torch.zeros_like(la))
        def overlaps_ref(inp, out):
            """deployment.overlaps.overlap_pairs_host, exact (tests/test_overlaps_gpu.py)"""
            from deadtrees_amd.deployment.overlaps import overlap_pairs_host
            la, lb = host_labels(inp)
            same_host(out, "out[0]", tuple(overlap_pairs_host(la, lb)))
            assert all(out[f"out[1][{i}]"].numel() == 0 for i in range(3))
        case(f"patch_overlaps {h}x{w}", "patch_overlaps", make, overlaps, ref=overlaps_ref)

        def proximity(cls, other, raster, probs):
            ops = _ops()
            la, lb, _ = labelled(cls, other)
            roots = torch.nonzero(ops.patch_areas(lb)).view(-1)
            own = torch.nonzero(ops.patch_areas(la)).view(-1)
            dist, nearest, flag = ops.proximity_tables(la, second=True)
            return (ops.patch_proximity(la, lb, roots), ops.patch_proximity(la, la, own, exclude_own=True, limit2=400), dist, nearest, flag,
                    ops.proximity_tables(la))
        def proximity_ref(inp, out):
            """deployment.proximity.patch_proximity_host, exact (tests/test_proximity_gpu.py)"""
            from deadtrees_amd.deployment.proximity import patch_proximity_host
            la, lb = host_labels(inp)
            roots = lambda l: np.unique(l[l > 0] - 1).astype(np.int64)      # noqa: E731
            same_host(out, "out[0]", tuple(patch_proximity_host(la, lb, roots(lb))))
            same_host(out, "out[1]", tuple(patch_proximity_host(la, la, roots(la), exclude_own=True, limit2=400)))
        case(f"proximity_tables / patch_proximity {h}x{w}", "proximity_tables", make, proximity, ref=proximity_ref)

        def attributes(cls, other, raster, probs):
            ops = _ops()
            la, _, _ = labelled(cls, other)
            roots = torch.nonzero(ops.patch_areas(la)).view(-1)
            return (ops.patch_attributes(la, roots, raster, cls, probs, indices=((3, 0), (1, 2))), ops.patch_attributes(la, roots, raster[:1]))
        def attributes_ref(inp, out):
            """deployment.attributes.attribute_tables_host, exact (tests/test_attributes_gpu.py)"""
            from deadtrees_amd.deployment.attributes import attribute_tables_host
            la, _ = host_labels(inp)
            roots = np.unique(la[la > 0] - 1).astype(np.int64)
            raster = _np(inp["raster"])
            same_host(out, "out[0]", tuple(attribute_tables_host(la, roots, raster, _np(inp["cls"]), _np(inp["probs"]), ((3, 0), (1, 2)))))
            same_host(out, "out[1]", tuple(attribute_tables_host(la, roots, raster[:1])))
        case(f"patch_attributes {h}x{w}", "patch_attributes", make, attributes, ref=attributes_ref)

        def crowns(cls, other, raster, probs):
            from deadtrees_amd.deployment.crowns import CrownConfig
            ops = _ops()
            la, _, _ = labelled(cls, other)
            return (ops.patch_depth2(cls, 3), ops.patch_depth2(cls, 3, cap2=100, core2=4),
                    ops.split_patches(cls, la, 3, 8, CrownConfig(min_core2=4, max_rounds=64)))
        def crowns_ref(inp, out):
            """deployment.crowns.depth2_host / split_patches_host / crown_depths_host, exact (tests/test_crowns_gpu.py)"""
            from deadtrees_amd.deployment.crowns import CrownConfig, crown_depths_host, depth2_host, split_patches_host
            la, _ = host_labels(inp)
            cls = _np(inp["cls"])
            np.testing.assert_array_equal(_np(out["out[0][0]"]), depth2_host(cls, 3))
            np.testing.assert_array_equal(_np(out["out[1][0]"]), depth2_host(cls, 3, 100))
            want = split_patches_host(cls, la, 3, 8, CrownConfig(min_core2=4, max_rounds=64))
            want = want[0] if isinstance(want, tuple) else want
            np.testing.assert_array_equal(_np(out["out[2][0]"]), want)
            np.testing.assert_array_equal(_np(out["out[2][1]"]), depth2_host(cls, 3))
            np.testing.assert_array_equal(_np(out["out[2][2]"]).reshape(-1), np.asarray(crown_depths_host(want, depth2_host(cls, 3))).reshape(-1))
        case(f"patch_depth2 / split_patches {h}x{w}", ("patch_depth2", "split_patches"), make, crowns, ref=crowns_ref)

    def distmap_ref(inp, out):
        """oracle/losses_ref.py::dist_map per image, exact (tests/test_distmap_gpu.py::test_distmap_matches_scipy_oracle)"""
        from oracle.losses_ref import dist_map
        m, got = _np(inp["labels"]), _np(out["out[0]"])
        K = got.shape[1]
        for i in range(m.shape[0]):
            oh = (m[i][None] == np.arange(K)[:, None, None]).astype(np.int32)
            np.testing.assert_array_equal(got[i], dist_map(oh).astype(np.float32))
        assert int(out["out[1]"]) == 0
    for B, K, H, W in ((1, 3, 37, 301), (2, 2, 1, 70)):           # two shapes of test_distmap_matches_scipy_oracle
        case(f"signed_distmap {B} x {K} x {H}x{W}", "signed_distmap",
             lambda B=B, K=K, H=H, W=W: dict(labels=class_map(H, B * H, W, K).view(B, H, W).long()),
             lambda labels, K=K: _ops().signed_distmap(labels, K), wide_u8=("signed_distmap",), ref=distmap_ref)


_maps()


# ------------------------------------------------------------------------------------------------ curves, decisions, objects
def _curves():
    def make(B, K, H, W):
        def f():
            g = _gen(B + K + H + W)
            return dict(src=torch.softmax(R(g, B, K, H, W, scale=2.0), 1).contiguous(), labels=torch.randint(0, K, (B, H, W), generator=g).to(DEV),
                        lu=torch.randint(0, 2, (B, H, W), generator=g).to(DEV))
        return f
    def hist_ref(inp, out):
        """loss.curves.prob_histogram_host and quantise, exact (tests/test_curves_gpu.py::test_probability_histogram_equals_the_host)"""
        from deadtrees_amd.loss.curves import prob_histogram_host, quantise
        p, labels, lu = (_np(inp[k]) for k in ("src", "labels", "lu"))
        want, want_err = prob_histogram_host(p, labels, lu)
        np.testing.assert_array_equal(_np(out["out[0][0]"]), want)
        assert int(out["out[0][1]"]) == want_err == 0
        np.testing.assert_array_equal(_np(out["out[0][2]"]).astype(np.int64), quantise(p))
        assert int(out["out[1][0]"][1].sum()) == 0 and int(out["out[1][0]"][0].sum()) == int(out["out[0][0]"][0].sum())
    for B, K, H, W in ((2, 3, 37, 61), (1, 2, 1, 1)):
        case(f"prob_histogram {B} x {K} x {H}x{W} with the quantised probabilities", "prob_histogram", make(B, K, H, W),
             lambda src, labels, lu: (_ops().prob_histogram(src, labels, lu, want_q=True), _ops().prob_histogram(src.log(), labels, logits=True)),
             ref=hist_ref)

    def field(K, h, w):
        import hysteresis_cases as hc
        return lambda: dict(p=torch.from_numpy(np.array(hc.field(K, h, w))).to(DEV))

    def decide(p):
        import hysteresis_cases as hc
        K = p.shape[0]
        return (_ops().decide_classes(p, hc.decision(K, 8, False)), _ops().decide_patchwise(p, hc.decision(K, 8, True), return_support=True),
                _ops().decide_patchwise(p, hc.decision(K, 4, False)))
    def decide_ref(inp, out):
        """loss.curves.decide_host / decide_patchwise_host, exact (tests/test_curves_gpu.py, tests/test_hysteresis_gpu.py)"""
        import hysteresis_cases as hc
        from deadtrees_amd.loss.curves import decide_host, decide_patchwise_host
        p = _np(inp["p"])
        K = p.shape[0]
        np.testing.assert_array_equal(_np(out["out[0]"]), decide_host(p, hc.decision(K, 8, False)))
        np.testing.assert_array_equal(_np(out["out[1][0]"]), decide_patchwise_host(p, hc.decision(K, 8, True)))
        np.testing.assert_array_equal(_np(out["out[2]"]), decide_patchwise_host(p, hc.decision(K, 4, False)))
    case("decide_classes / decide_patchwise 3 x 64x200", ("decide_classes", "decide_patchwise"), field(3, 64, 200), decide, ref=decide_ref)
    case("decide_classes / decide_patchwise 2 x 1x1", ("decide_classes", "decide_patchwise"), field(2, 1, 1), decide, ref=decide_ref)

    def objects(B, K, H, W):
        def make():
            import objects_cases as oc
            q, target = oc.blobs(B + K, B, K, H, W)
            return dict(q=torch.from_numpy(q).to(DEV), target=torch.from_numpy(target).to(DEV))

        def call(q, target):
            import objects_cases as oc
            from deadtrees_amd.loss.objects import ObjectSweep
            return _ops().object_histogram(q, target, ObjectSweep(oc.low_for(K), connectivity=8, min_pixels=2))
        def ref(inp, out):
            """loss.objects.object_histogram_host, exact (tests/test_objects_gpu.py::test_device_equals_the_host)"""
            import objects_cases as oc
            from deadtrees_amd.loss.objects import ObjectSweep, object_histogram_host
            want = object_histogram_host(_np(inp["q"]), _np(inp["target"]), ObjectSweep(oc.low_for(K), connectivity=8, min_pixels=2))
            np.testing.assert_array_equal(_np(out["out[0]"]), want[0])
            np.testing.assert_array_equal(_np(out["out[1]"]), want[1])
            assert int(out["out[2]"]) == want[2]
            assert H * W == 1 or int(want[0].sum()) > 0
        case(f"object_histogram {B} x {K} x {H}x{W}", "object_histogram", make, call, ref=ref)
    objects(3, 3, 19, 33)           # B = 3, K = 3, 19x33 and B = 1, K = 2, 1x1: shapes of test_device_equals_the_host
    objects(1, 2, 1, 1)


_curves()


# ------------------------------------------------------------------------------------------------ optimiser
def _adam():
    def make():
        g = _gen(41)
        return dict(p=R(g, 70001), grads=R(g, 70001, scale=0.01))

    def call(p, grads, ranges=None):
        opt = _ops().FlatAdam(p, lr=1e-3)
        if ranges:
            opt.set_trainable(ranges)
        norms = [opt.step(grads).clone() for _ in range(2)]
        return norms, opt.p, opt.m, opt.v, opt.coef
    def adam_ref(ranges):
        def ref(inp, out):
            """clip_grad_norm_(0.5) + torch.optim.Adam on the trainable ranges (all of the buffer without ranges), as
            test_flat_adam_matches_torch and the set_trainable test of tests/test_finetune_kernels_gpu.py: the norm at rel 1e-5,
            the parameters at 1e-6 of the largest, a frozen range untouched bit for bit"""
            p0, gr = inp["p"].cpu(), inp["grads"].cpu()
            rng = ranges or [(0, p0.numel())]
            params = [p0[a:b].clone().requires_grad_(True) for a, b in rng]
            opt = torch.optim.Adam(params, lr=1e-3)
            for step in range(2):
                for prm, (a, b) in zip(params, rng):
                    prm.grad = gr[a:b].clone()
                gn = torch.nn.utils.clip_grad_norm_(params, 0.5)
                opt.step()
                assert abs(float(out[f"out[0][{step}]"]) - float(gn)) <= 1e-5 * float(gn)
            want = p0.clone()
            for prm, (a, b) in zip(params, rng):
                want[a:b] = prm.detach()
            got = out["out[1]"].cpu()
            _assert_rel(got, want, 1e-6)
            frozen = torch.ones(p0.numel(), dtype=torch.bool)
            for a, b in rng:
                frozen[a:b] = False
            _assert_equal(got[frozen], p0[frozen])
            assert not torch.equal(got[~frozen], p0[~frozen])
        return ref
    case("FlatAdam two steps on 70001 floats", "FlatAdam", make, call, ref=adam_ref(None))
    case("FlatAdam two steps on two trainable ranges", "FlatAdam", make, lambda p, grads: call(p, grads, [(0, 1024), (4096, 70001)]),
         ref=adam_ref([(0, 1024), (4096, 70001)]))


_adam()
