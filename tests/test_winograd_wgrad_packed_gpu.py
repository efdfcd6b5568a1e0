"""Packed staging stream of the Winograd weight gradient (conv_wino_wgrad.hip, PK).

The default kernel issues the two-channel adds and subtractions of both transforms as v_pk_add_f32 (negations as source
modifiers) and reads the fragments of two k-steps with one LDS instruction; DT_FP32_WINO_WGRAD_PACKED=0 selects the scalar
form.  Both perform the same IEEE operations on the same values in the same MFMA slots, so the results must be
bit-identical.  Every case is checked

  * against torch CPU fp64 autograd of the same layer, at the bound of
    test_winograd_gpu.py::test_winograd_weight_gradient_matches_fp64_and_direct_kernel (2e-5 x the largest reference magnitude),
  * for bit equality with the scalar form, computed by ONE fresh child process with the switch at 0 from the same operands,
  * for run-to-run bit equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # B, H, W (stored size of source 0), C0, C1, mode0, Cout, transform
    (1, 16, 16, 64, 0, 0, 64, False),      # the smallest: 8 chunks in 4 splits
    (1, 5, 16, 64, 0, 0, 64, False),       # three rows of tiles, the last half empty; 3 chunks in 2 splits: one chunk past the end
    (2, 32, 48, 64, 0, 0, 128, True),      # tiles_x != tiles_y, two co blocks, input transform
    (2, 16, 16, 64, 64, 1, 128, True),     # up-sampled source plus skip, map 32 x 32
    (3, 16, 16, 512, 0, 0, 512, False),    # 64 blocks, several chunks per split
    (2, 16, 16, 64, 64, 1, 32, True),      # CO32 K-split form
    (4, 64, 64, 128, 0, 0, 32, False),
    (2, 16, 24, 64, 0, 0, 64, False), (2, 17, 24, 64, 0, 0, 32, True)]   # chunks that wrap around a row of tiles; ragged rows

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from deadtrees_amd import ops
src, n = np.load(sys.argv[2]), int(sys.argv[4])
out = {}
for k in range(n):
    t = lambda name: torch.from_numpy(src[f"{name}{k}"]).cuda() if f"{name}{k}" in src else None
    out[f"dw{k}"] = ops.conv2d_wgrad_winograd(t("x"), t("dy"), src1=t("s1"), mode0=int(src[f"mode{k}"]),
                                              in_scale=t("sc"), in_shift=t("sh")).cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _operands(case):
    """the operands of one case (NHWC, fp32, host) and the fp64 weight gradient, HWIO"""
    B, H, W, C0, C1, mode0, Cout, tf = case
    g = torch.Generator().manual_seed(B * 100 + H + W + C0 + Cout)
    x = torch.randn((B, C0, H, W), generator=g)
    Hin, Win = (H, W) if mode0 == 0 else (2 * H, 2 * W)
    s1 = torch.randn((B, C1, Hin, Win), generator=g) if C1 else None
    sc = 1 + 0.3 * torch.randn(C0, generator=g) if tf else None
    sh = 0.3 * torch.randn(C0, generator=g) + 0.2 if tf else None
    z = x.double()
    if tf:
        z = F.relu(x * sc[None, :, None, None] + sh[None, :, None, None]).double()
    if mode0 == 1:
        z = F.interpolate(z, scale_factor=2, mode="nearest")
    xin = torch.cat([z, s1.double()], 1) if C1 else z
    wt = (torch.randn((Cout, C0 + C1, 3, 3), generator=g, dtype=torch.float64) * 0.05).requires_grad_(True)
    y = F.conv2d(xin, wt, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    ops_in = {"x": nhwc(x), "dy": nhwc(dy)}
    if C1:
        ops_in["s1"] = nhwc(s1)
    if tf:
        ops_in["sc"], ops_in["sh"] = sc, sh
    return ops_in, wt.grad.permute(2, 3, 1, 0).contiguous()


def _run(ops_in, mode0):
    from deadtrees_amd import ops
    d = {k: v.to(DEV) for k, v in ops_in.items()}
    return ops.conv2d_wgrad_winograd(d["x"], d["dy"], src1=d.get("s1"), mode0=mode0, in_scale=d.get("sc"),
                                     in_shift=d.get("sh")).cpu()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """operands and fp64 references of every case, and the scalar form's results from one child process"""
    assert os.environ.get("DT_FP32_WINO_WGRAD_PACKED", "1") != "0", "the test compares the default form with the switch at 0"
    tmp = tmp_path_factory.mktemp("wgrad_packed")
    cases, blob = [], {}
    for k, case in enumerate(CASES):
        ops_in, want = _operands(case)
        cases.append((ops_in, want))
        for name, v in ops_in.items():
            blob[f"{name}{k}"] = v.numpy()
        blob[f"mode{k}"] = np.int64(case[5])
    src, dst = str(tmp / "operands.npz"), str(tmp / "scalar_form.npz")
    np.savez(src, **blob)
    env = dict(os.environ, DT_FP32_WINO_WGRAD_PACKED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, src, dst, str(len(CASES))], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = np.load(dst)
    return {case: (cases[k][0], cases[k][1], torch.from_numpy(res[f"dw{k}"])) for k, case in enumerate(CASES)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_packed_form_matches_fp64_and_is_bit_identical_to_scalar_form(world, case):
    ops_in, want, scalar_form = world[case]
    got = _run(ops_in, case[5])
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"case {case}: max err / max|ref| = {err / scale:.3e} (bound 2e-5)")
    assert err <= 2e-5 * scale, err / scale
    assert torch.equal(got, scalar_form)             # same IEEE operations on the same values
    assert torch.equal(_run(ops_in, case[5]), got)   # run to run
