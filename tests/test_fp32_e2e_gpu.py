"""Every unit of the fp32 training step against fp64, teacher-forced (the fp32 twin of
tests/test_bf16_e2e_gpu.py::test_bf16_train_step_teacher_forced_against_rounding_oracle).

One HIP training step (``forward`` / ``backward``: the schedules of ``engine_forward`` / ``engine_backward`` on
``FP32_UNITS``) with ``engine.trace`` on; every intermediate tensor —
forward activations and BatchNorm coefficients out of the saved activations, every activation gradient of the
hand-scheduled backward out of the trace — is compared with what the un-rounded oracle (oracle/unet_bf16_ref.py,
``rounding=False``, fp64) computes from the HIP path's OWN inputs of that unit, and then replaces the oracle's tensor.
No error cascades and no ReLU mask flips (the mask is recomputed from the forced y, scale, shift as the fp32
multiply-then-add the kernels do), so a dropped partial row of a fused BatchNorm-backward reduction, a wrong scale/shift
pairing, a join that accumulates twice or a skip gradient in the wrong slot is an O(1) error in the unit that has it
(tests/test_fp32_oracle_cpu.py shows that on the CPU), where the end-to-end bound of
test_model_gpu.py::test_train_step_gradient_parity (10x / 5x the fp32 CPU oracle's own distance) lets it pass.

The bounds are the loosest ones the per-kernel tests already hold, not measurements of this test:
  activations, activation gradients, logits   max|err| <= 2e-5 max|ref|   (test_winograd_gpu.py 1e-5 / 2e-5,
                                                                           test_kernels_gpu.py 2e-5)
  BatchNorm coefficient vectors               max|err| <= 1e-4 of the layer's largest coefficient (test_winograd_gpu.py)
  parameter gradients                         ||g_hip - g|| <= 2e-5 ||g|| + 1e-6 max_k ||g_k||
  stored activations (stem.z, z1, z2)         equal to relu(y * scale + shift) evaluated in fp32 on the CPU
The oracle's own share (fp32 torch-CPU run forced into fp64, tests/test_fp32_oracle_cpu.py): <= 1.2e-6 / 5e-7 / 1.5e-6.

A tensor the engine never materialises is left unforced: ``D{i}.dup`` where the up-sampling's backward rides in the
data-gradient epilogue (default engine: the fused kernels ran if that list is non-empty), the two-branch ResUnet block
(its branches' full-resolution gradients are never summed).  The dense Unet++ decoder has no fused form: nothing unforced.

Measured on an MI355X (tensors compared; unforced; worst tensor, coefficient, gradient):
  unet    2,64,96,3,2    default   364  D1-D3.dup   L3B0.y1 1.6e-6    L1B3.y1.bn.shift 1.1e-6    layer1.0.bn2.bias 3.4e-7
  unet    2,128,128,4,3  default   364  D1-D3.dup   L3B0.y1 1.2e-6    L0B0.y1.bn.shift 1.2e-6    layer1.0.bn2.bias 4.5e-7
  unet    2,64,96,3,2    direct    367  none        L3B2.dz1 2.1e-6   L3B2.y1.bn.scale 1.2e-6    layer1.0.conv1.weight 2.9e-7
  unet    2,64,96,3,2    unfused   368  none        L3B0.y1 1.2e-6    L3B2.y2.bn.invstd 1.3e-6   bn1.bias 2.8e-7
  resunet 2,64,96,4,3    default   367  D0-D4.dup   L3B0.y1 1.4e-6    L3B1.y2.bn.shift 1.1e-6    layer1.0.conv1.weight 2.8e-7
  unet++  2,64,96,3,2    default   479  none        L3B0.y1 1.6e-6    L1B3.y1.bn.shift 1.1e-6    layer1.0.bn2.bias 3.6e-7
all a tenth of the bound or less, as close to fp64 as the fp32 torch-CPU run is; 0.5-1.1 s per case.  (With the direct
kernels dec4's fused up-sampled data gradient still runs: it writes D4.g and the oracle takes the same form, so nothing
is unforced there.)
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TENSOR_BOUND, COEFF_BOUND, GRAD_BOUND = 2e-5, 1e-4, 2e-5
FUSION_ATTRS = ("_fuse_bn", "fuse_join_fp32", "_fuse_pool_bn", "_mat_z1", "_mat_z2")


def _nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


def _hip_step(ref, img, mask, engine="default", names=("GDICE", "FOCAL")):
    """one fp32 training step on the HIP path -> (model, loss, err flag, forced-tensor dict for the oracle, stored
    activations [(name, z, y, scale, shift)] as CPU NHWC tensors)"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    from deadtrees_amd.network.unet import UNetHIP
    C, K = img.shape[1], ref.segmentation_head[0].out_channels
    dense = isinstance(ref.decoder.blocks, torch.nn.ModuleDict)
    resunet = not dense and hasattr(ref.decoder.blocks[0], "identity_conv")
    kind = "unetplusplus" if dense else ("resunet" if resunet else "unet")
    m = UNetHIP(in_channels=C, classes=K, decoder=kind)
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    assert m.precision == "fp32"
    eng = m.engine
    if engine == "direct":
        eng.winograd = False
    elif engine == "unfused":
        for a in FUSION_ATTRS:
            assert hasattr(eng, a), a
            setattr(eng, a, False)
    else:
        assert engine == "default"
    eng.trace = {}
    logits = m(img.to(DEV))
    S = dict(logits.grad_fn.saved_acts.d)   # the autograd node owns the saved activations; backward clears the
                                            # dict entries, not the tensors
    loss, _, err = seg_loss(logits, mask.to(DEV), None, names)
    loss.backward()
    torch.cuda.synchronize()
    trace, eng.trace = eng.trace, None

    forced, stored = {}, []
    sp, nb = m.spec, m.spec.n_bn_channels
    bnws = S["bnws"].cpu()

    def coeffs(name, c):
        for j, k in enumerate(("mean", "invstd", "scale", "shift")):
            forced[f"{name}.bn.{k}"] = bnws[j * nb + c.bn_off: j * nb + c.bn_off + c.cout].clone()

    def act(name, z, y, c):
        if z is not None:
            stored.append((name, z.cpu(), y.cpu(), bnws[2 * nb + c.bn_off: 2 * nb + c.bn_off + c.cout],
                           bnws[3 * nb + c.bn_off: 3 * nb + c.bn_off + c.cout]))

    forced["stem.y"], forced["stem.z"] = _nchw(S["stem"]["y"]), _nchw(S["stem"]["z"])
    coeffs("stem.y", sp.stem)
    act("stem.z", S["stem"]["z"], S["stem"]["y"], sp.stem)
    for li, blocks in enumerate(sp.layers):
        for bi, blk in enumerate(blocks):
            r, n = S[f"L{li}B{bi}"], f"L{li}B{bi}"
            forced[f"{n}.y1"], forced[f"{n}.y2"], forced[f"{n}.out"] = _nchw(r["y1"]), _nchw(r["y2"]), _nchw(r["out"])
            coeffs(f"{n}.y1", blk.conv1)
            coeffs(f"{n}.y2", blk.conv2)
            act(f"{n}.z1", r.get("z1"), r["y1"], blk.conv1)
            if blk.down is not None:
                forced[f"{n}.yd"] = _nchw(r["yd"])
                coeffs(f"{n}.yd", blk.down)
    for i, blk in enumerate(sp.decoder):
        n = f"P{blk.name}" if dense else f"D{i}"
        d = S[n]
        forced[f"{n}.y1"], forced[f"{n}.y2"] = _nchw(d["y1"]), _nchw(d["y2"])
        coeffs(f"{n}.y1", blk.conv1)
        coeffs(f"{n}.y2", blk.conv2)
        act(f"{n}.z1", d.get("z1"), d["y1"], blk.conv1)
        act(f"{n}.z2", d.get("z2"), d["y2"], blk.conv2)
        if d.get("z2") is not None:
            forced[f"{n}.z2"] = _nchw(d["z2"])
    forced["logits"] = logits.detach().float().cpu()
    for k, t in trace.items():
        forced[k] = _nchw(t)
    for k, g in m.smp_grad_dict().items():
        forced[f"grad:{k}"] = g
    return m, float(loss.detach()), int(err), forced, stored


CASES = [("unet", 2, 64, 96, 3, 2, "default"),       # ragged Winograd tiles at every level (maps 32x48 ... 2x3)
         ("unet", 2, 128, 128, 4, 3, "default"),     # whole 16x16 tiles (epilogue forms 0/2/1/3/6), RGBN, 3 classes
         ("unet", 2, 64, 96, 3, 2, "direct"),        # engine.winograd = False: the direct kernels, same wiring
         ("unet", 2, 64, 96, 3, 2, "unfused"),       # FUSION_ATTRS off on the instance: the plain chain
         ("resunet", 2, 64, 96, 4, 3, "default"),    # _bwd_resunet_block
         ("unet++", 2, 64, 96, 3, 2, "default")]     # _bwd_unetpp: accumulating slots, channel slices


@pytest.mark.parametrize("arch,B,H,W,C,K,engine", CASES)
def test_fp32_train_step_teacher_forced_against_fp64(arch, B, H, W, C, K, engine):
    from conftest import parity_report
    from deadtrees_amd.data.synthetic import synth_batch
    from oracle.train_ref import loss_from_logits
    from oracle.unet_bf16_ref import Bf16TrainOracle
    from oracle.unet_ref import make_oracle
    from oracle.resunet_ref import make_resunet_oracle
    from oracle.unetpp_ref import make_unetpp_oracle
    ref = {"unet": make_oracle, "resunet": make_resunet_oracle, "unet++": make_unetpp_oracle}[arch](C, K, seed=0)
    ref.train()
    img, mask = synth_batch(B, H, W, C, K, seed=3)
    m, loss, err, forced, stored = _hip_step(ref, img, mask, engine)
    o = Bf16TrainOracle(copy.deepcopy(ref), torch.float64, forced=forced, rounding=False, update_running=False)
    lg = o.forward(img)                      # = the HIP logits (forced), after comparing the oracle's own
    lg = lg.clone().requires_grad_(True)
    loss_o, _ = loss_from_logits(lg, mask, ("GDICE", "FOCAL"))
    loss_o.backward()
    grads_o = o.backward(lg.grad)
    gh = m.smp_grad_dict()

    # ---- the figures first, then the assertions
    tag = f"[fp32 teacher-forced {arch} {B}x{H}x{W}x{C} K={K} {engine}]"
    worst = sorted(((v[1], k) for k, v in o.errs.items() if ".bn." not in k), reverse=True)
    wbn = max((v[1], k) for k, v in o.errs.items() if ".bn." in k)
    gscale = max(float(g.norm()) for g in grads_o.values())
    gerr = {k: (float((gh[k].double() - g.double()).norm()), float(g.norm())) for k, g in grads_o.items() if k in gh}
    wg = sorted(((e / (n + 1e-30), k) for k, (e, n) in gerr.items()), reverse=True)
    zbad = [n for n, z, y, sc, sh in stored if not torch.equal(z, torch.relu(y * sc + sh))]
    print(f"{tag} {len(o.errs)} tensors, unforced {o.unforced}; worst max|err|/max|ref|: " +
          ", ".join(f"{k} {e:.1e}" for e, k in worst[:5]))
    print("   worst parameter-gradient rel-L2: " + ", ".join(f"{k} {e:.1e}" for e, k in wg[:4]) +
          f"; {len(stored)} stored activations, {len(zbad)} differ from relu(y*scale+shift)")
    parity_report(f"{tag} {len(o.errs)} tensors compared, unforced {o.unforced}; worst tensor {worst[0][1]} "
                  f"{worst[0][0]:.2e} (bound {TENSOR_BOUND:.0e}), worst BatchNorm coefficient {wbn[1]} {wbn[0]:.2e} (bound "
                  f"{COEFF_BOUND:.0e}), worst parameter gradient {wg[0][1]} {wg[0][0]:.2e} (bound {GRAD_BOUND:.0e}); loss "
                  f"{loss:.7f} vs {float(loss_o.detach()):.7f}")

    assert err == 0
    assert loss == pytest.approx(float(loss_o.detach()), rel=2e-5)          # fused loss on the same logits
    # ---- which tensors were compared
    dups = {f"D{i}.dup" for i in range(5)}
    if engine == "unfused" or arch == "unet++":
        assert o.unforced == [], o.unforced            # every oracle tensor had a HIP twin
    else:
        assert set(o.unforced) <= dups, o.unforced
        if engine == "default":                        # the fused data-gradient kernels ran
            assert o.unforced, "no fused up-sampling backward ran"
    for n in o.unforced:                               # ... and what they wrote instead was compared
        blk = n.split(".")[0]
        assert f"{blk}.g" in o.errs and (f"{blk}.dskip" in o.errs or blk == "D4"), n
    if arch == "unet":
        assert len(o.errs) > 300, len(o.errs)
    # ---- per unit
    for k, (rel, mx) in o.errs.items():
        assert mx <= (COEFF_BOUND if ".bn." in k else TENSOR_BOUND), (k, rel, mx)
    assert set(gh) == set(grads_o)
    for k, (e, n) in gerr.items():
        assert e <= GRAD_BOUND * n + 1e-6 * gscale, (k, e, n)
    # ---- forward and backward agree on the mask: a stored activation is relu(y * scale + shift) of the HIP path's own
    # y, scale, shift, fp32 multiply then add
    assert stored and not zbad, zbad
