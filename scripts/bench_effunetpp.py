"""EfficientUnet++ inference: the fused inverted-residual kernels (csrc/mbconv.hip) against the same decoder composed from
ops the library already had plus torch element-wise calls, with ``unet`` and ``unet++`` beside them for scale.

  sides      ``fused``: ``UNetHIP(decoder="efficientunetplusplus")`` as shipped.  ``composed``: the same model object with
             the block replaced, inside this script, by 1x1 convolutions through ``dt_conv2d_affine`` (up-sampling and the
             concatenated skip still virtual), the depthwise 3x3 through ``torch.nn.functional.conv2d(groups=C)`` and
             Hardswish, BatchNorm affine, pooling, both gates, the gating product and the residual add as torch calls —
             encoder, concatenation and head are the very same launches on both sides.  Their logits must be
             ``torch.allclose`` (checked at 2 x 64 x 64 before anything is timed).
  figures    inference tiles/s of ``predict_classes(uint8, nhwc)`` at 256^2 B=64 and 512^2 B=32 (host clock around a device
             synchronise, ``--reps`` calls per sample, the sides in alternating rounds), and hipEvent times of the new
             kernels at the shapes of the first node (x_0_0: 1/16 resolution, 768 channels) and the last (x_0_4: full
             resolution, 16 channels), with the bytes and FLOPs the engine's profile attributes to them.

Every figure is taken in ``--children`` fresh processes, one after the other, each under its own time limit; the last line
is the median over them.

    python scripts/bench_effunetpp.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CONFIGS = (("256", 256, 64), ("512", 512, 32))
SIDES = ("fused", "composed", "unet", "unetpp")
NEW_KERNELS = ("pwconv_affine_kernel", "pwconv_affine_kernel<gated>", "dwconv3x3_affine_kernel", "scse_gates_kernel")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.nn.functional as F
    from deadtrees_amd import ops
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_effunetpp.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")

    def model(decoder, **kw):
        m = UNetHIP(in_channels=3, classes=2, decoder=decoder, **kw)
        m.reset_parameters(seed=0)
        g = torch.Generator().manual_seed(1)       # non-trivial BatchNorm statistics; decoder weights scaled to O(1) activations
        sd = m.smp_state_dict()
        for k, v in sd.items():
            if k.endswith("running_mean"):
                sd[k] = 0.1 * torch.randn(v.shape, generator=g)
            elif k.endswith("running_var"):
                sd[k] = 1.0 + 0.2 * torch.rand(v.shape, generator=g)
            elif k.startswith("decoder.") and v.dim() == 4 and decoder == "efficientunetplusplus":
                sd[k] = v * 0.5
            elif k.endswith(".bias") and v.dim() == 1:
                sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        m.load_smp_state_dict(sd)
        return m.to(dev).eval()

    eff = model("efficientunetplusplus", squeeze_ratio=a.squeeze, expansion_ratio=a.expansion)
    eng = eff.engine
    fused_mbconv = eng._mbconv
    plain = set()       # layers whose shape dt_conv2d_affine does not take: dt_conv2d + a torch affine there

    def affine_of(c, params, bn):
        """(scale, shift) of convolution c as the engine's workspace holds them (bias folded in)"""
        return eng._bn_eval_affine(c, params, bn)

    def pw_composed(c, params, bn, src0, src1, up0):
        scale, shift = affine_of(c, params, bn)
        w = c.w(params).view(1, 1, c.cin, c.cout)
        if c.key not in plain:
            try:
                return ops.conv2d_affine(src0, w, 1, 1, 0, scale, shift, relu=False, src1=src1, mode0=1 if up0 else 0)
            except RuntimeError:
                plain.add(c.key)
        return ops.conv2d(src0, w, 1, 1, 0, src1=src1, mode0=1 if up0 else 0)[0] * scale + shift

    def composed_mbconv(mb, params, bn, src0, src1, up0, B, H, W):
        a_ = F.hardswish(pw_composed(mb.pw1, params, bn, src0, src1, up0))
        scale, shift = affine_of(mb.dw, params, bn)
        wdw = mb.dw.w(params).view(9, mb.mid).t().reshape(mb.mid, 1, 3, 3)
        b_ = F.conv2d(a_.permute(0, 3, 1, 2), wdw, padding=1, groups=mb.mid).permute(0, 2, 3, 1)
        b_ = F.hardswish(b_ * scale + shift)
        mean = b_.mean(dim=(1, 2))
        hid = torch.relu(mean @ mb.cse1.w(params).view(mb.mid, -1) + mb.cse1.bias(params))
        gc = torch.sigmoid(hid @ mb.cse2.w(params).view(-1, mb.mid) + mb.cse2.bias(params))
        gs = torch.sigmoid(b_ @ mb.sse.w(params) + mb.sse.bias(params))
        g_ = (b_ * gc[:, None, None, :] + b_ * gs[..., None]).contiguous()
        res = pw_composed(mb.skip, params, bn, src0, src1, up0) if mb.skip is not None else src0
        return pw_composed(mb.pw2, params, bn, g_, None, False) + res

    def set_side(side):
        eng._mbconv = composed_mbconv if side == "composed" else fused_mbconv

    # ---- the two sides compute the same function
    x0 = torch.randn((2, 64, 64, 3), generator=torch.Generator().manual_seed(2)).to(dev)
    set_side("fused")
    lf = eff.predict_logits(x0, nhwc=True)
    set_side("composed")
    lc = eff.predict_logits(x0, nhwc=True)
    set_side("fused")
    scale = float(lf.abs().max())
    same = bool(torch.allclose(lf, lc, rtol=1e-4, atol=1e-4 * scale))
    row = {"what": "child", "squeeze": a.squeeze, "expansion": a.expansion, "allclose": same, "composed_plain_convs": len(plain),
           "max_abs_diff": float((lf - lc).abs().max()), "max_abs_logit": scale}
    if not same:
        print(json.dumps(row), flush=True)
        raise SystemExit("bench_effunetpp.py: fused and composed logits differ; nothing is timed")

    models = {"fused": eff, "composed": eff, "unet": model("unet"), "unetpp": model("unetplusplus")}

    def tiles_per_s(side, x):
        set_side(side)
        m = models[side]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            m.predict_classes(x, dtype="uint8", nhwc=True)
        torch.cuda.synchronize()
        set_side("fused")
        return a.reps * x.shape[0] / (time.perf_counter() - t)

    for name, size, batch in CONFIGS:
        x = torch.randn((batch, size, size, 3), generator=torch.Generator().manual_seed(3)).to(dev)
        for side in SIDES:
            tiles_per_s(side, x)                      # warm-up: allocator, weight images, eval affines
        samples = {s: [] for s in SIDES}
        for _ in range(a.rounds):                     # alternate, so that all see the same machine
            for side in SIDES:
                samples[side].append(tiles_per_s(side, x))
        for side in SIDES:
            row[f"{side}_{name}_tiles_s"] = round(statistics.median(samples[side]), 1)
        # ---- the new kernels one by one: the first node (x_0_0) and the last (x_0_4) of a profiled fused forward
        per = {}
        for _ in range(a.profile_runs):
            eng.profile = []
            eff.predict_classes(x, dtype="uint8", nhwc=True)
            torch.cuda.synchronize()
            prof, eng.profile = [p for p in eng.profile if p[0] in NEW_KERNELS], None
            n1 = 9                                    # launches of a node: 5 (first block, with skip projection) + 4
            for node, part in (("x_0_0", prof[:n1]), ("x_0_4", prof[-n1:])):
                for i, (kname, flops, e0, e1, nbytes) in enumerate(part):
                    per.setdefault((node, i, kname, flops, nbytes), []).append(e0.elapsed_time(e1) * 1e3)
        kernels = []
        for (node, i, kname, flops, nbytes), us in per.items():
            t = statistics.median(us)
            kernels.append({"node": node, "launch": i, "kernel": kname, "us": round(t, 1), "GB_s": round(nbytes / t / 1e3, 1),
                            "GFLOP_s": round(flops / t / 1e3, 1)})
        row[f"kernels_{name}"] = kernels
        del x
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--squeeze", type=int, default=1)
    ap.add_argument("--expansion", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile-runs", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("squeeze", "expansion", "reps", "rounds", "profile_runs"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_effunetpp.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {f"{s}_{n}_tiles_s": round(statistics.median(r[f"{s}_{n}_tiles_s"] for r in rows), 1)
           for n, _, _ in CONFIGS for s in SIDES}
    for n, _, _ in CONFIGS:
        med[f"fused_over_composed_{n}"] = round(med[f"fused_{n}_tiles_s"] / med[f"composed_{n}_tiles_s"], 3)
        ks = []
        for i, k in enumerate(rows[0][f"kernels_{n}"]):
            ks.append(dict(k, us=round(statistics.median(r[f"kernels_{n}"][i]["us"] for r in rows), 1),
                           GB_s=round(statistics.median(r[f"kernels_{n}"][i]["GB_s"] for r in rows), 1),
                           GFLOP_s=round(statistics.median(r[f"kernels_{n}"][i]["GFLOP_s"] for r in rows), 1)))
        med[f"kernels_{n}"] = ks
    print(json.dumps({"what": "median", "children": len(rows), "allclose": all(r["allclose"] for r in rows), **med}),
          flush=True)


if __name__ == "__main__":
    main()
