"""test-time augmentation and soft-vote ensembles on the stitched path: one 2048x2048 RGBN raster through ``infer_tile`` at
d = 256, overlap 64, blend "average", fp32, ``--batch`` forward tiles per batch, for tta none / "flips" / "d4" with one
model and with three models under a soft vote — raster milliseconds (host clock around a device synchronise, median of
``--runs`` timed runs of ``--reps`` calls each) — and, per view set, the views gather and the views accumulate of ONE
batch in isolation (hipEvents, median of ``--kernel-iters`` launches) next to the forward of the same batch.

    python scripts/bench_tta.py                      # every configuration, one JSON line each
    python scripts/bench_tta.py --only kernels       # the isolated kernel timings alone (--only rasters: the others)
    python scripts/bench_tta.py --digest [--root TREE]   # sha256 of every raster configuration's map and probabilities
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--subtile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--only", choices=("all", "rasters", "kernels"), default="all")
    ap.add_argument("--tag", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="tree to import deadtrees_amd from (default: this one)")
    ap.add_argument("--digest", action="store_true",
                    help="print a sha256 of each raster configuration's downloaded map and probabilities instead of timing: "
                         "two trees compute the same raster when the digests agree")
    a = ap.parse_args()

    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    d, o = a.subtile, a.overlap

    class Inf:      # PyTorchInference's run_windows on a freshly initialised model (no checkpoint file needed)
        in_channels = 3

        def __init__(self, seed):
            self.m = UNetHIP(in_channels=3, classes=2)
            self.m.reset_parameters(seed=seed)
            self.m.to(dev).eval()

        def run_windows(self, raster, d, overlap, first, count, want="classes", precision="fp32", views=None):
            x = ops.window_normalize_u8(raster, d, overlap, first, count, MEAN, STD, 3, views=views)
            if want == "classes":
                return self.m.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
            lg = self.m.predict_logits(x, precision=precision, nhwc=True)
            return lg if views is None else lg.reshape(count, len(views), *lg.shape[1:])

    class Soft:     # PyTorchEnsembleInference(..., vote="soft") as the tiler sees it
        in_channels, classes, vote = 3, 2, "soft"

        def __init__(self, members):
            self.members = tuple(members)

    models = [Inf(seed) for seed in (0, 1, 2)]
    ortho = np.random.default_rng(7).integers(0, 256, (4, a.size, a.size), dtype=np.uint8)
    ny, nx, _ = tiler.window_grid(a.size, a.size, d, o)
    n_win = ny * nx

    if a.only in ("all", "rasters"):
        for M in (1, 3):
            inference = models[0] if M == 1 else Soft(models)
            for tta in (None, "flips", "d4"):
                T = len(tiler.tta_views(tta))

                def call():
                    return tiler.infer_tile(inference, ortho, subtile=d, batch_size=a.batch, device="cuda:0", overlap=o,
                                            blend="average", tta=tta)

                if a.digest:
                    parts = tiler.infer_tile(inference, ortho, subtile=d, batch_size=a.batch, device="cuda:0", overlap=o,
                                             blend="average", tta=tta, return_probs=True)
                    print(json.dumps({"tag": a.tag, "what": "digest", "models": M, "tta": tta or "none",
                                      "arrays": [[str(p.dtype), list(p.shape)] for p in parts],
                                      "sha256": hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes()
                                                                        for p in parts)).hexdigest()}), flush=True)
                    continue
                for _ in range(2):
                    out = call()
                times = []
                for _ in range(a.runs):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(a.reps):
                        call()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t) / a.reps * 1e3)
                ms = statistics.median(times)
                print(json.dumps({"tag": a.tag, "what": "raster", "models": M, "tta": tta or "none", "views": T,
                                  "windows": n_win, "forward_tiles": n_win * T * M, "raster_ms": round(ms, 3),
                                  "runs_ms": [round(v, 3) for v in times],
                                  "forward_tiles_per_s": round(n_win * T * M / ms * 1e3, 1),
                                  "class1_share": round(float(out.mean()), 4)}), flush=True)

    if a.only in ("all", "kernels") and not a.digest:
        raster = torch.from_numpy(ortho[:3].copy()).to(dev)
        m = models[0]

        def event_us(fn):
            for _ in range(3):
                fn()
            samples = []
            for _ in range(a.kernel_iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                samples.append(e0.elapsed_time(e1) * 1e3)
            return round(statistics.median(samples), 2), round(min(samples), 2)

        sets = (("plain", None), ("identity", ((0, 0),)), ("flips", tiler.tta_views("flips")), ("d4", tiler.tta_views("d4")),
                ("transposing", ((0, 1), (0, 3), (1, 1), (1, 3))))
        for name, views in sets:
            T = len(views) if views else 1
            count = max(1, a.batch // T)
            x = ops.window_normalize_u8(raster, d, o, 0, count, MEAN, STD, 3, views=views)
            lg = m.m.predict_logits(x, nhwc=True)
            lg = lg if views is None else lg.reshape(count, T, *lg.shape[1:])
            acc = torch.zeros((lg.shape[-3], a.size, a.size), dtype=torch.float32, device=dev)
            gather = event_us(lambda: ops.window_normalize_u8(raster, d, o, 0, count, MEAN, STD, 3, views=views))
            accumulate = event_us(lambda: ops.stitch_accumulate(lg, acc, o, 0, views=views))
            forward = event_us(lambda: m.m.predict_logits(x, nhwc=True))
            row = {"tag": a.tag, "what": "kernels", "views": name, "T": T, "windows": count, "forward_tiles": count * T,
                   "gather_us": gather[0], "gather_min_us": gather[1], "accumulate_us": accumulate[0],
                   "accumulate_min_us": accumulate[1], "forward_us": forward[0], "forward_min_us": forward[1]}
            if views is not None:
                keep = event_us(lambda: ops.stitch_accumulate(lg, acc, o, 0, views=views, weight="keep"))
                row.update(accumulate_keep_us=keep[0], accumulate_keep_min_us=keep[1])
            row["stitch_share_of_forward"] = round((gather[0] + accumulate[0]) / forward[0], 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
