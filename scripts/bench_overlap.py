"""overlap-stitched whole-raster inference against the block path: one 2048x2048 RGBN raster through ``infer_tile`` at
d = 256, batch 64, for overlap 0 / 32 / 64 in both blend modes — raster milliseconds (host clock around a device
synchronise, median of ``--runs`` timed runs of ``--reps`` calls each) and windows per second.

    python scripts/bench_overlap.py                       # every setting, one JSON line each
    python scripts/bench_overlap.py --settings default    # infer_tile without the overlap arguments: also runs on a tree
                                                          # that predates them (``--root`` = that tree) — the baseline
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/bench_overlap.py --runs 1 --reps 2
    python scripts/bench_overlap.py --kernel-stats OUT/.../*_kernel_stats.csv     # the gather + stitch kernels' rows
    python scripts/bench_overlap.py --digest [--root TREE]                         # sha256 of every setting's result
"""
import argparse
import csv
import hashlib
import json
import os
import statistics
import sys
import time

STITCH_KERNELS = ("window_normalize_u8_kernel", "stitch_accumulate_kernel", "stitch_finalize_kernel",
                  "stitch_classes_u8_kernel", "split_normalize_u8_kernel")


def kernel_stats(path):
    """rows of a rocprofv3 ``*_kernel_stats.csv`` for the gather and the stitch kernels"""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in STITCH_KERNELS):
                print(json.dumps({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]),
                                  "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                  "max_us": float(row["MaxNs"]) / 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="tree to import deadtrees_amd from (default: this one)")
    ap.add_argument("--settings", default="default,0:crop,32:crop,64:crop,0:average,32:average,64:average",
                    help="comma list of 'default' (no overlap arguments) and OVERLAP:BLEND")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--subtile", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--digest", action="store_true",
                    help="print a sha256 of each setting's downloaded map (and probabilities, average mode) instead of timing: "
                         "two trees compute the same raster when the digests agree")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)

    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_overlap.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    m = UNetHIP(in_channels=3, classes=2)
    m.reset_parameters(seed=0)
    m.to(dev).eval()

    class Inf:      # PyTorchInference's device entry points on this model (no checkpoint file needed)
        in_channels = 3

        def run_blocks(self, raster, d, first, count):
            return m.predict_classes(ops.split_normalize_u8(raster, d, first, count, MEAN, STD, 3), dtype="uint8", nhwc=True)

        def run_windows(self, raster, d, overlap, first, count, want="classes", precision="fp32"):
            x = ops.window_normalize_u8(raster, d, overlap, first, count, MEAN, STD, 3)
            if want == "classes":
                return m.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
            return m.predict_logits(x, precision=precision, nhwc=True)

    d = a.subtile
    ortho = np.random.default_rng(7).integers(0, 256, (4, a.size, a.size), dtype=np.uint8)
    for setting in a.settings.split(","):
        if setting == "default":
            kw, overlap, blend = {}, 0, "blocks"
        else:
            overlap, blend = setting.split(":")
            overlap = int(overlap)
            kw = dict(overlap=overlap, blend=blend)
        s = d - overlap
        n_win = max(1, -(-(a.size - overlap) // s)) ** 2

        def call():
            return tiler.infer_tile(Inf(), ortho, subtile=d, batch_size=a.batch, device="cuda:0", **kw)

        if a.digest:
            want_probs = dict(return_probs=True) if overlap and blend == "average" else {}     # overlap 0 is the block path
            res = tiler.infer_tile(Inf(), ortho, subtile=d, batch_size=a.batch, device="cuda:0", **kw, **want_probs)
            parts = res if isinstance(res, tuple) else (res,)
            print(json.dumps({"tag": a.tag, "setting": setting, "arrays": [[str(p.dtype), list(p.shape)] for p in parts],
                              "sha256": hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for p in parts)).hexdigest()}),
                  flush=True)
            continue
        for _ in range(3):
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
        print(json.dumps({"tag": a.tag, "tree": os.path.relpath(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(tiler.__file__))))), "setting": setting, "overlap": overlap, "blend": blend, "windows": n_win,
                          "raster_ms": round(ms, 3), "runs_ms": [round(v, 3) for v in times],
                          "windows_per_s": round(n_win / ms * 1e3, 1), "class1_share": round(float(out.mean()), 4)}),
              flush=True)


if __name__ == "__main__":
    main()
