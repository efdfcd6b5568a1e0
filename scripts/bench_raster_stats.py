"""raster statistics before the download against numpy after it: one ``--size`` x ``--size`` (2048) uint8 class map with
K = 3, 97 % class 0, with and without a 2-zone forest mask.

  kernel     ``ops.zonal_counts`` on the map in HBM, hipEvents around one launch (median of ``--iters``)
  host       what the reference does with the downloaded map: ``np.unique(return_counts=True)``
             (computestats_inference.py) and, with zones, the two masked sums of aggregate_results.process_tile; host clock,
             the download itself not included
  infer_tile one RGBN raster of that size through ``infer_tile`` at overlap 0 and at ``overlap=64, blend="average"``, with and
             without ``stats=True`` — the two sides in alternating blocks, host clock around a device synchronise

Every figure is taken in ``--children`` fresh processes, one after the other; the last line is the median over them.

    python scripts/bench_raster_stats.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 3
FIGURES = ("kernel_us", "kernel_zones_us", "host_unique_ms", "host_masked_sums_ms", "blocks_ms", "blocks_stats_ms",
           "blocks_stats_zones_ms", "average_ms", "average_stats_ms", "average_stats_zones_ms")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.stats import zonal_counts_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_raster_stats.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size
    classes = np.where(rng.random((n, n)) < 0.97, 0, rng.integers(1, K, (n, n))).astype(np.uint8)
    forest = (rng.random((n, n)) < 0.4).astype(np.uint8)
    dc, dz = torch.from_numpy(classes).to(dev), torch.from_numpy(forest).to(dev)
    counts, err = ops.zonal_counts(dc, dz, K, 2)
    exact = bool(np.array_equal(counts.cpu().numpy(), zonal_counts_host(classes, forest, K, 2)) and int(err) == 0)

    def event_us(fn):
        for _ in range(3):
            fn()
        samples = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(samples)

    def host_ms(fn):
        fn()
        samples = []
        for _ in range(a.host_iters):
            t = time.perf_counter()
            fn()
            samples.append((time.perf_counter() - t) * 1e3)
        return statistics.median(samples)

    c1, e1 = torch.zeros((1, K), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    c2 = torch.zeros((2, K), dtype=torch.int64, device=dev)
    plain_us, zones_us = [], []
    for _ in range(3):                        # alternate, so that both see the same machine
        plain_us.append(event_us(lambda: ops.zonal_counts(dc, None, K, 1, counts=c1, err=e1)))
        zones_us.append(event_us(lambda: ops.zonal_counts(dc, dz, K, 2, counts=c2, err=e1)))

    def masked_sums():                        # aggregate_results.py:68-78
        return [classes[(classes == c) & (forest == 1)].sum() / forest.sum() for c in (1, 2)]

    unique_ms = host_ms(lambda: np.unique(classes, return_counts=True))
    sums_ms = host_ms(masked_sums)

    class Inf:      # PyTorchInference's device entry points on a freshly initialised model (no checkpoint file needed)
        in_channels, classes = 3, K

        def __init__(self):
            self.m = UNetHIP(in_channels=3, classes=K)
            self.m.reset_parameters(seed=0)
            self.m.to(dev).eval()

        def run_blocks(self, raster, d, first, count):
            x = ops.split_normalize_u8(raster, d, first, count, MEAN, STD, 3)
            return self.m.predict_classes(x, dtype="uint8", nhwc=True)

        def run_windows(self, raster, d, overlap, first, count, want="classes", precision="fp32", views=None):
            x = ops.window_normalize_u8(raster, d, overlap, first, count, MEAN, STD, 3, views=views)
            if want == "classes":
                return self.m.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
            return self.m.predict_logits(x, precision=precision, nhwc=True)

    inf = Inf()
    ortho = rng.integers(0, 256, (4, n, n), dtype=np.uint8)
    row = {"what": "child", "size": n, "K": K, "exact": exact,
           "kernel_us": round(statistics.median(plain_us), 2), "kernel_zones_us": round(statistics.median(zones_us), 2),
           "host_unique_ms": round(unique_ms, 3), "host_masked_sums_ms": round(sums_ms, 3)}
    for name, kw in (("blocks", dict(overlap=0)), ("average", dict(overlap=64, blend="average"))):
        sides = (("", dict()), ("_stats", dict(stats=True)), ("_stats_zones", dict(stats=True, zones=forest)))

        def block_ms(extra):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.reps):
                tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", **kw, **extra)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / a.reps * 1e3

        for _, extra in sides:
            block_ms(extra)
        times = {suffix: [] for suffix, _ in sides}
        for _ in range(a.rounds):             # alternate
            for suffix, extra in sides:
                times[suffix].append(block_ms(extra))
        for suffix, _ in sides:
            row[f"{name}{suffix}_ms"] = round(statistics.median(times[suffix]), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "iters", "host_iters", "reps", "rounds"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in FIGURES}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "children": len(rows),
                      "exact": all(r["exact"] for r in rows), **med}), flush=True)


if __name__ == "__main__":
    main()
