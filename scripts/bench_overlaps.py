"""the overlap table of two label planes built before the download against the host route after it: ``--size`` x ``--size``
(2048) planes with K = 3.  Pairs of maps: ``shift`` — the ~3 % dilated-seed map of ``bench_patches.py`` against a copy
shifted by (3, 5) pixels (this year against last year); ``full`` — one raster-sized patch against the seed map.
``--maps shift,full,checker`` adds the 4-connected 0 / 1 checkerboard against one raster-sized patch: ``h w / 2`` pairs of
one pixel each, the most a raster can have, and every pixel a run.

  count      the first launch alone (``dt_overlap_count``), hipEvents around it (median of ``--iters``)
  runs       the second launch alone (``dt_overlap_runs`` on the scanned counts)
  table      all of ``ops.patch_overlaps`` on two label planes in HBM: both launches, the scan, the read-backs, the sort
             over the runs, the segmented sum and the download of the three result arrays
  host       ``overlap_pairs_host`` on the two downloaded planes (host clock); ``download_ms`` is the D2H copy of the two
             int32 planes, which the host route needs and the device route does not
  infer_tile one RGBN raster of that size through ``infer_tile(stats=True, patches=True)`` at overlap 0 and at
             ``overlap=64, blend="average"``, without and with ``against=`` the seed map — the sides in alternating
             blocks, host clock around a device synchronise

Every child asserts that the two sides agree exactly.  Every figure is taken in ``--children`` fresh processes, one after
the other, each under its own time limit; the first child that fails ends the measurement; the last line is the median
over them.

    python scripts/bench_overlaps.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 3
MAPS = ("shift", "full")
MAP_FIGURES = ("count_us", "runs_us", "table_ms", "download_ms", "host_ms")
INFER_FIGURES = ("blocks_patches_ms", "blocks_against_ms", "average_patches_ms", "average_against_ms", "infer_host_ms")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.overlaps import overlap_pairs_host, patch_overlaps
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_overlaps.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size

    def event_us(fn):
        samples = []
        for it in range(a.iters + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
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

    def same(got, want):
        return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))

    row = {"what": "child", "size": n, "K": K, "exact": True}
    lib, st = _lib.load(), _lib.stream()
    cover = cover_map(n, rng)
    full = np.ones((n, n), np.uint8)
    for name in a.maps.split(","):
        if name == "shift":
            (map_a, conn_a), (map_b, conn_b) = (np.roll(cover, (3, 5), (0, 1)), 8), (cover, 8)
        elif name == "full":
            (map_a, conn_a), (map_b, conn_b) = (full, 8), (cover, 8)
        elif name == "checker":
            board = np.ascontiguousarray((np.add.outer(np.arange(n), np.arange(n)) & 1).astype(np.uint8))
            (map_a, conn_a), (map_b, conn_b) = (board, 4), (full, 8)
        else:
            raise SystemExit(f"bench_overlaps.py: unknown pair of maps {name!r} (shift, full, checker)")
        la, _ = ops.label_patches(torch.from_numpy(np.ascontiguousarray(map_a)).to(dev), K, conn_a)
        lb, _ = ops.label_patches(torch.from_numpy(np.ascontiguousarray(map_b)).to(dev), K, conn_b)
        host_a, host_b = la.cpu().numpy(), lb.cpu().numpy()
        got, want = ops.patch_overlaps(la, lb), overlap_pairs_host(host_a, host_b)
        row["exact"] = bool(row["exact"] and same(got, want))
        row[f"{name}_pairs"], row[f"{name}_shared_pixels"] = len(got[0]), int(got[2].sum())

        # the two launches alone, on buffers of their own
        counts = torch.empty((-(-n * n // ops.OVERLAP_CHUNK), 2), dtype=torch.int32, device=dev)
        lib.dt_overlap_count(la.data_ptr(), lb.data_ptr(), n, n, counts.data_ptr(), st)
        scan = torch.cumsum(counts, 0, dtype=torch.int32)
        R = int(scan[-1, 0])
        row[f"{name}_runs"] = R
        chunk_first = (scan[:, 0] - counts[:, 0]).contiguous()
        key = torch.empty(R, dtype=torch.int64, device=dev)
        start = torch.empty(R, dtype=torch.int32, device=dev)
        pinned = torch.empty((2, n, n), dtype=torch.int32, pin_memory=True)

        def download():
            pinned[0].copy_(la, non_blocking=True)
            pinned[1].copy_(lb, non_blocking=True)

        figures = {f: [] for f in ("count_us", "runs_us", "table_ms", "download_ms")}
        for _ in range(3):                    # alternate, so that all see the same machine
            figures["count_us"].append(event_us(lambda: lib.dt_overlap_count(la.data_ptr(), lb.data_ptr(), n, n,
                                                                             counts.data_ptr(), st)))
            figures["runs_us"].append(event_us(lambda: lib.dt_overlap_runs(la.data_ptr(), lb.data_ptr(), n, n,
                                                                           chunk_first.data_ptr(), R, key.data_ptr(),
                                                                           start.data_ptr(), st)))
            figures["table_ms"].append(event_us(lambda: ops.patch_overlaps(la, lb)) / 1e3)
            figures["download_ms"].append(event_us(download) / 1e3)
        for f, v in figures.items():
            row[f"{name}_{f}"] = round(statistics.median(v), 3 if f.endswith("ms") else 2)
        row[f"{name}_host_ms"] = round(host_ms(lambda: overlap_pairs_host(host_a, host_b)), 3)

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
    for name, kw in (("blocks", dict(overlap=0)), ("average", dict(overlap=64, blend="average"))):
        sides = (("_patches", dict()), ("_against", dict(against=cover)))

        def block_ms(extra):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.reps):
                tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, patches=True, **kw,
                                 **extra)
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
    m, stats = tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, patches=True,
                                against=cover)
    row["infer_pairs"], row["infer_patches"] = len(stats.overlaps), stats.patches.n
    row["infer_host_ms"] = round(host_ms(lambda: patch_overlaps(cover, m, K)), 3)      # labelling included
    row["exact"] = bool(row["exact"] and stats.overlaps == patch_overlaps(cover, m, K))
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_overlaps.py: the device table and the host table differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--maps", default=",".join(MAPS))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "iters", "host_iters", "reps", "rounds", "maps"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_overlaps.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = tuple(f"{m}_{f}" for m in a.maps.split(",") for f in MAP_FIGURES) + INFER_FIGURES
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in keys}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "children": len(rows),
                      "exact": all(r["exact"] for r in rows),
                      **{k: rows[0][k] for k in rows[0] if k.endswith(("_pairs", "_runs", "_shared_pixels", "_patches"))},
                      **med}), flush=True)


if __name__ == "__main__":
    main()
