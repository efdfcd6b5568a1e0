"""nearest-patch distances of label planes built before the download against the host route after it: ``--size`` x ``--size``
(2048) planes with K = 3.  Maps: ``shift`` — the ~3 % dilated-seed map of ``bench_patches.py`` queried against a copy shifted
by (3, 5) pixels (this year against last year: most patches overlap, the others are a few pixels apart); ``corner`` — the
seed map queried against a map with one dead pixel in a corner (every query pixel searches its row up to that column: the
longest searches there are); ``gaps`` — the seed map against itself with ``exclude_own``.

  columns    ``dt_proximity_columns`` alone (its three launches), hipEvents around it (median of ``--iters``)
  query      ``dt_proximity_query`` alone on those tables, ``best`` reset before every sample outside the events
  proximity  all of ``ops.patch_proximity`` on label planes in HBM: the tables, the root -> row plane, the query, the decoding
             and the download of the result
  host       ``patch_proximity_host`` on the downloaded planes (host clock, ``--host-iters`` samples); ``download_ms`` is
             the D2H copy of the int32 planes, which the host route needs and the device route does not
  infer_tile one RGBN raster of that size through ``infer_tile(stats=True, patches=True, against=...)`` at overlap 0 and at
             ``overlap=64, blend="average"``: plain, with ``distances=True``, with ``gaps=True`` — the sides in alternating
             blocks, host clock around a device synchronise

Every child asserts that the two sides agree exactly.  Every figure is taken in ``--children`` fresh processes, one after
the other, each under its own time limit; the first child that fails ends the measurement; the last line is the median
over them.

    python scripts/bench_proximity.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 3
MAPS = ("shift", "corner", "gaps")
MAP_FIGURES = ("columns_us", "query_us", "proximity_ms", "download_ms", "host_ms")
INFER_SIDES = ("against", "distances", "gaps")
INFER_FIGURES = tuple(f"{mode}_{side}_ms" for mode in ("blocks", "average") for side in INFER_SIDES)


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.proximity import patch_distances, patch_gaps, patch_proximity_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_proximity.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size

    def event_us(fn, before=None):
        samples = []
        for it in range(a.iters + 3):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                samples.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(samples)

    def host_ms(fn, iters):
        """(median milliseconds, the last result)"""
        samples = []
        for _ in range(iters):
            t = time.perf_counter()
            result = fn()
            samples.append((time.perf_counter() - t) * 1e3)
        return statistics.median(samples), result

    def same(got, want):
        return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))

    row = {"what": "child", "size": n, "K": K, "exact": True}
    lib, st = _lib.load(), _lib.stream()
    cover = cover_map(n, rng)
    corner = np.zeros((n, n), np.uint8)
    corner[0, 0] = 1
    lq, _ = ops.label_patches(torch.from_numpy(cover).to(dev), K, 8)
    roots = torch.nonzero(ops.patch_areas(lq)).view(-1)
    host_q, host_roots = lq.cpu().numpy(), roots.cpu().numpy()
    row["patches"] = len(host_roots)
    for name in a.maps.split(","):
        if name == "shift":
            source, exclude_own = np.roll(cover, (3, 5), (0, 1)), False
        elif name == "corner":
            source, exclude_own = corner, False
        elif name == "gaps":
            source, exclude_own = None, True
        else:
            raise SystemExit(f"bench_proximity.py: unknown map {name!r} (shift, corner, gaps)")
        ls = lq if source is None else ops.label_patches(torch.from_numpy(np.ascontiguousarray(source)).to(dev), K, 8)[0]
        host_s = host_q if source is None else ls.cpu().numpy()
        got = ops.patch_proximity(ls, lq, roots, exclude_own)
        ms, want = host_ms(lambda: patch_proximity_host(host_s, host_q, host_roots, exclude_own), a.host_iters)
        row[f"{name}_host_ms"] = round(ms, 3)
        row["exact"] = bool(row["exact"] and same(got, want))
        row[f"{name}_at_zero"], row[f"{name}_farthest_d2"] = int((got[0] == 0).sum()), int(got[0].max())

        # the query launch alone, on buffers of its own: best is reset in front of every sample, outside the events
        dist, nearest, flag = ops.proximity_tables(ls, second=exclude_own)
        dense = torch.full((n * n,), -1, dtype=torch.int32, device=dev)
        dense[roots] = torch.arange(len(host_roots), dtype=torch.int32, device=dev)
        best = torch.empty(len(host_roots), dtype=torch.int64, device=dev)

        def query():
            lib.dt_proximity_query(dist.data_ptr(), nearest.data_ptr(), flag.data_ptr(), lq.data_ptr(), n, n, dense.data_ptr(),
                                   len(host_roots), int(exclude_own), int(exclude_own), -1, best.data_ptr(), st)

        planes = 1 if source is None else 2
        pinned = torch.empty((planes, n, n), dtype=torch.int32, pin_memory=True)

        def download():
            pinned[0].copy_(lq, non_blocking=True)
            if planes == 2:
                pinned[1].copy_(ls, non_blocking=True)

        figures = {f: [] for f in ("columns_us", "query_us", "proximity_ms", "download_ms")}
        for _ in range(3):                    # alternate, so that all see the same machine
            figures["columns_us"].append(event_us(lambda: ops.proximity_tables(ls, second=exclude_own)))
            figures["query_us"].append(event_us(query, before=lambda: best.fill_(-1)))
            figures["proximity_ms"].append(event_us(lambda: ops.patch_proximity(ls, lq, roots, exclude_own)) / 1e3)
            figures["download_ms"].append(event_us(download) / 1e3)
        for f, v in figures.items():
            row[f"{name}_{f}"] = round(statistics.median(v), 3 if f.endswith("ms") else 2)

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

    if a.infer:
        inf = Inf()
        ortho = rng.integers(0, 256, (4, n, n), dtype=np.uint8)
        sides = (("against", dict()), ("distances", dict(distances=True)), ("gaps", dict(gaps=True)))
        for name, kw in (("blocks", dict(overlap=0)), ("average", dict(overlap=64, blend="average"))):

            def block_ms(extra):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.reps):
                    tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, patches=True,
                                     against=cover, **kw, **extra)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / a.reps * 1e3

            for _, extra in sides:
                block_ms(extra)
            times = {side: [] for side, _ in sides}
            for _ in range(a.rounds):             # alternate
                for side, extra in sides:
                    times[side].append(block_ms(extra))
            for side, _ in sides:
                row[f"{name}_{side}_ms"] = round(statistics.median(times[side]), 3)
        m, stats = tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, patches=True,
                                    against=cover, distances=True, gaps=True)
        row["infer_patches"] = stats.patches.n
        row["exact"] = bool(row["exact"] and stats.overlaps.distances == patch_distances(cover, m, K)
                            and stats.gaps == patch_gaps(m, K))
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_proximity.py: the device result and the host result differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--maps", default=",".join(MAPS))
    ap.add_argument("--infer", type=int, default=1, help="0 leaves the infer_tile figures out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "iters", "host_iters", "reps", "rounds", "maps", "infer"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_proximity.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = tuple(f"{m}_{f}" for m in a.maps.split(",") for f in MAP_FIGURES) + (INFER_FIGURES if a.infer else ())
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in keys}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "children": len(rows),
                      "exact": all(r["exact"] for r in rows),
                      **{k: rows[0][k] for k in rows[0] if k.endswith(("patches", "_at_zero", "_farthest_d2"))},
                      **med}), flush=True)


if __name__ == "__main__":
    main()
