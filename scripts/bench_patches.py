"""dead-tree patches before the download against scipy after it: one ``--size`` x ``--size`` (2048) uint8 class map with
K = 3, about 3 % dead cover drawn as dilated random seeds ("cover"), and the worst case of one raster-sized patch ("full").

  label / areas / sieve / measure   the launches of ``ops.label_patches`` / ``patch_areas`` / ``sieve_patches``
             (``min_pixels=4``, on fresh copies) / ``dt_patch_measure`` alone, hipEvents around each (median of ``--iters``);
             ``table`` is all of ``ops.patch_table``: compaction, read-back of the row count, measure, download of the table
  host       the same on the downloaded map: ``scipy.ndimage.label`` + ``np.bincount`` per class (host_label_ms) and the
             whole host contract, ``patches_host`` (host_all_ms); host clock, the download itself not included
  infer_tile one RGBN raster of that size through ``infer_tile(stats=True)`` at overlap 0 and at ``overlap=64,
             blend="average"``, without ``patches``, with ``patches=True`` and with ``PatchConfig(min_pixels=4)`` — the
             sides in alternating blocks, host clock around a device synchronise

Every figure is taken in ``--children`` fresh processes, one after the other, each under its own time limit; the last line
is the median over them.

    python scripts/bench_patches.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 3
MAPS = ("cover", "full")
FIGURES = tuple(f"{m}_{f}" for m in MAPS for f in ("label_us", "areas_us", "sieve_us", "measure_us", "table_ms",
                                                   "host_label_ms", "host_all_ms")) + (
    "blocks_stats_ms", "blocks_patches_ms", "blocks_sieve_ms", "average_stats_ms", "average_patches_ms", "average_sieve_ms")


def cover_map(n, rng):
    """about 3 % dead cover: random seeds of classes 1 and 2, dilated three times with a 3 x 3 square (7 x 7 crowns)"""
    import numpy as np
    from scipy import ndimage
    seeds = rng.random((n, n)) < 0.03 / 40
    kind = rng.integers(1, K, (n, n))
    out = np.zeros((n, n), np.uint8)
    for c in range(1, K):
        out[ndimage.binary_dilation(seeds & (kind == c), structure=np.ones((3, 3), bool), iterations=3) & (out == 0)] = c
    return out


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from scipy import ndimage
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.patches import (PatchConfig, label_patches_host, measure_patches_host, patches_host)
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_patches.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size

    def event_us(fn, setup=None):
        samples = []
        for it in range(a.iters + 3):
            if setup is not None:
                setup()
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

    row = {"what": "child", "size": n, "K": K, "exact": True}
    for name in MAPS:
        classes = cover_map(n, rng) if name == "cover" else np.ones((n, n), np.uint8)
        dc = torch.from_numpy(classes).to(dev)
        labels, err = ops.label_patches(dc, K)
        area = ops.patch_areas(labels)
        table = ops.patch_table(labels, dc, area)
        want = label_patches_host(classes, K)
        row["exact"] = bool(row["exact"] and np.array_equal(labels.cpu().numpy(), want) and int(err) == 0
                            and table == measure_patches_host(want, classes))
        row[f"{name}_patches"] = table.n
        row[f"{name}_dead_percent"] = round(100.0 * np.count_nonzero(classes) / classes.size, 2)

        lib = _lib.load()
        st = _lib.stream()
        area_out = torch.zeros(n * n, dtype=torch.int32, device=dev)
        root = torch.nonzero(area).view(-1)
        rows = int(root.numel())
        dense = torch.zeros(n * n, dtype=torch.int32, device=dev)
        dense[root] = torch.arange(rows, dtype=torch.int32, device=dev)
        cls = torch.empty(rows, dtype=torch.uint8, device=dev)
        bbox = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        sy, sx = (torch.empty(rows, dtype=torch.int64, device=dev) for _ in range(2))
        c2, l2, a2 = dc.clone(), labels.clone(), area.clone()

        def fresh():
            c2.copy_(dc)
            l2.copy_(labels)
            a2.copy_(area)

        figures = {f: [] for f in ("label_us", "areas_us", "sieve_us", "measure_us", "table_ms")}
        for _ in range(3):                    # alternate, so that all see the same machine
            figures["label_us"].append(event_us(lambda: lib.dt_label_patches_u8(dc.data_ptr(), n, n, K, 8, l2.data_ptr(),
                                                                                err.data_ptr(), st)))
            figures["areas_us"].append(event_us(lambda: lib.dt_patch_areas(labels.data_ptr(), n, n, area_out.data_ptr(), st),
                                                setup=area_out.zero_))
            figures["sieve_us"].append(event_us(lambda: lib.dt_sieve_patches_u8(c2.data_ptr(), l2.data_ptr(), a2.data_ptr(), n,
                                                                                n, 4, st), setup=fresh))
            figures["measure_us"].append(event_us(lambda: lib.dt_patch_measure(
                labels.data_ptr(), dc.data_ptr(), n, n, dense.data_ptr(), rows, cls.data_ptr(), bbox.data_ptr(),
                sy.data_ptr(), sx.data_ptr(), st)))
            figures["table_ms"].append(event_us(lambda: ops.patch_table(labels, dc, area)) / 1e3)
        for f, v in figures.items():
            row[f"{name}_{f}"] = round(statistics.median(v), 3 if f.endswith("ms") else 2)

        def host_label():
            for c in range(1, K):
                comp, _ = ndimage.label(classes == c, structure=np.ones((3, 3), bool))
                np.bincount(comp.ravel())

        row[f"{name}_host_label_ms"] = round(host_ms(host_label), 3)
        row[f"{name}_host_all_ms"] = round(host_ms(lambda: patches_host(classes, K, PatchConfig(8, 4))), 3)

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
        sides = (("_stats", dict()), ("_patches", dict(patches=True)), ("_sieve", dict(patches=PatchConfig(8, 4))))

        def block_ms(extra):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.reps):
                tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, **kw, **extra)
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
    row["infer_patches"] = tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True,
                                            patches=True)[1].patches.n
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "iters", "host_iters", "reps", "rounds"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_patches.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in FIGURES}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "children": len(rows),
                      "exact": all(r["exact"] for r in rows), **med}), flush=True)


if __name__ == "__main__":
    main()
