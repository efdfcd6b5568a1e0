"""patch attributes of a label plane built before the download against the host route after it: ``--size`` x ``--size``
(2048) planes, a C = 4 raster and K = 3, with and without probabilities.  Maps: ``cover`` — the ~3 % dilated-seed map of
``bench_patches.py``; ``single`` — one raster-sized patch (every wave adds into ONE table row: the atomic-contention case);
``checker`` — the 4-connected checkerboard (every second pixel a patch of its own: one set of atomics per labelled pixel).

  kernel      ``dt_patch_attributes_u8`` alone (its two launches), hipEvents around it (median of ``--iters``)
  attributes  all of ``ops.patch_attributes`` on planes in HBM: the root -> row plane, the two launches and the download of
              the two tables
  host        ``attribute_tables_host`` on the downloaded planes (host clock, ``--host-iters`` samples); ``download_ms`` is
              the D2H copy of what the host route needs and the device route does not: the int32 label plane and, with
              probabilities, the class map and the fp32 [K, h, w] planes
  infer_tile  one RGBN raster of that size through ``infer_tile(stats=True, patches=True)`` at overlap 0 — plain and with
              ``attributes=True`` — and at ``overlap=64, blend="average"`` — plain and with confidence —, the sides in
              alternating blocks, host clock around a device synchronise

Every child asserts that the two sides agree exactly.  Every figure is taken in ``--children`` fresh processes, one after
the other, each under its own time limit; the first child that fails ends the measurement; the last line is the median
over them.

    python scripts/bench_attributes.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 3
C = 4
PAIRS = ((3, 0),)
MAPS = ("cover", "single", "checker")
MAP_FIGURES = tuple(f"{f}{p}" for p in ("", "_probs") for f in ("kernel_us", "attributes_ms", "download_ms", "host_ms"))
INFER_FIGURES = ("blocks_plain_ms", "blocks_attributes_ms", "average_plain_ms", "average_confidence_ms")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ctypes
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.attributes import AttributeConfig, attribute_tables_host, patch_attributes_host
    from deadtrees_amd.deployment.patches import PatchConfig, labelled_patches_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_attributes.py measures on an MI355X: no HIP device here")
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

    def host_ms(fn, iters):
        """(median milliseconds, the last result)"""
        samples = []
        for _ in range(iters):
            t = time.perf_counter()
            result = fn()
            samples.append((time.perf_counter() - t) * 1e3)
        return statistics.median(samples), result

    row = {"what": "child", "size": n, "K": K, "C": C, "exact": True}
    lib, st = _lib.load(), _lib.stream()
    ortho = rng.integers(0, 256, (C, n, n), dtype=np.uint8)
    logits = rng.normal(0, 2, (K, n, n)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=0))
    host_probs = (e / e.sum(axis=0)).astype(np.float32)
    raster, probs = torch.from_numpy(ortho).to(dev), torch.from_numpy(host_probs).to(dev)
    pairs = (ctypes.c_int * 2)(*PAIRS[0])
    yy, xx = np.mgrid[0:n, 0:n]
    for name in a.maps.split(","):
        if name == "cover":
            m, conn = cover_map(n, rng), 8
        elif name == "single":
            m, conn = np.ones((n, n), np.uint8), 8
        elif name == "checker":
            m, conn = ((yy + xx) % 2).astype(np.uint8), 4
        else:
            raise SystemExit(f"bench_attributes.py: unknown map {name!r} ({', '.join(MAPS)})")
        classes = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        labels, _ = ops.label_patches(classes, K, conn)
        roots = torch.nonzero(ops.patch_areas(labels)).view(-1)
        host_labels, host_roots = labels.cpu().numpy(), roots.cpu().numpy()
        rows = len(host_roots)
        row[f"{name}_patches"] = rows
        dense = torch.full((n * n,), -1, dtype=torch.int32, device=dev)
        dense[roots] = torch.arange(rows, dtype=torch.int32, device=dev)
        for suffix, cp, host_cp in (("", (None, None), (None, None)), ("_probs", (classes, probs), (m, host_probs))):
            conf = cp[0] is not None
            got = ops.patch_attributes(labels, roots, raster, *cp, PAIRS)
            ms, want = host_ms(lambda: attribute_tables_host(host_labels, host_roots, ortho, *host_cp, PAIRS), a.host_iters)
            row[f"{name}_host_ms{suffix}"] = round(ms, 3)
            row["exact"] = bool(row["exact"] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
            sums = torch.empty((rows, 2 * C + 1 + conf), dtype=torch.int64, device=dev)
            extremes = torch.empty((rows, 2 * C + conf), dtype=torch.int32, device=dev)

            def kernel():
                lib.dt_patch_attributes_u8(labels.data_ptr(), raster.data_ptr(), C, n, n, dense.data_ptr(), rows,
                                           _lib.ptr(cp[0]), _lib.ptr(cp[1]), K if conf else 0, pairs, 1, sums.data_ptr(),
                                           extremes.data_ptr(), st)

            pinned = torch.empty((n, n), dtype=torch.int32, pin_memory=True)
            pinned_classes = torch.empty((n, n), dtype=torch.uint8, pin_memory=True)
            pinned_probs = torch.empty((K, n, n), dtype=torch.float32, pin_memory=True)

            def download():
                pinned.copy_(labels, non_blocking=True)
                if conf:
                    pinned_classes.copy_(classes, non_blocking=True)
                    pinned_probs.copy_(probs, non_blocking=True)

            figures = {f: [] for f in ("kernel_us", "attributes_ms", "download_ms")}
            for _ in range(3):                    # alternate, so that all see the same machine
                figures["kernel_us"].append(event_us(kernel))
                figures["attributes_ms"].append(event_us(lambda: ops.patch_attributes(labels, roots, raster, *cp, PAIRS)) / 1e3)
                figures["download_ms"].append(event_us(download) / 1e3)
            for f, v in figures.items():
                row[f"{name}_{f}{suffix}"] = round(statistics.median(v), 3 if f.endswith("ms") else 2)
            row["exact"] = bool(row["exact"] and np.array_equal(sums.cpu().numpy(), want[0])
                                and np.array_equal(extremes.cpu().numpy(), want[1]))

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
        common = dict(subtile=256, batch_size=64, device="cuda:0", stats=True, patches=True)
        for name, kw, side, extra in (("blocks", dict(overlap=0), "attributes", dict(attributes=True)),
                                      ("average", dict(overlap=64, blend="average"), "confidence",
                                       dict(attributes=AttributeConfig(confidence=True)))):

            def block_ms(extra):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.reps):
                    tiler.infer_tile(inf, ortho, **common, **kw, **extra)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / a.reps * 1e3

            sides = (("plain", dict()), (side, extra))
            for _, options in sides:
                block_ms(options)
            times = {s: [] for s, _ in sides}
            for _ in range(a.rounds):             # alternate
                for s, options in sides:
                    times[s].append(block_ms(options))
            for s, _ in sides:
                row[f"{name}_{s}_ms"] = round(statistics.median(times[s]), 3)
        m, p, stats = tiler.infer_tile(inf, ortho, overlap=64, blend="average", return_probs=True,
                                       attributes=AttributeConfig(confidence=True), **common)
        _, host_labels, table = labelled_patches_host(m, K, PatchConfig())
        row["infer_patches"] = stats.patches.n
        row["exact"] = bool(row["exact"] and stats.attributes == patch_attributes_host(host_labels, table, ortho, m, p))
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_attributes.py: the device result and the host result differ")


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
            raise SystemExit(f"bench_attributes.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = tuple(f"{m}_{f}" for m in a.maps.split(",") for f in MAP_FIGURES) + (INFER_FIGURES if a.infer else ())
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in keys}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "C": C, "children": len(rows),
                      "exact": all(r["exact"] for r in rows),
                      **{k: rows[0][k] for k in rows[0] if k.endswith("patches")}, **med}), flush=True)


if __name__ == "__main__":
    main()
