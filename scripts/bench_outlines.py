"""dead-tree patch outlines traced before the download against the host tracer after it: one ``--size`` x ``--size`` (2048)
uint8 class map with K = 3, about 3 % dead cover drawn as dilated random seeds ("cover"), and one raster-sized patch
("full") — the maps of ``bench_patches.py``.  ``--maps cover,full,checker`` adds the 0 / 1 checkerboard: under
connectivity 8 one patch with the most edges a raster can have, ``E = 2 h w`` (8.4 M at 2048², 268 MB of jump state).

  trace      all of ``ops.patch_outlines`` on a label plane in HBM: the launches, the two scalar read-backs, the ring sort
             and the download of the four ``PolygonSet`` arrays, hipEvents around it (median of ``--iters``); ``jump`` is
             the pointer-jumping launches alone (``dt_outline_jump`` on a linked state), ``count`` the first launch alone
  host       ``polygonize_host`` on the downloaded map with its label plane given (host_trace_ms) and from the class map
             alone (host_all_ms: scipy labelling + trace), host clock; ``download_ms`` is the map's D2H copy, which the
             host route needs and the device route does not
  infer_tile one RGBN raster of that size through ``infer_tile(stats=True, patches=True)`` at overlap 0 and at
             ``overlap=64, blend="average"``, without and with ``outlines=True`` — the sides in alternating blocks, host
             clock around a device synchronise

Every figure is taken in ``--children`` fresh processes, one after the other, each under its own time limit; the last line
is the median over them.

    python scripts/bench_outlines.py
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
MAP_FIGURES = ("count_us", "jump_us", "trace_ms", "download_ms", "host_trace_ms", "host_all_ms")
INFER_FIGURES = ("blocks_patches_ms", "blocks_outlines_ms", "average_patches_ms", "average_outlines_ms", "infer_host_all_ms")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.outlines import polygonize_host
    from deadtrees_amd.deployment.patches import label_patches_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_outlines.py measures on an MI355X: no HIP device here")
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

    def same(p, q):
        return all(np.array_equal(getattr(p, f), getattr(q, f)) for f in ("xy", "ring_offsets", "ring_polygon", "values"))

    row = {"what": "child", "size": n, "K": K, "exact": True}
    lib, st = _lib.load(), _lib.stream()
    for name in a.maps.split(","):
        if name == "cover":
            classes = cover_map(n, rng)
        elif name == "full":
            classes = np.ones((n, n), np.uint8)
        elif name == "checker":
            classes = np.ascontiguousarray((np.add.outer(np.arange(n), np.arange(n)) & 1).astype(np.uint8))
        else:
            raise SystemExit(f"bench_outlines.py: unknown map {name!r} (cover, full, checker)")
        dc = torch.from_numpy(classes).to(dev)
        labels, _ = ops.label_patches(dc, K)
        host_labels = label_patches_host(classes, K)
        got, want = ops.patch_outlines(labels, dc), polygonize_host(classes, K, labels=host_labels)
        row["exact"] = bool(row["exact"] and same(got, want))
        row[f"{name}_polygons"], row[f"{name}_rings"], row[f"{name}_vertices"] = len(got), len(got.ring_polygon), len(got.xy)

        # the first launch and the pointer-jumping rounds alone, on buffers of their own
        counts = torch.empty((-(-n * n // ops.OUTLINE_CHUNK), 2), dtype=torch.int32, device=dev)
        lib.dt_outline_count(labels.data_ptr(), n, n, counts.data_ptr(), st)
        scan = torch.cumsum(counts, 0, dtype=torch.int32)
        E = int(scan[-1, 0])
        row[f"{name}_edges"] = E
        chunk_first = (scan[:, 0] - counts[:, 0]).contiguous()
        first = torch.empty(n * n, dtype=torch.int32, device=dev)
        edges = torch.empty(E, dtype=torch.int32, device=dev)
        linked = torch.empty((E, 4), dtype=torch.int32, device=dev)
        state = torch.empty((2, E, 4), dtype=torch.int32, device=dev)
        head = torch.empty(E, dtype=torch.uint8, device=dev)
        lib.dt_outline_edges(labels.data_ptr(), n, n, 8, chunk_first.data_ptr(), E, first.data_ptr(), edges.data_ptr(),
                             linked.data_ptr(), st)
        host = torch.empty((n, n), dtype=torch.uint8, pin_memory=True)

        def download():
            host.copy_(dc, non_blocking=True)

        figures = {f: [] for f in ("count_us", "jump_us", "trace_ms", "download_ms")}
        for _ in range(3):                    # alternate, so that all see the same machine
            figures["count_us"].append(event_us(lambda: lib.dt_outline_count(labels.data_ptr(), n, n, counts.data_ptr(), st)))
            figures["jump_us"].append(event_us(lambda: lib.dt_outline_jump(state[0].data_ptr(), state[1].data_ptr(), E,
                                                                           head.data_ptr(), st),
                                               setup=lambda: state[0].copy_(linked)))
            figures["trace_ms"].append(event_us(lambda: ops.patch_outlines(labels, dc)) / 1e3)
            figures["download_ms"].append(event_us(download) / 1e3)
        for f, v in figures.items():
            row[f"{name}_{f}"] = round(statistics.median(v), 3 if f.endswith("ms") else 2)
        row[f"{name}_host_trace_ms"] = round(host_ms(lambda: polygonize_host(classes, K, labels=host_labels)), 3)
        row[f"{name}_host_all_ms"] = round(host_ms(lambda: polygonize_host(classes, K)), 3)

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
        sides = (("_patches", dict()), ("_outlines", dict(outlines=True)))

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
                                outlines=True)
    row["infer_polygons"], row["infer_vertices"] = len(stats.outlines), len(stats.outlines.xy)
    row["infer_host_all_ms"] = round(host_ms(lambda: polygonize_host(m, K)), 3)
    row["exact"] = bool(row["exact"] and same(stats.outlines, polygonize_host(m, K)))
    print(json.dumps(row), flush=True)


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
            raise SystemExit(f"bench_outlines.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = tuple(f"{m}_{f}" for m in a.maps.split(",") for f in MAP_FIGURES) + INFER_FIGURES
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in keys}
    print(json.dumps({"what": "median", "size": a.size, "K": K, "children": len(rows),
                      "exact": all(r["exact"] for r in rows),
                      **{k: rows[0][k] for k in rows[0] if k.endswith(("_edges", "_polygons", "_rings", "_vertices"))},
                      **med}), flush=True)


if __name__ == "__main__":
    main()
