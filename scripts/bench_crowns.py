"""the crown split (``deployment/crowns.py``, csrc/crowns.hip) on one MI355X against the host route: ``--size`` x ``--size``
(2048) class maps with K = 3, ``CrownConfig(--core2)`` (9).  Maps: ``cover`` — the ~3 % dilated-seed map of
``bench_patches.py`` (7 x 7 crowns, some of them touching); ``single`` — one raster-sized patch (every pixel a core: no round
labels anything, every merge atomic lands on ONE seg); ``checker`` — the 4-connected checkerboard (every second pixel a patch
of its own, no cores at all: every pixel of the remainder is a seg of its own).

  launches    hipEvents around each entry point alone (median of ``--iters``): ``depth`` (``dt_patch_depth2_u8``: four
              launches, depth and cores), ``grow`` (ONE ``dt_crown_grow`` round from the cores), ``remainder``, ``merge`` (the
              planes it adds into are reset outside the events) and ``relabel``.  ``*_floor_us`` next to each: the bytes the
              launches cannot avoid per pixel — depth 15 (the class map four times, the column distances written once and read
              twice, depth and cores written), grow 9, remainder 6, merge 12 and 4 more per labelled pixel, relabel 8 and 4
              more per labelled pixel — at the 6.3 TB/s a streaming copy reaches on this chip
  split       all of ``ops.split_patches`` (allocations, the two ``label_patches``, the rounds with their read-backs), host
              clock around a device synchronise, and the number of rounds it ran
  host        the route without this path: the download of the class map and the label plane, and ``split_patches_host``
  infer_tile  one RGB raster with ``stats=True, patches=True, against=...`` with and without ``crowns`` / ``against_crowns``,
              at ``overlap=0`` and at ``overlap=64, blend="average"``, host clock around a device synchronise

The sides of every comparison alternate in ``--rounds`` blocks.  Every child asserts that the device planes equal the host's
exactly.  Every figure is taken in ``--children`` fresh processes, one after the other, each under its own time limit; the
first child that fails ends the measurement; the last line is the median over them.  Nothing is gated on these numbers.

    python scripts/bench_crowns.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HBM_BYTES_PER_US = 6.3e6           # 6.3 TB/s: a float4 copy on this chip
K = 3
MAPS = ("cover", "single", "checker")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.crowns import CrownConfig, crown_depths_host, split_patches_host
    from deadtrees_amd.deployment.patches import PatchConfig
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_crowns.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size
    lib, st = _lib.load(), _lib.stream()
    config = CrownConfig(a.core2)

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

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.reps * 1e3

    row = {"what": "child", "size": n, "K": K, "core2": a.core2, "exact": True, "group": ops.CROWN_ROUND_GROUP}
    yy, xx = np.mgrid[0:n, 0:n]
    i32 = dict(dtype=torch.int32, device=dev)
    cover = None
    for name in a.maps.split(","):
        if name == "cover":
            m, conn = cover_map(n, rng), 8
            cover = m
        elif name == "single":
            m, conn = np.ones((n, n), np.uint8), 8
        elif name == "checker":
            m, conn = ((yy + xx) % 2).astype(np.uint8), 4
        else:
            raise SystemExit(f"bench_crowns.py: unknown map {name!r} ({', '.join(MAPS)})")
        classes = torch.from_numpy(m).to(dev)
        labels, _ = ops.label_patches(classes, K, conn)
        labelled = int((labels > 0).sum())
        crowns, depth2, crown_depth, flags = ops.split_patches(classes, labels, K, conn, config)
        row[f"{name}_rounds"] = int(flags[2])
        row[f"{name}_crowns"] = int((crown_depth > 0).sum())
        if a.check:
            t = time.perf_counter()
            host_classes, host_labels = classes.cpu().numpy(), labels.cpu().numpy()
            row[f"{name}_host_download_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            t = time.perf_counter()
            want, want_depth2, converged = split_patches_host(host_classes, host_labels, K, conn, config)
            row[f"{name}_host_split_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            row["exact"] = bool(row["exact"] and np.array_equal(crowns.cpu().numpy(), want)
                                and np.array_equal(depth2.cpu().numpy(), want_depth2)
                                and np.array_equal(crown_depth.cpu().numpy(), crown_depths_host(want, want_depth2))
                                and int(flags[1]) == int(not converged) and int(flags[0]) == 0)
        del crowns, crown_depth, flags
        # ---- the launches alone
        column = torch.empty((n, n), dtype=torch.int16, device=dev)
        carry = torch.empty((-(-n // ops.CROWN_SEGMENT), n, 4), **i32)
        core = torch.empty((n, n), dtype=torch.uint8, device=dev)
        err = torch.zeros(2, **i32)

        def depth_launch():
            _lib.check(lib.dt_patch_depth2_u8(classes.data_ptr(), n, n, K, config.depth_cap2, config.min_core2,
                                              column.data_ptr(), carry.data_ptr(), depth2.data_ptr(), core.data_ptr(),
                                              err.data_ptr(), st),
                       "dt_patch_depth2_u8")

        depth_launch()
        S, _ = ops.label_patches(core, K, conn)
        grown = torch.empty_like(S)

        def grow_launch():
            _lib.check(lib.dt_crown_grow(classes.data_ptr(), S.data_ptr(), grown.data_ptr(), n, n, conn, err[1:].data_ptr(), st),
                       "dt_crown_grow")

        rem = torch.empty((n, n), dtype=torch.uint8, device=dev)

        def remainder_launch():
            _lib.check(lib.dt_crown_remainder(classes.data_ptr(), S.data_ptr(), n, n, conn, rem.data_ptr(), err[1:].data_ptr(),
                                              st),
                       "dt_crown_remainder")

        remainder_launch()
        lr, _ = ops.label_patches(rem, K, conn)
        seg = torch.empty_like(lr)
        first, depth = torch.empty(n * n, **i32), torch.empty(n * n, **i32)
        out, out_depth = torch.empty((n, n), **i32), torch.zeros(n * n, **i32)

        def merge_reset():
            seg.copy_(lr), first.fill_(2 ** 31 - 1), depth.zero_()

        def merge_launch():
            _lib.check(lib.dt_crown_merge(S.data_ptr(), seg.data_ptr(), depth2.data_ptr(), n, n, first.data_ptr(),
                                          depth.data_ptr(), st), "dt_crown_merge")

        def relabel_launch():
            _lib.check(lib.dt_crown_relabel(seg.data_ptr(), first.data_ptr(), depth.data_ptr(), n, n, out.data_ptr(),
                                            out_depth.data_ptr(), st), "dt_crown_relabel")

        sides = {"depth": (depth_launch, None), "grow": (grow_launch, err.zero_), "remainder": (remainder_launch, err.zero_),
                 "merge": (merge_launch, merge_reset)}            # a flag that is up already spares the waves their atomic
        times = {s: [] for s in (*sides, "relabel")}
        for _ in range(a.rounds):
            for s, (fn, before) in sides.items():
                times[s].append(event_us(fn, before))
            merge_reset()
            merge_launch()
            times["relabel"].append(event_us(relabel_launch))
        for s, v in times.items():
            row[f"{name}_{s}_us"] = round(statistics.median(v), 2)
        px = n * n
        for s, bytes_ in (("depth", 15 * px), ("grow", 9 * px), ("remainder", 6 * px), ("merge", 12 * px + 4 * labelled),
                          ("relabel", 8 * px + 4 * labelled)):
            row[f"{name}_{s}_floor_us"] = round(bytes_ / HBM_BYTES_PER_US, 2)
        row[f"{name}_labelled"] = labelled
        row[f"{name}_split_ms"] = round(statistics.median(
            wall_ms(lambda: ops.split_patches(classes, labels, K, conn, config)) for _ in range(a.rounds)), 3)
        del column, carry, core, S, grown, rem, lr, seg, first, depth, out, out_depth, depth2, classes, labels
        torch.cuda.empty_cache()

    # ---- infer_tile with and without crowns
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
        ortho = rng.integers(0, 256, (3, n, n), dtype=np.uint8)
        against = cover if cover is not None else cover_map(n, rng)
        common = dict(subtile=256, batch_size=64, device="cuda:0", stats=True, patches=PatchConfig(), against=against)
        paths = {"blocks": {}, "average": dict(overlap=64, blend="average")}
        sides = (("patches", {}), ("crowns", dict(crowns=config, against_crowns=config)))
        for path, extra in paths.items():
            for _, options in sides:
                tiler.infer_tile(inf, ortho, **common, **extra, **options)
            times = {s: [] for s, _ in sides}
            for _ in range(a.rounds):
                for s, options in sides:
                    times[s].append(wall_ms(lambda: tiler.infer_tile(inf, ortho, **common, **extra, **options)))
            for s, _ in sides:
                row[f"{path}_{s}_ms"] = round(statistics.median(times[s]), 3)
            plain_map, plain = tiler.infer_tile(inf, ortho, **common, **extra)
            got_map, got = tiler.infer_tile(inf, ortho, **common, **extra, crowns=config, against_crowns=config)
            row[f"{path}_patches_n"], row[f"{path}_crowns_n"] = plain.patches.n, got.patches.n
            row["exact"] = bool(row["exact"] and np.array_equal(plain_map, got_map)
                                and got.crowns.n_patches == plain.patches.n)
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_crowns.py: the device result and the host result differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--maps", default=",".join(MAPS))
    ap.add_argument("--core2", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--check", type=int, default=1, help="0 leaves the comparison with the host out")
    ap.add_argument("--infer", type=int, default=1, help="0 leaves the infer_tile figures out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "maps", "core2", "iters", "reps", "rounds", "check", "infer"):
            cmd += [f"--{name}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_crowns.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = [k for k in rows[0] if k.endswith(("_us", "_ms", "_rounds", "_crowns", "_n"))]
    print(json.dumps({"what": "median", "children": len(rows), "exact": all(r["exact"] for r in rows), "size": rows[0]["size"],
                      **{k: round(statistics.median(r[k] for r in rows), 3) for k in keys}}),
          flush=True)


if __name__ == "__main__":
    main()
