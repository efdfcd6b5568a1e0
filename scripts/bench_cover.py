"""cover grids before the download against numpy after it: one ``--size`` x ``--size`` (2048) uint8 class map with K = 3,
97 % class 0, and a 2-zone forest mask, under three grids — 50-pixel cells at a fractional origin (10 m over 0.2 m), 500-pixel
cells, and cells of exactly one pixel at a fractional origin (the path of direct global atomics).

  kernel     ``dt_cover_grid_u8`` alone: tables already on the device, hipEvents around one launch (median of ``--iters``)
  op         all of ``ops.cover_grid``: checks, the upload of the two tables, the launch; hipEvents likewise
  host       the host route on this machine's CPU: the download of the map (``.cpu()``) and ``cover_grid_host``; host clock
  infer_tile one RGBN raster of that size through ``infer_tile(stats=True, zones=...)`` at overlap 0, with and without
             ``grid`` (the 50-pixel one) — the two sides in alternating blocks, host clock around a device synchronise

Every child asserts that the device equals the host exactly.  Every figure is taken in ``--children`` fresh processes, one
after the other; the last line is the median over them.

    python scripts/bench_cover.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K, Z = 3, 2
GRIDS = {"50px": dict(cell=50.0, origin=(-17.3, -31.85)), "500px": dict(cell=500.0, origin=(-17.3, -31.85)),
         "1px": dict(cell=1.0, origin=(0.3, -0.4))}
FIGURES = tuple(f"{what}_{g}" for g in GRIDS for what in ("kernel_us", "op_us", "host_ms")) + ("stats_ms", "stats_grid_ms")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.deployment.cover import GridConfig, cover_grid_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_cover.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size
    classes = np.where(rng.random((n, n)) < 0.97, 0, rng.integers(1, K, (n, n))).astype(np.uint8)
    forest = (rng.random((n, n)) < 0.4).astype(np.uint8)
    dc, dz = torch.from_numpy(classes).to(dev), torch.from_numpy(forest).to(dev)

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

    row = {"what": "child", "size": n, "K": K, "Z": Z, "exact": True}
    lib = _lib.load()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, spec in GRIDS.items():
        _, yq, _, xq = GridConfig(**spec).edges((n, n))
        gy, gx = len(yq) - 1, len(xq) - 1
        want, _ = cover_grid_host(classes, forest, K, Z, yq, xq)
        got, flag = ops.cover_grid(dc, dz, K, Z, yq, xq)
        assert np.array_equal(got.cpu().numpy(), want) and int(flag) == 0, name          # exact agreement, every child
        tables = torch.from_numpy(np.concatenate([yq, xq]).astype(np.int32)).to(dev)
        sums = torch.zeros((gy, gx, Z, K), dtype=torch.int64, device=dev)

        def kernel():
            _lib.check(lib.dt_cover_grid_u8(dc.data_ptr(), dz.data_ptr(), n, n, K, Z, tables.data_ptr(), gy,
                                            tables[gy + 1:].data_ptr(), gx, sums.data_ptr(), err.data_ptr(), _lib.stream()),
                       "dt_cover_grid_u8")

        kernel_us, op_us = [], []
        for _ in range(3):                    # alternate, so that both see the same machine
            kernel_us.append(event_us(kernel))
            op_us.append(event_us(lambda: ops.cover_grid(dc, dz, K, Z, yq, xq, sums=sums, err=err)))
        row[f"kernel_us_{name}"] = round(statistics.median(kernel_us), 2)
        row[f"op_us_{name}"] = round(statistics.median(op_us), 2)
        row[f"host_ms_{name}"] = round(host_ms(lambda: cover_grid_host(dc.cpu().numpy(), forest, K, Z, yq, xq)), 3)
        row[f"cells_{name}"] = [gy, gx]

    class Inf:      # PyTorchInference's device entry points on a freshly initialised model (no checkpoint file needed)
        in_channels, classes = 3, K

        def __init__(self):
            self.m = UNetHIP(in_channels=3, classes=K)
            self.m.reset_parameters(seed=0)
            self.m.to(dev).eval()

        def run_blocks(self, raster, d, first, count):
            x = ops.split_normalize_u8(raster, d, first, count, MEAN, STD, 3)
            return self.m.predict_classes(x, dtype="uint8", nhwc=True)

    inf = Inf()
    ortho = rng.integers(0, 256, (4, n, n), dtype=np.uint8)
    grid = GridConfig(**GRIDS["50px"])
    sides = (("stats_ms", dict()), ("stats_grid_ms", dict(grid=grid)))

    def block_ms(extra):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            out = tiler.infer_tile(inf, ortho, subtile=256, batch_size=64, device="cuda:0", stats=True, zones=forest, **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.reps * 1e3, out

    for _, extra in sides:
        ms, out = block_ms(extra)
    _, yq, _, xq = grid.edges((n, n))
    assert np.array_equal(out[1].grid.sums, cover_grid_host(out[0], forest, K, Z, yq, xq)[0])
    times = {key: [] for key, _ in sides}
    for _ in range(a.rounds):                 # alternate
        for key, extra in sides:
            times[key].append(block_ms(extra)[0])
    for key, _ in sides:
        row[key] = round(statistics.median(times[key]), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
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
    print(json.dumps({"what": "median", "size": a.size, "K": K, "Z": Z, "children": len(rows),
                      "exact": all(r["exact"] for r in rows), **med}), flush=True)


if __name__ == "__main__":
    main()
