"""masks and zones from polygons: burning a ``--size`` x ``--size`` (2048) uint8 plane on the device against burning it on
the host and uploading it, on two workloads.

  crowns        about ``--crowns`` (500) crown-sized polygons (stars of 8 .. 40 vertices, 10 .. 40 pixels across, values 1 / 2)
  region        one raster-sized polygon of about ``--vertices`` (10^4) vertices with a hole

  kernel_us     the one launch of ``ops.rasterize_polygons`` on tables already in HBM, hipEvents (median of ``--iters``)
  device_ms     ``rasterize(polys, shape, device)``: table upload + launch + synchronisation, host clock
  host_ms       ``rasterize_host`` + the h * w upload the device path replaces, host clock
  from_rasters  ``DevicePool.from_rasters(select="valid")`` over ``--rasters`` rasters in memory with the crowns as masks, per
                raster: masks as ``PolygonSet`` (burnt into the staged buffer) against masks as burnt arrays (uploaded; the
                host burn is outside this clock: it is the preprocessing the arrays stand for)

The two sides of each pair run in alternating blocks.  Every figure is taken in ``--children`` fresh processes, one after the
other; the last line is the median over them.

    python scripts/bench_polygons.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

FIGURES = ("crowns_kernel_us", "crowns_device_ms", "crowns_host_ms", "region_kernel_us", "region_device_ms",
           "region_host_ms", "from_rasters_polygons_ms", "from_rasters_arrays_ms")


def crowns(rng, n, S):
    import numpy as np
    out = []
    for i in range(n):
        k = int(rng.integers(8, 41))
        ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, k))
        rad = rng.uniform(5.0, 20.0) * rng.uniform(0.6, 1.0, k)
        cx, cy = rng.uniform(0, S, 2)
        out.append((1 + i % 2, np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1), []))
    return out


def region(rng, nv, S):
    import numpy as np

    def ring(k, radius):
        ang = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
        rad = radius * S / 2 * (1.0 + 0.2 * np.sin(9 * ang) + 0.02 * rng.uniform(-1.0, 1.0, k))
        return np.stack([S / 2 + rad * np.cos(ang), S / 2 + rad * np.sin(ang)], axis=1)

    return [(1, ring(nv - nv // 5, 0.8), [ring(nv // 5, 0.3)])]


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.polygons import PolygonSet, rasterize, rasterize_host
    from deadtrees_amd.data.pool import DevicePool

    if not torch.cuda.is_available():
        raise SystemExit("bench_polygons.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    S = a.size
    sets = {"crowns": PolygonSet.from_polygons(crowns(rng, a.crowns, S)),
            "region": PolygonSet.from_polygons(region(rng, a.vertices, S))}

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

    def clock_ms(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    row = {"what": "child", "size": S, "exact": True}
    for name, ps in sets.items():
        edges, table = (torch.from_numpy(t.copy()).to(dev) for t in ps.tables())
        plane = torch.empty((S, S), dtype=torch.uint8, device=dev)
        want = rasterize_host(ps, S, S)
        row["exact"] = row["exact"] and bool(np.array_equal(ops.rasterize_polygons(edges, table, (S, S), out=plane).cpu().numpy(),
                                                            want))
        row[f"{name}_polygons"], row[f"{name}_edges"] = len(ps), int(edges.shape[0])
        row[f"{name}_burnt"] = round(float(np.count_nonzero(want)) / want.size, 4)

        def host_side():
            plane.copy_(torch.from_numpy(rasterize_host(ps, S, S)))

        k_us, d_ms, h_ms = [], [], []
        for _ in range(a.rounds):                 # alternate
            k_us.append(event_us(lambda: ops.rasterize_polygons(edges, table, (S, S), out=plane)))
            d_ms.append(clock_ms(lambda: rasterize(ps, (S, S), out=plane), 5))
            h_ms.append(clock_ms(host_side, 1))
        row[f"{name}_kernel_us"] = round(statistics.median(k_us), 2)
        row[f"{name}_device_ms"] = round(statistics.median(d_ms), 3)
        row[f"{name}_host_ms"] = round(statistics.median(h_ms), 3)

    with_polys, with_arrays = [], []
    for r in range(a.rasters):
        rgbn = rng.integers(0, 256, (4, S, S), dtype=np.uint8)
        mask = PolygonSet.from_polygons(crowns(rng, a.crowns, S))
        with_polys.append((f"ortho_{r}", rgbn, mask, None))
        with_arrays.append((f"ortho_{r}", rgbn, rasterize_host(mask, S, S), None))
    t = a.tile
    a_pool = DevicePool.from_rasters(with_polys, t, S, select="valid", device=dev)
    b_pool = DevicePool.from_rasters(with_arrays, t, S, select="valid", device=dev)
    row["same_pool"] = bool(torch.equal(a_pool.images, b_pool.images) and torch.equal(a_pool.masks, b_pool.masks)
                            and torch.equal(a_pool.sums, b_pool.sums) and a_pool.stats == b_pool.stats)
    del a_pool, b_pool
    ours, theirs = [], []
    for _ in range(a.rounds):                     # alternate
        ours.append(clock_ms(lambda: DevicePool.from_rasters(with_polys, t, S, select="valid", device=dev), 1) / a.rasters)
        theirs.append(clock_ms(lambda: DevicePool.from_rasters(with_arrays, t, S, select="valid", device=dev), 1) / a.rasters)
    row["from_rasters_polygons_ms"] = round(statistics.median(ours), 3)
    row["from_rasters_arrays_ms"] = round(statistics.median(theirs), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--crowns", type=int, default=500)
    ap.add_argument("--vertices", type=int, default=10000)
    ap.add_argument("--rasters", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("size", "tile", "crowns", "vertices", "rasters", "iters", "rounds"):
            cmd += [f"--{name}", str(getattr(a, name))]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in FIGURES}
    print(json.dumps({"what": "median", "size": a.size, "children": len(rows), "exact": all(r["exact"] for r in rows),
                      "same_pool": all(r["same_pool"] for r in rows), **med}), flush=True)


if __name__ == "__main__":
    main()
