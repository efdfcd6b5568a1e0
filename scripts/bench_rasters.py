"""training pools from ortho rasters: per ``--size`` x ``--size`` (2048) rgbn raster with mask and land-use map, cut into
``--tile`` (256) sub-tiles.

  kernel        census launch + cut launch of ``ops.raster_cut`` on a raster already in HBM, hipEvents (median of
                ``--iters``); every sub-tile is written
  host          ``cut_raster_host`` on the same arrays, host clock
  from_rasters  ``DevicePool.from_rasters(select="valid")`` over ``--rasters`` rasters in memory, end to end (staging,
                upload, census, read-back, cut), per raster
  shard         ``DevicePool([shard])`` of a shard that holds the same sub-tiles as uncompressed TIFFs (what the reference's
                preprocessing hands over), per raster; the shard is written once, outside the clock

The two sides of each pair run in alternating blocks.  Every figure is taken in ``--children`` fresh processes, one after the
other; the last line is the median over them.

    python scripts/bench_rasters.py
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tarfile
import tempfile
import time

FIGURES = ("kernel_us", "host_ms", "from_rasters_ms", "shard_ms")


def _write_shard(path, samples):
    import numpy as np
    from PIL import Image

    def tiff(arr):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(arr)).save(buf, format="TIFF")
        return buf.getvalue()

    with tarfile.open(path, "w") as tar:
        for key, img, mask, lu, frac in samples:
            for field, data in (("rgbn.tif", tiff(img)), ("mask.tif", tiff(mask)), ("lu.tif", tiff(lu)),
                                ("txt", repr(frac).encode())):
                info = tarfile.TarInfo(f"{key}.{field}")
                info.size = len(data)
                tar.addfile(info, io.BytesIO(data))


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.pool import DevicePool
    from deadtrees_amd.data.rasters import cut_raster_host, subtile_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_rasters.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    S, t = a.size, a.tile
    n = (S // t) ** 2
    items = []
    for r in range(a.rasters):
        rgbn = rng.integers(0, 256, (4, S, S), dtype=np.uint8)
        mask = (rng.random((S, S)) < 0.03).astype(np.uint8)
        lu = rng.integers(0, 3, (S, S)).astype(np.uint8)
        items.append((f"ortho_{r}", rgbn, mask, lu))

    _, rgbn, mask, lu = items[0]
    d = [torch.from_numpy(x).to(dev) for x in (rgbn, mask, lu)]
    out = (torch.empty((n, t, t, 4), dtype=torch.uint8, device=dev), torch.empty((n, t, t), dtype=torch.uint8, device=dev),
           torch.empty((n, t, t), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
    slot = torch.arange(n, dtype=torch.int32, device=dev)
    census = torch.empty((n, 16), dtype=torch.int64, device=dev)

    def kernel():
        ops.raster_cut(*d, S, t, census=census)
        ops.raster_cut(*d, S, t, slot=slot, out=out, census=False)

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

    kernel()
    want = cut_raster_host(rgbn, mask, lu, S, t)
    exact = bool(np.array_equal(census.cpu().numpy(), want[4]) and np.array_equal(out[0].cpu().numpy(), want[0])
                 and np.array_equal(out[1].cpu().numpy(), want[1]) and np.array_equal(out[2].cpu().numpy(), want[2])
                 and np.array_equal(out[3].cpu().numpy().view(np.uint64), want[3]))
    kernel_us, host_ms = [], []
    for _ in range(a.rounds):                 # alternate
        kernel_us.append(event_us(kernel))
        host_ms.append(clock_ms(lambda: cut_raster_host(rgbn, mask, lu, S, t), 1))

    with tempfile.TemporaryDirectory() as tmp:
        samples = []
        for key, rgbn, mask, lu in items:
            images, masks, lus, _, c = cut_raster_host(rgbn, mask, lu, S, t)
            samples += [(name, images[int(name[-3:])], masks[int(name[-3:])], lus[int(name[-3:])], frac)
                        for name, frac, _ in subtile_table(key, c, t)]
        shard = os.path.join(tmp, "valid.tar")
        _write_shard(shard, samples)
        a_pool = DevicePool.from_rasters(items, t, S, select="valid", device=dev)
        b_pool = DevicePool([shard], device=dev)
        same = bool(torch.equal(a_pool.images, b_pool.images) and torch.equal(a_pool.masks, b_pool.masks)
                    and torch.equal(a_pool.sums, b_pool.sums) and a_pool.stats == b_pool.stats)
        del a_pool, b_pool
        ours, theirs = [], []
        for _ in range(a.rounds):             # alternate
            ours.append(clock_ms(lambda: DevicePool.from_rasters(items, t, S, select="valid", device=dev), 1) / a.rasters)
            theirs.append(clock_ms(lambda: DevicePool([shard], device=dev), 1) / a.rasters)
    print(json.dumps({"what": "child", "size": S, "tile": t, "rasters": a.rasters, "exact": exact, "same_pool": same,
                      "kernel_us": round(statistics.median(kernel_us), 2), "host_ms": round(statistics.median(host_ms), 3),
                      "from_rasters_ms": round(statistics.median(ours), 3),
                      "shard_ms": round(statistics.median(theirs), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=256)
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
        for name in ("size", "tile", "rasters", "iters", "rounds"):
            cmd += [f"--{name}", str(getattr(a, name))]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in FIGURES}
    print(json.dumps({"what": "median", "size": a.size, "tile": a.tile, "children": len(rows),
                      "exact": all(r["exact"] for r in rows), "same_pool": all(r["same_pool"] for r in rows), **med}),
          flush=True)


if __name__ == "__main__":
    main()
