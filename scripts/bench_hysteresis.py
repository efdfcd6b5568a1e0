"""patch-wise decisions (hysteresis and confidence filter) on one MI355X against the pixel rule and against the host route:
``--size`` x ``--size`` (2048) probabilities with K = 2, ``L = 0.3``, ``T = 0.6`` and, for the ``*_m`` figures, ``M = 0.45``.
Maps: ``cover`` — the ~3 % dilated-seed map of ``bench_patches.py`` (candidates on the crowns, a pixel at T in most of them);
``single`` — one raster-sized patch (every run adds into ONE root: the atomic-contention case); ``checker`` — the
4-connected checkerboard (every second pixel a patch of its own: one write per quantity and labelled pixel).

  launches    the three new launches alone, hipEvents around each (median of ``--iters``): ``candidates``
              (``dt_decide_candidates_u8``), ``support`` / ``support_m`` (``dt_patch_support`` without / with the sum and area
              planes; the planes are zeroed outside the events) and ``reject`` / ``reject_m`` (``dt_reject_patches_u8``; the
              candidates are restored outside the events).  ``*_floor_us`` next to each: the bytes the launch cannot avoid
              — candidates 4 (K - 1) + 3 per pixel; support 4 per pixel + 2 per labelled pixel; reject 4 per pixel + 1 per
              labelled pixel — at the 6.3 TB/s a streaming copy reaches on this chip
  decide      all of ``ops.decide_patchwise`` (allocations, the label launches and the four steps) against
              ``ops.decide_classes`` at T, the pixel rule, on the ``cover`` probabilities
  infer_tile  one RGB raster at ``overlap=64, blend="average"`` with a plain and with a patch-wise decision, host clock around
              a device synchronise
  host        the route without this path: the download of the fp32 probabilities and ``decide_patchwise_host`` on them

The sides of every comparison alternate in ``--rounds`` blocks.  Every child asserts that the device maps equal the host
rule exactly.  Every figure is taken in ``--children`` fresh processes, one after the other, each under its own time limit;
the first child that fails ends the measurement; the last line is the median over them.  Nothing is gated on these
numbers.

    python scripts/bench_hysteresis.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HBM_BYTES_PER_US = 6.3e6           # 6.3 TB/s: a float4 copy on this chip
K = 2
LOW, HIGH, MEAN = 0.3, 0.6, 0.45
MAPS = ("cover", "single", "checker")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ctypes
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN as BAND_MEAN, STD as BAND_STD
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.loss.curves import Decision, decide_host, decide_patchwise_host
    from deadtrees_amd.network.unet import UNetHIP

    if not torch.cuda.is_available():
        raise SystemExit("bench_hysteresis.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n = a.size
    lib, st = _lib.load(), _lib.stream()

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

    def probabilities(candidates):
        """fp32 [2, n, n]: class 1 uniform in [L + 0.02, T + 0.02) on the candidates, below 0.2 elsewhere"""
        p1 = np.where(candidates, rng.uniform(LOW + 0.02, HIGH + 0.02, (n, n)), rng.uniform(0.0, 0.2, (n, n))).astype(np.float32)
        return np.stack([1 - p1, p1]).astype(np.float32)

    row = {"what": "child", "size": n, "K": K, "exact": True, "span": ops.SUPPORT_SPAN}
    yy, xx = np.mgrid[0:n, 0:n]
    u16 = ctypes.c_uint16 * K
    host = {}
    for name in a.maps.split(","):
        if name == "cover":
            candidates, conn = cover_map(n, rng) > 0, 8
        elif name == "single":
            candidates, conn = np.ones((n, n), bool), 8
        elif name == "checker":
            candidates, conn = (yy + xx) % 2 == 1, 4
        else:
            raise SystemExit(f"bench_hysteresis.py: unknown map {name!r} ({', '.join(MAPS)})")
        p = probabilities(candidates)
        probs = torch.from_numpy(p).to(dev)
        plain = Decision({1: HIGH}, low={1: LOW}, connectivity=conn)
        filtered = Decision({1: HIGH}, low={1: LOW}, min_confidence={1: MEAN}, connectivity=conn)
        if a.check:
            for d in (plain, filtered):
                row["exact"] = bool(row["exact"] and np.array_equal(ops.decide_patchwise(probs, d).cpu().numpy(),
                                                                    decide_patchwise_host(p, d)))
        if name == "cover":
            host = {"p": p, "probs": probs, "plain": plain, "filtered": filtered}
        low, high, conf = u16(*plain.low_u16().tolist()), u16(*plain.thresholds_u16().tolist()), \
            u16(*filtered.min_confidence_u16().tolist())
        cand = torch.empty((n, n), dtype=torch.uint8, device=dev)
        q_own = torch.empty((n, n), dtype=torch.uint16, device=dev)
        work = torch.empty_like(cand)
        qmax = torch.zeros(n * n, dtype=torch.int32, device=dev)
        qsum = torch.zeros(n * n, dtype=torch.int64, device=dev)
        area = torch.zeros(n * n, dtype=torch.int32, device=dev)

        def candidates_launch():
            _lib.check(lib.dt_decide_candidates_u8(probs.data_ptr(), low, cand.data_ptr(), q_own.data_ptr(), K, n * n, st),
                       "dt_decide_candidates_u8")

        candidates_launch()
        labels, _ = ops.label_patches(cand, K, conn)
        labelled = int((labels > 0).sum())

        def support(with_sums):
            _lib.check(lib.dt_patch_support(labels.data_ptr(), q_own.data_ptr(), n, n, qmax.data_ptr(),
                                            qsum.data_ptr() if with_sums else None, area.data_ptr() if with_sums else None, st),
                       "dt_patch_support")

        def zero():
            qmax.zero_(), qsum.zero_(), area.zero_()

        def reject(with_sums):
            _lib.check(lib.dt_reject_patches_u8(work.data_ptr(), labels.data_ptr(), qmax.data_ptr(),
                                                qsum.data_ptr() if with_sums else None, area.data_ptr() if with_sums else None,
                                                high, conf if with_sums else None, K, n, n, st), "dt_reject_patches_u8")

        sides = {"candidates": (candidates_launch, None), "support": (lambda: support(False), zero),
                 "support_m": (lambda: support(True), zero)}
        times = {s: [] for s in ("candidates", "support", "support_m", "reject", "reject_m")}
        for _ in range(a.rounds):
            for s, (fn, before) in sides.items():
                times[s].append(event_us(fn, before))
            zero()
            support(True)                                   # the planes the rejection reads
            for s, with_sums in (("reject", False), ("reject_m", True)):
                times[s].append(event_us(lambda: reject(with_sums), lambda: work.copy_(cand)))
        for s, v in times.items():
            row[f"{name}_{s}_us"] = round(statistics.median(v), 2)
        row[f"{name}_labelled"] = labelled
        row[f"{name}_candidates_floor_us"] = round(n * n * (4 * (K - 1) + 3) / HBM_BYTES_PER_US, 2)
        row[f"{name}_support_floor_us"] = round((4 * n * n + 2 * labelled) / HBM_BYTES_PER_US, 2)
        row[f"{name}_reject_floor_us"] = round((4 * n * n + labelled) / HBM_BYTES_PER_US, 2)
        del probs, cand, q_own, work, qmax, qsum, area, labels
        torch.cuda.empty_cache()

    # ---- the whole decision against the pixel rule, and the host route
    if host:
        probs, out = host["probs"], torch.empty((n, n), dtype=torch.uint8, device=dev)
        pixel = Decision({1: HIGH})
        sides = {"classes": lambda: ops.decide_classes(probs, pixel, out=out),
                 "patchwise": lambda: ops.decide_patchwise(probs, host["plain"], out=out),
                 "patchwise_m": lambda: ops.decide_patchwise(probs, host["filtered"], out=out)}
        times = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():
                times[s].append(event_us(fn))
        for s in sides:
            row[f"decide_{s}_us"] = round(statistics.median(times[s]), 2)
        if a.check:
            row["exact"] = bool(row["exact"] and np.array_equal(ops.decide_classes(probs, pixel).cpu().numpy(),
                                                                decide_host(host["p"], pixel)))
        t = time.perf_counter()
        down = probs.cpu().numpy()
        row["host_download_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        for s in ("plain", "filtered"):
            t = time.perf_counter()
            decide_patchwise_host(down, host[s])
            row[f"host_{s}_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        del probs, out, down
        host.clear()
        torch.cuda.empty_cache()

    # ---- infer_tile with a plain and with a patch-wise decision
    class Inf:      # PyTorchInference's device entry points on a freshly initialised model (no checkpoint file needed)
        in_channels, classes = 3, 2

        def __init__(self):
            torch.manual_seed(0)
            self.m = UNetHIP().to("cuda")
            self.m.eval()

        def run_windows(self, raster, d, overlap, first, count, want="classes", precision="fp32", views=None):
            x = ops.window_normalize_u8(raster, d, overlap, first, count, BAND_MEAN, BAND_STD, 3, views=views)
            if want == "classes":
                return self.m.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
            return self.m.predict_logits(x, precision=precision, nhwc=True)

    if a.infer:
        inf = Inf()
        ortho = rng.integers(0, 256, (3, n, n), dtype=np.uint8)
        common = dict(subtile=256, batch_size=64, device="cuda:0", overlap=64, blend="average")
        _, probs = tiler.infer_tile(inf, ortho, return_probs=True, **common)
        q1 = np.sort(probs[1].reshape(-1))
        low, high = float(q1[int(0.5 * q1.size)]), float(q1[int(0.9 * q1.size)])      # quantiles of this model's output
        low, high = min(max(low, 1e-4), 1.0), min(max(high, 1e-4), 1.0)
        patchwise = Decision({1: max(low, high)}, low={1: low}, min_confidence={1: low})
        sides = (("plain", dict(decision=Decision({1: max(low, high)}))), ("patchwise", dict(decision=patchwise)))

        def block_ms(extra):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.reps):
                tiler.infer_tile(inf, ortho, **common, **extra)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / a.reps * 1e3

        for _, options in sides:
            block_ms(options)
        times = {s: [] for s, _ in sides}
        for _ in range(a.rounds):
            for s, options in sides:
                times[s].append(block_ms(options))
        for s, _ in sides:
            row[f"infer_{s}_ms"] = round(statistics.median(times[s]), 3)
        got = tiler.infer_tile(inf, ortho, **common, decision=patchwise)
        row["exact"] = bool(row["exact"] and np.array_equal(got, decide_patchwise_host(probs, patchwise)))
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_hysteresis.py: the device result and the host result differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--maps", default=",".join(MAPS))
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
        for name in ("size", "maps", "iters", "reps", "rounds", "check", "infer"):
            cmd += [f"--{name}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_hysteresis.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = [k for k in rows[0] if k.endswith(("_us", "_ms"))]
    print(json.dumps({"what": "median", "children": len(rows), "exact": all(r["exact"] for r in rows), "size": rows[0]["size"],
                      **{k: round(statistics.median(r[k] for r in rows), 3) for k in keys}}),
          flush=True)


if __name__ == "__main__":
    main()
