"""crown-level validation curves (``ops.object_histogram``, ``validate(objects=...)``) on one MI355X: ``--batch`` (32) images of
``--size`` x ``--size`` (512) with K = 2 and ``L = 0.3``.  Maps: ``cover`` — the ~3 % dilated-seed map of
``bench_patches.py`` as the prediction against a copy shifted by (1, 1) pixels as the target (most crowns match); ``single``
— one plane-sized patch against itself (every run merges into ONE vote word per image: the contention case);
``checker`` — the 4-connected checkerboard against a full target (every second pixel a patch of its own, one crown per
image).

  launches    hipEvents around every launch of ``ops.object_histogram`` (median of ``--iters`` calls): ``planes``
              (``dt_object_planes``), ``label_pred`` / ``label_target`` (``ops.label_patches``), ``areas_target``
              (``ops.patch_areas``), ``zero`` (the one memset of the workspace), ``support`` (``dt_patch_support``), ``vote``,
              ``inter``, ``targets`` and ``histogram`` (the four launches of ``csrc/objects.hip`` after the planes)
  total       all of ``ops.object_histogram`` (allocations included), events around the call
  host        ``object_histogram_host`` on the downloaded ``q``: the route without this path
  validate    one REPLAYED validation batch (``--val-batch`` x 3 x ``--val-size``^2, fp32, graph=True) with ``curves=True``
              alone — the path of the parent commit — against the same batch with ``objects=`` as well: the two captured
              graphs, events around ``graph.replay()``

The sides of every comparison alternate in ``--rounds`` blocks.  Every child asserts that the device histogram equals the
host's exactly, on every map and in the validation epoch.  Every figure is taken in ``--children`` fresh processes, one after
the other, each under its own time limit; the first child that fails ends the measurement; the last line is the median
over them.  Nothing is gated on these numbers.

    python scripts/bench_objects.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

K = 2
LOW = 0.3
MAPS = ("cover", "single", "checker")
STEPS = ("planes", "label_pred", "label_target", "areas_target", "zero", "support", "vote", "inter", "targets", "histogram")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from bench_patches import cover_map
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.loss.objects import ObjectCurves, ObjectSweep, object_histogram_host
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer

    if not torch.cuda.is_available():
        raise SystemExit("bench_objects.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    B, n = a.batch, a.size

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

    def quantised(candidates):
        """uint16 [B, 2, n, n]: class 1 uniform above L on the candidates, well below elsewhere"""
        lo = int(LOW * 65535) + 1000
        q1 = np.where(candidates, rng.integers(lo, 65536, candidates.shape), rng.integers(0, 12000, candidates.shape))
        return np.stack([65535 - q1, q1], axis=1).astype(np.uint16)

    row = {"what": "child", "batch": B, "size": n, "K": K, "exact": True}
    yy, xx = np.mgrid[0:n, 0:n]
    for name in a.maps.split(","):
        if name == "cover":
            few = np.stack([cover_map(n, rng) > 0 for _ in range(min(B, 4))])
            candidates, conn = few[np.arange(B) % len(few)], 8
            target = np.roll(candidates, (1, 1), axis=(1, 2)).astype(np.int64)
        elif name == "single":
            candidates, conn = np.ones((B, n, n), bool), 8
            target = np.ones((B, n, n), dtype=np.int64)
        elif name == "checker":
            candidates, conn = np.broadcast_to((yy + xx) % 2 == 1, (B, n, n)), 4
            target = np.ones((B, n, n), dtype=np.int64)
        else:
            raise SystemExit(f"bench_objects.py: unknown map {name!r} ({', '.join(MAPS)})")
        sweep = ObjectSweep({1: LOW}, connectivity=conn, min_pixels=2 if name == "cover" else 0)
        q_host = quantised(candidates)
        q, tgt = torch.from_numpy(q_host).to(dev), torch.from_numpy(np.ascontiguousarray(target)).to(dev)
        hist, targets, err = ops.object_histogram(q, tgt, sweep)
        t = time.perf_counter()
        down = q.cpu().numpy()
        row[f"{name}_download_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        t = time.perf_counter()
        want = object_histogram_host(down, target, sweep)
        row[f"{name}_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        row["exact"] = bool(row["exact"] and np.array_equal(hist.cpu().numpy(), want[0])
                            and np.array_equal(targets.cpu().numpy(), want[1]) and int(err.cpu()) == want[2])
        row[f"{name}_patches"], row[f"{name}_matched"] = int(want[0].sum()), int(want[0][:, 1].sum())
        row[f"{name}_crowns"] = int(want[1].sum())

        per_step = {s: [] for s in STEPS}

        def timed(step, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            per_step[step].append((e0, e1))
            return out

        totals = []
        for _ in range(a.rounds):
            totals.append(event_us(lambda: ops.object_histogram(q, tgt, sweep, hist=hist, targets=targets, err=err)))
            for it in range(a.iters):
                ops.object_histogram(q, tgt, sweep, hist=hist, targets=targets, err=err, _timed=timed)
        torch.cuda.synchronize()
        row[f"{name}_total_us"] = round(statistics.median(totals), 2)
        for s in STEPS:
            row[f"{name}_{s}_us"] = round(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in per_step[s]), 2)
        del q, tgt, hist, targets, down
        torch.cuda.empty_cache()

    # ---- one replayed validation batch: curves=True alone (the parent commit's path) against curves=True + objects
    if a.validate:
        torch.manual_seed(0)
        model = UNetHIP(in_channels=3, classes=K)
        model.reset_parameters(seed=0)
        tr = HipTrainer(model.to(dev), precision="fp32", losses=("GDICE", "FOCAL"), graph=True)
        img, mask = synth_batch(a.val_batch, a.val_size, a.val_size, 3, K, seed=3, p_fg=0.03)
        batches = [(img.to(dev), mask.to(dev), None, torch.ones_like(mask).to(dev))]
        sweep = ObjectSweep({1: LOW}, min_pixels=2)
        for _ in range(3):                                       # two eager batches, then the capture
            tr.validate(batches, curves=True)
            val = tr.validate(batches, curves=True, objects=sweep)
        replays = dict(zip(tr._val_replays.keys(), tr._val_replays.values()))
        sides = {"curves": next(r for k, r in replays.items() if k[-1] is True),
                 "objects": next(r for k, r in replays.items() if k[-1] == ("objects",) + sweep._key())}
        assert all(r.captured for r in sides.values())
        times = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, r in sides.items():
                times[s].append(event_us(r.graph.replay))
        for s in sides:
            row[f"validate_{s}_us"] = round(statistics.median(times[s]), 2)
        _, _, q = ops.prob_histogram(tr.model.predict_logits(batches[0][0], precision="fp32"), batches[0][1], logits=True,
                                     want_q=True)
        want = object_histogram_host(q.cpu().numpy(), batches[0][1].cpu().numpy(), sweep)
        row["exact"] = bool(row["exact"] and val["objects"] == ObjectCurves(want[0], want[1], sweep))
        row["validate_patches"], row["validate_crowns"] = int(want[0].sum()), int(want[1].sum())
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_objects.py: the device result and the host result differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--maps", default=",".join(MAPS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--validate", type=int, default=1, help="0 leaves the validation batch out")
    ap.add_argument("--val-batch", type=int, default=32)
    ap.add_argument("--val-size", type=int, default=256)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("batch", "size", "maps", "iters", "rounds", "validate", "val_batch", "val_size"):
            cmd += [f"--{name.replace('_', '-')}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_objects.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = [k for k in rows[0] if k.endswith(("_us", "_ms"))]
    print(json.dumps({"what": "median", "children": len(rows), "exact": all(r["exact"] for r in rows), "batch": rows[0]["batch"],
                      "size": rows[0]["size"], **{k: round(statistics.median(r[k] for r in rows), 3) for k in keys}}),
          flush=True)


if __name__ == "__main__":
    main()
