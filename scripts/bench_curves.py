"""operating points on one MI355X: the probability histogram of a validation batch, the decision kernel, and what they add
to a validation batch and to ``infer_tile``.

  histogram   ``dt_prob_histogram`` alone at B = 32, 512 x 512, K = 2 and K = 3 (probabilities, with ``lu``), hipEvents
              around it (median of ``--iters``), on three inputs: ``realistic`` — about 97 % confident background, the rest
              soft; ``uniform`` — uniform random probabilities (every lane another counter); ``one`` — every pixel in one
              counter per class (the contention case).  ``*_floor_us`` next to each: the bytes the kernel has to read
              (4 K + 16 per pixel) at the 6.3 TB/s a streaming copy reaches on this chip
  validate    one fp32 validation batch (B = 32, 512 x 512, K = 2), replayed graph: the fused evaluation head (what
              ``validate`` runs without curves) against ``curves=True`` (the unfused chain + one histogram launch)
  decide      ``dt_decide_classes_u8`` at 2048 x 2048, K = 2 and 3, and its floor (4 (K - 1) + 1 bytes per pixel)
  infer_tile  one 2048 x 2048 RGB raster at ``overlap=64, blend="average"`` with and without ``decision``, host clock around a
              device synchronise

The sides of every comparison alternate in ``--rounds`` blocks.  Every child asserts that device and host histograms and
maps agree exactly.  Every figure is taken in ``--children`` fresh processes, one after the other, each under its own
time limit; the first child that fails ends the measurement; the last line is the median over them.  Nothing is gated
on these numbers.

    python scripts/bench_curves.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HBM_BYTES_PER_US = 6.3e6           # 6.3 TB/s: a float4 copy on this chip
INPUTS = ("realistic", "uniform", "one")


def child(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from deadtrees_amd import _lib, ops
    from deadtrees_amd.data.synthetic import MEAN, STD, synth_batch
    from deadtrees_amd.deployment import tiler
    from deadtrees_amd.loss.curves import Decision, decide_host, prob_histogram_host
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer

    if not torch.cuda.is_available():
        raise SystemExit("bench_curves.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    lib, st = _lib.load(), _lib.stream()

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

    row = {"what": "child", "exact": True, "chunk": ops.CURVE_CHUNK}
    B, H, W = a.batch, a.tile, a.tile
    n = B * H * W
    lu_host = rng.integers(0, 2, (B, H, W))
    lu = torch.from_numpy(lu_host).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for K in (2, 3):
        inputs = {}
        dead = rng.random((B, H, W)) < 0.03
        soft = rng.random((B, K, H, W), dtype=np.float32)
        soft /= soft.sum(1, keepdims=True)
        confident = np.full((B, K, H, W), 0.002 / (K - 1), dtype=np.float32)
        confident[:, 0] = 0.998
        inputs["realistic"] = (np.where(dead[:, None], soft, confident), np.where(dead, rng.integers(1, K, (B, H, W)), 0))
        inputs["uniform"] = (rng.random((B, K, H, W), dtype=np.float32), rng.integers(0, K, (B, H, W)))
        one = np.zeros((B, K, H, W), dtype=np.float32)
        one[:, 0] = 1.0
        inputs["one"] = (one, np.zeros((B, H, W), dtype=np.int64))
        del soft, confident, one
        calls = {}
        for name in INPUTS:
            p, labels = inputs[name]
            src, lab = torch.from_numpy(p).to(dev), torch.from_numpy(labels.astype(np.int64)).to(dev)
            hist = torch.zeros((2, K, 2, 256), dtype=torch.int64, device=dev)
            calls[name] = (lambda src=src, lab=lab, hist=hist: lib.dt_prob_histogram(
                src.data_ptr(), lab.data_ptr(), lu.data_ptr(), hist.data_ptr(), err.data_ptr(), None, B, K, H, W, 0, st), hist)
            if a.check:
                got, _ = ops.prob_histogram(src, lab, lu)
                row["exact"] = bool(row["exact"] and np.array_equal(got.cpu().numpy(), prob_histogram_host(p, labels, lu_host)[0]))
        del inputs
        times = {name: [] for name in INPUTS}
        for _ in range(a.rounds):                 # alternate, so that all see the same machine
            for name in INPUTS:
                times[name].append(event_us(calls[name][0]))
        for name in INPUTS:
            row[f"hist_k{K}_{name}_us"] = round(statistics.median(times[name]), 2)
        row[f"hist_k{K}_floor_us"] = round(n * (4 * K + 16) / HBM_BYTES_PER_US, 2)
        calls.clear()
        torch.cuda.empty_cache()

    # ---- one validation batch, replayed: fused head against curves=True
    torch.manual_seed(0)
    m = UNetHIP().to("cuda")
    img, mask = (t.to(dev) for t in synth_batch(B, H, W, 3, 2, seed=1))
    lu3 = torch.randint(0, 3, mask.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    tr = HipTrainer(m, precision="fp32", losses=("GDICE", "FOCAL"), graph=True)
    sides = {"plain": lambda: tr._val_graph_batch(img, mask, lu3, None, 1.0),
             "curves": lambda: tr._val_graph_batch(img, mask, lu3, None, 1.0, True)}
    with torch.no_grad():
        for fn in sides.values():
            for _ in range(3):                    # two eager batches, then the capture
                fn()
        torch.cuda.synchronize()
        times = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, fn in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[s].append(e0.elapsed_time(e1) / a.steps)
    for s in sides:
        row[f"validate_{s}_ms"] = round(statistics.median(times[s]), 3)
    del tr, img, mask, lu3
    torch.cuda.empty_cache()

    # ---- the decision kernel
    S = a.size
    for K in (2, 3):
        p = rng.random((K, S, S), dtype=np.float32)
        probs = torch.from_numpy(p).to(dev)
        decision = Decision({c: 0.3 for c in range(1, K)})
        out = torch.empty((S, S), dtype=torch.uint8, device=dev)
        row[f"decide_k{K}_us"] = round(event_us(lambda: ops.decide_classes(probs, decision, out=out)), 2)
        row[f"decide_k{K}_floor_us"] = round(S * S * (4 * (K - 1) + 1) / HBM_BYTES_PER_US, 2)
        if a.check:
            row["exact"] = bool(row["exact"] and np.array_equal(out.cpu().numpy(), decide_host(p, decision)))

    # ---- infer_tile with and without a decision
    class Inf:      # PyTorchInference's device entry points on a freshly initialised model (no checkpoint file needed)
        in_channels, classes = 3, 2

        def __init__(self):
            self.m = m
            self.m.eval()

        def run_windows(self, raster, d, overlap, first, count, want="classes", precision="fp32", views=None):
            x = ops.window_normalize_u8(raster, d, overlap, first, count, MEAN, STD, 3, views=views)
            if want == "classes":
                return self.m.predict_classes(x, dtype="uint8", precision=precision, nhwc=True)
            return self.m.predict_logits(x, precision=precision, nhwc=True)

    if a.infer:
        inf = Inf()
        ortho = rng.integers(0, 256, (3, S, S), dtype=np.uint8)
        common = dict(subtile=256, batch_size=64, device="cuda:0", overlap=64, blend="average")
        sides = (("plain", dict()), ("decision", dict(decision=Decision({1: 0.3}))))

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
        _, probs = tiler.infer_tile(inf, ortho, return_probs=True, **common)
        got = tiler.infer_tile(inf, ortho, **common, **sides[1][1])
        row["exact"] = bool(row["exact"] and np.array_equal(got, decide_host(probs, sides[1][1]["decision"])))
    print(json.dumps(row), flush=True)
    if not row["exact"]:
        raise SystemExit("bench_curves.py: the device result and the host result differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
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
        for name in ("batch", "tile", "size", "iters", "steps", "reps", "rounds", "check", "infer"):
            cmd += [f"--{name}", str(getattr(a, name))]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:              # a child that failed or ran out of time ends the measurement
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_curves.py: child ended with status {done.returncode}; nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    keys = [k for k in rows[0] if k.endswith(("_us", "_ms"))]
    print(json.dumps({"what": "median", "children": len(rows), "exact": all(r["exact"] for r in rows),
                      "chunk": rows[0]["chunk"], **{k: round(statistics.median(r[k] for r in rows), 3) for k in keys}}),
          flush=True)


if __name__ == "__main__":
    main()
