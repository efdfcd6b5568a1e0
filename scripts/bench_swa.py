"""Cost of weight averaging and of the BatchNorm recalibration pass, one MI355X, 512x512 tiles.

    python scripts/bench_swa.py [--steps 20] [--repeats 3]

Each case runs in a child process of its own (fresh allocator and kernel state), `--repeats` times; the median is
reported.  fp32 at B=32, bf16 at B=64:
    step:none / step:ema     training step, HIP-graph replay, without / with average=("ema", 0.999)
    recal:graph / recal:eager   one batch of HipTrainer.update_bn (statistics-only forward), replayed / launched eagerly
    recal:forward            the same result without this feature: model.train(); torch.no_grad(); model(x)
                             (an fp32 forward whatever the trainer's precision, eager)
Prints one JSON line per child, then per case the median ms per step, tiles/s and the ratios.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(p, b, mode) for p, b in (("fp32", 32), ("bf16", 64))
         for mode in ("step:none", "step:ema", "recal:graph", "recal:eager", "recal:forward")]


def run_case(precision, batch, mode, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer
    torch.manual_seed(0)
    m = UNetHIP().to("cuda")
    kind, what = mode.split(":")
    img, mask = (t.to("cuda") for t in synth_batch(batch, 512, 512, 3, 2, seed=1))
    if kind == "step":
        tr = HipTrainer(m, precision=precision, graph=True, average=("ema", 0.999) if what == "ema" else None)

        def one():
            tr.step(img, mask)
    elif what == "forward":
        m.train()

        def one():
            with torch.no_grad():
                m(img)
    else:
        tr = HipTrainer(m, precision=precision, graph=(what == "graph"))
        tr.update_bn([img] * max(warmup, 3))      # (two eager batches, then the capture)
        run = tr._recal_graph_batch if what == "graph" else m.recalibrate_batch

        def one():
            with torch.no_grad():
                run(img, precision)
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        one()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return {"precision": precision, "batch": batch, "mode": mode, "ms_per_step": ms, "tiles_per_s": batch * 1e3 / ms,
            "finite": bool(torch.isfinite(m.bn_state).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="fp32 or bf16")
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    if a.case:
        p, b, mode = a.case.split(",")
        print(json.dumps(run_case(p, int(b), mode, a.steps, a.warmup)))
        return
    res = {}
    for p, b, mode in CASES:
        if a.only and p != a.only:
            continue
        runs = []
        for _ in range(a.repeats):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{p},{b},{mode}", "--steps",
                                  str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:     # stop at the first failure: nothing else is started on the device
                print(out.stdout, out.stderr, file=sys.stderr)
                raise SystemExit(f"case {p},{b},{mode} failed with status {out.returncode}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs.append(r)
            print(json.dumps(r), flush=True)
        ms = statistics.median(r["ms_per_step"] for r in runs)
        res[(p, mode)] = ms
        each = ", ".join("%.3f" % r["ms_per_step"] for r in runs)
        print(f"{p} B={b} {mode}: median {ms:.3f} ms, {b * 1e3 / ms:.1f} tiles/s (runs: {each})", flush=True)
    for p in ("fp32", "bf16"):
        if (p, "step:none") not in res:
            continue
        print(f"{p}: step with EMA / without = {res[(p, 'step:ema')] / res[(p, 'step:none')]:.4f}; recalibration "
              f"replayed / train-mode forward = {res[(p, 'recal:graph')] / res[(p, 'recal:forward')]:.3f}, eager / "
              f"train-mode forward = {res[(p, 'recal:eager')] / res[(p, 'recal:forward')]:.3f}")


if __name__ == "__main__":
    main()
