"""Cost of the training state file next to one training epoch, one MI355X: default Unet, fp32, B=32 at 512x512.

    python scripts/bench_resume.py [--repeats 3] [--dir DIR]

Each repeat is a child process of its own (fresh allocator and kernel state); the median is reported.  A child runs one
warm-up epoch of 8 eager steps, then times
    epoch    8 training steps (wall clock, device synchronised)
    save     utils.train_state.save_training_state: download, smp tensors, torch.save, os.replace
    load     load_training_state (file -> host tensors)
    restore  HipTrainer.load_state_dict (host tensors -> the trainer's device buffers, caches dropped)
and reports the file size.  The file goes to --dir (default: a temporary directory, removed afterwards).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, BATCH, SIDE = 8, 32, 512


def run_child(directory):
    sys.path.insert(0, ROOT)
    import torch
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer
    from deadtrees_amd.utils.train_state import load_training_state, save_training_state
    torch.manual_seed(0)
    tr = HipTrainer(UNetHIP().to("cuda"))
    img, mask = (t.to("cuda") for t in synth_batch(BATCH, SIDE, SIDE, 3, 2, seed=1))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def epoch():
        for _ in range(STEPS):
            tr.step(img, mask)
    epoch()
    path = os.path.join(directory, "state.pt")
    fit_state = {"epoch": 0, "history": [], "sched": {"base_lr": 3e-4, "t_max": 10, "start": 0}, "swa_from": None,
                 "swa": None, "base_lr": 3e-4, "t_max": 10, "stopped": False, "selection": None, "loader_next_epoch": 1}
    res = {"epoch_ms": timed(epoch)[0]}
    res["save_ms"] = timed(lambda: save_training_state(path, tr, fit_state))[0]
    res["file_mb"] = os.path.getsize(path) / 2 ** 20
    res["load_ms"], file = timed(lambda: load_training_state(path))
    res["restore_ms"] = timed(lambda: tr.load_state_dict(file["trainer"]))[0]
    os.remove(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_child(a.child)))
        return
    with tempfile.TemporaryDirectory(dir=a.dir) as directory:
        runs = []
        for _ in range(a.repeats):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", directory], capture_output=True,
                                 text=True, timeout=300)
            if out.returncode != 0:     # stop at the first failure: nothing else is started on the device
                print(out.stdout, out.stderr, file=sys.stderr)
                raise SystemExit(f"child failed with status {out.returncode}")
            runs.append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    print(f"fp32 B={BATCH} {SIDE}x{SIDE}: epoch of {STEPS} steps {med['epoch_ms']:.1f} ms; state file {med['file_mb']:.1f} MiB: "
          f"save {med['save_ms']:.1f} ms, load {med['load_ms']:.1f} ms, restore {med['restore_ms']:.1f} ms "
          f"(save / epoch = {med['save_ms'] / med['epoch_ms']:.2f})")


if __name__ == "__main__":
    main()
