"""Training-step time with a frozen encoder vs the full step, one MI355X, HIP-graph replay, 512x512 tiles.

    python scripts/bench_freeze.py [--steps 20]

Each case runs in a child process of its own (fresh allocator and kernel state):
    fp32 B=32: full step, encoder-eval step (weights trainable), frozen step (eval + requires_grad_(False))
    bf16 B=64: full step, frozen step
Prints one line per case (tiles/s, ms per step, the convolutions whose gradients the step launched) and the time ratios
frozen / full.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("fp32", 32, "full"), ("fp32", 32, "enc_eval"), ("fp32", 32, "frozen"), ("bf16", 64, "full"),
         ("bf16", 64, "frozen")]


def run_case(precision, batch, mode, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer
    torch.manual_seed(0)
    m = UNetHIP().to("cuda")
    if mode in ("enc_eval", "frozen"):
        m.encoder.eval()
    if mode == "frozen":
        m.encoder.requires_grad_(False)
    tr = HipTrainer(m, precision=precision, graph=True)
    img, mask = (t.to("cuda") for t in synth_batch(batch, 512, 512, 3, 2, seed=1))
    for _ in range(warmup):
        tr.step(img, mask)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.step(img, mask)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    rec = m.engine.launches
    fam = {k: sorted({"encoder" if n.startswith("encoder.") else "decoder/head" for n in v}) for k, v in rec.items()}
    return {"precision": precision, "batch": batch, "mode": mode, "ms_per_step": ms, "tiles_per_s": batch * 1e3 / ms,
            "dgrad_convs": len(rec["dgrad"]), "wgrad_convs": len(rec["wgrad"]), "families": fam}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    if a.case:
        p, b, mode = a.case.split(":")
        print(json.dumps(run_case(p, int(b), mode, a.steps, a.warmup)))
        return
    res = {}
    for p, b, mode in CASES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{p}:{b}:{mode}", "--steps",
                              str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            print(out.stdout, out.stderr, file=sys.stderr)
            raise SystemExit(f"case {p}:{b}:{mode} failed with status {out.returncode}")
        r = json.loads(out.stdout.strip().splitlines()[-1])
        res[(p, mode)] = r
        print(json.dumps(r), flush=True)
    for p in ("fp32", "bf16"):
        full, fr = res[(p, "full")]["ms_per_step"], res[(p, "frozen")]["ms_per_step"]
        print(f"{p}: frozen / full step time = {fr / full:.3f}")


if __name__ == "__main__":
    main()
