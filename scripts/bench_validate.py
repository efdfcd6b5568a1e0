"""Cost of one validation batch, one MI355X, 512x512 tiles: the fused evaluation head against the unfused chain.

    python scripts/bench_validate.py [--steps 10] [--rounds 3] [--repeats 3]

fp32 at B=32, bf16 at B=64.  Every child process (fresh allocator and kernel state) measures all three variants,
alternating them `--rounds` times so that clock and thermal drift hit them alike, and reports the median round of each:
    fused:graph    HipTrainer(graph=True).validate's batch: eval forward -> dt_head_eval -> algebra -> accumulate, replayed
    fused:eager    the same launches from Python
    unfused        eval forward with dt_head_fwd (fp32 logits + int64 arg-max map) -> loss_forward -> confusion_matrix
                   -> accumulate: the chain of SemSegment.validation_step, eager (the comparator; it stays as it is)
`--repeats` child processes per precision; printed per variant: the median over the children of ms per batch, tiles/s,
the spread (max - min over the children) and torch.cuda.max_memory_allocated during the variant's timed batches.
The requirement this serves: fused is no slower than unfused by more than the spread of the unfused case itself.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("fp32", 32), ("bf16", 64)]
VARIANTS = ("fused:graph", "fused:eager", "unfused")


def run_case(precision, batch, steps, rounds, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.synthetic import synth_batch
    from deadtrees_amd.loss.seg_loss import loss_forward
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer
    torch.manual_seed(0)
    m = UNetHIP().to("cuda")
    losses = ("GDICE", "FOCAL")
    img, mask = (t.to("cuda") for t in synth_batch(batch, 512, 512, 3, 2, seed=1))
    lu = torch.randint(0, 3, mask.shape, generator=torch.Generator().manual_seed(2)).to("cuda")
    tg = HipTrainer(m, precision=precision, losses=losses, graph=True)
    te = HipTrainer(m, precision=precision, losses=losses, graph=False)
    eng, params = m.engine, m.flat_params.detach()
    st = te._val_buffers()

    def unfused():
        if precision == "bf16":
            logits, am = eng.forward_bf16_eval(img, params, m.bn_state, want_argmax="int64")
        else:
            logits, am = eng.forward(img, params, m.bn_state, False, save=False, want_argmax="int64")
        parts, err, _ = loss_forward(logits, mask, None, {"losses": losses, "alpha": 1.0})
        ops.confusion_matrix(am, mask, lu, K=2, counts=st["counts"])
        ops.eval_accumulate(parts, float(batch), st["epoch"])

    fns = {"fused:graph": lambda: tg._val_graph_batch(img, mask, lu, None, 1.0),
           "fused:eager": lambda: te._val_batch(img, mask, lu, None, 1.0),
           "unfused": unfused}
    with torch.no_grad():
        for name in VARIANTS:
            for _ in range(max(warmup, 3)):       # (fused:graph: two eager batches, then the capture)
                fns[name]()
        torch.cuda.synchronize()
        ms = {name: [] for name in VARIANTS}
        mem = {name: 0 for name in VARIANTS}
        for _ in range(rounds):
            for name in VARIANTS:
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    fns[name]()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / steps)
                mem[name] = max(mem[name], torch.cuda.max_memory_allocated())
    return {"precision": precision, "batch": batch,
            "ms_per_batch": {n: statistics.median(v) for n, v in ms.items()}, "rounds_ms": ms,
            "max_memory_allocated": mem, "finite": bool(torch.isfinite(st["epoch"]).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="fp32 or bf16")
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    if a.case:
        p, b = a.case.split(",")
        print(json.dumps(run_case(p, int(b), a.steps, a.rounds, a.warmup)))
        return
    for p, b in CASES:
        if a.only and p != a.only:
            continue
        runs = []
        for _ in range(a.repeats):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{p},{b}", "--steps", str(a.steps),
                                  "--rounds", str(a.rounds), "--warmup", str(a.warmup)], capture_output=True, text=True,
                                 timeout=300)
            if out.returncode != 0:     # stop at the first failure: nothing else is started on the device
                print(out.stdout, out.stderr, file=sys.stderr)
                raise SystemExit(f"case {p},{b} failed with status {out.returncode}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs.append(r)
            print(json.dumps(r), flush=True)
        med = {}
        for name in VARIANTS:
            vals = [r["ms_per_batch"][name] for r in runs]
            med[name] = statistics.median(vals)
            mem = max(r["max_memory_allocated"][name] for r in runs)
            each = ", ".join("%.3f" % v for v in vals)
            print(f"{p} B={b} {name}: median {med[name]:.3f} ms, {b * 1e3 / med[name]:.1f} tiles/s, spread "
                  f"{max(vals) - min(vals):.3f} ms (children: {each}), max_memory_allocated {mem / 2 ** 20:.0f} MiB", flush=True)
        print(f"{p}: fused replayed / unfused = {med['fused:graph'] / med['unfused']:.4f}, fused eager / unfused = "
              f"{med['fused:eager'] / med['unfused']:.4f}", flush=True)


if __name__ == "__main__":
    main()
