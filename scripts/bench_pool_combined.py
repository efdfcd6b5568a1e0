"""The combined batch of the reference's multi-dataset configurations — 256 x 256 tiles, batch 32 = 15 main + extras
[2, 15], C = 3 — made two ways out of three resident pools of ``--pool`` random samples each:

  fused_us    one ``dt_pool_gather_combined`` launch
  chain_us    what it replaces: one ``dt_pool_gather_batch`` per set and the four ``torch.cat`` of ``concat_extra`` (image,
              mask, lu; no distance maps: a graph trainer makes its own) — 3 gather launches + 3 concatenations
              (hipEvents around one batch, median of ``--iters`` batches, every batch another slice of the epoch's plan)
  step_*_ms   one ``HipTrainer(graph=True)`` step fed each way — fused: the gather writes into ``static_batch()``; chain:
              the concatenated batch goes through the step's two staging copies — in alternating blocks of ``--steps``
              steps, host clock around a device synchronise, median of ``--rounds`` blocks each

Every figure is taken in ``--children`` fresh processes, one after the other; the last line is the median over them.

    python scripts/bench_pool_combined.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256
BATCH, EXTRA = 32, (2, 15)


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.pool import combined_plan
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer

    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_combined.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    N, C = a.pool, 3
    sizes = (BATCH - sum(EXTRA),) + EXTRA
    gen = torch.Generator(device=dev).manual_seed(0)
    sources = []
    for _ in sizes:
        images = torch.randint(0, 256, (N, SIZE, SIZE, 4), dtype=torch.uint8, device=dev, generator=gen)
        masks = torch.randint(0, 3, (N, SIZE, SIZE), dtype=torch.uint8, device=dev, generator=gen)
        lu = torch.randint(0, 6, (N, SIZE, SIZE), dtype=torch.uint8, device=dev, generator=gen)
        sources.append((images, masks, lu, images.reshape(N, -1).sum(dim=1, dtype=torch.int64)))
    L, src, idx, geo, bc = combined_plan([N] * len(sizes), sizes, 0, 0, True, True)
    src, idx, geo, bc = (t.to(dev) for t in (src, idx, geo, bc))
    # the same plan as one tensor per set, the way one PoolLoader per set would hold it
    cols = [slice(sum(sizes[:j]), sum(sizes[:j + 1])) for j in range(len(sizes))]
    per_set = [tuple(t.reshape((L, BATCH) + tuple(t.shape[1:]))[:, c].contiguous() for t in (idx, geo, bc)) for c in cols]

    def fused(k, out=None):
        s = slice(k % L * BATCH, (k % L + 1) * BATCH)
        return ops.pool_gather_combined(sources, src[s], idx[s], geo[s], bc[s], MEAN, STD, C, True, out=out)

    def chain(k):
        parts = [ops.pool_gather_batch(*sources[j], i[k % L], g[k % L], b[k % L], MEAN, STD, C, True)
                 for j, (i, g, b) in enumerate(per_set)]
        return tuple(torch.cat([p[f] for p in parts], dim=0) for f in range(3))

    a_, b_ = fused(1), chain(1)
    same = bool(torch.equal(a_[0], b_[0]) and torch.equal(a_[1], b_[1]) and torch.equal(a_[2], b_[2]))

    def event_us(fn):
        for k in range(3):
            fn(k)
        samples = []
        for k in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            e1.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(samples)

    fused_us, chain_us = [], []
    for _ in range(3):                        # alternate, so that both see the same machine
        fused_us.append(event_us(fused))
        chain_us.append(event_us(chain))

    model = UNetHIP(in_channels=C, classes=2)
    model.reset_parameters(seed=0)
    tr = HipTrainer(model.to(dev), precision=a.precision, graph=True)
    for k in range(4):                        # two eager steps, the capture, one replay
        img, m, _, _ = fused(k)
        tr.step(img, m)
    static = tr.static_batch()
    assert static is not None
    lu_buf = torch.empty((BATCH, SIZE, SIZE), dtype=torch.int64, device=dev)

    def step_fused(k):
        img, m, _, _ = fused(k, out=(static[0], static[1], lu_buf))
        tr.step(img, m)

    def step_chain(k):
        img, m, _ = chain(k)
        tr.step(img, m)

    def block_ms(fn, k0):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(a.steps):
            fn(k0 + k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.steps * 1e3

    for fn in (step_fused, step_chain):
        block_ms(fn, 0)
    t_fused, t_chain = [], []
    for r in range(a.rounds):
        t_fused.append(block_ms(step_fused, r * a.steps))
        t_chain.append(block_ms(step_chain, r * a.steps))
    print(json.dumps({"what": "child", "B": BATCH, "extra": list(EXTRA), "C": C, "size": SIZE, "pool": N,
                      "precision": a.precision, "bit_identical": same,
                      "fused_us": round(statistics.median(fused_us), 2), "chain_us": round(statistics.median(chain_us), 2),
                      "step_fused_ms": round(statistics.median(t_fused), 4),
                      "step_chain_ms": round(statistics.median(t_chain), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for _ in range(a.children):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"]
        for name in ("pool", "iters", "steps", "rounds", "precision"):
            cmd += [f"--{name}", str(getattr(a, name))]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in rows), 4)
           for k in ("fused_us", "chain_us", "step_fused_ms", "step_chain_ms")}
    print(json.dumps({"what": "median", "B": BATCH, "extra": list(EXTRA), "children": len(rows),
                      "precision": a.precision, "bit_identical": all(r["bit_identical"] for r in rows), **med}), flush=True)


if __name__ == "__main__":
    main()
