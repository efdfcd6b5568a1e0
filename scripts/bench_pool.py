"""The device-resident pool against the kernels it replaces: one training batch of 256 x 256 tiles out of a pool of
``--pool`` random samples, B = 64 and B = 32, C = 3.

  gather_us   the fused ``dt_pool_gather_batch`` (one launch, planar NCHW + int64 labels)
  chain_us    the same batch by the unfused kernels: ``index_select`` of the three arrays, ``augment_normalize_u8`` (byte
              sums + gather), two ``.long()`` casts and two ``augment_labels``
              (hipEvents around one batch, median of ``--iters`` batches, every batch another slice of the epoch plan)
  step_*_ms   one ``HipTrainer(graph=True)`` step fed each way — fused: the gather writes into ``static_batch()``; chain:
              the unfused batch goes through the step's staging copies — in alternating blocks of ``--steps`` steps, host
              clock around a device synchronise, median of ``--rounds`` blocks each

Every figure is taken in ``--children`` fresh processes, one after the other; the last line is the median over them.

    python scripts/bench_pool.py
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


def child(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from deadtrees_amd import ops
    from deadtrees_amd.data.deadtreedata import draw_train_params
    from deadtrees_amd.data.synthetic import MEAN, STD
    from deadtrees_amd.network.unet import UNetHIP
    from deadtrees_amd.trainer import HipTrainer

    if not torch.cuda.is_available():
        raise SystemExit("bench_pool.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    N, C = a.pool, 3
    gen = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (N, SIZE, SIZE, 4), dtype=torch.uint8, device=dev, generator=gen)
    masks = torch.randint(0, 3, (N, SIZE, SIZE), dtype=torch.uint8, device=dev, generator=gen)
    lu = torch.randint(0, 6, (N, SIZE, SIZE), dtype=torch.uint8, device=dev, generator=gen)
    sums = images.reshape(N, -1).sum(dim=1, dtype=torch.int64)

    for B in (64, 32):
        rng = np.random.default_rng([0, B])
        n_batches = N // B
        idx = torch.from_numpy(rng.permutation(N)[:n_batches * B].astype(np.int32)).to(dev)
        geo, bc = (t.to(dev) for t in draw_train_params(n_batches * B, rng))
        idx64 = idx.long()

        def fused(k, out=None):
            s = slice(k % n_batches * B, (k % n_batches + 1) * B)
            return ops.pool_gather_batch(images, masks, lu, sums, idx[s], geo[s], bc[s], MEAN, STD, C, True, out=out)

        def chain(k):
            s = slice(k % n_batches * B, (k % n_batches + 1) * B)
            sel, g = idx64[s], geo[s]
            img = ops.augment_normalize_u8(images.index_select(0, sel), g, bc[s], MEAN, STD, C).permute(0, 3, 1, 2)
            m = ops.augment_labels(masks.index_select(0, sel).long().clamp_(max=1), g)
            return img, m, ops.augment_labels(lu.index_select(0, sel).long(), g)

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

        gather_us, chain_us = event_us(fused), event_us(chain)

        model = UNetHIP(in_channels=C, classes=2)
        model.reset_parameters(seed=0)
        tr = HipTrainer(model.to(dev), precision=a.precision, graph=True)
        for k in range(4):                    # two eager steps, the capture, one replay
            img, m, _, _ = fused(k)
            tr.step(img, m)
        static = tr.static_batch()
        assert static is not None
        lu_buf = torch.empty((B, SIZE, SIZE), dtype=torch.int64, device=dev)

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
        for r in range(a.rounds):             # alternate, so that both see the same machine
            t_fused.append(block_ms(step_fused, r * a.steps))
            t_chain.append(block_ms(step_chain, r * a.steps))
        print(json.dumps({"what": "child", "B": B, "C": C, "size": SIZE, "pool": N, "precision": a.precision,
                          "bit_identical": same, "gather_us": round(gather_us, 2), "chain_us": round(chain_us, 2),
                          "step_fused_ms": round(statistics.median(t_fused), 4),
                          "step_chain_ms": round(statistics.median(t_chain), 4)}), flush=True)
        del tr, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=512)
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
    for B in (64, 32):
        mine = [r for r in rows if r["B"] == B]
        med = {k: round(statistics.median(r[k] for r in mine), 4)
               for k in ("gather_us", "chain_us", "step_fused_ms", "step_chain_ms")}
        print(json.dumps({"what": "median", "B": B, "children": len(mine), "precision": a.precision,
                          "bit_identical": all(r["bit_identical"] for r in mine), **med,
                          "tiles_per_s_fused": round(B / med["step_fused_ms"] * 1e3, 1),
                          "tiles_per_s_chain": round(B / med["step_chain_ms"] * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
