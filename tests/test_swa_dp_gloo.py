"""world_size-2 (gloo, both ranks on one MI355X) test of weight averaging under data parallelism: the average is local
and stays equal across ranks, and after the recalibration pass every rank holds rank 0's BatchNorm statistics."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from deadtrees_amd.data.synthetic import synth_batch
        from deadtrees_amd.network.unet import UNetHIP
        from deadtrees_amd.trainer import HipTrainer
        dev = "cuda:0"
        torch.cuda.set_device(0)
        m = UNetHIP()
        m.reset_parameters(seed=5)
        m.to(dev)
        tr = HipTrainer(m, distributed=True, average=("ema", 0.9))
        tr.broadcast_parameters(0)
        for s in range(3):      # every rank trains on its own batches
            img, mask = synth_batch(2, 64, 64, 3, 2, seed=70 + 10 * s + rank)
            tr.step(img.to(dev), mask.to(dev))
        avgs = [torch.empty_like(tr.averager.avg) for _ in range(world)]
        dist.all_gather(avgs, tr.averager.avg)
        tr.swap_in_average()
        imgs = lambda r: [synth_batch(2, 64, 64, 3, 2, seed=200 + 10 * i + r)[0].to(dev) for i in range(3)]   # noqa: E731
        k = tr.update_bn(imgs(rank))
        states = [torch.empty_like(m.bn_state) for _ in range(world)]
        dist.all_gather(states, m.bn_state)
        got = m.bn_state.clone()
        m.update_bn(imgs(0))        # rank 0's batches, no collective: what rank 0 computed
        q.put((rank, k, tr.averager.n_averaged, bool(torch.equal(avgs[0], avgs[1])),
               bool(torch.equal(states[0], states[1])), bool(torch.equal(got, m.bn_state)),
               bool(torch.isfinite(got).all())))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_average_is_local_and_recalibrated_statistics_come_from_rank0():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=250) for _ in range(2)]
    for p in procs:
        p.join(60)
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, k, n_avg, avg_equal, bn_equal, bn_is_rank0, finite in res:
        assert k == 3 and n_avg == 3, (rank, k, n_avg)
        assert avg_equal, "ranks hold different averages"
        assert bn_equal and bn_is_rank0, f"rank {rank}: BatchNorm statistics are not rank 0's"
        assert finite
