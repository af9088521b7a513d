"""The metrics' buffers over torch.distributed: two ranks (gloo, 127.0.0.1) add DIFFERENT numbers of samples; ``get_buffer`` / ``aggregate`` on every rank
see all of them in rank order (``Cumulative._sync``: rows padded to the longest rank for the collective, trimmed afterwards).  The per-sample values come
from the kernels of the SIMT-emulator build."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _samples():
    gen = torch.Generator().manual_seed(4800)
    lp, ly = torch.randint(0, 3, (5, 1, 6, 5, 4), generator=gen), torch.randint(0, 3, (5, 1, 6, 5, 4), generator=gen)
    return lp, ly


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys

        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [here, os.path.dirname(here)]
        from emu_backend import emu_backend

        from monai_amd.metrics import DiceMetric

        lp, ly = _samples()
        mine = slice(0, 3) if rank == 0 else slice(3, 5)      # three samples on rank 0, two on rank 1
        with emu_backend():
            dm = DiceMetric(num_classes=3, reduction="mean_batch", get_not_nans=True)
            dm(lp[mine], ly[mine])
            buf = dm.get_buffer()
            f, nn = dm.aggregate()
            ret[rank] = (buf, f, nn, len(dm))
    finally:
        dist.destroy_process_group()


def test_two_rank_buffers_gather_uneven_batches(emu):
    from monai_amd.metrics import DiceMetric

    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    lp, ly = _samples()
    single = DiceMetric(num_classes=3, reduction="mean_batch", get_not_nans=True)
    single(lp, ly)
    f, nn = single.aggregate()
    for rank in (0, 1):
        buf, f_r, nn_r, n_r = ret[rank]
        assert n_r == 5 and torch.equal(buf, single.get_buffer()), rank      # all five samples, in rank order
        assert torch.equal(f_r, f) and torch.equal(nn_r, nn), rank
