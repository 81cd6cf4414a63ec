"""Several ranks on the one GPU of a test box (not a test module): a free port and the process-group bootstrap around a
per-test job.  The jobs are module-level functions of their test files (spawn pickles them by name)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bootstrap(rank, world, port, backend, job, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        job(rank, world, out_dir)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()


def run_ranks(job, world, out_dir, backend="gloo"):
    """``job(rank, world, out_dir)`` on ``world`` processes that share cuda:0, inside one process group"""
    mp.spawn(_bootstrap, args=(world, free_port(), backend, job, str(out_dir)), nprocs=world, join=True)
