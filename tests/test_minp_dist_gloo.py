"""The one exchange of the Westfall-Young minima (dist.all_reduce_min) over gloo, without a GPU: every rank's
[T, P] minima over its own genes -> the element-wise minimum on every rank, bit patterns preserved."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_minima(rank, T, P):
    rng = np.random.default_rng(100 + rank)
    m = rng.random((T, P)) ** 8                    # p-like: many small values, all in (0, 1)
    m[:, rank::5] = 1.0                            # columns this rank's genes never lowered
    return m


def _worker(rank, world, port, outq):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from scoary_amd import dist as sd
    sd.init_from_env()
    t = torch.from_numpy(_rank_minima(rank, 3, 41))
    out = sd.all_reduce_min(t)
    assert out is t                                # in place
    outq.put((rank, out.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_min_gloo():
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.minimum.reduce([_rank_minima(r, 3, 41) for r in range(world)])
    for r in range(world):
        assert np.array_equal(got[r].view(np.uint64), want.view(np.uint64))


def test_all_reduce_min_is_the_identity_for_one_process():
    from scoary_amd import dist as sd
    t = torch.from_numpy(_rank_minima(0, 2, 7))
    keep = t.clone()
    assert sd.all_reduce_min(t) is t and torch.equal(t, keep)
