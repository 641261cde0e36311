"""evaluator.synchronize_between_processes() (evaluation.py, csrc/eval_merge.hip): two ranks on the one GPU over gloo, as
tests/test_gpu_graph_ddp.py runs its two replicas.  The 47 images are dealt out the way torch's DistributedSampler deals them (padded
with the first image to 2 x 24), every rank evaluates its 24 frames and calls the collective, and the summary of EVERY rank must equal,
bit for bit, that of one evaluator over the 47 distinct images in one process."""
import datetime
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMAGES, WORLD = 47, 2
STEP_SECONDS = 120                                              # the limit of every step of the parent: a result, a join


def _frames(kind):
    """(image_id, frame) of the 47 images: the seeded pool of tests/test_gpu_eval_merge.py, reused under new ids."""
    import test_gpu_eval_merge as M
    pool = M._pool(kind)
    return [(3000 - 17 * k, pool[k % len(pool)]) for k in range(N_IMAGES)]


def _shard(items, rank, world):
    idx = list(range(len(items)))
    total = -(-len(idx) // world) * world
    idx += idx[:total - len(idx)]
    return [items[i] for i in idx[rank::world]]


def _summary(kind, items, ledger):
    import test_gpu_eval_merge as M
    fd = M._Feeder(kind, M._ev(kind, image_capacity=64 if ledger else None))
    for iid, f in items:
        fd.feed(f, image_id=iid)
    return fd


def _keys(kind):
    return ("ap", "map", "npos", "tp", "fp") if kind == "voc" else ("stats", "precision", "recall", "npig")


def _worker(rank, world, port, kind, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_SECONDS))
    mine = _shard(_frames(kind), rank, world)
    fd = _summary(kind, mine, True)
    before = fd.ev.state()["n_images"]
    out = fd.ev.synchronize_between_processes()
    res = fd.ev.summarize()
    st = fd.ev.state()
    q.put((rank, len(mine), before, out is fd.ev, st["n_images"], sorted(st["led_image"].cpu().tolist()),
           {k: np.asarray(res[k]) for k in _keys(kind)}, res["n_records"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["voc", "coco"])
def test_two_ranks_synchronize_to_the_single_process_result(kind):
    import torch.multiprocessing as mp
    items = _frames(kind)
    one = _summary(kind, items, False).ev.summarize()
    alone = _summary(kind, _shard(items, 0, 2) + _shard(items, 1, 2), True).ev           # no process group: deduplication only
    assert alone.synchronize_between_processes() is alone and alone.state()["n_images"] == N_IMAGES
    for k in _keys(kind):
        assert np.array_equal(np.asarray(alone.summarize()[k]).view(np.uint8), np.asarray(one[k]).view(np.uint8)), k
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 1000 + (500 if kind == "coco" else 0)
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, kind, q)) for r in range(WORLD)]          # a fresh child process per rank
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=STEP_SECONDS) for _ in procs], key=lambda t: t[0])
        for p in procs:
            p.join(STEP_SECONDS)
            assert p.exitcode == 0, "rank process ended with %r" % (p.exitcode,)
    finally:
        for p in procs:                                         # after a failure nothing is left running and nothing further starts
            if p.is_alive():
                p.kill()
                p.join(10)
    assert [r[0] for r in res] == [0, 1]
    for rank, n_mine, before, returned_self, n_images, ids, summary, n_records in res:
        assert n_mine == 24 and before == 24 and returned_self and n_images == N_IMAGES
        assert ids == sorted(i for i, _ in items)
        assert n_records == one["n_records"]
        for k in _keys(kind):
            a, b = summary[k], np.asarray(one[k])
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (rank, k)
