"""GPU time of the device-side mosaic augmentation (transforms.mosaic, csrc/mosaic.hip) at the reference's size, recorded, never asserted.

    python tools/mosaic_bench.py [--size 600] [--replays 200] [--rounds 7] [--warmup 20] [--cpu-reps 5] [--out profiles/mosaic_bench.json]

Four seeded 375 x 500 uint8 frames with 8 boxes each, regions drawn by DeviceMosaicStage.draw_regions from a seeded generator.
  * mosaic alone, and mosaic + the final stage (DeviceMosaicStage.__call__: resize to 800, ToTensor, Normalize): each captured once
    into a graph; GPU time per call = HIP-event time around `replays` back-to-back replays / replays, the median over `rounds`,
    after `warmup` replays.  The launches per call are counted from the in-library profiler on one eager call.
  * per-kernel GPU time of one eager mosaic from the in-library profiler (events around every launch; median over `replays` calls).
  * baseline: wall time of the same composition through the CPU restatement (tests/mosaic_ref.py: the oracle's Pillow-exact resize,
    numpy paste, torch-CPU boxes) on the same machine, the median of `cpu-reps` -- a stand-in for the reference's Pillow path, which
    needs torchvision.  The device result is compared with it (exactly) before anything is timed.
Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

from faster_rcnn_pytorch_amd import _lib, transforms as T  # noqa: E402
import mosaic_ref  # noqa: E402


def inputs(size):
    rng = np.random.RandomState(17)
    imgs = [rng.randint(0, 256, (375, 500, 3)).astype(np.uint8) for _ in range(4)]
    boxes, labels = [], []
    for _ in range(4):
        x1, y1 = rng.uniform(0, 300, 8), rng.uniform(0, 220, 8)
        boxes.append(np.stack([x1, y1, x1 + rng.uniform(30, 200, 8), y1 + rng.uniform(30, 150, 8)], 1).astype(np.float32))
        labels.append(rng.randint(0, 20, 8).astype(np.int64))
    stage = T.DeviceMosaicStage(size=size, min_crop=min(384, size))
    return imgs, boxes, labels, stage.draw_regions([im.shape[:2] for im in imgs], random.Random(17)), stage


def graph_us(fn, replays, rounds, warmup):
    """fn captured once; microseconds of GPU time per replay (median over rounds, min, max)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / replays)
    return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out)), "replays_per_round": replays, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=600)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mosaic_bench needs a HIP device: nothing is measured without one")
    imgs, boxes, labels, regions, stage = inputs(a.size)
    d_imgs = [torch.from_numpy(x).cuda() for x in imgs]
    d_boxes, d_labels = torch.from_numpy(np.concatenate(boxes)).cuda(), torch.from_numpy(np.concatenate(labels)).cuda()
    counts = [len(b) for b in boxes]

    def run_mosaic():
        return T.mosaic(d_imgs, d_boxes, d_labels, regions, a.size, 1333, counts=counts)

    def run_stage():
        return stage(d_imgs, d_boxes, d_labels, regions, False, counts=counts)

    ref = mosaic_ref.mosaic_ref(imgs, boxes, labels, regions, a.size, 1333)
    canvas, rb, rl = run_mosaic().to_host()
    if not (np.array_equal(canvas, ref[0]) and np.array_equal(rb, ref[1]) and np.array_equal(rl, ref[2])):
        sys.exit("the device mosaic differs from the restatement: not timing a wrong result")
    res = {"device": torch.cuda.get_device_name(0), "size": a.size, "sources_hw": [list(im.shape[:2]) for im in imgs], "boxes_per_tile": counts,
           "regions": [list(map(int, r)) for r in regions], "fallback": ref[3].tolist(), "live_boxes": int(len(rb)),
           "equal_to_cpu_restatement": True}
    res["mosaic_graph_replay_us"] = graph_us(run_mosaic, a.replays, a.rounds, a.warmup)
    res["mosaic_plus_final_stage_graph_replay_us"] = graph_us(run_stage, a.replays, a.rounds, a.warmup)
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(a.replays):
        run_mosaic()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    samples = _lib.prof_samples()
    res["kernel_us_eager"] = {k: {"median": float(np.median(v)) * 1e3, "launches_per_call": len(v) / a.replays} for k, v in sorted(samples.items())}
    res["launches_per_mosaic"] = sum(len(v) for v in samples.values()) / a.replays
    cpu, cpu_full = [], []
    for _ in range(a.cpu_reps):
        t0 = time.perf_counter()
        c, b, _, _, _ = mosaic_ref.mosaic_ref(imgs, boxes, labels, regions, a.size, 1333)
        t1 = time.perf_counter()
        mosaic_ref.final_stage_ref(c, b)
        cpu.append(1e3 * (t1 - t0))
        cpu_full.append(1e3 * (time.perf_counter() - t0))
    res["cpu_restatement_wall_ms"] = {"mosaic": float(np.median(cpu)), "mosaic_plus_final_stage": float(np.median(cpu_full)), "reps": a.cpu_reps}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
