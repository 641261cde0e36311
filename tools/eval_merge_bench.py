"""GPU time of one merge of evaluator shards (evaluation.merge_shards -> ops.eval_merge, csrc/eval_merge.hip), recorded, never asserted.

    python tools/eval_merge_bench.py [--replays 200] [--rounds 9] [--warmup 20] [--out profiles/eval_merge_bench.json]

W = 8 shards of a COCO-val-sized record set: 5000 images dealt out as torch's DistributedSampler deals them (625 frames per rank, no
padding at 5000 / 8), each rank's last 25 frames repeated on the next rank so that the merge has duplicates to drop, 0 .. 100 records
per image (COCO's maxDets), 80 categories.  Both protocols: VOC-shaped records (one flag word, 80 counter words) and COCO-shaped ones
(four flag words, 320 counter words).
  * ops.eval_merge on the gathered buffers [8, capacity, ...] captured once into a graph; GPU time per merge = HIP-event time around
    `replays` back-to-back replays / replays, once per round, after `warmup` replays: median / p10 / p90 over `rounds`.
  * a same-bytes device copy measured the same way in the same run: one dense device-to-device copy that moves as many bytes in total
    (read + written) as the merge's hot loop must -- every kept record read and written once, 2 x (16 + 4 x flag words) bytes each --
    and the copy's time as a fraction of the merge's (1.0 = as fast as the copy).  The merge also reads the flags of the dropped
    records, fills its table and walks the ledger: the fraction says what all of that costs next to the bytes that have to move.
  * per-kernel GPU time of eager calls from the in-library profiler (median).
The device result is compared with the numpy restatement (tests/eval_merge_ref.py), bit for bit, before anything is timed.  Prints one
JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

from faster_rcnn_pytorch_amd import _lib, evaluation  # noqa: E402
import eval_merge_ref as R  # noqa: E402

W, N_IMAGES, OVERLAP, NUM_CLASSES = 8, 5000, 25, 81


def graph_us(fn, replays, rounds, warmup):
    """fn captured once; microseconds of GPU time per replay: median / p10 / p90 over the rounds."""
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
    return {"median": float(np.median(out)), "p10": float(np.percentile(out, 10)), "p90": float(np.percentile(out, 90)),
            "replays_per_round": replays, "rounds": rounds}


def copy_us(total_bytes, a):
    n = int(total_bytes) // 2
    src, dst = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    return dict(graph_us(lambda: dst.copy_(src), a.replays, a.rounds, a.warmup), bytes_copied=n)


def kernel_us(fn, calls):
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    return {k: float(np.median(v)) * 1e3 for k, v in sorted(_lib.prof_samples().items())}


def make_shards(fw, cw):
    rng = np.random.RandomState(2017)
    ids = 139 + 113 * rng.permutation(N_IMAGES)                 # COCO-like: sparse, unordered
    per = [list(ids[r::W]) for r in range(W)]
    for r in range(W):
        per[(r + 1) % W] += per[r][-OVERLAP:]                   # what a padded or re-run tail looks like: seen twice
    return [R.make_shard(rng, per[r], fw, cw, shard=r, counts=[int(c) for c in rng.randint(0, 101, len(per[r]))]) for r in range(W)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_merge_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "shards": W, "images": N_IMAGES, "repeated_images": W * OVERLAP, "protocols": {}}
    for name, fw in (("voc", 1), ("coco", 4)):
        cw = (NUM_CLASSES - 1) * fw
        shards = make_shards(fw, cw)
        want = R.merge(shards)
        cap, icap = 1 << 19, 8192
        assert want["n_records"] <= cap and want["n_images"] == N_IMAGES <= icap
        if name == "voc":
            ev = evaluation.DetectionEvaluator(NUM_CLASSES, record_capacity=cap, image_capacity=icap, device="cuda")
        else:
            ev = evaluation.CocoDetectionEvaluator(NUM_CLASSES, record_capacity=cap, image_capacity=icap, device="cuda")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
        views = [dict({k: t(s[k]) for k in R.COLUMNS + ("led_image", "led_range", "led_delta")},
                      n_records=torch.tensor([s["n_records"]], dtype=torch.int64, device="cuda"),
                      n_images=torch.tensor([s["n_images"]], dtype=torch.int64, device="cuda"),
                      error=torch.zeros(1, dtype=torch.int32, device="cuda")) for s in shards]
        sr = (max(len(s["score"]) for s in shards) + 3) // 4 * 4
        si = max(len(s["led_image"]) for s in shards)
        gathered = {k: ev._padded([v[k] for v in views], sr) for k in R.COLUMNS}          # what an all-gather hands over
        gathered.update({k: ev._padded([v[k] for v in views], si) for k in ("led_image", "led_range", "led_delta")})
        gathered.update({k: torch.cat([v[k] for v in views]) for k in ("n_records", "n_images", "error")})
        run = lambda: ev._merge(gathered)                                        # noqa: E731
        run()
        s = ev.state()
        got = {k: s[k].cpu().numpy() for k in ("score", "label", "image_id", "flags", "led_image", "led_range", "led_delta")}
        got.update(order=s[ev._COLUMN].cpu().numpy(), n_records=s["n_records"], n_images=s["n_images"], error=int(s["error"].item()),
                   counter=s[ev._COUNTER[0]].reshape(-1).cpu().numpy())
        try:
            R.same(got, want, name)
        except AssertionError as e:
            sys.exit("the device merge differs from the restatement (%s): not timing a wrong result" % (e,))
        moved = 2 * want["n_records"] * (16 + 4 * fw)
        r = {"flag_words": fw, "counter_words": cw, "shard_record_capacity": sr, "shard_image_capacity": si,
             "records_in": int(sum(x["n_records"] for x in shards)), "records_kept": int(want["n_records"]),
             "ledger_rows_in": int(sum(x["n_images"] for x in shards)), "ledger_rows_kept": int(want["n_images"]),
             "hot_loop_bytes": int(moved), "workspace_bytes": _lib.workspace_bytes(_lib.OP_EVAL_MERGE, W * sr, W * si), "equal_to_cpu_restatement": True}
        r["merge_graph_replay_us"] = graph_us(run, a.replays, a.rounds, a.warmup)
        r["same_bytes_copy_us"] = copy_us(moved, a)
        r["fraction_of_copy"] = r["same_bytes_copy_us"]["median"] / r["merge_graph_replay_us"]["median"]
        r["kernel_us_eager"] = kernel_us(run, 50)
        res["protocols"][name] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
