"""What test-time augmentation costs per frame: graph replays of one view (inference.DetectGraph), of flip TTA and of flip plus a
second scale (inference.TTADetectGraph), with and without box voting, and the GPU time of the merge's two kernels
(csrc/detect_merge.hip) from the in-library profiler -- the VGG mirror at 600x1000.

    python tools/tta_bench.py [--steps N] [--warmup W] [--second-hw H W] [--commit REV] [--out profiles/tta_bench.json]

One synthetic frame per size (tools/infer_bench.py's model).  Prints one JSON line; --out writes it too.  Times are recorded, not
asserted."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import infer_bench as ib  # noqa: E402
from faster_rcnn_pytorch_amd import _lib, ops  # noqa: E402
from faster_rcnn_pytorch_amd.inference import DetectGraph, TTADetectGraph  # noqa: E402

VOTE = 0.5


def kernel_us(fn, steps):
    """Median / min GPU time of the merge's kernels over `steps` eager calls of fn: the profiler's events bracket each launch."""
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    samples = _lib.prof_samples()
    out = {}
    for kernel in ("detect_merge_class_kernel", "detect_merge_emit_kernel"):
        us = sorted(1e3 * v for v in samples.get(kernel, []))
        out[kernel] = {"median": us[len(us) // 2], "min": us[0], "launches": len(us)} if us else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--second-hw", type=int, nargs=2, default=(480, 800), help="the second scale's input size")
    ap.add_argument("--commit", default=None, help="the revision the times are measured on (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, (H, W) = ib.build("vgg", dev)
    H2, W2 = a.second_hw
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(21)).to(dev)
    x2 = torch.randn(1, 3, H2, W2, generator=torch.Generator().manual_seed(22)).to(dev)
    one = DetectGraph(m, (H, W), threshold=ib.THRESHOLD)
    rates = {"one_view": ib.rate(lambda: one(x), a.steps, a.warmup)}
    for name, vote in (("nms", None), ("vote", VOTE)):
        flip = TTADetectGraph(m, [(H, W)], threshold=ib.THRESHOLD, vote_threshold=vote)
        both = TTADetectGraph(m, [(H, W), (H2, W2)], threshold=ib.THRESHOLD, vote_threshold=vote)
        rates["flip_tta_" + name] = ib.rate(lambda: flip(x), a.steps, a.warmup)
        rates["flip_and_second_scale_tta_" + name] = ib.rate(lambda: both([x, x2]), a.steps, a.warmup)
    # the merge alone, on the detections of the two and of the four views
    views = [m.detect(v, ib.THRESHOLD) for v in (x, x.flip(-1), x2, x2.flip(-1))]
    merge = {}
    for n_views in (2, 4):
        for name, vote in (("nms", None), ("vote", VOTE)):
            def call():
                return ops.merge_detections(views[:n_views], hflip=[False, True, False, True][:n_views], num_classes=m.num_classes,
                                            min_score=float("-inf"), vote_threshold=vote)
            out = call()
            rec = kernel_us(call, a.steps)
            rec["live_rows_in"] = [int(v.count.item()) for v in views[:n_views]]
            rec["rows_out"] = int(out.count.item())
            merge["%d_views_%s" % (n_views, name)] = rec
    res = {"tool": "tools/tta_bench.py", "commit": a.commit, "device": torch.cuda.get_device_name(0), "config": "vgg", "image_hw": [H, W],
           "second_hw": [H2, W2], "threshold": ib.THRESHOLD, "nms_threshold": 0.3, "vote_threshold": VOTE, "steps": a.steps, "warmup": a.warmup,
           "images_per_s": rates, "merge_kernels_us": merge}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
