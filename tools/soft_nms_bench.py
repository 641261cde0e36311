"""What Soft-NMS costs per frame: graph replays of one view (inference.DetectGraph) and of flip TTA (inference.TTADetectGraph) with hard
NMS, linear and gaussian Soft-NMS, and the GPU time of the soft class kernel (csrc/detect_soft.hip) on m = 64, 300, 1000 and 2048
candidates in one class, from the in-library profiler -- the VGG mirror at 600x1000.

    python tools/soft_nms_bench.py [--steps N] [--warmup W] [--commit REV] [--out profiles/soft_nms_bench.json]

One synthetic frame (tools/infer_bench.py's model).  The one-class inputs come in two kinds: "chain", m boxes that each overlap only
their two neighbours, so that every candidate is emitted and the scan runs all m steps (its upper bound), and "objects", m boxes around
four objects, where most candidates fall under the floor after a few decays and the scan is short.  Every shape is warmed up before it is
timed; the kernel times are the medians of per-launch device events with the profiler on, the frame rates are taken with it off.
Prints one JSON line; --out writes it too.  Times are recorded, not asserted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import infer_bench as ib  # noqa: E402
from faster_rcnn_pytorch_amd import _lib, ops  # noqa: E402
from faster_rcnn_pytorch_amd.inference import DetectGraph, TTADetectGraph  # noqa: E402

KERNELS = ("detect_soft_class_kernel", "detect_merge_class_kernel", "detect_merge_emit_kernel")
SIZES = (64, 300, 1000, 2048)


def kernel_us(fn, steps, warmup):
    """Median / min GPU time of the merge's kernels over `steps` eager calls of fn: the profiler's events bracket each launch."""
    for _ in range(max(warmup, 1)):
        fn()
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    samples = _lib.prof_samples()
    out = {}
    for kernel in KERNELS:
        us = sorted(1e3 * v for v in samples.get(kernel, []))
        if us:
            out[kernel] = {"median": us[len(us) // 2], "min": us[0], "launches": len(us)}
    return out


def one_class(kind, m, dev):
    rng = np.random.RandomState(m)
    if kind == "chain":                                           # two cells wide on a 64-column grid: IoU 1/3 with the row neighbours only
        i = np.arange(m)
        x, y = (i % 64) / 66.0, (i // 64) / 32.0
        b = np.stack([x, y, x + 2 / 66.0, y + 1 / 32.0], 1)
    else:
        o = rng.randint(0, 4, m)
        c = (rng.rand(4, 2) * 0.6 + 0.2)[o] + (rng.rand(m, 2) - 0.5) * 0.15
        wh = (rng.rand(4, 2) * 0.2 + 0.1)[o] * (1 + (rng.rand(m, 2) - 0.5) * 0.6)
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)
    s = rng.rand(m) * 0.9 + 0.05
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)      # noqa: E731
    return ops.Detections(t(b, np.float32), torch.zeros(m, dtype=torch.int32, device=dev), t(s, np.float32), t(np.array([m]), np.int32), None, None, None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the revision the times are measured on (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, _, (H, W) = ib.build("vgg", dev)
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(21)).to(dev)
    modes = (("hard_nms", None), ("linear", ops.SoftNMS("linear")), ("gaussian", ops.SoftNMS("gaussian")))
    rates, rows = {}, {}
    graphs = [("detect_" + name, DetectGraph(m, (H, W), threshold=ib.THRESHOLD, soft_nms=soft)) for name, soft in modes]
    graphs += [("flip_tta_" + name, TTADetectGraph(m, [(H, W)], threshold=ib.THRESHOLD, soft_nms=soft)) for name, soft in modes]
    for rep in range(2):                                          # the variants in turn, twice: the second round is the record, the first shows the spread
        for name, g in graphs:
            rates.setdefault(name, []).append(ib.rate(lambda: g(x), a.steps, a.warmup))
            rows[name] = int(g(x).count.item())
    # the class kernel alone: the model's own candidates, then one class of m candidates
    kernels = {}
    with torch.no_grad():
        features, rois, n_rois = m._test_proposals(x)
        head_cls, head_reg = m._head(features, rois, x)
    cands = ops.detect_postprocess(head_cls, head_reg, rois, n_rois, ib.THRESHOLD, float("inf"))
    cc = cands.class_counts.cpu().numpy()
    for name, soft in modes[1:] + (("hard_by_the_soft_scan", ops.SoftNMS("hard")),):
        def call():
            return ops.merge_detections([cands], num_classes=m.num_classes, min_score=float("-inf"), soft_nms=soft)
        rec = kernel_us(call, a.steps, a.warmup)
        rec.update(candidates=int(cands.count.item()), largest_class=int(cc.max()), rows_out=int(call().count.item()))
        kernels["frame_" + name] = rec
    for kind in ("chain", "objects"):
        for n in SIZES:
            d = one_class(kind, n, dev)
            for name, soft in modes:
                def call():
                    return ops.merge_detections([d], num_classes=2, soft_nms=soft)
                rec = kernel_us(call, a.steps, a.warmup)
                rec.update(candidates=n, rows_out=int(call().count.item()))
                kernels["%s_m%d_%s" % (kind, n, name)] = rec
    res = {"tool": "tools/soft_nms_bench.py", "commit": a.commit, "device": torch.cuda.get_device_name(0), "config": "vgg", "image_hw": [H, W],
           "threshold": ib.THRESHOLD, "nms_threshold": 0.3, "sigma": 0.5, "score_floor": 1e-3, "steps": a.steps, "warmup": a.warmup,
           "images_per_s": {k: v[-1] for k, v in rates.items()}, "images_per_s_first_round": {k: v[0] for k, v in rates.items()},
           "rows_out": rows, "kernels_us": kernels}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
