"""What proposal recall costs per frame: inference.DetectGraph replays with and without the pooled COCO update
(evaluation.ProposalEvaluator, csrc/coco_eval_pooled.hip) in the graph, and the update's GPU time from the in-library profiler, at the two
bench configurations -- VGG16 at 600x1000 (P = 300 proposals, max_dets (100, 200, 300)) and ResNet-50-FPN at 800x1344 (P = 1000,
max_dets (100, 300, 1000)).

    python tools/proposal_eval_bench.py [--config vgg|fpn|both] [--steps N] [--warmup W] [--commit REV] [--out profiles/proposal_eval_bench.json]

One synthetic frame per configuration (tools/infer_bench.py's models and frames); its ground truth is cut from its own proposals, with
labels spread over the classes.  Prints one JSON line; --out writes it too.  Times are recorded, not asserted."""
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
from faster_rcnn_pytorch_amd import _lib  # noqa: E402
from faster_rcnn_pytorch_amd.evaluation import CocoGroundTruth, ProposalEvaluator  # noqa: E402
from faster_rcnn_pytorch_amd.inference import DetectGraph  # noqa: E402

N_GT = 16


def one(config, steps, warmup, dev):
    m, _, (H, W) = ib.build(config, dev)
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(21)).to(dev)
    props = m.proposals(x)
    P, n = props.labels.numel(), int(props.count.item())
    max_dets = (100, 300, 1000) if P >= 1000 else (100, min(200, P), P)
    w, h = 640, 480
    pick = np.arange(0, max(n, 1), max(n // N_GT, 1))[:N_GT] if n > 0 else np.zeros(0, np.int64)
    px = np.round(props.boxes[:max(n, 0)].cpu().numpy()[pick].astype(np.float64) * np.array([w, h, w, h])).reshape(-1, 4)
    gtb = np.stack([px[:, 0], px[:, 1], px[:, 2] - px[:, 0], px[:, 3] - px[:, 1]], 1)
    gtl, crowd = (np.arange(len(pick)) % (m.num_classes - 1)).astype(np.int32), (np.arange(len(pick)) % 8 == 3).astype(np.uint8)
    pe = ProposalEvaluator(max_dets=max_dets, record_capacity=1 << 22, gt_capacity=64, device=dev)
    gt = CocoGroundTruth(64, dev)
    plain = DetectGraph(m, (H, W), threshold=ib.THRESHOLD)
    fused = DetectGraph(m, (H, W), threshold=ib.THRESHOLD, proposal_evaluator=pe, gt=gt)
    frame = [0]

    def with_update():
        gt.set(gtb, gtl, crowd, None, orig_wh=(w, h), image_id=frame[0])
        frame[0] += 1
        fused(x)
    res = {"config": config, "image_hw": [H, W], "proposal_capacity": P, "proposals": n, "gt_per_image": int(len(pick)), "max_dets": list(max_dets),
           "images_per_s": {"detect_graph_no_sync": ib.rate(lambda: plain(x), steps, warmup),
                            "detect_graph_with_pooled_update": ib.rate(with_update, steps, warmup)}}
    pe.reset()
    _lib.prof_reset()
    _lib.prof_enable(True)
    for k in range(steps):                                     # eager updates: the profiler's events bracket each launch
        gt.set(gtb, gtl, crowd, None, orig_wh=(w, h), image_id=k)
        pe.update(props, gt)
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    samples = _lib.prof_samples()
    for key, kernel in (("rank_kernel_us", "coco_pooled_rank_kernel"), ("match_kernel_us", "coco_pooled_match_kernel")):
        us = sorted(1e3 * v for v in samples.get(kernel, []))
        res[key] = {"median": us[len(us) // 2], "min": us[0], "launches": len(us)} if us else None
    out = pe.summarize()
    res["records"], res["ar"] = out["n_records"], [float(v) for v in out["ar"]]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("vgg", "fpn", "both"), default="both")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the revision the times are measured on (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "tools/proposal_eval_bench.py", "commit": a.commit, "device": torch.cuda.get_device_name(0), "threshold": ib.THRESHOLD,
           "steps": a.steps, "warmup": a.warmup,
           "runs": [one(c, a.steps, a.warmup, dev) for c in (("vgg", "fpn") if a.config == "both" else (a.config,))]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
