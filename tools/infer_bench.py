"""Inference throughput of one frame at a time (the reference's test.py:60 loop): FRCNN.predict eager, FRCNN.detect eager and
inference.DetectGraph replays, every result brought to the host; and the GPU time of the post-process alone, the op chain behind
predict (softmax ... decode ... batched_nms, with its host syncs) against ops.detect_postprocess, from HIP events.

    python tools/infer_bench.py --config vgg|fpn [--amp bf16] [--steps N] [--warmup W] [--only detect] [--eval [--protocol voc|coco]] [--out FILE]

Synthetic frames (600x1000 for VGG16, 800x1344 for ResNet-50-FPN), head weights spread as tests/test_gpu_detect.py spreads them (a
random-init head gives near-constant scores).  Prints one JSON line.  --only detect runs the eager detect loop alone (for a
kernel trace).  --eval measures the detection evaluator instead (faster_rcnn_pytorch_amd/evaluation.py): images/s of DetectGraph
replays with and without the evaluator's update in the graph, the update kernel's GPU time from the in-library profiler, and the
host alternative -- to_host() per frame plus the reference-form matching in numpy -- in the same run.  --eval --protocol coco
measures the COCO protocol (evaluation.CocoDetectionEvaluator): replays with and without its update, the update kernel's GPU time,
the accumulate kernel's and summarize(); the VOC update's kernel time is taken in the same run for comparison.  --out writes the JSON
too.  No time is asserted anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from faster_rcnn_pytorch_amd import ops  # noqa: E402
from faster_rcnn_pytorch_amd.inference import DetectGraph  # noqa: E402

THRESHOLD = 0.05


def build(config, dev):
    torch.manual_seed(0)
    if config == "vgg":
        from faster_rcnn_pytorch_amd.model import FRCNN
        m = FRCNN(num_classes=21, sampling="host").to(dev)
        rpn_cls, rpn_reg, head, seed, hw = m.rpn.cls_layer, m.rpn.reg_layer, m.fast_rcnn_head, 5, (600, 1000)
        rpn_scale = (30, 10)
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
        m = FRCNN(num_classes=91, sampling="host").to(dev)
        rpn_cls, rpn_reg, head, seed, hw = m.rpn.rpn_head.cls_layer, m.rpn.rpn_head.reg_layer, m.frcnn_head, 6, (800, 1344)
        rpn_scale = (30, 2)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        rpn_cls.weight.mul_(rpn_scale[0])
        rpn_reg.weight.mul_(rpn_scale[1])
        head.cls_head.weight.copy_(torch.randn(head.cls_head.weight.shape, generator=g) * 0.8)
        head.reg_head.weight.copy_(torch.randn(head.reg_head.weight.shape, generator=g) * 0.5)
    return m.eval(), head, hw


def old_chain(m, rois, n, hc, hr, thr):
    """The post-processing lines of FRCNN.predict (model._Detector), on the head outputs of n live rows."""
    return m._suppress(*m._decode(rois[:n], hc, hr), thr)


def rate(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def host_match(b, l, s, gtb, gtl, gtd, w, h, thr=0.5):
    """The reference-form matching of one frame on the host (evaluation/voc_eval.py:90-91, 162-197 without its JSON files): float64
    pixel boxes, the +1 overlap against the same-class ground truths, first maximum, TP / FP / ignored in score order."""
    px = b.astype(np.float32) * np.array([w, h, w, h])
    gt = gtb.astype(np.float64)
    ga = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    used, flags = set(), np.zeros(len(l), np.int8)
    for i in np.argsort(-s, kind="stable"):
        bb = px[i]
        iw = np.minimum(bb[2], gt[:, 2]) - np.maximum(bb[0], gt[:, 0]) + 1
        ih = np.minimum(bb[3], gt[:, 3]) - np.maximum(bb[1], gt[:, 1]) + 1
        ok = (gtl == l[i]) & (iw > 0) & (ih > 0)
        flags[i] = 2
        if ok.any():
            ov = np.where(ok, iw * ih / ((bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + ga - iw * ih), -np.inf)
            m = int(np.argmax(ov))
            if ov[m] >= thr:
                if gtd[m]:
                    flags[i] = 3
                elif m not in used:
                    used.add(m)
                    flags[i] = 1
    return flags


def eval_bench(a, m, x, H, W, res):
    """DetectGraph with and without the evaluator's update, and the host alternative, on one synthetic frame whose ground truth is cut
    from its own detections."""
    from faster_rcnn_pytorch_amd import _lib
    from faster_rcnn_pytorch_amd.evaluation import DetectionEvaluator, GroundTruth
    b, l, s = (t.numpy() for t in m.detect(x, THRESHOLD).to_host())
    w, h = 500, 375
    pick = np.arange(0, max(len(l), 1), max(len(l) // 8, 1))[:8] if len(l) else np.zeros(0, np.int64)
    gtb = np.round(b[pick].astype(np.float64) * np.array([w, h, w, h])).astype(np.float32).reshape(-1, 4)
    gtl, gtd = l[pick].astype(np.int32), (np.arange(len(pick)) % 4 == 1).astype(np.uint8)
    ev = DetectionEvaluator(m.num_classes, (0.5,), record_capacity=1 << 22, gt_capacity=64, device=x.device)
    gt = GroundTruth(64, x.device)
    plain = DetectGraph(m, (H, W), threshold=THRESHOLD)
    fused = DetectGraph(m, (H, W), threshold=THRESHOLD, evaluator=ev, gt=gt)
    frame = [0]

    def with_update():
        gt.set(gtb, gtl, gtd, (w, h), frame[0])
        frame[0] += 1
        fused(x)

    def host_path():
        hb, hl, hs = (t.numpy() for t in plain(x).to_host())
        host_match(hb, hl, hs, gtb, gtl, gtd, w, h)
    ips = {"detect_graph_no_sync": rate(lambda: plain(x), a.steps, a.warmup),
           "detect_graph_with_eval_update": rate(with_update, a.steps, a.warmup),
           "detect_graph_to_host_plus_numpy_matching": rate(host_path, a.steps, a.warmup)}
    res["images_per_s"] = ips
    ev.reset()
    _lib.prof_reset()
    _lib.prof_enable(True)
    for k in range(a.steps):                                   # eager updates: the profiler's events bracket each launch
        gt.set(gtb, gtl, gtd, (w, h), k)
        ev.update(plain.out, gt)
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    us = sorted(1e3 * v for v in _lib.prof_samples().get("eval_update_kernel", []))
    res["eval_update_kernel_us"] = {"median": us[len(us) // 2], "min": us[0], "launches": len(us)} if us else None
    t0 = time.perf_counter()
    out = ev.summarize()
    res["summarize_ms"] = 1e3 * (time.perf_counter() - t0)
    res["detections_per_image"], res["gt_per_image"], res["records"] = int(len(l)), int(len(pick)), out["n_records"]
    res["map_at_0.5"] = float(out["map"][0])


def coco_eval_bench(a, m, x, H, W, res):
    """DetectGraph with and without the COCO evaluator's update on one synthetic frame whose annotations are cut from its own
    detections, the update and accumulate kernels' GPU times, and the VOC update's kernel time on the same detections."""
    from faster_rcnn_pytorch_amd import _lib
    from faster_rcnn_pytorch_amd.evaluation import CocoDetectionEvaluator, CocoGroundTruth, DetectionEvaluator, GroundTruth
    b, l, s = (t.numpy() for t in m.detect(x, THRESHOLD).to_host())
    w, h = 640, 480
    pick = np.arange(0, max(len(l), 1), max(len(l) // 8, 1))[:8] if len(l) else np.zeros(0, np.int64)
    px = np.round(b[pick].astype(np.float64) * np.array([w, h, w, h])).reshape(-1, 4)
    gtb = np.stack([px[:, 0], px[:, 1], px[:, 2] - px[:, 0], px[:, 3] - px[:, 1]], 1)
    gtl, crowd = l[pick].astype(np.int32), (np.arange(len(pick)) % 4 == 1).astype(np.uint8)
    ev = CocoDetectionEvaluator(m.num_classes, record_capacity=1 << 20, gt_capacity=64, device=x.device)
    gt = CocoGroundTruth(64, x.device)
    plain = DetectGraph(m, (H, W), threshold=THRESHOLD)
    fused = DetectGraph(m, (H, W), threshold=THRESHOLD, evaluator=ev, gt=gt)
    frame = [0]

    def with_update():
        gt.set(gtb, gtl, crowd, None, orig_wh=(w, h), image_id=frame[0])
        frame[0] += 1
        fused(x)
    res["protocol"] = "coco"
    res["images_per_s"] = {"detect_graph_no_sync": rate(lambda: plain(x), a.steps, a.warmup),
                           "detect_graph_with_coco_eval_update": rate(with_update, a.steps, a.warmup)}
    ev.reset()
    voc, vgt = DetectionEvaluator(m.num_classes, (0.5,), record_capacity=1 << 20, gt_capacity=64, device=x.device), GroundTruth(64, x.device)
    vgt.set(px.astype(np.float32), gtl, crowd, (w, h), 0)
    _lib.prof_reset()
    _lib.prof_enable(True)
    for k in range(a.steps):                                   # eager updates: the profiler's events bracket each launch
        gt.set(gtb, gtl, crowd, None, orig_wh=(w, h), image_id=k)
        ev.update(plain.out, gt)
        voc.update(plain.out, vgt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ev.summarize()
    res["summarize_ms"] = 1e3 * (time.perf_counter() - t0)
    _lib.prof_enable(False)
    samples = _lib.prof_samples()
    for key, kernel in (("coco_update_kernel_us", "coco_update_kernel"), ("voc_eval_update_kernel_us", "eval_update_kernel"),
                        ("coco_accumulate_kernel_us", "coco_accumulate_kernel")):
        us = sorted(1e3 * v for v in samples.get(kernel, []))
        res[key] = {"median": us[len(us) // 2], "min": us[0], "launches": len(us)} if us else None
    res["detections_per_image"], res["gt_per_image"], res["records"] = int(len(l)), int(len(pick)), out["n_records"]
    res["stats"] = [float(v) for v in out["stats"]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("vgg", "fpn"), default="vgg")
    ap.add_argument("--amp", choices=("none", "bf16"), default="none")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("all", "detect"), default="all")
    ap.add_argument("--eval", action="store_true", help="measure the detection evaluator (DetectGraph with / without its update, and the host path)")
    ap.add_argument("--protocol", choices=("voc", "coco"), default="voc", help="with --eval: the VOC AP evaluator (default) or the COCO protocol")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, head, (H, W) = build(a.config, dev)
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(21)).to(dev)
    amp = torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False) if a.amp == "bf16" else torch.autocast("cuda", enabled=False)
    res = {"config": a.config, "amp": a.amp, "image_hw": [H, W], "threshold": THRESHOLD, "steps": a.steps,
           "device": torch.cuda.get_device_name(0)}
    with amp:
        if a.eval:
            (coco_eval_bench if a.protocol == "coco" else eval_bench)(a, m, x, H, W, res)
            print(json.dumps(res))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
            return
        if a.only == "detect":
            res["images_per_s"] = {"detect_eager": rate(lambda: m.detect(x, THRESHOLD).to_host(), a.steps, a.warmup)}
            print(json.dumps(res))
            return
        ips = {"predict_eager": rate(lambda: m.predict(x, THRESHOLD), a.steps, a.warmup),
               "detect_eager": rate(lambda: m.detect(x, THRESHOLD).to_host(), a.steps, a.warmup)}
        dg = DetectGraph(m, (H, W), threshold=THRESHOLD)
        ips["detect_graph"] = rate(lambda: dg(x).to_host(), a.steps, a.warmup)
        res["images_per_s"] = ips
        # the post-process alone, on the head outputs of one detect call
        cap = {}
        h = head.register_forward_hook(lambda mod, i, o: cap.__setitem__("head", (i[1], o[0].detach(), o[1].detach())))
        det = m.detect(x, THRESHOLD, want_prob=True)
        h.remove()
        rois, hc, hr = cap["head"]
        n = int(det.n_rois.item())
        hcn, hrn = hc[:n].float().contiguous(), hr[:n].float().contiguous()
        res["postprocess_ms"] = {"old_chain_softmax_to_nms_classed": event_ms(lambda: old_chain(m, rois, n, hcn, hrn, THRESHOLD), a.steps),
                                 "fused_detect_postprocess": event_ms(lambda: ops.detect_postprocess(hc, hr, rois, det.n_rois, THRESHOLD), a.steps)}
        prob = det.prob[:n, 1:]
        res["rois_per_image"] = n
        res["candidates_per_image"] = int((prob > THRESHOLD).sum().item())
        res["detections_per_image"] = int(det.count.item())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
