"""The COCO protocol of the device evaluator (csrc/coco_eval.hip, evaluation.CocoDetectionEvaluator, DetectGraph(evaluator=, gt=))
against its restatement (tests/coco_eval_ref.py; known answers in tests/test_coco_eval_host.py).

Everything is compared with np.array_equal: the records (order, scores, ranks, the flag word of every area range), precision, recall,
npig and the 12 stats.  Every device operation is an IEEE float64 + - * / in the order of the restatement and the means are taken by
the same numpy calls, so there is no tolerance to choose."""
import numpy as np
import pytest
import torch

import coco_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mods():
    from faster_rcnn_pytorch_amd import evaluation, ops
    return evaluation, ops


def _dets(f, cap=None, count=None):
    """ops.Detections of a frame dict at a fixed capacity; the rows past the count hold NaN boxes and a wrong label."""
    _, ops = _mods()
    D = len(f["labels"])
    cap = max(D, 1) if cap is None else cap
    boxes = torch.full((cap, 4), float("nan"), dtype=torch.float32)
    labels = torch.full((cap,), 10 ** 6, dtype=torch.int32)
    scores = torch.full((cap,), 2.0, dtype=torch.float32)
    boxes[:D] = torch.from_numpy(np.ascontiguousarray(f["boxes"], np.float32).reshape(-1, 4))
    labels[:D] = torch.from_numpy(np.ascontiguousarray(f["labels"], np.int32))
    scores[:D] = torch.from_numpy(np.ascontiguousarray(f["scores"], np.float32))
    cnt = torch.tensor([D if count is None else count], dtype=torch.int32)
    return ops.Detections(boxes.to(DEV), labels.to(DEV), scores.to(DEV), cnt.to(DEV), None, None, None)


def _set_gt(gt, f):
    return gt.set(f["gt_boxes"], f["gt_labels"], f["gt_iscrowd"], f["gt_area"], orig_wh=(f["w"], f["h"]), image_id=f["image_id"])


def _run(frames, num_classes, record_capacity=1 << 14, gt_capacity=128, det_capacity=None, ev=None, **kw):
    evaluation, _ = _mods()
    ev = ev or evaluation.CocoDetectionEvaluator(num_classes, record_capacity=record_capacity, gt_capacity=gt_capacity, device=DEV, **kw)
    gt = evaluation.CocoGroundTruth(gt_capacity, DEV)
    for f in frames:
        _set_gt(gt, f)
        ev.update(_dets(f, det_capacity), gt)
    return ev


def _same_records(a, b):
    assert len(a["label"]) == len(b["label"])
    for k in ("label", "image_id", "rank"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), "score"
    assert a["flags"].dtype == np.uint32 and a["flags"].shape == b["flags"].shape and np.array_equal(a["flags"], b["flags"]), "flags"


def _same_result(res, r):
    assert res["precision"].dtype == np.float64 and res["precision"].shape == r["precision"].shape
    assert np.array_equal(res["npig"], r["npig"]), "npig"
    assert np.array_equal(res["recall"], r["recall"]), "recall"
    assert np.array_equal(res["precision"], r["precision"]), "precision"
    assert np.array_equal(res["stats"], r["stats"]), (res["stats"], r["stats"])
    assert res["n_records"] == len(r["records"]["label"])


def _check(frames, num_classes, r, **kw):
    ev = _run(frames, num_classes, **kw)
    _same_records(ev.records_sorted(), r["records"])
    res = ev.summarize()
    _same_result(res, r)
    return ev, res


# ------------------------------------------------------------------------------------------------------------ 1. synthetic sets
SETS = {21: dict(num_classes=7, max_gt=24), 22: dict(num_classes=9, max_gt=128)}
_cache = {}


def _synthetic(seed):
    """(frames, num_classes, restatement's result), computed once and never modified."""
    if seed not in _cache:
        kw = SETS[seed]
        frames = ref.make_set(seed, n_images=20, **kw)
        _cache[seed] = (frames, kw["num_classes"], ref.run(frames, kw["num_classes"]))
    return _cache[seed]


@pytest.mark.parametrize("seed", sorted(SETS))
def test_synthetic_sets_bit_for_bit(seed):
    frames, nc, r = _synthetic(seed)
    kinds = ref.kinds(frames, r)
    print(kinds)
    for k, v in kinds.items():
        assert v >= 1, k
    assert max(len(f["labels"]) for f in frames) <= 300 and max(len(f["gt_labels"]) for f in frames) <= 128
    codes = set(np.unique((r["records"]["flags"][:, :, None] >> (2 * np.arange(10, dtype=np.uint32))) & 3))
    assert codes == {ref.TP, ref.FP, ref.IGNORED} and (r["stats"][[0, 1, 2, 8]] > 0).all()
    _check(frames, nc, r, det_capacity=320)


def test_frame_of_2000_detections_1024_ground_truths_16_thresholds():
    """More than 100 detections per category (the radix select), 1024 ground truths (tiles of 4 detections), all 64 chains."""
    thr = np.linspace(0.05, 0.8, 16)
    frames = [ref.make_big_frame(5, 2000, 1024, 5, image_id=3), ref.make_big_frame(6, 37, 1024, 5, image_id=1)]
    r = ref.run(frames, 5, thrs=thr)
    assert (r["npig"][:, 0] > 100).all() and len(r["records"]["label"]) == 4 * 100 + 37
    _check(frames, 5, r, gt_capacity=1024, det_capacity=2048, iou_thresholds=thr)


# ------------------------------------------------------------------------------------------------------------ 2. known answers
ONE = 1.0 / (1.0 + 2.0 ** -52)
GT_M, DET_M = [100, 100, 50, 50], [100, 100, 150, 150]
CLUTTER = [[300 + (i % 10) * 8, 300 + (i // 10) * 8, 340 + (i % 10) * 8, 340 + (i // 10) * 8] for i in range(100)]


def _known_cases():
    """The frames of tests/test_coco_eval_host.py, case by case: (name, frame, num_classes, {stat index: value} or None)."""
    f = ref.one_frame
    return [("01", f([DET_M], [0.9], [GT_M]), 2, {6: 1.0, 3: -1.0, 5: -1.0}),
            ("02a", f([DET_M, DET_M], [0.9, 0.8], [GT_M]), 2, None),
            ("02b", f([[100, 100, 150, 120], DET_M], [0.95, 0.9], [GT_M]), 2, {1: 0.5}),
            ("03", f([[0, 0, 10, 10]], [0.9], [[0, 0, 10, 5]]), 2, None),
            ("04", f([[0, 0, 10, 10], [0, 0, 10, 5], [0, 5, 10, 10]], [0.9, 0.8, 0.7], [[0, 0, 10, 5], [0, 5, 10, 5]]), 2, None),
            ("05", f([[0, 0, 80, 80]], [0.9], [[0, 0, 80, 80], [0, 0, 80, 50]], iscrowd=[1, 0]), 2, None),
            ("06", f([[210, 210, 250, 250], [220, 220, 260, 260], DET_M], [0.9, 0.8, 0.7], [[200, 200, 100, 100], GT_M], iscrowd=[1, 0]), 2, {8: 1.0}),
            ("07", f([[300, 300, 310, 310], DET_M], [0.95, 0.9], [GT_M]), 2, {0: 0.5, 3: -1.0}),
            ("08", f([[300, 300, 360, 360], [400, 300, 460, 360], DET_M], [0.9, 0.8, 0.7], [GT_M]), 2, {6: 0.0, 7: 1.0}),
            ("09a", f([DET_M] + CLUTTER, [0.1] + [0.2 + 0.005 * i for i in range(100)], [GT_M]), 2, {0: 0.0, 8: 0.0}),
            ("09b", f(CLUTTER + [DET_M], [0.5] * 101, [GT_M]), 2, {8: 0.0}),
            ("09c", f(CLUTTER[:99] + [DET_M] + CLUTTER[99:], [0.5] * 101, [GT_M]), 2, {8: 1.0}),
            ("10", f([DET_M, [300, 300, 360, 360]], [0.9, 0.8], [GT_M], labels=[0, 1]), 3, {8: 1.0})]


def test_known_answers_through_the_device():
    for name, frame, nc, stats in _known_cases():
        r = ref.run([frame], nc)
        ev, res = _check([frame], nc, r, record_capacity=256, gt_capacity=4)
        for i, v in (stats or {}).items():
            assert res["stats"][i] == v, (name, i, res["stats"][i])
        if name == "01":
            assert (res["precision"][:, :, 0, [0, 2], :] == ONE).all() and (res["precision"][:, :, 0, [1, 3], :] == -1).all()
        if name == "03":
            assert ((ev.records_sorted()["flags"][0, 0] >> (2 * np.arange(10))) & 3).tolist() == [ref.TP] + [ref.FP] * 9
        if name == "09c":
            assert (res["precision"][0, :, 0, 0, 2] == 0.01).all()


# ------------------------------------------------------------------------------------------------------------ 3. invariance
def test_shuffled_detections_and_frame_order():
    """The kernel ranks the detections itself.  Shuffled rows compare with the restatement on the same shuffled rows (ties go by
    position); with distinct scores the shuffle changes nothing at all, and neither does the order of the frames."""
    frames, nc, r = _synthetic(21)
    rng = np.random.RandomState(9)
    shuffled, distinct, distinct_shuffled = [], [], []
    for f in frames:
        p = rng.permutation(len(f["labels"]))
        g = dict(f, scores=((rng.permutation(len(p)) + 1) / np.float32(len(p) + 1)).astype(np.float32))
        shuffled.append(dict(f, boxes=f["boxes"][p], labels=f["labels"][p], scores=f["scores"][p]))
        distinct.append(g)
        distinct_shuffled.append(dict(g, boxes=g["boxes"][p], labels=g["labels"][p], scores=g["scores"][p]))
    _check(shuffled, nc, ref.run(shuffled, nc), det_capacity=320)
    a = _run(distinct, nc, det_capacity=320)
    b = _run(distinct_shuffled[::-1], nc, det_capacity=320)
    _same_records(a.records_sorted(), b.records_sorted())
    ra, rb = a.summarize(), b.summarize()
    for k in ("precision", "recall", "npig", "stats"):
        assert np.array_equal(ra[k], rb[k]), k
    c = _run(frames[::-1], nc, det_capacity=320)
    _same_records(c.records_sorted(), r["records"])
    _same_result(c.summarize(), r)


def test_merge_and_reset():
    evaluation, _ = _mods()
    frames, nc, r = _synthetic(21)
    a, b = _run(frames[0::2], nc), _run(frames[1::2], nc, record_capacity=4096)
    a.merge(b)
    _same_records(a.records_sorted(), r["records"])
    _same_result(a.summarize(), r)
    c = evaluation.CocoDetectionEvaluator(nc, record_capacity=1 << 14, device=DEV).merge(_run(frames[:7], nc).state()).merge(_run(frames[7:], nc))
    _same_records(c.records_sorted(), r["records"])
    with pytest.raises(ValueError):
        c.merge(evaluation.CocoDetectionEvaluator(nc + 1, record_capacity=16, device=DEV))
    a.reset()
    empty = a.summarize()
    assert empty["n_records"] == 0 and (empty["npig"] == 0).all() and (empty["precision"] == -1).all() and (empty["stats"] == -1).all()
    _run(frames, nc, ev=a)
    _same_records(a.records_sorted(), r["records"])
    _same_result(a.summarize(), r)


# ------------------------------------------------------------------------------------------------------------ 4. loud failure
def _bad_frame(kind):
    f = dict(ref.make_set(1, n_images=1, max_det=60, max_gt=8)[0])
    assert len(f["labels"]) >= 20 and len(f["gt_labels"]) >= 1
    if kind == "det_label":
        f["labels"] = f["labels"].copy()
        f["labels"][3] = 6                                       # num_classes = 7: labels 0 .. 5
    if kind == "gt_label":
        f["gt_labels"] = f["gt_labels"].copy()
        f["gt_labels"][0] = -1
    return f


@pytest.mark.parametrize("kind,match", [("abort", "aborted proposal scan"), ("count", "detection count exceeded"), ("gt_overflow", "more ground truths"),
                                        ("det_label", "label outside"), ("gt_label", "label outside")])
def test_every_error_bit_raises_and_the_frame_records_nothing(kind, match):
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    f = _bad_frame(kind)
    gcap = len(f["gt_labels"]) - 1 if kind == "gt_overflow" and len(f["gt_labels"]) > 1 else 8
    if kind == "gt_overflow" and len(f["gt_labels"]) == 1:
        f.update(gt_boxes=np.tile(f["gt_boxes"], (9, 1)), gt_area=np.tile(f["gt_area"], 9), gt_labels=np.tile(f["gt_labels"], 9),
                 gt_iscrowd=np.tile(f["gt_iscrowd"], 9))
    ev = evaluation.CocoDetectionEvaluator(7, record_capacity=1024, gt_capacity=8, device=DEV)
    gt = _set_gt(evaluation.CocoGroundTruth(gcap, DEV), f)
    ev.update(_dets(f, 64, count={"abort": -1, "count": 65}.get(kind)), gt)
    with pytest.raises(FrcnnError, match=match):
        ev.summarize()
    with pytest.raises(FrcnnError, match=match):
        ev.records_sorted()
    assert int(ev.cursor.item()) == 0 and int(ev.npig.sum().item()) == 0
    ev.reset()
    good = _bad_frame(None)
    ev.update(_dets(good, 64), _set_gt(evaluation.CocoGroundTruth(8, DEV), good))
    assert ev.summarize()["n_records"] == len(ref.run([good], 7)["records"]["label"])


def test_full_record_store_raises_and_counts_the_dropped():
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    frames, nc, r = _synthetic(21)
    n = len(r["records"]["label"])
    ev = _run(frames, nc, record_capacity=n - 100)
    with pytest.raises(FrcnnError, match="100 of %d records were dropped" % n):
        ev.summarize()
    with pytest.raises(FrcnnError, match="dropped"):
        ev.records_sorted()


# ------------------------------------------------------------------------------------------------------------ 5. capture
H, W, THRES = 600, 1000, 0.05
SIZES = [(500, 375), (353, 500), (480, 320)]


@pytest.fixture(scope="module")
def vgg():
    from faster_rcnn_pytorch_amd.model import FRCNN
    torch.manual_seed(0)
    m = FRCNN(num_classes=21, sampling="host").to(DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                        # as tests/test_gpu_detect.py: non-trivial RPN outputs, spread head logits and deltas
        m.rpn.cls_layer.weight.mul_(30)
        m.rpn.reg_layer.weight.mul_(10)
        m.fast_rcnn_head.cls_head.weight.copy_(torch.randn(m.fast_rcnn_head.cls_head.weight.shape, generator=g) * 0.8)
        m.fast_rcnn_head.reg_head.weight.copy_(torch.randn(m.fast_rcnn_head.reg_head.weight.shape, generator=g) * 0.5)
    return m.eval()


def _test_frames(vgg, n=3):
    """n input frames, and for each a ground truth cut from its own eager detections (so that matches exist), as frame dicts."""
    xs, frames = [], []
    for k in range(n):
        x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed((21, 41, 42)[k])).to(DEV)
        b, l, s = (t.numpy() for t in vgg.detect(x, THRES).to_host())
        assert len(l) >= 4, "degenerate test frame"
        w, h = SIZES[k]
        pick = np.arange(0, len(l), max(len(l) // (6 + k), 1))[:12]
        px = np.round(b[pick].astype(np.float64) * np.array([w, h, w, h]))
        gtb = np.stack([px[:, 0], px[:, 1], px[:, 2] - px[:, 0], px[:, 3] - px[:, 1]], 1)
        xs.append(x)
        frames.append({"image_id": 10 + k, "w": w, "h": h, "boxes": b, "labels": l, "scores": s, "gt_boxes": gtb, "gt_area": gtb[:, 2] * gtb[:, 3],
                       "gt_labels": l[pick].astype(np.int32), "gt_iscrowd": (np.arange(len(pick)) % 4 == 1).astype(np.uint8)})
    return xs, frames


def test_detect_graph_with_the_coco_evaluator_replayed_on_three_frames(vgg):
    """detect + the COCO update in one captured graph (a host sync inside update would raise during capture), replayed on three frames
    whose ground truth and image_id are written into the static buffers between the replays: equal to the eager loop and to the
    restatement on Detections.to_host()."""
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    xs, frames = _test_frames(vgg)
    r = ref.run(frames, 21)
    assert r["stats"][0] > 0 and len(r["records"]["label"]) >= 12
    ev_e = evaluation.CocoDetectionEvaluator(21, record_capacity=1 << 14, gt_capacity=16, device=DEV)
    gt = evaluation.CocoGroundTruth(16, DEV)
    for x, f in zip(xs, frames):
        _set_gt(gt, f)
        ev_e.update(vgg.detect(x, THRES), gt)
    _same_records(ev_e.records_sorted(), r["records"])
    ev_g = evaluation.CocoDetectionEvaluator(21, record_capacity=1 << 14, gt_capacity=16, device=DEV)
    dg = DetectGraph(vgg, (H, W), threshold=THRES, evaluator=ev_g, gt=gt)
    assert ev_g.summarize()["n_records"] == 0                               # warm-up and capture score nothing
    for x, f in zip(xs, frames):
        _set_gt(gt, f)
        out = dg(x)
        b, l, s = out.to_host()
        assert np.array_equal(b.numpy(), f["boxes"]) and np.array_equal(l.numpy(), f["labels"]) and np.array_equal(s.numpy(), f["scores"])
    _same_records(ev_g.records_sorted(), ev_e.records_sorted())
    rg, re_ = ev_g.summarize(), ev_e.summarize()
    for k in ("precision", "recall", "npig", "stats"):
        assert np.array_equal(rg[k], re_[k]), k
    _same_result(rg, r)


# ------------------------------------------------------------------------------------------------------------ 6. scan boundaries
RECORDS = (63, 64, 65, 255, 256, 257, 0)                        # per category: both sides of a wave and of the 256-thread chunk


def _boundary_frames():
    """Three frames (at most 100 detections of a category in each) whose categories end with RECORDS records; category 6 has ground
    truths and no detection.  Detections are exact, shifted or unrelated copies of the ground truths, pixel multiples of 1/8."""
    rng = np.random.RandomState(17)
    frames = []
    for i in range(3):
        gx, gy = rng.randint(0, 300, 28) * 1.0, rng.randint(0, 300, 28) * 1.0
        gwh = np.array([16, 24, 40, 64, 100, 120])[rng.randint(0, 6, (28, 2))] * 1.0
        gtl = np.arange(28) % 7
        px, dl = [], []
        for k, total in enumerate(RECORDS):
            mine = np.nonzero(gtl == k)[0]
            for _ in range(total // 3 + (i < total % 3)):
                g = mine[rng.randint(0, len(mine))]
                s = rng.randint(-3, 4, 2) * gwh[g] / 8.0 * (rng.rand() < 0.6)        # a shift by eighths of the box, or none
                if rng.rand() < 0.25:
                    s = s + 450.0                                                    # far from every ground truth
                px.append([gx[g] + s[0], gy[g] + s[1], gx[g] + s[0] + gwh[g, 0], gy[g] + s[1] + gwh[g, 1]])
                dl.append(k)
        frames.append(ref.one_frame(np.clip(px, 0, 1024), rng.randint(1, 50, len(dl)) / 50.0, np.stack([gx, gy, gwh[:, 0], gwh[:, 1]], 1),
                                    iscrowd=rng.rand(28) < 0.1, labels=dl, gt_labels=gtl, w=1024, h=1024, image_id=5 + i))
    return frames


def test_accumulate_scan_at_wave_and_chunk_boundaries():
    frames = _boundary_frames()
    r = ref.run(frames, 8)
    assert np.bincount(r["records"]["label"], minlength=7).tolist() == list(RECORDS) and (r["npig"][:, 0] > 0).all()
    codes = (r["records"]["flags"][:, 0] & 3)
    assert all(len(set(codes[r["records"]["label"] == k])) >= 2 for k in range(6))      # true and false positives in every segment
    _check(frames, 8, r, det_capacity=512)
