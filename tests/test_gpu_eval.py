"""The sync-free VOC AP evaluator on the device (csrc/eval.hip, faster_rcnn_pytorch_amd/evaluation.py, DetectGraph(evaluator=, gt=))
against the reference's own results (tests/golden/voc_eval.npz, from evaluation/voc_eval.py) and the restatement of its protocol
(tests/eval_ref.py, pinned to the reference on the CPU by tests/test_eval_host.py).

Records: bit for bit (order, scores, ids, the flags of every threshold).  AP: |dAP_c| <= npos_c * 2^-52 -- derived, not measured: the
integer cumulative sums and the IEEE float64 divisions are exact on both sides, only the order of the <= npos_c additions of terms
<= 1 may differ."""
import numpy as np
import pytest
import torch

import eval_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR3 = (0.3, 0.5, 0.75)


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


def _run(frames, num_classes, thr, record_capacity=1 << 16, gt_capacity=64, det_capacity=None, ev=None):
    evaluation, _ = _mods()
    ev = ev or evaluation.DetectionEvaluator(num_classes, thr, record_capacity=record_capacity, gt_capacity=gt_capacity, device=DEV)
    gt = evaluation.GroundTruth(gt_capacity, DEV)
    for f in frames:
        gt.set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), f["image_id"])
        ev.update(_dets(f, det_capacity), gt)
    return ev


def _same_records(a, b):
    assert len(a["label"]) == len(b["label"])
    for k in ("label", "image_id", "position"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)), "score"
    assert a["flags"].dtype == np.uint32 and np.array_equal(a["flags"], b["flags"]), "flags"


def _ap_within_bound(ap, ref, npos):
    """|dAP_c| <= npos_c * 2^-52; NaN exactly where npos = 0."""
    assert ap.shape == ref.shape and ap.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(ref)) and np.array_equal(np.isnan(ap[0]), npos == 0)
    for t in range(ap.shape[0]):
        for c in range(ap.shape[1]):
            if npos[c] > 0:
                d = abs(ap[t, c] - ref[t, c])
                print("t=%d class=%d npos=%d |dAP|=%.3e bound=%.3e" % (t, c, npos[c], d, npos[c] * 2.0 ** -52))
                assert d <= npos[c] * 2.0 ** -52, (t, c, ap[t, c], ref[t, c])


def _check_set(frames, num_classes, thr, ref_records, ref_npos, ref_ap=None, **kw):
    ev = _run(frames, num_classes, thr, **kw)
    _same_records(ev.records_sorted(), ref_records)
    res = ev.summarize()
    assert np.array_equal(res["npos"], ref_npos) and res["n_records"] == len(ref_records["label"])
    ap_r, _ = eval_ref.average_precision(ref_records, ref_npos, len(thr))
    _ap_within_bound(res["ap"], ap_r, ref_npos)
    if ref_ap is not None:
        _ap_within_bound(res["ap"], ref_ap, ref_npos)
    mean = eval_ref.mean_ap(res["ap"])                        # map = the reference's mean over the classes it knows, NaN classes left out
    assert np.array_equal(res["map"], mean, equal_nan=True)
    for t in range(len(thr)):
        for c in range(num_classes - 1):
            fl = (ref_records["flags"][ref_records["label"] == c] >> (2 * t)) & 3
            assert res["tp"][t, c] == (fl == eval_ref.TP).sum() and res["fp"][t, c] == (fl == eval_ref.FP).sum()
    return ev, res


# ------------------------------------------------------------------------------------------------------------ 1. frame by frame
def test_golden_set_records_and_ap(golden):
    z = golden("voc_eval")
    frames, nc, thr = eval_ref.frames_from_golden(z), int(z["num_classes"]), tuple(z["thresholds"].tolist())
    rec, npos = eval_ref.sequential(frames, nc, thr)
    assert np.array_equal(npos, z["npos"])
    _, res = _check_set(frames, nc, thr, rec, npos, ref_ap=z["ap"], det_capacity=64)
    known = [c for c in range(nc - 1) if z["npos"][c] > 0]
    bound = max(z["npos"][c] for c in known) * 2.0 ** -52 + len(known) * 2.0 ** -53     # the mean of errors <= the largest, + its own additions
    assert np.abs(res["map"] - z["map"]).max() <= bound


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_sets_records_and_ap(seed):
    frames = eval_ref.make_set(seed, n_images=50, num_classes=8, max_gt=10, max_det=80, quantise=0.1 if seed % 2 else 0.0)
    rec, npos = eval_ref.sequential(frames, 8, THR3)
    _check_set(frames, 8, THR3, rec, npos, det_capacity=7 * 300)


@pytest.mark.parametrize("G", [1, 64, 1024])
def test_frames_of_6000_detections(G):
    """D = 6000 live detections of a 6144-row capacity (24 workgroups and the last-workgroup hand-off), 16 thresholds."""
    thr = tuple(np.linspace(0.05, 0.8, 16).tolist())
    frames = [eval_ref.make_big_frame(100 + G, 6000, G, 4, image_id=0), eval_ref.make_big_frame(200 + G, 6000, G, 4, image_id=1),
              eval_ref.make_big_frame(300 + G, 37, G, 4, image_id=2)]
    rec, npos = eval_ref.parallel(frames, 4, thr, fast=True)
    assert ((rec["flags"] & 3) == eval_ref.TP).sum() >= 1
    _check_set(frames, 4, thr, rec, npos, gt_capacity=G, det_capacity=6144)


# ------------------------------------------------------------------------------------------------------------ 2. known answers
def _one(boxes, scores, gt_boxes, gt_difficult, thr=(0.5,), w=2048, h=512):
    n, g = len(boxes), len(gt_boxes)
    f = {"image_id": 0, "w": w, "h": h, "boxes": (np.array(boxes, np.float64).reshape(-1, 4) / np.array([w, h, w, h])).astype(np.float32),
         "labels": np.zeros(n, np.int32), "scores": np.array(scores, np.float32), "gt_boxes": np.array(gt_boxes, np.float32).reshape(-1, 4),
         "gt_labels": np.zeros(g, np.int32), "gt_difficult": np.array(gt_difficult, np.uint8)}
    ev = _run([f], 2, thr)
    return ev.records_sorted()["flags"].tolist(), ev.summarize()


def test_one_gt_two_identical_detections_tp_then_fp():
    flags, res = _one([[100, 100, 299, 299]] * 2, [0.5, 0.5], [[100, 100, 299, 299]], [0])
    assert flags == [eval_ref.TP, eval_ref.FP] and res["ap"][0, 0] == 1.0 and res["map"][0] == 1.0
    assert res["tp"][0, 0] == 1 and res["fp"][0, 0] == 1


def test_best_match_difficult_is_neither_tp_nor_fp():
    flags, res = _one([[100, 100, 299, 299], [600, 100, 799, 299]], [0.9, 0.8], [[100, 100, 299, 299], [600, 100, 799, 299]], [1, 0])
    assert flags == [eval_ref.IGNORED, eval_ref.TP]
    assert res["npos"][0] == 1 and res["tp"][0, 0] == 1 and res["fp"][0, 0] == 0 and res["ap"][0, 0] == 1.0      # precision unaffected


def test_overlap_equal_to_the_threshold_counts():
    """[0, 0, k - 1, 511] against [0, 0, 1279, 511] on 2048 x 512 (exact fp32 coordinates): ov = k / 1280 = 0.5 at k = 640."""
    flags, _ = _one([[0, 0, 639, 511], [0, 0, 638, 511]], [0.9, 0.8], [[0, 0, 1279, 511]], [0])
    assert flags == [eval_ref.TP, eval_ref.FP]            # ov = 0.5 counts (>=); 639 / 1280 < 0.5 does not
    flags, _ = _one([[0, 0, 638, 511]], [0.9], [[0, 0, 1279, 511]], [0], thr=(0.5, 639 / 1280))
    assert flags == [eval_ref.FP | eval_ref.TP << 2]


def test_iw_zero_is_no_overlap():
    flags, res = _one([[201, 100, 300, 200]], [0.9], [[100, 100, 200, 200]], [0], thr=(1e-9,), w=1024, h=512)
    assert flags == [eval_ref.FP] and res["ap"][0, 0] == 0.0
    flags, _ = _one([[200, 100, 300, 200]], [0.9], [[100, 100, 200, 200]], [0], thr=(1e-9,), w=1024, h=512)       # iw = 1
    assert flags == [eval_ref.TP]


# ------------------------------------------------------------------------------------------------------------ 3. invariance
def test_shuffle_merge_and_reset(golden):
    evaluation, _ = _mods()
    z = golden("voc_eval")
    frames, nc, thr = eval_ref.frames_from_golden(z), int(z["num_classes"]), tuple(z["thresholds"].tolist())
    ev = _run(frames, nc, thr)
    rec, ap = ev.records_sorted(), ev.summarize()["ap"]
    perm = np.random.RandomState(5).permutation(len(frames))
    ev2 = _run([frames[i] for i in perm], nc, thr)
    _same_records(ev2.records_sorted(), rec)
    assert np.array_equal(ev2.summarize()["ap"], ap, equal_nan=True)
    a, b = _run(frames[0::2], nc, thr), _run(frames[1::2], nc, thr, record_capacity=4096)
    a.merge(b)
    _same_records(a.records_sorted(), rec)
    ra = a.summarize()
    assert np.array_equal(ra["ap"], ap, equal_nan=True) and np.array_equal(ra["npos"], z["npos"])
    c = evaluation.DetectionEvaluator(nc, thr, record_capacity=4096, device=DEV).merge(_run(frames[:7], nc, thr).state()).merge(_run(frames[7:], nc, thr))
    _same_records(c.records_sorted(), rec)
    ev.reset()
    assert ev.summarize()["n_records"] == 0
    _run(frames, nc, thr, ev=ev)
    _same_records(ev.records_sorted(), rec)
    assert np.array_equal(ev.summarize()["ap"], ap, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ 4. loud failure
def test_full_record_store_raises_and_counts_the_dropped(golden):
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    z = golden("voc_eval")
    frames, nc = eval_ref.frames_from_golden(z), int(z["num_classes"])
    n = len(z["det_labels"])
    ev = _run(frames, nc, (0.5,), record_capacity=n - 100)
    with pytest.raises(FrcnnError, match="100 of %d records were dropped" % n):
        ev.summarize()
    with pytest.raises(FrcnnError, match="dropped"):
        ev.records_sorted()


def test_count_minus_one_raises():
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    f = eval_ref.make_set(1, n_images=1)[0]
    ev = evaluation.DetectionEvaluator(6, device=DEV, record_capacity=1024)
    gt = evaluation.GroundTruth(64, DEV).set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), 0)
    ev.update(_dets(f, 64, count=-1), gt)
    with pytest.raises(FrcnnError, match="aborted proposal scan"):
        ev.summarize()
    ev.reset()
    ev.update(_dets(f, 64), gt)
    assert ev.summarize()["n_records"] == len(f["labels"])


def test_more_ground_truths_than_capacity_raises():
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    f = eval_ref.make_big_frame(1, 50, 9, 4)
    ev = evaluation.DetectionEvaluator(4, device=DEV, record_capacity=1024, gt_capacity=8)
    gt = evaluation.GroundTruth(8, DEV).set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), 0)
    ev.update(_dets(f), gt)
    with pytest.raises(FrcnnError, match="more ground truths"):
        ev.summarize()


# ------------------------------------------------------------------------------------------------------------ 5. capture
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


H, W, THRES = 600, 1000, 0.05
SIZES = [(500, 375), (353, 500), (480, 320), (500, 333)]


def _test_frames(vgg, n=4):
    """n input frames, and for each a ground truth cut from its own eager detections (so that matches exist), as frame dicts."""
    xs, frames = [], []
    for k in range(n):
        x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed((21, 41, 42, 43)[k % 4] + 100 * (k // 4))).to(DEV)
        b, l, s = (t.numpy() for t in vgg.detect(x, THRES).to_host())
        assert len(l) >= 4, "degenerate test frame"
        w, h = SIZES[k % len(SIZES)]
        pick = np.arange(0, len(l), max(len(l) // (6 + k), 1))[:12]
        gtb = np.round(b[pick].astype(np.float64) * np.array([w, h, w, h])).astype(np.float32)
        xs.append(x)
        frames.append({"image_id": 10 + k, "w": w, "h": h, "boxes": b, "labels": l, "scores": s, "gt_boxes": gtb, "gt_labels": l[pick].astype(np.int32),
                       "gt_difficult": (np.arange(len(pick)) % 4 == 1).astype(np.uint8)})
    return xs, frames


def _set_gt(gt, f):
    gt.set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), f["image_id"])


def test_detect_and_update_capture_into_one_graph(vgg):
    """A host sync inside update would raise during capture.  The replays see the ground truth and image_id written into the static
    buffers between them."""
    evaluation, _ = _mods()
    xs, frames = _test_frames(vgg)
    rec, npos = eval_ref.sequential(frames, 21, THR3)                       # Detections.to_host() + the restatement
    assert ((rec["flags"] & 3) == eval_ref.TP).sum() >= 4 and ((rec["flags"] & 3) == eval_ref.FP).sum() >= 4
    # eager loop
    ev_e = evaluation.DetectionEvaluator(21, THR3, record_capacity=1 << 15, gt_capacity=16, device=DEV)
    gt = evaluation.GroundTruth(16, DEV)
    for x, f in zip(xs, frames):
        _set_gt(gt, f)
        ev_e.update(vgg.detect(x, THRES), gt)
    _same_records(ev_e.records_sorted(), rec)
    # one graph: detect + update
    ev_g = evaluation.DetectionEvaluator(21, THR3, record_capacity=1 << 15, gt_capacity=16, device=DEV)
    xbuf = xs[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev_g.update(vgg.detect(xbuf, THRES), gt)
    torch.cuda.current_stream().wait_stream(s)
    ev_g.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev_g.update(vgg.detect(xbuf, THRES), gt)
    ev_g.reset()                                                            # whatever the capture itself may have run
    for x, f in zip(xs, frames):
        xbuf.copy_(x)
        _set_gt(gt, f)
        g.replay()
    _same_records(ev_g.records_sorted(), ev_e.records_sorted())
    _same_records(ev_g.records_sorted(), rec)
    rg, re_ = ev_g.summarize(), ev_e.summarize()
    assert np.array_equal(rg["ap"], re_["ap"], equal_nan=True) and np.array_equal(rg["npos"], npos)
    ap_r, _ = eval_ref.average_precision(rec, npos, 3)
    _ap_within_bound(rg["ap"], ap_r, npos)


def test_detect_graph_with_an_evaluator(vgg):
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    xs, frames = _test_frames(vgg)
    rec, npos = eval_ref.sequential(frames, 21, THR3)
    ev = evaluation.DetectionEvaluator(21, THR3, record_capacity=1 << 15, gt_capacity=16, device=DEV)
    gt = evaluation.GroundTruth(16, DEV)
    dg = DetectGraph(vgg, (H, W), threshold=THRES, evaluator=ev, gt=gt)
    assert ev.summarize()["n_records"] == 0                                 # warm-up and capture score nothing
    for x, f in zip(xs, frames):
        _set_gt(gt, f)
        out = dg(x)
        b, l, s = out.to_host()
        assert np.array_equal(b.numpy(), f["boxes"]) and np.array_equal(l.numpy(), f["labels"]) and np.array_equal(s.numpy(), f["scores"])
    _same_records(ev.records_sorted(), rec)
    res = ev.summarize()
    ap_r, _ = eval_ref.average_precision(rec, npos, 3)
    _ap_within_bound(res["ap"], ap_r, npos)
    with pytest.raises(ValueError):
        DetectGraph(vgg, (H, W), threshold=THRES, evaluator=ev)


def test_detect_graph_without_an_evaluator_is_unchanged(vgg):
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    xa = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(41)).to(DEV)
    xb = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(42)).to(DEV)
    ea, eb = [t.clone() for t in vgg.detect(xa, THRES).to_host()], [t.clone() for t in vgg.detect(xb, THRES).to_host()]
    dg = DetectGraph(vgg, (H, W), threshold=THRES)
    assert dg.evaluator is None and dg.gt is None
    for x, e in ((xa, ea), (xb, eb), (xa, ea)):
        r = dg(x).to_host()
        assert len(e[1]) > 0 and all(torch.equal(p, q) for p, q in zip(r, e))


# ------------------------------------------------------------------------------------------------------------ 6. scan boundaries
SEGMENTS = (0, 1, 63, 64, 65, 255, 256, 257, 513)               # records per class: both sides of a wave and of the 256-thread chunk


def test_ap_scan_at_wave_and_chunk_boundaries():
    """ops.eval_average_precision on hand-built sorted records, two thresholds, random TP / FP / IGNORED codes.  Class 1 (one record)
    has npos = 0, class 3 (64 records) no true positive, class 0 no record at all.  tp / fp totals are the counts of the codes; AP
    within npos_c * 2^-52 of the restatement, NaN exactly where npos = 0."""
    _, ops = _mods()
    rng = np.random.RandomState(3)
    nc, n, cap = len(SEGMENTS), sum(SEGMENTS), sum(SEGMENTS) + 26
    label = np.repeat(np.arange(nc), SEGMENTS).astype(np.int32)
    codes = rng.choice([eval_ref.TP, eval_ref.FP, eval_ref.IGNORED], (n, 2), p=[0.35, 0.45, 0.2]).astype(np.uint32)
    codes[label == 3] = rng.choice([eval_ref.FP, eval_ref.IGNORED], (64, 2))
    flags = codes[:, 0] | codes[:, 1] << 2
    tp = np.array([[((codes[:, t] == eval_ref.TP) & (label == c)).sum() for c in range(nc)] for t in range(2)])
    fp = np.array([[((codes[:, t] == eval_ref.FP) & (label == c)).sum() for c in range(nc)] for t in range(2)])
    npos = tp.max(0) + rng.randint(0, 4, nc)                     # recall <= 1
    npos[0], npos[1], npos[3] = 3, 0, 5
    assert tp[:, 3].sum() == 0 and (tp[:, 4:] > 0).all() and (fp[:, 4:] > 0).all()
    dead = np.full(cap - n, 0x7FFFFFFF, np.int32)                # the slots past the cursor, as _sorted() leaves them
    ap_d, tp_d, fp_d = ops.eval_average_precision(torch.from_numpy(np.concatenate([label, dead])).to(DEV),
                                                  torch.from_numpy(np.concatenate([flags, dead.view(np.uint32)]).view(np.int32)).to(DEV),
                                                  torch.tensor([n], dtype=torch.int64, device=DEV), torch.from_numpy(npos).to(DEV), 2, nc + 1)
    assert np.array_equal(tp_d.cpu().numpy(), tp) and np.array_equal(fp_d.cpu().numpy(), fp)
    ap_r, _ = eval_ref.average_precision({"flags": flags, "label": label}, npos, 2)
    assert ap_r[0, 0] == 0.0 and ap_r[0, 3] == 0.0 and (ap_r[:, 4:] > 0).all()
    _ap_within_bound(ap_d.cpu().numpy(), ap_r, npos)
