"""Detection evaluator on the device: the VOC average-precision protocol of the reference (evaluation/voc_eval.py:67-112 save_pred,
:115-135 voc_ap, :138-225 cal_mAP), fed by ops.Detections without a host sync.

The reference's test loop (test.py:60) is predict + evaluator; its evaluator goes through JSON files on disk.  Here

    ev = DetectionEvaluator(num_classes=21, iou_thresholds=(0.5,))
    gt = GroundTruth(capacity=64, device=dev)
    for image_id, (x, boxes_px, labels, difficult, (w, h)) in enumerate(test_set):
        gt.set(boxes_px, labels, difficult, (w, h), image_id)
        ev.update(model.detect(x, 0.05), gt)          # one HIP launch on the current stream, no sync: capturable with detect
    res = ev.summarize()                              # the only device -> host copy: res["ap"][0], res["map"][0]

Matches, counters and score records stay in HBM for the whole test set.  Labels are the detections' 0-based labels (class c of
num_classes - 1).  The order of the records is defined as (score descending, image_id ascending, position ascending) -- Python's
stable sort over the reference's insertion order -- so image_id must follow the order in which the reference would have seen the images.
Not reproduced: save_pred's `class_num == 20: continue` (a FIXME for a background id that never occurs with 0-based labels).

The COCO protocol -- what the reference's test loop actually reports (test.py:17-18, 60-88, 124-128: CocoEvaluator.update / accumulate /
summarize, i.e. pycocotools' COCOeval for iouType "bbox" with useCats = 1) -- runs on the same kind of record store:

    ev = CocoDetectionEvaluator(num_classes=91, device=dev)
    gt = CocoGroundTruth(capacity=128, device=dev)
    for image_id, x, anns, (w, h) in test_set:        # ascending image_id is the protocol's order; any order of calls gives the same result
        gt.set(boxes_xywh, labels, iscrowd, area, orig_wh=(w, h), image_id=image_id)
        ev.update(model.detect(x, 0.05), gt)          # one HIP launch, no sync, capturable: DetectGraph(model, hw, evaluator=ev, gt=gt)
    res = ev.summarize()                              # the only device -> host copy: res["stats"] = COCOeval.stats (12 numbers)

The evaluator takes the xyxy boxes of detect; the reference also passes predict's boxes through cxcy_to_xy (test.py:68), which is the
caller's business.  Restated from the published algorithm and NOT pinned to pycocotools' own code, which is not available to this
project's tests (docs/PARITY.md); tests/test_coco_crosscheck.py compares with it wherever it can be imported.
Not built: the segm and keypoints IoU types, useCats = 0."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import FrcnnError

MAX_THRESHOLDS, MAX_GT, MAX_CLASSES = 16, 1024, 256


class GroundTruth(object):
    """Fixed-capacity device buffers of one frame's ground truth: boxes [capacity,4] f32 pixel xyxy, labels i32, difficult u8, n i32[1],
    frame i32[3] = (original width, original height, image_id).  set() copies in place and never reallocates, so a captured graph that
    read these buffers sees the new frame at its next replay."""

    def __init__(self, capacity, device):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_GT:
            raise ValueError("GroundTruth: capacity %d outside 1 .. %d" % (capacity, MAX_GT))
        self.capacity = capacity
        self.device = torch.device(device)
        # one allocation, so that a frame from the host is ONE copy: (w, h, image_id, n) | boxes | labels | difficult
        self._o_lab, self._o_dif = 16 + 16 * capacity, 16 + 20 * capacity
        self._buf = torch.zeros(16 + 21 * capacity, dtype=torch.uint8, device=self.device)
        self.frame = self._buf[0:12].view(torch.int32)
        self.n = self._buf[12:16].view(torch.int32)
        self.boxes = self._buf[16:self._o_lab].view(torch.float32).view(capacity, 4)
        self.labels = self._buf[self._o_lab:self._o_dif].view(torch.int32)
        self.difficult = self._buf[self._o_dif:]
        # pinned staging buffers in a ring: the copy of frame k is asynchronous, so frame k + 1 must not be written over it.  A slot is
        # reused only after the event behind its last copy has completed (it has, unless the host runs 8 frames ahead).
        self._ring = [torch.zeros(16 + 21 * capacity, dtype=torch.uint8) for _ in range(8)]
        if self.device.type == "cuda":
            self._ring = [h.pin_memory() for h in self._ring]
        self._events = [None] * len(self._ring)
        self._k = 0

    def _stage(self):
        k = self._k % len(self._ring)
        self._k += 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        return k, self._ring[k]

    def _sent(self, k):
        if self.device.type == "cuda":
            self._events[k] = torch.cuda.Event()
            self._events[k].record(torch.cuda.current_stream(self.device))

    def set(self, boxes_px, labels, difficult, orig_wh, image_id):
        """boxes_px [n,4] pixel xyxy, labels [n] (0-based), difficult [n] (0 / 1 or None), orig_wh = (w, h) of the original image,
        image_id = the image's sequence number.  Host arrays go over in one copy; device tensors are copied in place (no sync).  More
        rows than the capacity are NOT silently cut: n keeps the true number and the evaluator's update reports the overflow."""
        n = int(len(labels))
        m = min(n, self.capacity)
        head = np.array([int(orig_wh[0]), int(orig_wh[1]), int(image_id), n], np.int32)
        if isinstance(boxes_px, torch.Tensor) and boxes_px.is_cuda:
            self.boxes[:m].copy_(boxes_px.reshape(-1, 4)[:m].to(torch.float32))
            self.labels[:m].copy_(labels[:m].to(torch.int32))
            if difficult is None:
                self.difficult[:m].zero_()
            else:
                self.difficult[:m].copy_(difficult[:m].to(torch.uint8))
            k, host = self._stage()
            host[:16].copy_(torch.from_numpy(head.view(np.uint8)))
            self._buf[:16].copy_(host[:16], non_blocking=True)
            self._sent(k)
            return self
        k, host = self._stage()
        h = host.numpy()
        h[:16] = head.view(np.uint8)
        h[16:16 + 16 * m] = np.ascontiguousarray(np.asarray(boxes_px, np.float32).reshape(-1, 4)[:m]).view(np.uint8).reshape(-1)
        h[self._o_lab:self._o_lab + 4 * m] = np.ascontiguousarray(np.asarray(labels, np.int32)[:m]).view(np.uint8)
        h[self._o_dif:self._o_dif + m] = 0 if difficult is None else np.asarray(difficult)[:m].astype(np.uint8)
        self._buf.copy_(host, non_blocking=True)
        self._sent(k)
        return self


def _score_key(score):
    """fp32 scores -> int64 keys that ascend as the score DESCENDS (-0 folded onto +0: Python's sort sees them as equal)."""
    u = (score + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    o = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    return 0xFFFFFFFF - o


class DetectionEvaluator(object):
    """VOC AP at T IoU thresholds in one pass.  update() is one HIP launch on the current stream and has no host sync; summarize() does
    the only device -> host copy."""

    def __init__(self, num_classes, iou_thresholds=(0.5,), record_capacity=1 << 20, gt_capacity=128, device=None):
        thr = [float(t) for t in iou_thresholds]
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("DetectionEvaluator: num_classes %d outside 2 .. %d" % (num_classes, MAX_CLASSES))
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError("DetectionEvaluator: %d IoU thresholds, 1 .. %d supported" % (len(thr), MAX_THRESHOLDS))
        if not 1 <= int(gt_capacity) <= MAX_GT:
            raise ValueError("DetectionEvaluator: gt_capacity %d outside 1 .. %d" % (gt_capacity, MAX_GT))
        if int(record_capacity) < 1:
            raise ValueError("DetectionEvaluator: record_capacity must be >= 1")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("DetectionEvaluator runs only on a HIP device (no CPU fallback)")
        self.device = dev
        self.num_classes = int(num_classes)
        self.iou_thresholds = tuple(thr)
        self.record_capacity = int(record_capacity)
        self.gt_capacity = int(gt_capacity)
        self.thresholds = torch.tensor(thr, dtype=torch.float64, device=dev)
        cap = self.record_capacity
        self.rec_score = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.rec_label = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_image = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_position = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_flags = torch.zeros(cap, dtype=torch.int32, device=dev)          # bit pattern: 2 bits per threshold
        self.npos = torch.zeros(self.num_classes - 1, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = {}

    # ---- per frame ----------------------------------------------------------------------------------------------------------
    def _workspace(self, D, G):
        """The update kernel's ticket and winner words: zero before the first call, left zero by the kernel, owned by this evaluator."""
        ws = self._ws.get((D, G))
        if ws is None:
            nb = _lib.workspace_bytes(_lib.OP_EVAL, D, G)
            if nb == 0:
                raise FrcnnError("eval_update: detection capacity %d / ground-truth capacity %d outside the kernel's limits" % (D, G))
            ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)
            self._ws[(D, G)] = ws
        return ws

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame, gt = its GroundTruth.  No sync; capturable into a graph with detect."""
        if gt.capacity > self.gt_capacity:
            raise ValueError("DetectionEvaluator: GroundTruth capacity %d > gt_capacity %d" % (gt.capacity, self.gt_capacity))
        ops.eval_update(dets, gt.boxes, gt.labels, gt.difficult, gt.n, gt.frame, self.thresholds, self.num_classes, self.npos, self.rec_score,
                        self.rec_label, self.rec_image, self.rec_position, self.rec_flags, self.cursor, self.error,
                        workspace=self._workspace(dets.labels.numel(), gt.capacity))

    def reset(self):
        self.cursor.zero_()
        self.npos.zero_()
        self.error.zero_()

    # ---- per test set -------------------------------------------------------------------------------------------------------
    def _records(self):
        return (self.rec_score, self.rec_label, self.rec_image, self.rec_position, self.rec_flags)

    def state(self):
        """The evaluator's state as device tensors (one sync for the record count): the live records in slot order, npos, n_records
        (what update counted: more than len(score) when the store overflowed) and the error word."""
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        s = dict(zip(("score", "label", "image_id", "position", "flags"), (r[:n].clone() for r in self._records())))
        s.update(npos=self.npos.clone(), n_records=n_all, error=self.error.clone(), iou_thresholds=self.iou_thresholds, num_classes=self.num_classes)
        return s

    def merge(self, other):
        """Appends the records of `other` (a DetectionEvaluator, or a state() of one, of the same classes and thresholds) and adds its
        counters: evaluating shards separately and merging equals one evaluator over all of them."""
        s = other.state() if isinstance(other, DetectionEvaluator) else other
        if tuple(s["iou_thresholds"]) != self.iou_thresholds or s["num_classes"] != self.num_classes:
            raise ValueError("DetectionEvaluator.merge: the evaluators differ in classes or thresholds")
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        m = min(int(s["score"].numel()), self.record_capacity - n)
        for dst, key in zip(self._records(), ("score", "label", "image_id", "position", "flags")):
            dst[n:n + m].copy_(s[key][:m].to(self.device))
        self.cursor += int(s["n_records"])                     # keeps counting past the capacity: summarize() reports the loss
        self.npos += s["npos"].to(self.device)
        self.error |= s["error"].to(self.device)
        return self

    def _sorted(self):
        """(order, labels_sorted) on the device, no sync: the live slots first, in (label ascending, score descending, image_id
        ascending, position ascending); the slots past the cursor sort behind every class."""
        cap = self.record_capacity
        live = torch.arange(cap, device=self.device) < self.cursor
        o1 = torch.sort((self.rec_image.to(torch.int64) << 32) | self.rec_position.to(torch.int64), stable=True)[1]
        lab = torch.where(live, self.rec_label, torch.full_like(self.rec_label, 0x7FFFFFFF))
        key = ((lab.to(torch.int64) << 32) | _score_key(self.rec_score))[o1]
        o2 = torch.sort(key, stable=True)[1]
        order = o1[o2]
        return order, lab[order].contiguous()

    def _raise_on_error(self, err, n_all):
        if err:
            what = [w for b, w in ((_lib.EVAL_ERR_UPSTREAM_ABORT, "a frame's detection count was -1 (an aborted proposal scan upstream)"),
                                   (_lib.EVAL_ERR_GT_OVERFLOW, "a frame had more ground truths than the GroundTruth capacity"),
                                   (_lib.EVAL_ERR_COUNT_RANGE, "a frame's detection count exceeded its capacity"),
                                   (_lib.EVAL_ERR_LABEL_RANGE, "a label outside 0 .. num_classes - 2")) if err & b]
            raise FrcnnError("DetectionEvaluator: error word %d: %s" % (err, "; ".join(what)))
        if n_all > self.record_capacity:
            raise FrcnnError("DetectionEvaluator: the record store is full: %d of %d records were dropped (record_capacity = %d)"
                             % (n_all - self.record_capacity, n_all, self.record_capacity))

    def summarize(self):
        """{"ap": float64 [T, C-1] (NaN for the classes without a countable ground truth), "map": float64 [T] (the mean over the other
        classes, voc_eval.py:249-257), "npos": int64 [C-1], "n_records", "tp", "fp": int64 [T, C-1]}.  Raises FrcnnError when a frame
        reported an error or records were dropped.  One device -> host copy."""
        T, nc = len(self.iou_thresholds), self.num_classes - 1
        order, lab = self._sorted()
        ap, tp, fp = ops.eval_average_precision(lab, self.rec_flags[order].contiguous(), self.cursor, self.npos, T, self.num_classes)
        host = torch.cat([ap.view(torch.int64).reshape(-1), tp.reshape(-1), fp.reshape(-1), self.npos, self.cursor,
                          self.error.to(torch.int64)]).cpu().numpy()
        k = T * nc
        self._raise_on_error(int(host[3 * k + nc + 1]), int(host[3 * k + nc]))
        ap_h = host[:k].copy().view(np.float64).reshape(T, nc)
        mean = np.full(T, np.nan, np.float64)
        for t in range(T):                                     # sum_AP / len(gt_classes): added in class order like the reference
            vals = [float(v) for v in ap_h[t] if not np.isnan(v)]
            if vals:
                mean[t] = sum(vals, 0.0) / len(vals)
        return {"ap": ap_h, "map": mean, "npos": host[3 * k:3 * k + nc].copy(), "n_records": int(host[3 * k + nc]),
                "tp": host[k:2 * k].reshape(T, nc).copy(), "fp": host[2 * k:3 * k].reshape(T, nc).copy()}

    def records_sorted(self):
        """The records on the host in the order (label ascending, score descending, image_id ascending, position ascending): score
        f32, label i32, image_id i32, position i32, flags u32 (2 bits per threshold: _lib.EVAL_TP / EVAL_FP / EVAL_IGNORED).  For tests
        and for precision / recall curves."""
        order, _ = self._sorted()
        n_all, err = int(self.cursor.item()), int(self.error.item())
        self._raise_on_error(err, n_all)
        out = {k: r[order[:n_all]].cpu().numpy() for k, r in zip(("score", "label", "image_id", "position", "flags"), self._records())}
        out["flags"] = out["flags"].view(np.uint32)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the COCO protocol (bbox, useCats = 1)
# ---------------------------------------------------------------------------------------------------------------------------------
COCO_MAX_DET = 100
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large


class CocoGroundTruth(object):
    """Fixed-capacity device buffers of one frame's COCO annotations: boxes [capacity,4] f64 pixel xywh, area f64, labels i32, iscrowd
    u8, n i32[1], frame i32[3] = (original width, original height, image_id).  The same contract as GroundTruth: one allocation, a
    pinned staging ring, set() copies in place and never reallocates, n keeps the true count on overflow."""

    def __init__(self, capacity, device):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_GT:
            raise ValueError("CocoGroundTruth: capacity %d outside 1 .. %d" % (capacity, MAX_GT))
        self.capacity = capacity
        self.device = torch.device(device)
        # one allocation, so that a frame from the host is ONE copy: (w, h, image_id, n) | boxes f64 | area f64 | labels | iscrowd
        self._o_area, self._o_lab, self._o_crowd = 16 + 32 * capacity, 16 + 40 * capacity, 16 + 44 * capacity
        nbytes = 16 + 45 * capacity
        self._buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.frame = self._buf[0:12].view(torch.int32)
        self.n = self._buf[12:16].view(torch.int32)
        self.boxes = self._buf[16:self._o_area].view(torch.float64).view(capacity, 4)
        self.area = self._buf[self._o_area:self._o_lab].view(torch.float64)
        self.labels = self._buf[self._o_lab:self._o_crowd].view(torch.int32)
        self.iscrowd = self._buf[self._o_crowd:]
        self._ring = [torch.zeros(nbytes, dtype=torch.uint8) for _ in range(8)]
        if self.device.type == "cuda":
            self._ring = [h.pin_memory() for h in self._ring]
        self._events = [None] * len(self._ring)
        self._k = 0

    _stage = GroundTruth._stage
    _sent = GroundTruth._sent

    def set(self, boxes_xywh, labels, iscrowd=None, area=None, orig_wh=None, image_id=0):
        """boxes_xywh [n,4] pixel xywh (float64 is kept), labels [n] (0-based), iscrowd [n] (0 / 1 or None), area [n] (the annotations'
        own areas; None = w * h of the box), orig_wh = (w, h) of the original image, image_id = the image's id.  Host arrays go over in
        one copy; device tensors are copied in place (no sync).  More rows than the capacity are NOT silently cut: n keeps the true
        number and the evaluator's update reports the overflow."""
        if orig_wh is None:
            raise ValueError("CocoGroundTruth.set: orig_wh = (w, h) is required")
        n = int(len(labels))
        m = min(n, self.capacity)
        head = np.array([int(orig_wh[0]), int(orig_wh[1]), int(image_id), n], np.int32)
        if isinstance(boxes_xywh, torch.Tensor) and boxes_xywh.is_cuda:
            b = boxes_xywh.reshape(-1, 4)[:m].to(torch.float64)
            self.boxes[:m].copy_(b)
            self.area[:m].copy_(b[:, 2] * b[:, 3] if area is None else area[:m].to(torch.float64))
            self.labels[:m].copy_(labels[:m].to(torch.int32))
            if iscrowd is None:
                self.iscrowd[:m].zero_()
            else:
                self.iscrowd[:m].copy_(iscrowd[:m].to(torch.uint8))
            k, host = self._stage()
            host[:16].copy_(torch.from_numpy(head.view(np.uint8)))
            self._buf[:16].copy_(host[:16], non_blocking=True)
            self._sent(k)
            return self
        k, host = self._stage()
        h = host.numpy()
        b = np.ascontiguousarray(np.asarray(boxes_xywh, np.float64).reshape(-1, 4)[:m])
        ar = b[:, 2] * b[:, 3] if area is None else np.ascontiguousarray(np.asarray(area, np.float64).reshape(-1)[:m])
        h[:16] = head.view(np.uint8)
        h[16:16 + 32 * m] = b.view(np.uint8).reshape(-1)
        h[self._o_area:self._o_area + 8 * m] = ar.view(np.uint8)
        h[self._o_lab:self._o_lab + 4 * m] = np.ascontiguousarray(np.asarray(labels, np.int32)[:m]).view(np.uint8)
        h[self._o_crowd:self._o_crowd + m] = 0 if iscrowd is None else (np.asarray(iscrowd)[:m] != 0).astype(np.uint8)
        self._buf.copy_(host, non_blocking=True)
        self._sent(k)
        return self


class CocoDetectionEvaluator(object):
    """COCOeval (bbox, useCats = 1) over a record store in HBM.  update() is one HIP launch on the current stream and has no host sync;
    summarize() runs the accumulate kernel, does the only device -> host copy and takes the 12 means with numpy as pycocotools does."""

    def __init__(self, num_classes, record_capacity=1 << 20, gt_capacity=128, device=None, iou_thresholds=None, max_dets=(1, 10, 100)):
        thr = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thresholds is None \
            else np.array([float(t) for t in iou_thresholds], np.float64)
        md = tuple(int(v) for v in max_dets)
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("CocoDetectionEvaluator: num_classes %d outside 2 .. %d" % (num_classes, MAX_CLASSES))
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError("CocoDetectionEvaluator: %d IoU thresholds, 1 .. %d supported" % (len(thr), MAX_THRESHOLDS))
        if not 1 <= int(gt_capacity) <= MAX_GT:
            raise ValueError("CocoDetectionEvaluator: gt_capacity %d outside 1 .. %d" % (gt_capacity, MAX_GT))
        if int(record_capacity) < 1:
            raise ValueError("CocoDetectionEvaluator: record_capacity must be >= 1")
        if len(md) != 3 or list(md) != sorted(md) or md[0] < 1 or md[2] > COCO_MAX_DET:
            raise ValueError("CocoDetectionEvaluator: max_dets must be three ascending values in 1 .. %d" % COCO_MAX_DET)
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("CocoDetectionEvaluator runs only on a HIP device (no CPU fallback)")
        self.device = dev
        self.num_classes = int(num_classes)
        self.iou_thresholds = tuple(float(t) for t in thr)
        self.max_dets = md
        self.record_capacity = int(record_capacity)
        self.gt_capacity = int(gt_capacity)
        self.thresholds = torch.from_numpy(thr.copy()).to(dev)
        self.rec_thresholds_host = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.rec_thresholds = torch.from_numpy(self.rec_thresholds_host.copy()).to(dev)
        cap = self.record_capacity
        self.rec_score = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.rec_label = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_image = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_rank = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_flags = torch.zeros((cap, 4), dtype=torch.int32, device=dev)     # per area range: 2 bits per threshold
        self.npig = torch.zeros((self.num_classes - 1, 4), dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = {}

    # ---- per frame ----------------------------------------------------------------------------------------------------------
    def _workspace(self, D, G):
        """The update kernel's key segments: owned by this evaluator, so that a captured graph keeps a valid address."""
        ws = self._ws.get((D, G))
        if ws is None:
            nb = _lib.workspace_bytes(_lib.OP_COCO_EVAL, D, G)
            if nb == 0:
                raise FrcnnError("coco_eval_update: detection capacity %d / ground-truth capacity %d outside the kernel's limits" % (D, G))
            ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)
            self._ws[(D, G)] = ws
        return ws

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame (rows in any order), gt = its CocoGroundTruth.  No sync; capturable
        into a graph with detect."""
        if gt.capacity > self.gt_capacity:
            raise ValueError("CocoDetectionEvaluator: CocoGroundTruth capacity %d > gt_capacity %d" % (gt.capacity, self.gt_capacity))
        ops.coco_eval_update(dets, gt.boxes, gt.area, gt.labels, gt.iscrowd, gt.n, gt.frame, self.thresholds, self.num_classes, self.max_dets[-1],
                             self.npig, self.rec_score, self.rec_label, self.rec_image, self.rec_rank, self.rec_flags, self.cursor, self.error,
                             workspace=self._workspace(dets.labels.numel(), gt.capacity))

    def reset(self):
        self.cursor.zero_()
        self.npig.zero_()
        self.error.zero_()

    # ---- per test set -------------------------------------------------------------------------------------------------------
    _KEYS = ("score", "label", "image_id", "rank", "flags")

    def _records(self):
        return (self.rec_score, self.rec_label, self.rec_image, self.rec_rank, self.rec_flags)

    def _config(self):
        return (self.iou_thresholds, self.num_classes, self.max_dets)

    def state(self):
        """The evaluator's state as device tensors (one sync for the record count): the live records in slot order, npig, n_records
        (what update counted: more than len(score) when the store overflowed) and the error word."""
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        s = dict(zip(self._KEYS, (r[:n].clone() for r in self._records())))
        s.update(npig=self.npig.clone(), n_records=n_all, error=self.error.clone(), config=self._config())
        return s

    def merge(self, other):
        """Appends the records of `other` (a CocoDetectionEvaluator, or a state() of one, of the same classes, thresholds and maxDets)
        and adds its counters: evaluating shards separately and merging equals one evaluator over all of them."""
        s = other.state() if isinstance(other, CocoDetectionEvaluator) else other
        if s["config"] != self._config():
            raise ValueError("CocoDetectionEvaluator.merge: the evaluators differ in classes, thresholds or maxDets")
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        m = min(int(s["score"].numel()), self.record_capacity - n)
        for dst, key in zip(self._records(), self._KEYS):
            dst[n:n + m].copy_(s[key][:m].to(self.device))
        self.cursor += int(s["n_records"])                     # keeps counting past the capacity: summarize() reports the loss
        self.npig += s["npig"].to(self.device)
        self.error |= s["error"].to(self.device)
        return self

    def _sorted(self):
        """(order, labels_sorted) on the device, no sync: the live slots first, in (label ascending, score descending, image_id
        ascending, rank ascending); the slots past the cursor sort behind every class."""
        cap = self.record_capacity
        live = torch.arange(cap, device=self.device) < self.cursor
        o1 = torch.sort((self.rec_image.to(torch.int64) << 32) | self.rec_rank.to(torch.int64), stable=True)[1]
        lab = torch.where(live, self.rec_label, torch.full_like(self.rec_label, 0x7FFFFFFF))
        key = ((lab.to(torch.int64) << 32) | _score_key(self.rec_score))[o1]
        o2 = torch.sort(key, stable=True)[1]
        order = o1[o2]
        return order, lab[order].contiguous()

    def _raise_on_error(self, err, n_all):
        if err:
            what = [w for b, w in ((_lib.EVAL_ERR_UPSTREAM_ABORT, "a frame's detection count was -1 (an aborted proposal scan upstream)"),
                                   (_lib.EVAL_ERR_GT_OVERFLOW, "a frame had more ground truths than the CocoGroundTruth capacity"),
                                   (_lib.EVAL_ERR_COUNT_RANGE, "a frame's detection count exceeded its capacity"),
                                   (_lib.EVAL_ERR_LABEL_RANGE, "a label outside 0 .. num_classes - 2")) if err & b]
            raise FrcnnError("CocoDetectionEvaluator: error word %d: %s" % (err, "; ".join(what)))
        if n_all > self.record_capacity:
            raise FrcnnError("CocoDetectionEvaluator: the record store is full: %d of %d records were dropped (record_capacity = %d)"
                             % (n_all - self.record_capacity, n_all, self.record_capacity))

    def summarize(self):
        """{"stats": float64 [12] (COCOeval.stats: AP, AP50, AP75, APs, APm, APl, AR@maxDets[0], AR@maxDets[1], AR@maxDets[2], ARs, ARm,
        ARl), "precision": float64 [T, 101, K, 4, 3], "recall": float64 [T, K, 4, 3] (-1 where npig == 0), "npig": int64 [K, 4],
        "n_records"}.  Raises FrcnnError when a frame reported an error or records were dropped.  One device -> host copy."""
        T, nc, R = len(self.iou_thresholds), self.num_classes - 1, self.rec_thresholds.numel()
        order, lab = self._sorted()
        precision, recall = ops.coco_eval_accumulate(lab, self.rec_rank[order].contiguous(), self.rec_flags[order].contiguous(), self.cursor,
                                                     self.npig, self.rec_thresholds, T, self.num_classes, self.max_dets)
        host = torch.cat([precision.view(torch.int64).reshape(-1), recall.view(torch.int64).reshape(-1), self.npig.reshape(-1), self.cursor,
                          self.error.to(torch.int64)]).cpu().numpy()
        np_, nr = T * R * nc * 12, T * nc * 12
        n_all, err = int(host[np_ + nr + 4 * nc]), int(host[np_ + nr + 4 * nc + 1])
        self._raise_on_error(err, n_all)
        prec = host[:np_].copy().view(np.float64).reshape(T, R, nc, 4, 3)
        rec = host[np_:np_ + nr].copy().view(np.float64).reshape(T, nc, 4, 3)
        return {"stats": coco_stats(prec, rec, np.array(self.iou_thresholds, np.float64)), "precision": prec, "recall": rec,
                "npig": host[np_ + nr:np_ + nr + 4 * nc].reshape(nc, 4).copy(), "n_records": n_all}

    def records_sorted(self):
        """The records on the host in the order (label ascending, score descending, image_id ascending, rank ascending): score f32,
        label i32, image_id i32, rank i32, flags u32 [n, 4] (per area range 2 bits per threshold: _lib.EVAL_TP / EVAL_FP /
        EVAL_IGNORED).  For tests and for precision / recall curves."""
        order, _ = self._sorted()
        n_all, err = int(self.cursor.item()), int(self.error.item())
        self._raise_on_error(err, n_all)
        out = {k: r[order[:n_all]].cpu().numpy() for k, r in zip(self._KEYS, self._records())}
        out["flags"] = out["flags"].view(np.uint32)
        return out


def coco_stats(precision, recall, iou_thresholds):
    """COCOeval.summarize's 12 numbers from precision [T,R,K,A,M] and recall [T,K,A,M] with numpy, as pycocotools takes them (np.mean's
    pairwise sum over the cells > -1 of the slice; -1 when there are none).  AP50 / AP75 pick the threshold equal to 0.5 / 0.75."""
    def one(ap, iou_thr, a, m):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thresholds)[0]]
        s = s[:, :, :, [a], [m]] if ap else s[:, :, [a], [m]]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1, None, 0, 2), one(1, .5, 0, 2), one(1, .75, 0, 2), one(1, None, 1, 2), one(1, None, 2, 2), one(1, None, 3, 2),
                     one(0, None, 0, 0), one(0, None, 0, 1), one(0, None, 0, 2), one(0, None, 1, 2), one(0, None, 2, 2), one(0, None, 3, 2)],
                    np.float64)
