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


class _FrameBuffer(object):
    """Fixed-capacity device buffers of one frame's ground truth in ONE allocation, so that a frame from the host is one copy: a 16-byte
    head (original width, original height, image_id, n) as int32 -- frame i32[3] and n i32[1] are views of it -- and then the fields of
    _FIELDS, one after the other, each [capacity, width] and each an attribute of its name.  The evaluators' kernels read exactly this
    layout.  _set() copies in place and never reallocates, so a captured graph that read these buffers sees the new frame at its next
    replay."""
    _FIELDS = ()                        # (name, numpy dtype, width) in buffer order

    def __init__(self, capacity, device):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_GT:
            raise ValueError("%s: capacity %d outside 1 .. %d" % (type(self).__name__, capacity, MAX_GT))
        self.capacity = capacity
        self.device = torch.device(device)
        sizes = [np.dtype(dt).itemsize * w * capacity for _, dt, w in self._FIELDS]
        self._offsets = [16 + sum(sizes[:i]) for i in range(len(sizes) + 1)]
        nbytes = self._offsets[-1]
        self._buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.frame = self._buf[0:12].view(torch.int32)
        self.n = self._buf[12:16].view(torch.int32)
        for i, (name, dt, w) in enumerate(self._FIELDS):
            v = self._buf[self._offsets[i]:self._offsets[i + 1]].view(getattr(torch, np.dtype(dt).name))
            setattr(self, name, v.view(capacity, w) if w > 1 else v)
        # pinned staging buffers in a ring: the copy of frame k is asynchronous, so frame k + 1 must not be written over it.  A slot is
        # reused only after the event behind its last copy has completed (it has, unless the host runs 8 frames ahead).
        self._ring = [torch.zeros(nbytes, dtype=torch.uint8) for _ in range(8)]
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

    def _set(self, columns, n, orig_wh, image_id):
        """columns: one array of n rows per field of _FIELDS (None = zeros), all device tensors or all host arrays.  Host arrays go over
        in one copy; device tensors are copied in place (no sync).  More rows than the capacity are NOT silently cut: n keeps the true
        number and the evaluator's update reports the overflow."""
        m = min(n, self.capacity)
        head = torch.from_numpy(np.array([int(orig_wh[0]), int(orig_wh[1]), int(image_id), n], np.int32).view(np.uint8))
        if isinstance(columns[0], torch.Tensor) and columns[0].is_cuda:
            for (name, _, _), col in zip(self._FIELDS, columns):
                dst = getattr(self, name)
                if col is None:
                    dst[:m].zero_()
                else:
                    dst[:m].copy_(col.reshape((-1,) + dst.shape[1:])[:m].to(dst.dtype))
            k, host = self._stage()
            host[:16].copy_(head)
            self._buf[:16].copy_(host[:16], non_blocking=True)
        else:
            k, host = self._stage()
            host[:16].copy_(head)
            h = host.numpy()
            for off, (_, dt, w), col in zip(self._offsets, self._FIELDS, columns):
                rows = h[off:off + np.dtype(dt).itemsize * w * m]
                rows[:] = 0 if col is None else np.ascontiguousarray(np.asarray(col).reshape(-1, w)[:m].astype(dt)).view(np.uint8).reshape(-1)
            self._buf.copy_(host, non_blocking=True)
        self._sent(k)
        return self


class GroundTruth(_FrameBuffer):
    """One frame's VOC ground truth on the device: boxes [capacity,4] f32 pixel xyxy, labels i32, difficult u8, n i32[1], frame i32[3] =
    (original width, original height, image_id)."""
    _FIELDS = (("boxes", np.float32, 4), ("labels", np.int32, 1), ("difficult", np.uint8, 1))

    def set(self, boxes_px, labels, difficult, orig_wh, image_id):
        """boxes_px [n,4] pixel xyxy, labels [n] (0-based), difficult [n] (0 / 1 or None), orig_wh = (w, h) of the original image,
        image_id = the image's sequence number.  Host arrays go over in one copy; device tensors are copied in place (no sync).  More
        rows than the capacity are NOT silently cut: n keeps the true number and the evaluator's update reports the overflow."""
        return self._set((boxes_px, labels, difficult), int(len(labels)), orig_wh, image_id)


def _score_key(score):
    """fp32 scores -> int64 keys that ascend as the score DESCENDS (-0 folded onto +0: Python's sort sees them as equal)."""
    u = (score + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    o = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    return 0xFFFFFFFF - o


class _RecordStore(object):
    """What the two evaluators share: the configuration, the record store in HBM -- rec_score f32, rec_label / rec_image / rec_<_COLUMN>
    i32 [record_capacity], rec_flags i32 [record_capacity] or [record_capacity, _FLAGS_WIDTH] --, a counter tensor i64 [C-1, ...] named
    by _COUNTER, the device cursor and error word, the update kernel's workspace, and everything that reads the store back.  A subclass
    names its protocol's parts and adds update() and summarize()."""
    _COLUMN = None                      # the fourth record column: the order of a frame's records ("position" / "rank")
    _FLAGS_WIDTH = 1                    # flag words per record
    _COUNTER = None                     # (attribute name, trailing shape) of the per-class ground-truth counter
    _OP = None                          # (name of the update op in messages, its _lib.OP_* code)
    _GT = None                          # the frame-buffer class update() takes
    _CONFIG_WORDS = None                # what merge() says two evaluators may differ in

    def __init__(self, num_classes, thr, record_capacity, gt_capacity):
        """Validates and keeps the configuration; _allocate(device) follows once the subclass has checked its own extras."""
        name = type(self).__name__
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError("%s: num_classes %d outside 2 .. %d" % (name, num_classes, MAX_CLASSES))
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError("%s: %d IoU thresholds, 1 .. %d supported" % (name, len(thr), MAX_THRESHOLDS))
        if not 1 <= int(gt_capacity) <= MAX_GT:
            raise ValueError("%s: gt_capacity %d outside 1 .. %d" % (name, gt_capacity, MAX_GT))
        if int(record_capacity) < 1:
            raise ValueError("%s: record_capacity must be >= 1" % name)
        self.num_classes = int(num_classes)
        self.iou_thresholds = tuple(float(t) for t in thr)
        self.record_capacity = int(record_capacity)
        self.gt_capacity = int(gt_capacity)

    def _allocate(self, device):
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("%s runs only on a HIP device (no CPU fallback)" % type(self).__name__)
        self.device = dev
        self.thresholds = torch.tensor(self.iou_thresholds, dtype=torch.float64, device=dev)
        cap = self.record_capacity
        self.rec_score = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.rec_label = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_image = torch.zeros(cap, dtype=torch.int32, device=dev)
        self._rec_order = torch.zeros(cap, dtype=torch.int32, device=dev)
        setattr(self, "rec_" + self._COLUMN, self._rec_order)
        # bit pattern: 2 bits per threshold, one word per area range where the protocol has them
        self.rec_flags = torch.zeros(cap if self._FLAGS_WIDTH == 1 else (cap, self._FLAGS_WIDTH), dtype=torch.int32, device=dev)
        self._counter = torch.zeros((self.num_classes - 1,) + self._COUNTER[1], dtype=torch.int64, device=dev)
        setattr(self, self._COUNTER[0], self._counter)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = {}

    # ---- per frame ----------------------------------------------------------------------------------------------------------
    def _workspace(self, D, G):
        """The update kernel's workspace (VOC: the ticket and winner words, zero before the first call and left zero by the kernel;
        COCO: the key segments): owned by this evaluator, so that a captured graph keeps a valid address."""
        ws = self._ws.get((D, G))
        if ws is None:
            nb = _lib.workspace_bytes(self._OP[1], D, G)
            if nb == 0:
                raise FrcnnError("%s: detection capacity %d / ground-truth capacity %d outside the kernel's limits" % (self._OP[0], D, G))
            ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)
            self._ws[(D, G)] = ws
        return ws

    def _check_gt(self, gt):
        if gt.capacity > self.gt_capacity:
            raise ValueError("%s: %s capacity %d > gt_capacity %d" % (type(self).__name__, self._GT.__name__, gt.capacity, self.gt_capacity))

    def reset(self):
        self.cursor.zero_()
        self._counter.zero_()
        self.error.zero_()

    # ---- per test set -------------------------------------------------------------------------------------------------------
    def _keys(self):
        return ("score", "label", "image_id", self._COLUMN, "flags")

    def _records(self):
        return (self.rec_score, self.rec_label, self.rec_image, self._rec_order, self.rec_flags)

    def state(self):
        """The evaluator's state as device tensors (one sync for the record count): the live records in slot order, the counter,
        n_records (what update counted: more than len(score) when the store overflowed), the error word and the configuration."""
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        s = dict(zip(self._keys(), (r[:n].clone() for r in self._records())))
        s.update(n_records=n_all, error=self.error.clone(), **self._config())
        s[self._COUNTER[0]] = self._counter.clone()
        return s

    def merge(self, other):
        """Appends the records of `other` (an evaluator of this class, or a state() of one, of the same configuration) and adds its
        counters: evaluating shards separately and merging equals one evaluator over all of them."""
        s = other.state() if isinstance(other, type(self)) else other
        if any((tuple(s[k]) if isinstance(v, tuple) else s[k]) != v for k, v in self._config().items()):
            raise ValueError("%s.merge: the evaluators differ in %s" % (type(self).__name__, self._CONFIG_WORDS))
        n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        m = min(int(s["score"].numel()), self.record_capacity - n)
        for dst, key in zip(self._records(), self._keys()):
            dst[n:n + m].copy_(s[key][:m].to(self.device))
        self.cursor += int(s["n_records"])                     # keeps counting past the capacity: summarize() reports the loss
        self._counter += s[self._COUNTER[0]].to(self.device)
        self.error |= s["error"].to(self.device)
        return self

    def _sorted(self):
        """(order, labels_sorted) on the device, no sync: the live slots first, in (label ascending, score descending, image_id
        ascending, position or rank ascending); the slots past the cursor sort behind every class."""
        cap = self.record_capacity
        live = torch.arange(cap, device=self.device) < self.cursor
        o1 = torch.sort((self.rec_image.to(torch.int64) << 32) | self._rec_order.to(torch.int64), stable=True)[1]
        lab = torch.where(live, self.rec_label, torch.full_like(self.rec_label, 0x7FFFFFFF))
        key = ((lab.to(torch.int64) << 32) | _score_key(self.rec_score))[o1]
        o2 = torch.sort(key, stable=True)[1]
        order = o1[o2]
        return order, lab[order].contiguous()

    def _raise_on_error(self, err, n_all):
        name = type(self).__name__
        if err:
            what = [w for b, w in ((_lib.EVAL_ERR_UPSTREAM_ABORT, "a frame's detection count was -1 (an aborted proposal scan upstream)"),
                                   (_lib.EVAL_ERR_GT_OVERFLOW, "a frame had more ground truths than the %s capacity" % self._GT.__name__),
                                   (_lib.EVAL_ERR_COUNT_RANGE, "a frame's detection count exceeded its capacity"),
                                   (_lib.EVAL_ERR_LABEL_RANGE, "a label outside 0 .. num_classes - 2")) if err & b]
            raise FrcnnError("%s: error word %d: %s" % (name, err, "; ".join(what)))
        if n_all > self.record_capacity:
            raise FrcnnError("%s: the record store is full: %d of %d records were dropped (record_capacity = %d)"
                             % (name, n_all - self.record_capacity, n_all, self.record_capacity))

    def records_sorted(self):
        """The records on the host in the order (label ascending, score descending, image_id ascending, position or rank ascending):
        score f32, label i32, image_id i32, position or rank i32, flags u32 [n] or [n, 4] (per area range 2 bits per threshold:
        _lib.EVAL_TP / EVAL_FP / EVAL_IGNORED).  For tests and for precision / recall curves."""
        order, _ = self._sorted()
        n_all, err = int(self.cursor.item()), int(self.error.item())
        self._raise_on_error(err, n_all)
        out = {k: r[order[:n_all]].cpu().numpy() for k, r in zip(self._keys(), self._records())}
        out["flags"] = out["flags"].view(np.uint32)
        return out


class DetectionEvaluator(_RecordStore):
    """VOC AP at T IoU thresholds in one pass.  update() is one HIP launch on the current stream and has no host sync; summarize() does
    the only device -> host copy."""
    _COLUMN, _FLAGS_WIDTH, _COUNTER, _OP = "position", 1, ("npos", ()), ("eval_update", _lib.OP_EVAL)
    _GT, _CONFIG_WORDS = GroundTruth, "classes or thresholds"

    def __init__(self, num_classes, iou_thresholds=(0.5,), record_capacity=1 << 20, gt_capacity=128, device=None):
        super().__init__(num_classes, [float(t) for t in iou_thresholds], record_capacity, gt_capacity)
        self._allocate(device)

    def _config(self):
        return {"iou_thresholds": self.iou_thresholds, "num_classes": self.num_classes}

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame, gt = its GroundTruth.  No sync; capturable into a graph with detect."""
        self._check_gt(gt)
        ops.eval_update(dets, gt.boxes, gt.labels, gt.difficult, gt.n, gt.frame, self.thresholds, self.num_classes, self.npos, self.rec_score,
                        self.rec_label, self.rec_image, self.rec_position, self.rec_flags, self.cursor, self.error,
                        workspace=self._workspace(dets.labels.numel(), gt.capacity))

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


# ---------------------------------------------------------------------------------------------------------------------------------
# the COCO protocol (bbox, useCats = 1)
# ---------------------------------------------------------------------------------------------------------------------------------
COCO_MAX_DET = 100
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large


class CocoGroundTruth(_FrameBuffer):
    """One frame's COCO annotations on the device: boxes [capacity,4] f64 pixel xywh, area f64, labels i32, iscrowd u8, n i32[1], frame
    i32[3] = (original width, original height, image_id).  The same contract as GroundTruth."""
    _FIELDS = (("boxes", np.float64, 4), ("area", np.float64, 1), ("labels", np.int32, 1), ("iscrowd", np.uint8, 1))

    def set(self, boxes_xywh, labels, iscrowd=None, area=None, orig_wh=None, image_id=0):
        """boxes_xywh [n,4] pixel xywh (float64 is kept), labels [n] (0-based), iscrowd [n] (0 / 1 or None), area [n] (the annotations'
        own areas; None = w * h of the box), orig_wh = (w, h) of the original image, image_id = the image's id.  Host arrays go over in
        one copy; device tensors are copied in place (no sync).  More rows than the capacity are NOT silently cut: n keeps the true
        number and the evaluator's update reports the overflow."""
        if orig_wh is None:
            raise ValueError("CocoGroundTruth.set: orig_wh = (w, h) is required")
        if isinstance(boxes_xywh, torch.Tensor) and boxes_xywh.is_cuda:
            boxes_xywh = boxes_xywh.reshape(-1, 4).to(torch.float64)
        else:
            boxes_xywh = np.asarray(boxes_xywh, np.float64).reshape(-1, 4)
            iscrowd = None if iscrowd is None else np.asarray(iscrowd) != 0
        if area is None:
            area = boxes_xywh[:, 2] * boxes_xywh[:, 3]
        return self._set((boxes_xywh, area, labels, iscrowd), int(len(labels)), orig_wh, image_id)


class CocoDetectionEvaluator(_RecordStore):
    """COCOeval (bbox, useCats = 1) over a record store in HBM.  update() is one HIP launch on the current stream and has no host sync;
    summarize() runs the accumulate kernel, does the only device -> host copy and takes the 12 means with numpy as pycocotools does."""
    _COLUMN, _FLAGS_WIDTH, _COUNTER, _OP = "rank", 4, ("npig", (4,)), ("coco_eval_update", _lib.OP_COCO_EVAL)
    _GT, _CONFIG_WORDS = CocoGroundTruth, "classes, thresholds or maxDets"

    def __init__(self, num_classes, record_capacity=1 << 20, gt_capacity=128, device=None, iou_thresholds=None, max_dets=(1, 10, 100)):
        thr = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thresholds is None \
            else np.array([float(t) for t in iou_thresholds], np.float64)
        md = tuple(int(v) for v in max_dets)
        super().__init__(num_classes, thr, record_capacity, gt_capacity)
        if len(md) != 3 or list(md) != sorted(md) or md[0] < 1 or md[2] > COCO_MAX_DET:
            raise ValueError("CocoDetectionEvaluator: max_dets must be three ascending values in 1 .. %d" % COCO_MAX_DET)
        self.max_dets = md
        self._allocate(device)
        self.rec_thresholds_host = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.rec_thresholds = torch.from_numpy(self.rec_thresholds_host.copy()).to(self.device)

    def _config(self):
        return {"config": (self.iou_thresholds, self.num_classes, self.max_dets)}

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame (rows in any order), gt = its CocoGroundTruth.  No sync; capturable
        into a graph with detect."""
        self._check_gt(gt)
        ops.coco_eval_update(dets, gt.boxes, gt.area, gt.labels, gt.iscrowd, gt.n, gt.frame, self.thresholds, self.num_classes, self.max_dets[-1],
                             self.npig, self.rec_score, self.rec_label, self.rec_image, self.rec_rank, self.rec_flags, self.cursor, self.error,
                             workspace=self._workspace(dets.labels.numel(), gt.capacity))

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
