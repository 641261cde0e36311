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
Not built: the segm and keypoints IoU types.

With every category pooled (COCOeval's useCats = 0) the same store measures the proposal path, the metric of the Faster R-CNN paper's RPN
ablations (AR@100 / 300 / 1000), and class-agnostic detection AP:

    pe = ProposalEvaluator(max_dets=(100, 300, 1000), device=dev)            # a CocoDetectionEvaluator(use_cats=False) underneath
    dets, props = model.detect(x, 0.05, want_proposals=True)                 # one forward serves both; or props = model.proposals(x)
    ev.update(dets, gt)
    pe.update(props, gt)                                                      # DetectGraph(model, hw, evaluator=ev, gt=gt, proposal_evaluator=pe)
    pe.summarize()["ar"]                                                      # AR@100, AR@300, AR@1000

On N GPUs (the reference's test loop is distributed: test.py:60-128, evaluation/coco_eval.py:46-49, 161-190) every rank evaluates its shard
with an evaluator built with image_capacity > 0, which keeps one ledger row per frame (image_id, the frame's record slots, its share of
the counter), and then calls

    ev.synchronize_between_processes()                # all ranks; afterwards every rank holds the merged store
    res = ev.summarize()

The merge keeps the FIRST occurrence of every image_id in (rank, order of update) -- the reference's np.unique(..., return_index=True) --,
so the images a DistributedSampler evaluates twice to pad the shards count once.  merge_shards(states) is the same merge without the
collective; both run in HIP (csrc/eval_merge.hip).  For the VOC protocol this is the project's extension: the reference evaluates VOC
on rank 0 only."""
import zlib

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

    def __init__(self, num_classes, thr, record_capacity, gt_capacity, image_capacity=0):
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
        if int(image_capacity) < 0:
            raise ValueError("%s: image_capacity must be >= 0 (0 = no image ledger)" % name)
        self.image_capacity = int(image_capacity)

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
        self._counter = torch.zeros((self._counter_rows(),) + self._COUNTER[1], dtype=torch.int64, device=dev)
        setattr(self, self._COUNTER[0], self._counter)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = {}
        if self.image_capacity:
            # the image ledger: one row per update -- image_id, the record slots [begin, end) the frame took, its share of the counter --
            # and the snapshots of cursor and counter the next row is measured from.  Owned here, so that a captured graph replays.
            ic, cw = self.image_capacity, self._counter.numel()
            self.led_image = torch.zeros(ic, dtype=torch.int32, device=dev)
            self.led_range = torch.zeros((ic, 2), dtype=torch.int64, device=dev)
            self.led_delta = torch.zeros((ic, cw), dtype=torch.int32, device=dev)
            self.led_count = torch.zeros(1, dtype=torch.int64, device=dev)
            self._snap_cursor = torch.zeros(1, dtype=torch.int64, device=dev)
            self._snap_counter = torch.zeros(cw, dtype=torch.int64, device=dev)

    def _counter_rows(self):
        return self.num_classes - 1

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

    def _ledger_append(self, gt):
        """The ledger row of the frame the update before it scored: one further launch on the same stream, no sync, capturable."""
        if self.image_capacity:
            ops.eval_ledger_append(gt.frame, self.cursor, self._counter, self._snap_cursor, self._snap_counter, self.led_image, self.led_range,
                                   self.led_delta, self.led_count, self.error)

    def reset(self):
        self.cursor.zero_()
        self._counter.zero_()
        self.error.zero_()
        if self.image_capacity:
            for t in (self.led_image, self.led_range, self.led_delta, self.led_count, self._snap_cursor, self._snap_counter):
                t.zero_()

    # ---- per test set -------------------------------------------------------------------------------------------------------
    def _keys(self):
        return ("score", "label", "image_id", self._COLUMN, "flags")

    def _records(self):
        return (self.rec_score, self.rec_label, self.rec_image, self._rec_order, self.rec_flags)

    def state(self):
        """The evaluator's state as device tensors (one sync for the record count): the live records in slot order, the counter,
        n_records (what update counted: more than len(score) when the store overflowed), the error word and the configuration.  With an
        image ledger also its live rows -- led_image, led_range, led_delta -- and n_images (what update counted)."""
        if self.image_capacity:
            n_all, m_all = (int(v) for v in torch.cat([self.cursor, self.led_count]).tolist())
        else:
            n_all = int(self.cursor.item())
        n = min(n_all, self.record_capacity)
        s = dict(zip(self._keys(), (r[:n].clone() for r in self._records())))
        s.update(n_records=n_all, error=self.error.clone(), **self._config())
        s[self._COUNTER[0]] = self._counter.clone()
        if self.image_capacity:
            m = min(m_all, self.image_capacity)
            s.update(led_image=self.led_image[:m].clone(), led_range=self.led_range[:m].clone(), led_delta=self.led_delta[:m].clone(), n_images=m_all)
        return s

    def merge(self, other):
        """Appends the records of `other` (an evaluator of this class, or a state() of one, of the same configuration) and adds its
        counters: evaluating shards separately and merging equals one evaluator over all of them.  Appends only: an image that two
        shards have seen counts twice, so an evaluator with an image ledger refuses it and names merge_shards()."""
        if self.image_capacity:
            raise ValueError("%s.merge appends without looking at image ids and keeps no ledger: an evaluator built with image_capacity > 0 "
                             "merges with merge_shards(states) or synchronize_between_processes()" % type(self).__name__)
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

    # ---- across shards -----------------------------------------------------------------------------------------------------
    def _need_ledger(self, what):
        if not self.image_capacity:
            raise ValueError("%s.%s needs the image ledger: build the evaluator with image_capacity > 0" % (type(self).__name__, what))

    def _check_config(self, cfg, what):
        if any((tuple(cfg[k]) if isinstance(v, tuple) else cfg[k]) != v for k, v in self._config().items()):
            raise ValueError("%s.%s: the evaluators differ in %s" % (type(self).__name__, what, self._CONFIG_WORDS))

    def _shard(self, s, what):
        """One shard as device tensors with device counts: an evaluator of this class as it stands (its whole buffers and its device
        counts: no sync, capturable) or a state() of one.  The counts are the LIVE ones (a shard's padding is no record); a shard that had
        lost records to its own capacity says so in its error word."""
        if isinstance(s, _RecordStore):
            if type(s) is not type(self):
                raise ValueError("%s.%s: a shard is a %s" % (type(self).__name__, what, type(s).__name__))
            s._need_ledger(what + " (a shard)")
            self._check_config(s._config(), what)
            v = dict(zip(("score", "label", "image_id", "order", "flags"), s._records()))
            lost = torch.where(s.cursor > s.record_capacity, _lib.EVAL_ERR_SHARD_TRUNCATED, 0).to(torch.int32)
            v.update(led_image=s.led_image, led_range=s.led_range, led_delta=s.led_delta, n_records=s.cursor.clamp(max=s.record_capacity),
                     n_images=s.led_count.clamp(max=s.image_capacity), error=s.error | lost)
        else:
            if "led_image" not in s:
                raise ValueError("%s.%s: a shard's state() has no image ledger (image_capacity = 0)" % (type(self).__name__, what))
            self._check_config(s, what)
            v = dict(zip(("score", "label", "image_id", "order", "flags"), (s[k] for k in self._keys())))
            v.update({k: s[k] for k in ("led_image", "led_range", "led_delta")})
            lost = _lib.EVAL_ERR_SHARD_TRUNCATED if int(s["n_records"]) > int(s["score"].shape[0]) else 0
            v.update(n_records=torch.tensor([min(int(s["n_records"]), int(s["score"].shape[0]))], dtype=torch.int64),
                     n_images=torch.tensor([min(int(s["n_images"]), int(s["led_image"].shape[0]))], dtype=torch.int64),
                     error=s["error"].reshape(1) | lost)
        return {k: t.to(self.device) for k, t in v.items()}

    def _merge(self, shards):
        ops.eval_merge(shards, dict(score=self.rec_score, label=self.rec_label, image_id=self.rec_image, order=self._rec_order, flags=self.rec_flags,
                                    led_image=self.led_image, led_range=self.led_range, led_delta=self.led_delta, counter=self._counter,
                                    cursor=self.cursor, led_count=self.led_count, error=self.error, snap_cursor=self._snap_cursor,
                                    snap_counter=self._snap_counter))
        return self

    @staticmethod
    def _padded(cols, rows):
        """[W, rows, ...] of the shards' columns [n_w, ...], zero behind each."""
        out = torch.zeros((len(cols), rows) + tuple(cols[0].shape[1:]), dtype=cols[0].dtype, device=cols[0].device)
        for w, c in enumerate(cols):
            out[w, :c.shape[0]].copy_(c)
        return out

    def merge_shards(self, states):
        """REPLACES this evaluator's content by the merge of `states`, a list in rank order of evaluators of this class and configuration
        (taken as they stand: no sync, capturable) or of their state() dicts, all with an image ledger.  The reference's merge
        (evaluation/coco_eval.py:161-190): occurrences are ordered (shard, ledger row) and an occurrence is kept iff no earlier one has
        its image_id, so duplicates inside one shard go too.  The kept records arrive in (shard, slot) order, bit for bit; the kept
        ledger rows in the same order with rebased ranges; the counter is the sum of their deltas; the cursor counts the kept records
        even past record_capacity and summarize() reports the loss; the error word is the OR of the shards' words.  summarize() and
        records_sorted() then equal those of one evaluator fed every distinct image once.  Merge into a fresh or reset evaluator (or
        pass this evaluator itself as one of the shards: they are copied first)."""
        self._need_ledger("merge_shards")
        views = [self._shard(s, "merge_shards") for s in states]
        if not 1 <= len(views) <= _lib.EVAL_MERGE_MAX_SHARDS:
            raise ValueError("%s.merge_shards: %d shards outside 1 .. %d" % (type(self).__name__, len(views), _lib.EVAL_MERGE_MAX_SHARDS))
        sr = max(4, (max(v["score"].shape[0] for v in views) + 3) // 4 * 4)
        si = max(1, max(v["led_image"].shape[0] for v in views))
        shards = {k: self._padded([v[k] for v in views], sr) for k in ("score", "label", "image_id", "order", "flags")}
        shards.update({k: self._padded([v[k] for v in views], si) for k in ("led_image", "led_range", "led_delta")})
        shards.update({k: torch.cat([v[k].reshape(1) for v in views]) for k in ("n_records", "n_images", "error")})
        return self._merge(shards)

    def synchronize_between_processes(self, group=None):
        """Named after the reference's CocoEvaluator.synchronize_between_processes (evaluation/coco_eval.py:46-49): EVERY rank of `group`
        calls it after its last update, and afterwards every rank's evaluator holds the merge of all shards in rank order
        (merge_shards).  A collective: it reads the live counts on the host, checks that the ranks agree in class and configuration,
        all-gathers the columns, the ledger and the deltas padded to the largest count -- device tensors on the nccl backend, through
        the host on any other (gloo) -- and merges in HIP.  Without an initialised process group it is merge_shards([self.state()]):
        deduplication only."""
        import torch.distributed as dist
        self._need_ledger("synchronize_between_processes")
        name = type(self).__name__
        if not (dist.is_available() and dist.is_initialized()):
            return self.merge_shards([self.state()])
        v = self._shard(self.state(), "synchronize_between_processes")
        W = dist.get_world_size(group)
        if W > _lib.EVAL_MERGE_MAX_SHARDS:
            raise ValueError("%s.synchronize_between_processes: %d ranks, at most %d supported" % (name, W, _lib.EVAL_MERGE_MAX_SHARDS))
        on_device = dist.get_backend(group) == "nccl"

        def gather(t):
            t = t.contiguous()
            if on_device:
                out = torch.empty((W,) + tuple(t.shape), dtype=t.dtype, device=self.device)
                dist.all_gather_into_tensor(out, t, group=group)
                return out
            h = t.cpu()
            outs = [torch.empty_like(h) for _ in range(W)]
            dist.all_gather(outs, h, group=group)
            return torch.stack(outs).to(self.device)

        cfg = zlib.crc32(repr((name, sorted(self._config().items()))).encode())
        head = gather(torch.cat([torch.tensor([cfg, v["score"].shape[0], v["led_image"].shape[0]], dtype=torch.int64, device=self.device),
                                 v["n_records"], v["n_images"], v["error"].to(torch.int64)]))
        head_h = head.cpu()
        if bool((head_h[:, 0] != cfg).any()):
            raise ValueError("%s.synchronize_between_processes: the ranks' evaluators differ in class, %s" % (name, self._CONFIG_WORDS))
        sr = max(4, (int(head_h[:, 1].max()) + 3) // 4 * 4)
        si = max(1, int(head_h[:, 2].max()))
        shards = {k: gather(self._padded([v[k]], sr)[0]) for k in ("score", "label", "image_id", "order", "flags")}
        shards.update({k: gather(self._padded([v[k]], si)[0]) for k in ("led_image", "led_range", "led_delta")})
        shards.update(n_records=head[:, 3].contiguous(), n_images=head[:, 4].contiguous(), error=head[:, 5].to(torch.int32))
        return self._merge(shards)

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
                                   (_lib.EVAL_ERR_LABEL_RANGE, "a label outside 0 .. num_classes - 2"),
                                   (_lib.EVAL_ERR_LEDGER_OVERFLOW, "more frames than the image ledger holds (image_capacity = %d)" % self.image_capacity),
                                   (_lib.EVAL_ERR_SHARD_TRUNCATED, "a merged shard had lost records or ledger rows to its own capacity")) if err & b]
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

    def __init__(self, num_classes, iou_thresholds=(0.5,), record_capacity=1 << 20, gt_capacity=128, device=None, image_capacity=0):
        """image_capacity > 0 keeps an image ledger of that many frames (one further launch per update): what merge_shards() and
        synchronize_between_processes() need."""
        super().__init__(num_classes, [float(t) for t in iou_thresholds], record_capacity, gt_capacity, image_capacity)
        self._allocate(device)

    def _config(self):
        return {"iou_thresholds": self.iou_thresholds, "num_classes": self.num_classes}

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame, gt = its GroundTruth.  No sync; capturable into a graph with detect."""
        self._check_gt(gt)
        ops.eval_update(dets, gt.boxes, gt.labels, gt.difficult, gt.n, gt.frame, self.thresholds, self.num_classes, self.npos, self.rec_score,
                        self.rec_label, self.rec_image, self.rec_position, self.rec_flags, self.cursor, self.error,
                        workspace=self._workspace(dets.labels.numel(), gt.capacity))
        self._ledger_append(gt)

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
# the COCO protocol (bbox; useCats = 1, or every category pooled: useCats = 0)
# ---------------------------------------------------------------------------------------------------------------------------------
COCO_MAX_DET = 100
COCO_MAX_DET_POOLED = 2048
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
    """COCOeval (bbox) over a record store in HBM.  update() is one HIP launch on the current stream (two with use_cats=False) and has no
    host sync; summarize() runs the accumulate kernel, does the only device -> host copy and takes the 12 means with numpy as pycocotools
    does.

    use_cats=False is COCOeval's useCats = 0: a frame's detections and ground truths are each ONE list in the order (label ascending,
    position ascending), the detections are ranked by score descending with a stable sort over that order and cut to max_dets[-1] (up to
    2048), and a detection may match a ground truth of any label; num_classes only bounds the labels.  There is one pooled category:
    npig is [1, 4], precision [T, 101, 1, 4, 3], and the 12 stats have their usual meaning over the pooled set."""
    _COLUMN, _FLAGS_WIDTH, _COUNTER, _OP = "rank", 4, ("npig", (4,)), ("coco_eval_update", _lib.OP_COCO_EVAL)
    _GT, _CONFIG_WORDS = CocoGroundTruth, "classes, thresholds or maxDets"

    def __init__(self, num_classes, record_capacity=1 << 20, gt_capacity=128, device=None, iou_thresholds=None, max_dets=(1, 10, 100),
                 image_capacity=0, use_cats=True):
        """image_capacity > 0 keeps an image ledger of that many frames (one further launch per update): what merge_shards() and
        synchronize_between_processes() need."""
        thr = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thresholds is None \
            else np.array([float(t) for t in iou_thresholds], np.float64)
        md = tuple(int(v) for v in max_dets)
        super().__init__(num_classes, thr, record_capacity, gt_capacity, image_capacity)
        self.use_cats = bool(use_cats)
        limit = COCO_MAX_DET if self.use_cats else COCO_MAX_DET_POOLED
        if len(md) != 3 or list(md) != sorted(md) or md[0] < 1 or md[2] > limit:
            raise ValueError("%s: max_dets must be three ascending values in 1 .. %d" % (type(self).__name__, limit))
        self.max_dets = md
        if not self.use_cats:
            self._OP = ("coco_eval_update_pooled", _lib.OP_COCO_EVAL_POOLED)
            self._CONFIG_WORDS = "classes, thresholds, maxDets or use_cats"
        self._allocate(device)
        self.rec_thresholds_host = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.rec_thresholds = torch.from_numpy(self.rec_thresholds_host.copy()).to(self.device)

    def _counter_rows(self):
        return self.num_classes - 1 if self.use_cats else 1

    def _config(self):
        if self.use_cats:
            return {"config": (self.iou_thresholds, self.num_classes, self.max_dets)}
        return {"config": (self.iou_thresholds, self.num_classes, self.max_dets, "pooled")}

    def update(self, dets, gt):
        """Scores one frame: dets = ops.Detections of the frame (rows in any order), gt = its CocoGroundTruth.  No sync; capturable
        into a graph with detect."""
        self._check_gt(gt)
        (ops.coco_eval_update if self.use_cats else ops.coco_eval_update_pooled)(
            dets, gt.boxes, gt.area, gt.labels, gt.iscrowd, gt.n, gt.frame, self.thresholds, self.num_classes, self.max_dets[-1], self.npig,
            self.rec_score, self.rec_label, self.rec_image, self.rec_rank, self.rec_flags, self.cursor, self.error,
            workspace=self._workspace(dets.labels.numel(), gt.capacity))
        self._ledger_append(gt)

    def summarize(self):
        """{"stats": float64 [12] (COCOeval.stats: AP, AP50, AP75, APs, APm, APl, AR@maxDets[0], AR@maxDets[1], AR@maxDets[2], ARs, ARm,
        ARl), "precision": float64 [T, 101, K, 4, 3], "recall": float64 [T, K, 4, 3] (-1 where npig == 0), "npig": int64 [K, 4],
        "n_records"}; K = num_classes - 1, or 1 with use_cats=False.  Raises FrcnnError when a frame reported an error or records were
        dropped.  One device -> host copy."""
        T, nc, R = len(self.iou_thresholds), self._counter_rows(), self.rec_thresholds.numel()
        order, lab = self._sorted()
        precision, recall = ops.coco_eval_accumulate(lab, self.rec_rank[order].contiguous(), self.rec_flags[order].contiguous(), self.cursor,
                                                     self.npig, self.rec_thresholds, T, nc + 1, self.max_dets)
        host = torch.cat([precision.view(torch.int64).reshape(-1), recall.view(torch.int64).reshape(-1), self.npig.reshape(-1), self.cursor,
                          self.error.to(torch.int64)]).cpu().numpy()
        np_, nr = T * R * nc * 12, T * nc * 12
        n_all, err = int(host[np_ + nr + 4 * nc]), int(host[np_ + nr + 4 * nc + 1])
        self._raise_on_error(err, n_all)
        prec = host[:np_].copy().view(np.float64).reshape(T, R, nc, 4, 3)
        rec = host[np_:np_ + nr].copy().view(np.float64).reshape(T, nc, 4, 3)
        return {"stats": coco_stats(prec, rec, np.array(self.iou_thresholds, np.float64)), "precision": prec, "recall": rec,
                "npig": host[np_ + nr:np_ + nr + 4 * nc].reshape(nc, 4).copy(), "n_records": n_all}


class ProposalEvaluator(CocoDetectionEvaluator):
    """Proposal recall: COCO's "proposal" evaluation and the metric of the Faster R-CNN paper's RPN ablations -- AR at max_dets proposals
    per image with every category pooled.  A CocoDetectionEvaluator(use_cats=False) fed with model.proposals(x) (or detect(...,
    want_proposals=True)[1]), whose scores are a rank ramp: only the order within a frame is meaningful.

    summarize() therefore returns only what a ramp supports: "ar" float64 [3] (AR@max_dets, area range "all"), "ar_small", "ar_medium",
    "ar_large" (at max_dets[-1]), "recall" float64 [T, 4, 3] (threshold, area range, max_dets; -1 where npig == 0), "npig" int64 [4] and
    "n_records".  The AP entries are left out on purpose: precision orders the records of ALL images by score, and the ramp's scores say
    nothing across images.  num_classes only bounds the ground truths' labels (default: every label the kernels accept)."""

    def __init__(self, max_dets=(100, 300, 1000), iou_thresholds=None, gt_capacity=128, image_capacity=0, record_capacity=1 << 20, device=None,
                 num_classes=MAX_CLASSES):
        super().__init__(num_classes, record_capacity=record_capacity, gt_capacity=gt_capacity, device=device, iou_thresholds=iou_thresholds,
                         max_dets=max_dets, image_capacity=image_capacity, use_cats=False)

    def summarize(self):
        res = CocoDetectionEvaluator.summarize(self)
        st = res["stats"]
        return {"ar": st[6:9].copy(), "ar_small": float(st[9]), "ar_medium": float(st[10]), "ar_large": float(st[11]),
                "recall": res["recall"][:, 0].copy(), "npig": res["npig"][0].copy(), "n_records": res["n_records"]}


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
