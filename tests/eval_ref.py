"""Restatement of the VOC AP protocol the reference's evaluator implements (evaluation/voc_eval.py:67-112 save_pred, :115-135 voc_ap,
:138-225 cal_mAP), written from the protocol (numpy + plain Python float64, the same operations in the same order), for the tests of
faster_rcnn_pytorch_amd.evaluation.  Two forms:

  sequential(frames, ...)  the literal loop: per class the detections in (score descending, image order, position) with `used` flags;
  parallel(frames, ...)    the per-frame form the device kernel uses: a detection is TP iff it is the first, in (score descending,
                           position ascending), of the frame's detections that share its match and reach the threshold.

A frame is a dict: image_id, w, h, boxes f32 [D,4] normalised xyxy, labels i32 [D], scores f32 [D], gt_boxes f32 [G,4] pixel xyxy,
gt_labels i32 [G], gt_difficult u8 [G].  Labels are 0-based (class c of num_classes - 1).  Flags: 2 bits per threshold, TP = 1,
FP = 2, IGNORED = 3.  Records come back in the defined order (label ascending, score descending, image_id ascending, position
ascending) as a dict of arrays: score f32, label i32, image_id i32, position i32, flags u32."""
import numpy as np

TP, FP, IGNORED = 1, 2, 3
EPS = float(np.finfo(np.float64).eps)


def pixel_boxes(boxes, w, h):
    """voc_eval.py:90-91: the normalised fp32 boxes times the int (w, h, w, h) -- numpy promotes to float64."""
    return np.asarray(boxes, np.float32).reshape(-1, 4) * np.array([w, h, w, h])


def best_match(bb, label, gt_px, gt_labels):
    """voc_eval.py:162-180 for one detection: (ovmax, index of the match or -1)."""
    ovmax, match = -1, -1
    for g in range(len(gt_labels)):
        if int(gt_labels[g]) != label:
            continue
        bbgt = gt_px[g]
        bi = [max(bb[0], bbgt[0]), max(bb[1], bbgt[1]), min(bb[2], bbgt[2]), min(bb[3], bbgt[3])]
        iw = bi[2] - bi[0] + 1
        ih = bi[3] - bi[1] + 1
        if iw > 0 and ih > 0:
            ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (bbgt[2] - bbgt[0] + 1) * (bbgt[3] - bbgt[1] + 1) - iw * ih
            ov = iw * ih / ua
            if ov > ovmax:
                ovmax, match = ov, g
    return ovmax, match


def _frame_matches_np(f):
    """best_match for every detection of a frame with the loop over the ground truths written as numpy float64 array operations: the
    same IEEE operations element by element (finite boxes only: np.maximum and Python's max differ on NaN), the first maximum of the
    valid overlaps = strict > from -1.  For the large frames of the GPU tests; tests/test_eval_host.py pins it to the literal loop."""
    px = pixel_boxes(f["boxes"], int(f["w"]), int(f["h"]))
    gt = np.asarray(f["gt_boxes"], np.float32).reshape(-1, 4).astype(np.float64)
    gl = np.asarray(f["gt_labels"]).astype(np.int64)
    ga = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    out = []
    for i in range(len(f["labels"])):
        bb = px[i]
        iw = np.minimum(bb[2], gt[:, 2]) - np.maximum(bb[0], gt[:, 0]) + 1
        ih = np.minimum(bb[3], gt[:, 3]) - np.maximum(bb[1], gt[:, 1]) + 1
        ok = (gl == int(f["labels"][i])) & (iw > 0) & (ih > 0)
        if not ok.any():
            out.append((-1, -1))
            continue
        ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + ga - iw * ih
        with np.errstate(all="ignore"):
            ov = np.where(ok, iw * ih / ua, -np.inf)
        m = int(np.argmax(ov))
        out.append((float(ov[m]), m))
    return out


def _frame_matches(f, fast=False):
    if fast:
        return _frame_matches_np(f)
    px = pixel_boxes(f["boxes"], int(f["w"]), int(f["h"]))
    gt_px = [[float(v) for v in b] for b in np.asarray(f["gt_boxes"], np.float32).reshape(-1, 4)]
    out = []
    for i in range(len(f["labels"])):
        out.append(best_match([float(v) for v in px[i]], int(f["labels"][i]), gt_px, f["gt_labels"]))
    return out


def npos_of(frames, num_classes):
    npos = np.zeros(num_classes - 1, np.int64)
    for f in frames:
        for l, d in zip(f["gt_labels"], f["gt_difficult"]):
            if not d:
                npos[int(l)] += 1
    return npos


def _records(frames, flags_of):
    """flags_of[(image_id, position)] -> u32; the records in the defined order."""
    rows = []
    for f in frames:
        for i in range(len(f["labels"])):
            rows.append((int(f["labels"][i]), np.float32(f["scores"][i]), int(f["image_id"]), i))
    rows.sort(key=lambda r: r[3])
    rows.sort(key=lambda r: r[2])
    rows.sort(key=lambda r: float(r[1]), reverse=True)          # stable, like save_pred's sort (:109)
    rows.sort(key=lambda r: r[0])
    return {"label": np.array([r[0] for r in rows], np.int32), "score": np.array([r[1] for r in rows], np.float32),
            "image_id": np.array([r[2] for r in rows], np.int32), "position": np.array([r[3] for r in rows], np.int32),
            "flags": np.array([flags_of[(r[2], r[3])] for r in rows], np.uint32)}


def sequential(frames, num_classes, thresholds):
    """The literal loop of cal_mAP: returns (records, npos)."""
    frames = sorted(frames, key=lambda f: int(f["image_id"]))
    matches = {int(f["image_id"]): _frame_matches(f) for f in frames}
    flags_of = {(int(f["image_id"]), i): 0 for f in frames for i in range(len(f["labels"]))}
    for t, thr in enumerate(thresholds):
        for c in range(num_classes - 1):
            dets = [(float(np.float32(f["scores"][i])), int(f["image_id"]), i, f)
                    for f in frames for i in range(len(f["labels"])) if int(f["labels"][i]) == c]
            dets.sort(key=lambda d: d[0], reverse=True)
            used = {}
            for _, im, i, f in dets:
                ovmax, m = matches[im][i]
                flag = FP
                if ovmax >= thr:
                    if not f["gt_difficult"][m]:
                        if not used.get((im, m), False):
                            flag = TP
                            used[(im, m)] = True
                    else:
                        flag = IGNORED
                flags_of[(im, i)] |= flag << (2 * t)
    return _records(frames, flags_of), npos_of(frames, num_classes)


def parallel(frames, num_classes, thresholds, fast=False):
    """The per-frame form: returns (records, npos).  fast: the overlaps by _frame_matches_np."""
    flags_of = {}
    for f in frames:
        ms = _frame_matches(f, fast)
        im = int(f["image_id"])
        order = sorted(range(len(ms)), key=lambda i: (-float(np.float32(f["scores"][i])), i))
        for i in range(len(ms)):
            flags_of[(im, i)] = 0
        for t, thr in enumerate(thresholds):
            taken = set()
            for i in order:
                ovmax, m = ms[i]
                flag = FP
                if ovmax >= thr:
                    if f["gt_difficult"][m]:
                        flag = IGNORED
                    elif m not in taken:
                        flag = TP
                        taken.add(m)
                flags_of[(im, i)] |= flag << (2 * t)
    return _records(frames, flags_of), npos_of(frames, num_classes)


def voc_ap(rec, prec):
    """voc_eval.py:115-135."""
    mrec = [0.0] + list(rec) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap


def average_precision(records, npos, n_thresholds):
    """voc_eval.py:199-219 per class and threshold: ap [T, C-1] float64, NaN for the classes with npos = 0; and map [T]."""
    nc = len(npos)
    ap = np.full((n_thresholds, nc), np.nan, np.float64)
    for t in range(n_thresholds):
        for c in range(nc):
            if npos[c] == 0:
                continue
            fl = (records["flags"][records["label"] == c] >> (2 * t)) & 3
            tp, fp, rec, prec = 0, 0, [], []
            for v in fl:
                tp += int(v == TP)
                fp += int(v == FP)
                rec.append(float(tp) / int(npos[c]))
                prec.append(float(tp) / max(fp + tp, EPS))
            ap[t, c] = voc_ap(rec, prec)
    return ap, mean_ap(ap)


def mean_ap(ap):
    """voc_eval.py:220-223 over the classes the reference knows (npos > 0), in class order."""
    out = np.full(ap.shape[0], np.nan, np.float64)
    for t in range(ap.shape[0]):
        vals = [float(v) for v in ap[t] if not np.isnan(v)]
        if vals:
            s = 0.0
            for v in vals:
                s += v
            out[t] = s / len(vals)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# seeded sets
# --------------------------------------------------------------------------------------------------------------------------
def make_set(seed, n_images=12, num_classes=6, max_gt=6, max_det=40, quantise=0.05, difficult=0.25, duplicate_gt=0.2,
             empty_class=True, sizes=((500, 375), (353, 500), (1000, 600))):
    """Frames with the adverse kinds mixed in: quantised (tied) scores, duplicated ground-truth boxes, difficult ground truths,
    detections that are jittered copies of ground truths (and repeats of them), frames without ground truth or without detections,
    a class that never has a ground truth (the last one, when empty_class) and one that never has a detection (class 0 of odd seeds)."""
    rng = np.random.RandomState(seed)
    nc = num_classes - 1
    gt_classes = nc - 1 if empty_class and nc > 1 else nc
    no_det_class = 0 if (seed % 2 == 1 and nc > 2) else -1
    frames = []
    for im in range(n_images):
        w, h = sizes[rng.randint(len(sizes))]
        G = 0 if im % 7 == 3 else rng.randint(1, max_gt + 1)
        x1 = rng.randint(1, w - 40, G)
        y1 = rng.randint(1, h - 40, G)
        gt = np.stack([x1, y1, np.minimum(x1 + rng.randint(8, w // 2, G), w), np.minimum(y1 + rng.randint(8, h // 2, G), h)], 1).astype(np.float32).reshape(-1, 4)
        gl = rng.randint(0, gt_classes, G).astype(np.int32)
        for g in range(1, G):
            if rng.rand() < duplicate_gt:
                gt[g], gl[g] = gt[g - 1], gl[g - 1]
        gd = (rng.rand(G) < difficult).astype(np.uint8)
        D = 0 if im % 7 == 5 else rng.randint(1, max_det + 1)
        boxes = np.zeros((D, 4), np.float32)
        labels = np.zeros(D, np.int32)
        for i in range(D):
            if G and rng.rand() < 0.7:
                g = rng.randint(G)
                j = rng.randint(-12, 13, 4) * (rng.rand() < 0.8)
                b = gt[g] + j
                labels[i] = gl[g] if rng.rand() < 0.85 else rng.randint(0, nc)
            else:
                bx, by = rng.randint(0, w - 20), rng.randint(0, h - 20)
                b = np.array([bx, by, bx + rng.randint(5, w // 2), by + rng.randint(5, h // 2)], np.float64)
                labels[i] = rng.randint(0, nc)
            boxes[i] = np.clip(np.array([b[0] / w, b[1] / h, b[2] / w, b[3] / h]), 0, 1).astype(np.float32)
        if no_det_class >= 0:
            labels[labels == no_det_class] = 1
        scores = rng.rand(D).astype(np.float32)
        if quantise:
            scores = (np.round(scores / quantise) * quantise).astype(np.float32)
        frames.append({"image_id": im, "w": w, "h": h, "boxes": boxes, "labels": labels, "scores": scores,
                       "gt_boxes": gt, "gt_labels": gl, "gt_difficult": gd})
    return frames


def frames_from_golden(z):
    """The frames stored in tests/golden/voc_eval.npz (flat arrays with per-image offsets)."""
    frames = []
    do, go = z["det_offsets"], z["gt_offsets"]
    for im in range(len(z["sizes"])):
        d, g = slice(int(do[im]), int(do[im + 1])), slice(int(go[im]), int(go[im + 1]))
        frames.append({"image_id": im, "w": int(z["sizes"][im, 0]), "h": int(z["sizes"][im, 1]), "boxes": z["det_boxes"][d],
                       "labels": z["det_labels"][d], "scores": z["det_scores"][d], "gt_boxes": z["gt_boxes"][g],
                       "gt_labels": z["gt_labels"][g], "gt_difficult": z["gt_difficult"][g]})
    return frames


def make_big_frame(seed, D, G, num_classes, image_id=0, w=1000, h=600):
    """One frame with D detections and G ground truths: most detections are jittered copies of ground truths (so every ground truth is
    contested by many), scores on a grid of 64 values (ties), a quarter of the ground truths difficult, some of them duplicated."""
    rng = np.random.RandomState(seed)
    nc = num_classes - 1
    x1, y1 = rng.randint(0, w - 60, G), rng.randint(0, h - 60, G)
    gt = np.stack([x1, y1, np.minimum(x1 + rng.randint(10, 300, G), w), np.minimum(y1 + rng.randint(10, 300, G), h)], 1).astype(np.float32)
    gl = rng.randint(0, nc, G).astype(np.int32)
    dup = np.nonzero(rng.rand(G) < 0.1)[0]
    dup = dup[dup > 0]
    gt[dup], gl[dup] = gt[dup - 1], gl[dup - 1]
    gd = (rng.rand(G) < 0.25).astype(np.uint8)
    src = rng.randint(0, G, D)
    b = gt[src].astype(np.float64) + rng.randint(-15, 16, (D, 4)) * (rng.rand(D, 1) < 0.8)
    far = rng.rand(D) < 0.15
    b[far] = np.stack([rng.randint(0, w // 2, far.sum()), rng.randint(0, h // 2, far.sum()), rng.randint(w // 2, w, far.sum()),
                       rng.randint(h // 2, h, far.sum())], 1)
    boxes = np.clip(b / np.array([w, h, w, h]), 0, 1).astype(np.float32)
    labels = np.where(rng.rand(D) < 0.9, gl[src], rng.randint(0, nc, D)).astype(np.int32)
    scores = (rng.randint(1, 65, D) / 64.0).astype(np.float32)
    return {"image_id": image_id, "w": w, "h": h, "boxes": boxes, "labels": labels, "scores": scores, "gt_boxes": gt, "gt_labels": gl,
            "gt_difficult": gd}
