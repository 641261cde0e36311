"""The COCO detection protocol (iouType "bbox", useCats = 1) restated from the published algorithm of pycocotools' COCOeval
(evaluate / computeIoU / evaluateImg / accumulate / summarize) and maskUtils.iou on boxes, as literal Python and numpy loops: what the
reference's test loop scores with (test.py:17-18, 60-88, 124-128; evaluation/coco_eval.py).  Written for reading, not for speed.
pycocotools itself is not available to this project's tests, so this restatement is NOT pinned to its code (docs/PARITY.md);
tests/test_coco_crosscheck.py compares the two wherever pycocotools can be imported.

A frame is a dict: image_id, w, h, boxes f32 [n,4] (normalised xyxy), labels i32 [n] (0-based), scores f32 [n], gt_boxes f64 [g,4]
(pixel xywh), gt_area f64 [g], gt_labels i32 [g], gt_iscrowd u8 [g]."""
import numpy as np

TP, FP, IGNORED = 1, 2, 3
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]          # all, small, medium, large


# ------------------------------------------------------------------------------------------------------------------ inputs
def det_xywh(f):
    """test.py:70-71 and convert_to_xywh in fp32, then .tolist(): float64 [n,4]."""
    scale = np.array([f["w"], f["h"], f["w"], f["h"]], np.float32)
    px = (np.asarray(f["boxes"], np.float32).reshape(-1, 4) * scale).astype(np.float32)
    out = np.stack([px[:, 0], px[:, 1], (px[:, 2] - px[:, 0]).astype(np.float32), (px[:, 3] - px[:, 1]).astype(np.float32)], 1)
    return out.astype(np.float64)


def box_iou(d, g, crowd):
    """maskUtils.iou (bbIou) for one pair of xywh boxes, float64, in its operation order."""
    w = np.fmin(d[0] + d[2], g[0] + g[2]) - np.fmax(d[0], g[0])
    if w <= 0:
        return 0.0
    h = np.fmin(d[1] + d[3], g[1] + g[3]) - np.fmax(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def _outside(area, rng):
    return bool(area < rng[0] or area > rng[1])


# ------------------------------------------------------------------------------------------------------------------ evaluateImg
def _prepare(f, k, max_det):
    """The category's detections of one frame in score order (mergesort on -score: ties by position), cut to max_det, with their
    IoUs against the category's ground truths in original order (computeIoU)."""
    lab, gl = np.asarray(f["labels"]), np.asarray(f["gt_labels"])
    di, gi = np.nonzero(lab == k)[0], np.nonzero(gl == k)[0]
    if len(di) == 0 and len(gi) == 0:
        return None
    sc = np.asarray(f["scores"], np.float32)[di]
    order = np.argsort(-sc.astype(np.float64), kind="mergesort")[:max_det]
    di = di[order]
    dbox = det_xywh(f)[di]
    gbox = np.asarray(f["gt_boxes"], np.float64).reshape(-1, 4)[gi]
    crowd = np.asarray(f["gt_iscrowd"])[gi].astype(bool)
    ious = np.zeros((len(di), len(gi)), np.float64)
    for a in range(len(di)):
        for b in range(len(gi)):
            ious[a, b] = box_iou(dbox[a], gbox[b], crowd[b])
    return {"pos": di, "score": np.asarray(f["scores"], np.float32)[di], "dbox": dbox, "darea": dbox[:, 2] * dbox[:, 3], "crowd": crowd,
            "garea": np.asarray(f["gt_area"], np.float64)[gi], "ious": ious}


def evaluate_img(p, rng, thrs):
    """COCOeval.evaluateImg for one (image, category, area range): (matched [T,D], dtIg [T,D], gtIg [G] in original order)."""
    G, D, T = len(p["garea"]), len(p["pos"]), len(thrs)
    gt_ig = np.array([bool(p["crowd"][g]) or _outside(p["garea"][g], rng) for g in range(G)], bool)
    gtind = np.argsort(gt_ig.astype(np.int64), kind="mergesort")            # non-ignored first, stable
    g_ig, iscrowd = gt_ig[gtind], p["crowd"][gtind]
    ious = p["ious"][:, gtind] if G else p["ious"]
    gtm = np.zeros((T, G), bool)
    dtm = np.zeros((T, D), bool)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(thrs):
        for dind in range(D):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind, gind] and not iscrowd[gind]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gind]:
                    break
                if ious[dind, gind] < iou:
                    continue
                iou = ious[dind, gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = g_ig[m]
            dtm[tind, dind] = True
            gtm[tind, m] = True
    a = np.array([_outside(ar, rng) for ar in p["darea"]], bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(a, T, 0)))
    return dtm, dt_ig, gt_ig


def evaluate_img_two_pass(p, rng, thrs):
    """The same decisions without sorting the ground truths: a pass over the non-ignored ones in original order, then -- only if it
    matched nothing -- a pass over the ignored ones.  The form the device kernel runs."""
    G, D, T = len(p["garea"]), len(p["pos"]), len(thrs)
    gt_ig = np.array([bool(p["crowd"][g]) or _outside(p["garea"][g], rng) for g in range(G)], bool)
    gtm = np.zeros((T, G), bool)
    dtm = np.zeros((T, D), bool)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(thrs):
        for dind in range(D):
            best, m = min([t, 1 - 1e-10]), -1
            for ignored in (False, True):
                if ignored and m > -1:
                    break
                for g in range(G):
                    if gt_ig[g] != ignored or (gtm[tind, g] and not p["crowd"][g]) or p["ious"][dind, g] < best:
                        continue
                    best, m = p["ious"][dind, g], g
            if m > -1:
                dtm[tind, dind], dt_ig[tind, dind], gtm[tind, m] = True, gt_ig[m], True
            elif _outside(p["darea"][dind], rng):
                dt_ig[tind, dind] = True
    return dtm, dt_ig, gt_ig


def evaluate(frames, num_classes, thrs=IOU_THRS, max_det=MAX_DETS[-1], img_fn=evaluate_img):
    """COCOeval.evaluate: {(k, a, image_id): per-image result} for every pair with a ground truth or a detection."""
    out = {}
    for f in frames:
        for k in range(num_classes - 1):
            p = _prepare(f, k, max_det)
            if p is None:
                continue
            for a, rng in enumerate(AREA_RNG):
                dtm, dt_ig, gt_ig = img_fn(p, rng, thrs)
                out[(k, a, int(f["image_id"]))] = {"score": p["score"], "pos": p["pos"], "dtm": dtm, "dtIg": dt_ig, "gtIg": gt_ig}
    return out


# ------------------------------------------------------------------------------------------------------------------ accumulate
def accumulate(ev, num_classes, thrs=IOU_THRS, max_dets=MAX_DETS, rec_thrs=REC_THRS):
    """COCOeval.accumulate: precision [T,R,K,A,M], recall [T,K,A,M] (-1 where nothing was evaluated), npig [K,A]."""
    T, R, K, A, M = len(thrs), len(rec_thrs), num_classes - 1, len(AREA_RNG), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    npig_all = np.zeros((K, A), np.int64)
    images = sorted(set(i for (_, _, i) in ev))
    for k in range(K):
        for a in range(A):
            E = [ev[(k, a, i)] for i in images if (k, a, i) in ev]
            if len(E) == 0:
                continue
            gt_ig = np.concatenate([e["gtIg"] for e in E])
            npig = np.count_nonzero(gt_ig == 0)
            npig_all[k, a] = npig
            for m, max_det in enumerate(max_dets):
                dt_scores = np.concatenate([e["score"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores.astype(np.float64), kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIg"][:, 0:max_det] for e in E], axis=1)[:, inds]
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(inds_r):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[:, :, k, a, m][t] = q
    return precision, recall, npig_all


def summarize(precision, recall, thrs=IOU_THRS):
    """COCOeval.summarize: the 12 stats."""
    def one(ap, iou_thr, a, m):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == thrs)[0]]
        s = s[:, :, :, [a], [m]] if ap else s[:, :, [a], [m]]
        return -1.0 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    return np.array([one(1, None, 0, 2), one(1, .5, 0, 2), one(1, .75, 0, 2), one(1, None, 1, 2), one(1, None, 2, 2), one(1, None, 3, 2),
                     one(0, None, 0, 0), one(0, None, 0, 1), one(0, None, 0, 2), one(0, None, 1, 2), one(0, None, 2, 2), one(0, None, 3, 2)],
                    np.float64)


def run(frames, num_classes, thrs=IOU_THRS, max_dets=MAX_DETS, img_fn=evaluate_img):
    """The whole protocol: {"ev", "precision", "recall", "npig", "stats", "records"}."""
    thrs = np.asarray(thrs, np.float64)
    ev = evaluate(frames, num_classes, thrs, max_dets[-1], img_fn)
    precision, recall, npig = accumulate(ev, num_classes, thrs, max_dets)
    return {"ev": ev, "precision": precision, "recall": recall, "npig": npig, "stats": summarize(precision, recall, thrs),
            "records": records(ev, len(thrs))}


# ------------------------------------------------------------------------------------------------------------------ records
def records(ev, T):
    """The per-image results as the device stores them, in the defined order (label ascending, score descending, image_id ascending,
    rank ascending): score f32, label, image_id, rank i32, flags u32 [n,4] (per area range 2 bits per threshold)."""
    rows = []
    for (k, a, i), e in ev.items():
        if a != 0:
            continue
        for r in range(len(e["score"])):
            fl = []
            for aa in range(len(AREA_RNG)):
                ee, w = ev[(k, aa, i)], 0
                for t in range(T):
                    code = IGNORED if ee["dtIg"][t, r] else (TP if ee["dtm"][t, r] else FP)
                    w |= code << (2 * t)
                fl.append(w)
            rows.append((k, -float(e["score"][r]), i, r, e["score"][r], fl))
    rows.sort(key=lambda x: x[:4])
    return {"label": np.array([x[0] for x in rows], np.int32), "score": np.array([x[4] for x in rows], np.float32),
            "image_id": np.array([x[2] for x in rows], np.int32), "rank": np.array([x[3] for x in rows], np.int32),
            "flags": np.array([x[5] for x in rows], np.uint32).reshape(-1, 4)}


# ------------------------------------------------------------------------------------------------------------------ synthetic sets
def _frame(image_id, w, h, px_xyxy, labels, scores, gt_xywh, gt_labels, gt_iscrowd, gt_area=None):
    gt = np.asarray(gt_xywh, np.float64).reshape(-1, 4)
    return {"image_id": int(image_id), "w": int(w), "h": int(h),
            "boxes": (np.asarray(px_xyxy, np.float64).reshape(-1, 4) / np.array([w, h, w, h], np.float64)).astype(np.float32),
            "labels": np.asarray(labels, np.int32).reshape(-1), "scores": np.asarray(scores, np.float32).reshape(-1), "gt_boxes": gt,
            "gt_area": gt[:, 2] * gt[:, 3] if gt_area is None else np.asarray(gt_area, np.float64).reshape(-1),
            "gt_labels": np.asarray(gt_labels, np.int32).reshape(-1), "gt_iscrowd": np.asarray(gt_iscrowd, np.uint8).reshape(-1)}


def one_frame(dets_px_xyxy, scores, gt_xywh, iscrowd=None, labels=None, gt_labels=None, gt_area=None, w=512, h=512, image_id=0):
    """A hand-made frame on a 512 x 512 image: pixel coordinates that are multiples of 1/8 survive the fp32 round trip exactly."""
    n, g = len(scores), len(gt_xywh)
    return _frame(image_id, w, h, dets_px_xyxy, np.zeros(n) if labels is None else labels, scores, gt_xywh,
                  np.zeros(g) if gt_labels is None else gt_labels, np.zeros(g) if iscrowd is None else iscrowd, gt_area)


def make_set(seed, n_images=20, num_classes=7, max_det=300, max_gt=24, sizes=((512, 256), (640, 427), (1024, 512), (500, 375))):
    """A synthetic test set with the adverse kinds kinds() counts.  The last category (num_classes - 2) is never used.  Ground truths
    lie on a quarter-pixel grid; detections are jittered, exact or nested copies of ground truths plus clutter; scores are drawn from
    a few values so that ties within and across images are common."""
    rng = np.random.RandomState(seed)
    K = num_classes - 2
    frames = []
    for i in range(n_images):
        w, h = sizes[i % len(sizes)]
        ng = 0 if i % 7 == 3 else int(rng.randint(1, max_gt + 1))
        if i == 1:
            ng = max_gt
        side = np.array([8, 24, 32, 40, 64, 96, 120, 200])[rng.randint(0, 8, ng)].astype(np.float64)
        gw = np.minimum(side * np.array([1.0, 1.0, 0.5, 2.0])[rng.randint(0, 4, ng)], w / 2.0)
        gh = np.minimum(side, h / 2.0)
        gx = np.floor(rng.rand(ng) * (w - gw) * 4) / 4
        gy = np.floor(rng.rand(ng) * (h - gh) * 4) / 4
        gtb = np.stack([gx, gy, gw, gh], 1).reshape(-1, 4)
        gtl = rng.randint(0, K, ng)
        crowd = (rng.rand(ng) < 0.2).astype(np.uint8)
        area = gw * gh
        if ng >= 3:                                                       # annotation areas exactly on 32^2 and 96^2
            area[0], area[1] = 1024.0, 9216.0
        nd = 0 if i % 7 == 5 else int(rng.randint(max_det // 3, max_det + 1))
        px, dl = np.zeros((nd, 4)), np.zeros(nd, np.int64)
        for j in range(nd):
            kind = rng.randint(0, 5) if ng else 4
            if kind < 4:
                g = rng.randint(0, ng)
                x, y, bw, bh = gtb[g]
                dl[j] = gtl[g] if rng.rand() < 0.9 else rng.randint(0, K)
                if kind == 1:                                             # jitter
                    x, y = x + rng.randint(-8, 9) / 4.0 * (bw / 16), y + rng.randint(-8, 9) / 4.0 * (bh / 16)
                elif kind == 2:                                           # the upper half, three quarters, ...: IoU = 1/2, 3/4, ... exactly
                    bh = bh * (0.5, 0.75, 0.625)[rng.randint(0, 3)]
                elif kind == 3:                                           # a larger box around it
                    bw, bh = bw * 1.25, bh * 1.25
                px[j] = [max(x, 0), max(y, 0), min(x + bw, w), min(y + bh, h)]
            else:
                x, y = rng.rand() * w * 0.8, rng.rand() * h * 0.8
                px[j] = [x, y, x + rng.rand() * w * 0.2 + 1, y + rng.rand() * h * 0.2 + 1]
                dl[j] = rng.randint(0, K)
        if i % 5 == 0 and nd > 120:                                       # one category with more than 100 detections in a frame
            dl[:120] = 0
        sc = rng.randint(1, 40, nd) / 40.0 if i % 2 else rng.rand(nd)
        frames.append(_frame(100 + 3 * i, w, h, px, dl, sc, gtb, gtl, crowd, area))
    return frames


def make_big_frame(seed, n_det=2000, n_gt=1024, num_classes=5, w=2048, h=1024, image_id=0):
    rng = np.random.RandomState(seed)
    K = num_classes - 1
    gw, gh = rng.randint(4, 64, n_gt) * 2.0, rng.randint(4, 64, n_gt) * 2.0
    gx, gy = np.floor(rng.rand(n_gt) * (w - gw)), np.floor(rng.rand(n_gt) * (h - gh))
    gtb = np.stack([gx, gy, gw, gh], 1)
    gtl = rng.randint(0, K, n_gt)
    g = rng.randint(0, n_gt, n_det)
    j = rng.randint(-2, 3, (n_det, 4)) * (rng.rand(n_det, 1) < 0.7)
    px = np.stack([gx[g] + j[:, 0], gy[g] + j[:, 1], gx[g] + gw[g] + j[:, 2], gy[g] + gh[g] + j[:, 3]], 1).clip(0, [w, h, w, h])
    return _frame(image_id, w, h, px, gtl[g], rng.randint(1, 500, n_det) / 500.0, gtb, gtl, rng.rand(n_gt) < 0.15)


def kinds(frames, res, thrs=IOU_THRS):
    """How often each adverse kind occurs in a set (res = run(frames, ...))."""
    c = dict.fromkeys(("tied_scores_within_image", "tied_scores_across_images", "category_over_100_dets", "crowd_matched_more_than_once",
                       "gt_area_below_32sq", "gt_area_equal_32sq", "gt_area_between", "gt_area_equal_96sq", "gt_area_above_96sq",
                       "iou_equal_threshold", "frame_without_detections", "frame_without_gt"), 0)
    seen = {}
    for f in frames:
        c["frame_without_detections"] += len(f["labels"]) == 0
        c["frame_without_gt"] += len(f["gt_labels"]) == 0
        for k in np.unique(f["labels"]):
            sc = f["scores"][f["labels"] == k]
            c["category_over_100_dets"] += len(sc) > 100
            c["tied_scores_within_image"] += len(np.unique(sc)) < len(sc)
            for s in np.unique(sc):
                c["tied_scores_across_images"] += seen.get((int(k), float(s)), f["image_id"]) != f["image_id"]
                seen[(int(k), float(s))] = f["image_id"]
        ar = f["gt_area"]
        c["gt_area_below_32sq"] += int((ar < 1024).sum())
        c["gt_area_equal_32sq"] += int((ar == 1024).sum())
        c["gt_area_between"] += int(((ar > 1024) & (ar < 9216)).sum())
        c["gt_area_equal_96sq"] += int((ar == 9216).sum())
        c["gt_area_above_96sq"] += int((ar > 9216).sum())
        for k in np.unique(f["gt_labels"]):
            p = _prepare(f, int(k), 100)
            c["iou_equal_threshold"] += int(np.isin(p["ious"], thrs).sum())
            if p["crowd"].any() and len(p["pos"]):
                hits = ((p["ious"] >= thrs[0]) & p["crowd"][None, :]).sum(0)
                c["crowd_matched_more_than_once"] += int((hits > 1).sum())
    last = res["npig"].shape[0] - 1
    c["category_never_seen"] = int(all((f["labels"] != last).all() and (f["gt_labels"] != last).all() for f in frames))
    return c


def to_coco(frames, num_classes):
    """(ground-truth dataset dict, detection list) in the COCO json layout, category ids 1-based, for pycocotools."""
    gt = {"images": [{"id": int(f["image_id"]), "width": f["w"], "height": f["h"]} for f in frames],
          "categories": [{"id": k + 1} for k in range(num_classes - 1)], "annotations": []}
    dets = []
    for f in frames:
        for b, a, l, c in zip(f["gt_boxes"].tolist(), f["gt_area"].tolist(), f["gt_labels"].tolist(), f["gt_iscrowd"].tolist()):
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": int(f["image_id"]), "category_id": l + 1, "bbox": b,
                                      "area": a, "iscrowd": int(c)})
        for b, l, s in zip(det_xywh(f).tolist(), f["labels"].tolist(), f["scores"].tolist()):
            dets.append({"image_id": int(f["image_id"]), "category_id": l + 1, "bbox": b, "score": s})
    return gt, dets
