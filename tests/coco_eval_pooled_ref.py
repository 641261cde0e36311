"""The COCO bbox protocol with every category pooled (pycocotools' COCOeval with params.useCats = 0) restated from the published
algorithm, on top of tests/coco_eval_ref.py: evaluateImg, its two-pass form, accumulate, summarize and the record layout are THAT
module's functions, imported; the only thing that changes is what is in the lists.  pycocotools itself is not available to this
project's tests, so this restatement is NOT pinned to its code (docs/PARITY.md); tests/test_coco_pooled_crosscheck.py compares the two
wherever pycocotools can be imported.

Pooled lists (COCOeval.evaluateImg with useCats = 0: `[_ for cId in p.catIds for _ in self._dts[imgId, cId]]`, the same for the ground
truths): a frame's detections and its ground truths are each ONE list in the order (label ascending, original position ascending).  The
detections are then ordered by np.argsort(-score, kind="mergesort") over that list -- equal scores go label ascending, position
ascending -- and cut to maxDets[-1].  A detection may match a ground truth of any label.  There is one category, 0.

Frames are the dicts of tests/coco_eval_ref.py."""
import numpy as np

import coco_eval_ref as ref
from coco_eval_ref import accumulate, evaluate_img, evaluate_img_two_pass, records, summarize

MAX_DETS = (100, 300, 1000)


# ------------------------------------------------------------------------------------------------------------------ inputs
def iou_matrix(dbox, gbox, crowd):
    """maskUtils.iou (bbIou) for every pair, float64, in box_iou's operation order: [D, G]."""
    D, G = len(dbox), len(gbox)
    if D == 0 or G == 0:
        return np.zeros((D, G), np.float64)
    d, g = dbox[:, None, :], gbox[None, :, :]
    w = np.fmin(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.fmax(d[..., 0], g[..., 0])
    h = np.fmin(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.fmax(d[..., 1], g[..., 1])
    i = w * h
    u = np.where(crowd[None, :], d[..., 2] * d[..., 3], d[..., 2] * d[..., 3] + g[..., 2] * g[..., 3] - i)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = i / u
    return np.where((w <= 0) | (h <= 0), 0.0, q)


def pooled_order(labels):
    """The positions of a list in pooled order: label ascending, then original position."""
    return np.argsort(np.asarray(labels, np.int64), kind="mergesort")


def _prepare(f, max_det, literal_iou=False):
    """The frame's pooled detections in score order (mergesort on -score over the pooled order), cut to max_det, with their IoUs
    against the pooled ground truths (computeIoU).  "pos" / "gpos" are original positions.  literal_iou: box_iou pair by pair."""
    dpool, gpool = pooled_order(f["labels"]), pooled_order(f["gt_labels"])
    if len(dpool) == 0 and len(gpool) == 0:
        return None
    sc = np.asarray(f["scores"], np.float32)[dpool]
    di = dpool[np.argsort(-sc.astype(np.float64), kind="mergesort")[:max_det]]
    dbox = ref.det_xywh(f)[di]
    gbox = np.asarray(f["gt_boxes"], np.float64).reshape(-1, 4)[gpool]
    crowd = np.asarray(f["gt_iscrowd"])[gpool].astype(bool)
    if literal_iou:
        ious = np.zeros((len(di), len(gpool)), np.float64)
        for a in range(len(di)):
            for b in range(len(gpool)):
                ious[a, b] = ref.box_iou(dbox[a], gbox[b], crowd[b])
    else:
        ious = iou_matrix(dbox, gbox, crowd)
    return {"pos": di, "gpos": gpool, "score": np.asarray(f["scores"], np.float32)[di], "dbox": dbox, "darea": dbox[:, 2] * dbox[:, 3],
            "crowd": crowd, "garea": np.asarray(f["gt_area"], np.float64)[gpool], "ious": ious}


# ------------------------------------------------------------------------------------------------------------------ evaluateImg, vectorised
def evaluate_img_argmax(p, rng, thrs):
    """evaluate_img_two_pass with the inner loop over the ground truths as one arg-max: among the eligible ground truths (not matched,
    or crowd; IoU >= the walk's start) of a pass, "< best: continue" keeps the LAST of the largest IoUs.  The form the device kernel
    runs, and fast enough for frames of 1000 x 1024."""
    G, D, T = len(p["garea"]), len(p["pos"]), len(thrs)
    gt_ig = np.logical_or(p["crowd"], np.logical_or(p["garea"] < rng[0], p["garea"] > rng[1])) if G else np.zeros(0, bool)
    d_out = np.logical_or(p["darea"] < rng[0], p["darea"] > rng[1])
    dtm = np.zeros((T, D), bool)
    dt_ig = np.zeros((T, D), bool)
    crowd, ious = p["crowd"], p["ious"]
    idx = np.arange(G)
    for tind, t in enumerate(thrs):
        best0 = min([t, 1 - 1e-10])
        gtm = np.zeros(G, bool)
        for dind in range(D):
            m = -1
            if G:
                row = ious[dind]
                eligible = np.logical_and(np.logical_or(~gtm, crowd), row >= best0)
                for ignored in (False, True):
                    c = np.logical_and(eligible, gt_ig == ignored)
                    if c.any():
                        m = int(idx[np.logical_and(c, row == row[c].max())].max())
                        break
            if m > -1:
                dtm[tind, dind], dt_ig[tind, dind], gtm[m] = True, gt_ig[m], True
            elif d_out[dind]:
                dt_ig[tind, dind] = True
    return dtm, dt_ig, gt_ig


# ------------------------------------------------------------------------------------------------------------------ the protocol
def evaluate(frames, thrs=ref.IOU_THRS, max_det=MAX_DETS[-1], img_fn=evaluate_img_argmax, literal_iou=False):
    """COCOeval.evaluate with useCats = 0: {(0, a, image_id): per-image result} for every frame with a ground truth or a detection."""
    out = {}
    for f in frames:
        p = _prepare(f, max_det, literal_iou)
        if p is None:
            continue
        for a, rng in enumerate(ref.AREA_RNG):
            dtm, dt_ig, gt_ig = img_fn(p, rng, thrs)
            out[(0, a, int(f["image_id"]))] = {"score": p["score"], "pos": p["pos"], "dtm": dtm, "dtIg": dt_ig, "gtIg": gt_ig}
    return out


def run(frames, thrs=ref.IOU_THRS, max_dets=MAX_DETS, img_fn=evaluate_img_argmax, literal_iou=False):
    """The whole pooled protocol: {"ev", "precision" [T,R,1,4,3], "recall" [T,1,4,3], "npig" [1,4], "stats", "records"}."""
    thrs = np.asarray(thrs, np.float64)
    ev = evaluate(frames, thrs, max_dets[-1], img_fn, literal_iou)
    precision, recall, npig = accumulate(ev, 2, thrs, max_dets)
    return {"ev": ev, "precision": precision, "recall": recall, "npig": npig, "stats": summarize(precision, recall, thrs),
            "records": records(ev, len(thrs))}


def proposal_summary(r):
    """What evaluation.ProposalEvaluator.summarize() keeps of run()'s result."""
    return {"ar": r["stats"][6:9], "ar_small": r["stats"][9], "ar_medium": r["stats"][10], "ar_large": r["stats"][11],
            "recall": r["recall"][:, 0], "npig": r["npig"][0]}


# ------------------------------------------------------------------------------------------------------------------ synthetic frames
SIDES = np.array([8, 16, 32, 48, 64, 96, 128], np.float64)          # 32 x 32 and 96 x 96 lie exactly on the area ranges' edges


def grid_frame(seed, n_det, n_gt, num_labels=5, image_id=0, n_scores=12, crowd=0.15, span=384):
    """A frame on a 512 x 512 image whose coordinates are integers (exact in fp32 and float64): ground truths drawn from a coarse grid, so
    that identical boxes with different labels occur; detections are exact copies (IoU 1), upper halves and three quarters (IoU exactly
    1/2, 3/4: threshold hits), shifted copies and clutter, labelled like their ground truth or not; scores from n_scores values, so that
    ties within a frame are common.  Vectorised: fast at 2048 detections and 1024 ground truths."""
    rng = np.random.RandomState(seed)
    gw, gh = SIDES[rng.randint(0, len(SIDES), n_gt)], SIDES[rng.randint(0, len(SIDES), n_gt)]
    gx, gy = rng.randint(0, span // 16, n_gt) * 16.0, rng.randint(0, span // 16, n_gt) * 16.0
    gtl = rng.randint(0, num_labels, n_gt)
    if n_gt > 1:                                                    # a quarter of the ground truths repeat an earlier one's box: exact IoU ties
        src = np.where(rng.rand(n_gt) < 0.25, (rng.rand(n_gt) * np.arange(n_gt)).astype(np.int64), np.arange(n_gt))
        gx, gy, gw, gh = gx[src], gy[src], gw[src], gh[src]
    if n_gt:
        g = rng.randint(0, n_gt, n_det)
        kind = rng.randint(0, 5, n_det)
        x, y, w, h = gx[g].copy(), gy[g].copy(), gw[g].copy(), gh[g].copy()
        h = np.where(kind == 1, h * 0.5, np.where(kind == 2, h * 0.75, h))
        x = x + np.where(kind == 3, rng.randint(-2, 3, n_det) * (w / 8), 0.0)
        y = y + np.where(kind == 3, rng.randint(-2, 3, n_det) * (h / 8), 0.0)
        clutter = kind == 4
        x, y = np.where(clutter, rng.randint(0, 440, n_det) * 1.0, x), np.where(clutter, rng.randint(0, 440, n_det) * 1.0, y)
        w, h = np.where(clutter, rng.randint(4, 70, n_det) * 1.0, w), np.where(clutter, rng.randint(4, 70, n_det) * 1.0, h)
        dl = np.where(rng.rand(n_det) < 0.6, gtl[g], rng.randint(0, num_labels, n_det))
    else:
        x, y = rng.randint(0, 440, n_det) * 1.0, rng.randint(0, 440, n_det) * 1.0
        w, h = rng.randint(4, 70, n_det) * 1.0, rng.randint(4, 70, n_det) * 1.0
        dl = rng.randint(0, num_labels, n_det)
    px = np.stack([np.maximum(x, 0), np.maximum(y, 0), np.minimum(x + w, 512), np.minimum(y + h, 512)], 1).reshape(-1, 4)
    sc = rng.randint(1, n_scores + 1, n_det) / np.float64(n_scores + 1)
    return ref.one_frame(px, sc, np.stack([gx, gy, gw, gh], 1).reshape(-1, 4), iscrowd=rng.rand(n_gt) < crowd, labels=dl, gt_labels=gtl,
                         image_id=image_id)


def make_set(seed, shapes, num_labels=5, **kw):
    """One grid_frame per (n_det, n_gt) of `shapes`, image ids 100, 103, ..."""
    return [grid_frame(seed * 1000 + i, nd, ng, num_labels, image_id=100 + 3 * i, **kw) for i, (nd, ng) in enumerate(shapes)]


def kinds(frames, thrs=ref.IOU_THRS, max_det=MAX_DETS[-1]):
    """How often the adverse kinds occur in a set: exact IoU ties between eligible ground truths of a detection, IoUs exactly on a
    threshold, matches across labels, equal scores across labels."""
    c = dict.fromkeys(("iou_ties", "iou_equal_threshold", "best_gt_has_another_label", "score_ties_across_labels"), 0)
    for f in frames:
        p = _prepare(f, max_det)
        if p is None:
            continue
        io = p["ious"]
        if io.size:
            best = io.max(1)
            c["iou_ties"] += int(((io == best[:, None]).sum(1)[best >= thrs[0]] > 1).sum())
            c["iou_equal_threshold"] += int(np.isin(io, thrs).sum())
            lab_d, lab_g = np.asarray(f["labels"])[p["pos"]], np.asarray(f["gt_labels"])[p["gpos"]]
            c["best_gt_has_another_label"] += int(((lab_g[io.argmax(1)] != lab_d) & (best >= thrs[0])).sum())
        sc, lab = np.asarray(f["scores"]), np.asarray(f["labels"])
        for s in np.unique(sc):
            c["score_ties_across_labels"] += len(np.unique(lab[sc == s])) > 1
    return c
