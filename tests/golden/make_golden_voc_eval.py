"""Generates tests/golden/voc_eval.npz by RUNNING the reference's own evaluator (evaluation/voc_eval.py: save_gt, save_pred, cal_mAP)
on a small synthetic set, the way make_golden.py runs anchor.py and losses/loss.py.  The module is loaded by file path (the
`evaluation` package's __init__ pulls pycocotools, which is not installed).  Only inputs and results are stored: boxes, labels,
scores, sizes, difficult flags, the float64 per-class AP and mAP at each threshold, npos, and the counts of the adverse kinds the
set is asserted to contain.  Re-run:  python tests/golden/make_golden_voc_eval.py

cal_mAP is called with one class at a time (gt_classes=[name]) so that the exact float64 AP comes back instead of the two-decimal
print, and the ground-truth cache is rewritten before every call because cal_mAP marks the `used` flags in it."""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("FRCNN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import eval_ref  # noqa: E402  (tests/eval_ref.py: the seeded sets, and the overlap used to COUNT the adverse kinds below)

THRESHOLDS = (0.3, 0.5, 0.75)
NUM_CLASSES = 7                                   # 6 object classes; the last never has a ground truth


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_voc_eval", os.path.join(REF, "evaluation", "voc_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hand_frames(first_id):
    """Frames built for the adverse kinds (class 0 and 1).  On a 2048 x 512 image every coordinate k / 2048 is exact in fp32, and the
    overlap of [0, 0, k - 1, 511] with [0, 0, 1279, 511] is k / 1280: exactly 0.3 / 0.5 / 0.75 at k = 384 / 640 / 960."""
    w, h = 2048, 512

    def nb(b):
        return np.array([b[0] / w, b[1] / h, b[2] / w, b[3] / h], np.float32)
    fr = []
    # overlaps just below / above / on each threshold, one frame per threshold (one ground truth each)
    for t in THRESHOLDS:
        k = int(round(1280 * t))
        fr.append({"w": w, "h": h, "gt_boxes": np.array([[0, 0, 1279, 511]], np.float32), "gt_labels": np.array([0], np.int32),
                   "gt_difficult": np.array([0], np.uint8),
                   "boxes": np.stack([nb([0, 0, k - 1 - 0.4, 511]), nb([0, 0, k - 1 + 0.4, 511]), nb([0, 0, k - 1, 511])]),
                   "labels": np.zeros(3, np.int32), "scores": np.array([0.9, 0.8, 0.7], np.float32)})
    # two identical ground truths (an overlap tie), three equal-score detections on them (a second and a third on a used one)
    fr.append({"w": w, "h": h, "gt_boxes": np.array([[100, 100, 299, 299], [100, 100, 299, 299]], np.float32), "gt_labels": np.array([1, 1], np.int32),
               "gt_difficult": np.array([0, 0], np.uint8), "boxes": np.stack([nb([100, 100, 299, 299])] * 3),
               "labels": np.ones(3, np.int32), "scores": np.array([0.5, 0.5, 0.5], np.float32)})
    # the best match is difficult although an easy ground truth overlaps too
    fr.append({"w": w, "h": h, "gt_boxes": np.array([[100, 100, 299, 299], [110, 100, 309, 299]], np.float32), "gt_labels": np.array([1, 1], np.int32),
               "gt_difficult": np.array([1, 0], np.uint8), "boxes": np.stack([nb([100, 100, 299, 299]), nb([400, 100, 450, 300])]),
               "labels": np.ones(2, np.int32), "scores": np.array([0.5, 0.95], np.float32)})
    # iw == 0: the boxes touch with the +1 convention exactly cancelled
    fr.append({"w": w, "h": h, "gt_boxes": np.array([[100, 100, 200, 200]], np.float32), "gt_labels": np.array([0], np.int32),
               "gt_difficult": np.array([0], np.uint8), "boxes": np.stack([nb([201, 100, 300, 200])]),
               "labels": np.zeros(1, np.int32), "scores": np.array([0.5], np.float32)})
    for i, f in enumerate(fr):
        f["image_id"] = first_id + i
    return fr


def adverse_counts(frames):
    """How often each adverse kind occurs, counted with the restated overlap (tests/eval_ref.py)."""
    nc = NUM_CLASSES - 1
    c = dict.fromkeys(["tied_scores_within_image", "tied_scores_across_images", "identical_gt_boxes", "best_match_difficult", "second_on_used_gt",
                       "ov_just_below_threshold", "ov_just_above_threshold", "ov_equal_threshold", "class_dets_without_npos", "class_gt_without_dets",
                       "image_without_gt", "image_without_det"], 0)
    seen = [dict() for _ in range(nc)]
    for f in frames:
        c["image_without_gt"] += len(f["gt_labels"]) == 0
        c["image_without_det"] += len(f["labels"]) == 0
        pairs = set()
        for i in range(len(f["labels"])):
            key = (int(f["labels"][i]), float(f["scores"][i]))
            c["tied_scores_within_image"] += key in pairs
            pairs.add(key)
        for key in pairs:
            c["tied_scores_across_images"] += key[1] in seen[key[0]]
        for key in pairs:
            seen[key[0]][key[1]] = True
        G = len(f["gt_labels"])
        for a in range(G):
            for b in range(a + 1, G):
                c["identical_gt_boxes"] += int(f["gt_labels"][a] == f["gt_labels"][b] and np.array_equal(f["gt_boxes"][a], f["gt_boxes"][b]))
        ms = eval_ref._frame_matches(f)
        for t in THRESHOLDS:
            hits = {}
            for (ov, m) in ms:
                if m < 0:
                    continue
                c["ov_just_below_threshold"] += t - 1e-3 < ov < t
                c["ov_just_above_threshold"] += t < ov < t + 1e-3
                c["ov_equal_threshold"] += ov == t
                if ov >= t:
                    c["best_match_difficult"] += bool(f["gt_difficult"][m])
                    hits[m] = hits.get(m, 0) + 1
            c["second_on_used_gt"] += sum(v - 1 for m, v in hits.items() if not f["gt_difficult"][m])
    npos = eval_ref.npos_of(frames, NUM_CLASSES)
    for k in range(nc):
        nd = sum(int((f["labels"] == k).sum()) for f in frames)
        c["class_dets_without_npos"] += int(nd > 0 and npos[k] == 0)
        c["class_gt_without_dets"] += int(nd == 0 and npos[k] > 0)
    return {k: int(v) for k, v in c.items()}


def write_xml(path, f, names):
    objs = "".join("<object><name>%s</name><difficult>%d</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                   % (names[int(l)], int(d), int(b[0]), int(b[1]), int(b[2]), int(b[3]))
                   for b, l, d in zip(f["gt_boxes"], f["gt_labels"], f["gt_difficult"]))
    with open(path, "w") as fh:
        fh.write("<annotation>%s</annotation>" % objs)


def main():
    ref = load_reference()
    frames = eval_ref.make_set(20240, n_images=40, num_classes=NUM_CLASSES, max_gt=6, max_det=30)
    # class 4 keeps its ground truths and loses its detections (to class 5, which never has a ground truth)
    for f in frames:
        f["labels"][f["labels"] == 4] = 5
    frames += hand_frames(len(frames))
    for f in frames:
        assert np.array_equal(f["gt_boxes"], np.floor(f["gt_boxes"])), "VOC annotations are integers"
    counts = adverse_counts(frames)
    for k, v in counts.items():
        assert v >= 1, "the golden set lacks the adverse kind '%s'" % k
    nc = NUM_CLASSES - 1
    names = ["c%02d" % c for c in range(nc)]
    img_names = ["im%04d" % int(f["image_id"]) for f in frames]
    additional = [(int(f["w"]), int(f["h"])) for f in frames]
    ap = np.full((len(THRESHOLDS), nc), np.nan, np.float64)
    mean = np.zeros(len(THRESHOLDS), np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        xml_dir = os.path.join(tmp, "xml")
        os.mkdir(xml_dir)
        for f, n in zip(frames, img_names):
            write_xml(os.path.join(xml_dir, n + ".xml"), f, names)
        for t, thr in enumerate(THRESHOLDS):
            known, total = [], 0.0
            for c, name in enumerate(names):
                cache = os.path.join(tmp, "cache_%d_%d" % (t, c))
                os.mkdir(cache)
                gt_classes, counter = [], {}
                for n in img_names:
                    gt_classes, counter = ref.save_gt(os.path.join(xml_dir, n + ".xml"), cache, gt_classes, counter)
                if name not in counter:
                    continue                                   # a class the reference does not know: AP stays NaN
                ref.save_pred(img_names, additional, [f["boxes"] for f in frames], [f["scores"] for f in frames], [f["labels"] for f in frames],
                              name, names, cache)
                with contextlib.redirect_stdout(io.StringIO()):
                    ap[t, c] = ref.cal_mAP(cache, [name], counter, thr)
                known.append(c)
                total += ap[t, c]
            mean[t] = total / len(known)
            if t == 0:
                npos = np.array([counter.get(n, 0) for n in names], np.int64)
    assert np.array_equal(npos, eval_ref.npos_of(frames, NUM_CLASSES))
    d = {"thresholds": np.array(THRESHOLDS, np.float64), "num_classes": np.array(NUM_CLASSES), "ap": ap, "map": mean, "npos": npos,
         "sizes": np.array(additional, np.int32),
         "det_offsets": np.cumsum([0] + [len(f["labels"]) for f in frames]).astype(np.int64),
         "gt_offsets": np.cumsum([0] + [len(f["gt_labels"]) for f in frames]).astype(np.int64),
         "det_boxes": np.concatenate([f["boxes"].reshape(-1, 4) for f in frames]).astype(np.float32),
         "det_labels": np.concatenate([f["labels"] for f in frames]).astype(np.int32),
         "det_scores": np.concatenate([f["scores"] for f in frames]).astype(np.float32),
         "gt_boxes": np.concatenate([f["gt_boxes"].reshape(-1, 4) for f in frames]).astype(np.float32),
         "gt_labels": np.concatenate([f["gt_labels"] for f in frames]).astype(np.int32),
         "gt_difficult": np.concatenate([f["gt_difficult"] for f in frames]).astype(np.uint8),
         "adverse_kinds": np.array(sorted(counts)), "adverse_counts": np.array([counts[k] for k in sorted(counts)], np.int64)}
    np.savez_compressed(os.path.join(OUT, "voc_eval.npz"), **d)
    print("voc_eval.npz: %d images, %d detections, %d ground truths" % (len(frames), len(d["det_labels"]), len(d["gt_labels"])))
    print("AP:", ap, "mAP:", mean, "npos:", npos, "adverse:", counts)


if __name__ == "__main__":
    main()
