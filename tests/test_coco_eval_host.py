"""CPU-only checks of the COCO protocol of the device evaluator (faster_rcnn_pytorch_amd/evaluation.py, csrc/coco_eval.hip): hand-derived
known answers on the restatement the GPU tests compare against (tests/coco_eval_ref.py), the two-pass form of the ground-truth walk
that the kernel runs against the sorted form flag for flag, and the two new entry points declared, exported, bound and refusing bad
arguments without a device.

"1" below is ONE = 1 / (1 + 2^-52) = 1 - 2^-52: accumulate's pr = tp / (fp + tp + np.spacing(1)) keeps the spacing term when
fp + tp = 1, so a perfect precision-recall curve of this protocol holds ONE, not 1.0 (it prints as 1.000)."""
import os
import re
import subprocess

import numpy as np
import pytest

import coco_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1.0 / (1.0 + 2.0 ** -52)
ALL, SMALL, MEDIUM, LARGE = 0, 1, 2, 3


def mean_one(n):
    """A stat is np.mean over the n cells of its slice; over n cells that all hold ONE its pairwise sum does not return ONE itself
    (101 cells give 1 - 2^-53), so the expected stat is that mean of a hand-counted number of cells: T * 101 for an AP over T
    thresholds of one category."""
    return float(np.mean(np.full(n, ONE)))


AP_ONE, AP50_ONE = mean_one(1010), mean_one(101)
GT_M = [100, 100, 50, 50]                    # a medium ground truth (area 2500) and its exact detection
DET_M = [100, 100, 150, 150]


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _codes(res, a=ALL, t=0):
    """The 2-bit codes of the records (in record order) for one area range and threshold."""
    return ((res["records"]["flags"][:, a] >> (2 * t)) & 3).tolist()


# ------------------------------------------------------------------------------------------------------------ known answers
def test_01_one_gt_one_exact_detection():
    """tp = [1], fp = [0]: rc = [1], pr = [1 / (0 + 1 + 2^-52)] = ONE at every threshold (IoU = 1) and every recall threshold
    (searchsorted(rc, r) = 0 for r <= 1).  The ground truth is medium: 'all' and 'medium' hold ONE, 'small' and 'large' have npig = 0 and
    stay -1, so do their stats."""
    assert ONE == 1.0 - 2.0 ** -52
    res = ref.run([ref.one_frame([DET_M], [0.9], [GT_M])], 2)
    assert res["npig"].tolist() == [[1, 0, 1, 0]]
    assert (res["precision"][:, :, 0, [ALL, MEDIUM], :] == ONE).all() and (res["recall"][:, 0, [ALL, MEDIUM], :] == 1.0).all()
    assert (res["precision"][:, :, 0, [SMALL, LARGE], :] == -1).all() and (res["recall"][:, 0, [SMALL, LARGE], :] == -1).all()
    assert res["stats"].tolist() == [AP_ONE, AP50_ONE, AP50_ONE, -1, AP_ONE, -1, 1, 1, 1, -1, 1, -1]
    assert ONE <= AP_ONE <= 1.0 and ONE <= AP50_ONE <= 1.0


def test_02_true_positive_and_false_positive_on_one_gt():
    """(a) the exact detection (0.9) and a copy of it (0.8): the copy finds the ground truth matched -> FP.  tp = [1, 1], fp = [0, 1],
    pr = [ONE, 1/2], rc = [1, 1]: every recall threshold reads index 0 -> AP50 = ONE.
    (b) a detection of IoU 50*20 / 50*50 = 0.4 scoring 0.95 above the exact one (0.9): tp = [0, 1], fp = [1, 1], pr = [0 / (1 + eps),
    1 / (2 + eps)] = [0, 0.5] (2 + 2^-52 rounds to 2), envelope [0.5, 0.5], rc = [0, 1]: r = 0 reads index 0, r > 0 index 1 -> AP50 = 0.5."""
    a = ref.run([ref.one_frame([DET_M, DET_M], [0.9, 0.8], [GT_M])], 2)
    assert _codes(a) == [ref.TP, ref.FP] and (a["precision"][0, :, 0, ALL, 2] == ONE).all() and a["stats"][1] == AP50_ONE
    b = ref.run([ref.one_frame([[100, 100, 150, 120], DET_M], [0.95, 0.9], [GT_M])], 2)
    assert _codes(b) == [ref.FP, ref.TP]
    assert (b["precision"][0, :, 0, ALL, 2] == 0.5).all() and b["stats"][1] == 0.5


def test_03_iou_exactly_on_the_threshold():
    """[0,0,10,10] against [0,0,10,5]: i = 50, u = 100 + 50 - 50 = 100, IoU = 0.5 exactly: not < min(0.5, 1 - 1e-10), so matched at
    t = 0.5; 0.5 < 0.55, so unmatched from there on."""
    f = ref.one_frame([[0, 0, 10, 10]], [0.9], [[0, 0, 10, 5]])
    assert ref.box_iou(ref.det_xywh(f)[0], f["gt_boxes"][0], False) == 0.5 == ref.IOU_THRS[0]
    res = ref.run([f], 2)
    assert [_codes(res, t=t)[0] for t in range(10)] == [ref.TP] + [ref.FP] * 9


def test_04_equal_ious_the_later_gt_wins():
    """[0,0,10,10] (0.9) has IoU 0.5 with the upper half g0 = [0,0,10,5] and the lower half g1 = [0,5,10,5]; >= keeps the later, g1.
    So at t = 0.5 the exact copy of g0 (0.8) still finds g0 free (TP) and the exact copy of g1 (0.7) finds g1 taken (FP); from t = 0.55
    on the first detection matches nothing and both copies are TP."""
    res = ref.run([ref.one_frame([[0, 0, 10, 10], [0, 0, 10, 5], [0, 5, 10, 10]], [0.9, 0.8, 0.7], [[0, 0, 10, 5], [0, 5, 10, 5]])], 2)
    assert _codes(res, t=0) == [ref.TP, ref.TP, ref.FP]
    assert _codes(res, t=1) == [ref.FP, ref.TP, ref.TP]


def test_05_a_non_ignored_gt_above_the_threshold_beats_a_better_crowd():
    """The crowd g0 = [0,0,80,80] has IoU 1 with the detection [0,0,80,80] (union = the detection's area), the non-crowd g1 =
    [0,0,80,50] has 0.625.  Non-ignored first: g1 matches while t <= 0.625 and the walk stops at the ignored g0 -> TP at t = 0.5, 0.55,
    0.6.  From t = 0.65 on g1 is below, the crowd matches and the detection is ignored."""
    res = ref.run([ref.one_frame([[0, 0, 80, 80]], [0.9], [[0, 0, 80, 80], [0, 0, 80, 50]], iscrowd=[1, 0])], 2)
    assert [_codes(res, t=t)[0] for t in range(10)] == [ref.TP] * 3 + [ref.IGNORED] * 7
    assert res["npig"][0, ALL] == 1


def test_06_two_detections_on_one_crowd_region():
    """Both detections lie inside the crowd box (IoU = their own area / their own area = 1) and a crowd can be matched again: both are
    ignored, neither TP nor FP, and npig counts only the other ground truth, whose exact detection (scoring below them) gives tp =
    [0, 0, 1], fp = [0, 0, 0], pr = [0, 0, ONE] -> envelope ONE everywhere, AP = ONE."""
    res = ref.run([ref.one_frame([[210, 210, 250, 250], [220, 220, 260, 260], DET_M], [0.9, 0.8, 0.7], [[200, 200, 100, 100], GT_M],
                                 iscrowd=[1, 0])], 2)
    assert all(_codes(res, t=t) == [ref.IGNORED, ref.IGNORED, ref.TP] for t in range(10))
    assert res["npig"][0].tolist() == [1, 0, 1, 0] and (res["precision"][:, :, 0, ALL, 2] == ONE).all() and res["stats"][0] == AP_ONE
    assert res["stats"][8] == 1.0


def test_07_unmatched_detection_outside_the_area_range():
    """A 10 x 10 clutter box (area 100: small) scores above the exact detection of the medium ground truth.  'all': FP first, tp =
    [0, 1], fp = [1, 1] -> AP = 0.5 (case 2b).  'medium': the clutter is unmatched and outside the range -> ignored, AP = ONE.  'small':
    it is an FP there, but npig = 0, so the cells stay -1.  'large': ignored."""
    res = ref.run([ref.one_frame([[300, 300, 310, 310], DET_M], [0.95, 0.9], [GT_M])], 2)
    assert [_codes(res, a=a)[0] for a in range(4)] == [ref.FP, ref.FP, ref.IGNORED, ref.IGNORED]
    assert (res["precision"][:, :, 0, MEDIUM, 2] == ONE).all()
    assert res["stats"][0] == 0.5 and res["stats"][3] == -1 and res["stats"][4] == AP_ONE and res["stats"][5] == -1


def test_08_true_positive_at_rank_2():
    """Two clutter boxes outscore the exact detection.  M = 1 keeps rank 0 only: tp = [0] -> recall 0 / 1 = 0.  M = 10 keeps all three:
    tp = [0, 0, 1] -> recall 1."""
    res = ref.run([ref.one_frame([[300, 300, 360, 360], [400, 300, 460, 360], DET_M], [0.9, 0.8, 0.7], [GT_M])], 2)
    assert res["records"]["rank"].tolist() == [0, 1, 2]
    assert res["stats"][6] == 0.0 and res["stats"][7] == 1.0 and res["stats"][8] == 1.0


def test_09_the_101st_detection_is_dropped():
    """(a) 101 detections with distinct scores, the exact one scoring lowest: it has rank 100 and is cut -> 100 FPs, recall 0, AP 0.
    (b) equal scores are ranked by position: the exact detection at position 100 is cut (AP 0), at position 99 it is kept with rank 99:
    tp = [0]*99 + [1], fp = [1]*99 + [99] -> pr[-1] = 1 / (100 + eps) = 0.01, envelope 0.01 everywhere, recall 1."""
    clutter = [[300 + (i % 10) * 8, 300 + (i // 10) * 8, 340 + (i % 10) * 8, 340 + (i // 10) * 8] for i in range(100)]
    a = ref.run([ref.one_frame([DET_M] + clutter, [0.1] + [0.2 + 0.005 * i for i in range(100)], [GT_M])], 2)
    assert len(a["records"]["rank"]) == 100 and ref.TP not in _codes(a) and a["stats"][0] == 0.0 and a["stats"][8] == 0.0
    b = ref.run([ref.one_frame(clutter + [DET_M], [0.5] * 101, [GT_M])], 2)
    assert len(b["records"]["rank"]) == 100 and ref.TP not in _codes(b) and b["stats"][8] == 0.0
    c = ref.run([ref.one_frame(clutter[:99] + [DET_M] + clutter[99:], [0.5] * 101, [GT_M])], 2)
    assert _codes(c) == [ref.FP] * 99 + [ref.TP] and c["records"]["rank"].tolist() == list(range(100))
    assert 1.0 / (100.0 + 2.0 ** -52) == 0.01 and (c["precision"][0, :, 0, ALL, 2] == 0.01).all()
    assert c["stats"][8] == 1.0 and c["stats"][1] == float(np.mean(np.full(101, 0.01)))          # the mean of 101 cells, as np.mean sums them


def test_10_category_with_detections_and_no_gt():
    """Category 1 has a detection and no ground truth: npig = 0, its cells stay -1 and the means run over category 0 alone -> ONE."""
    res = ref.run([ref.one_frame([DET_M, [300, 300, 360, 360]], [0.9, 0.8], [GT_M], labels=[0, 1])], 3)
    assert res["npig"].tolist() == [[1, 0, 1, 0], [0, 0, 0, 0]]
    assert (res["precision"][:, :, 1] == -1).all() and (res["recall"][:, 1] == -1).all()
    assert len(res["records"]["label"]) == 2 and res["stats"][0] == AP_ONE and res["stats"][8] == 1.0


def test_package_stats_equal_the_restatement():
    from faster_rcnn_pytorch_amd import evaluation
    res = ref.run(ref.make_set(3, n_images=4, max_det=60, max_gt=8), 7)
    assert np.array_equal(evaluation.coco_stats(res["precision"], res["recall"], ref.IOU_THRS), res["stats"])
    assert evaluation.COCO_AREA_RANGES == tuple(tuple(float(v) for v in r) for r in ref.AREA_RNG)


# ------------------------------------------------------------------------------------------------------------ the kernel's form
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_pass_walk_equals_the_sorted_walk(seed):
    frames = ref.make_set(seed, n_images=8, max_det=90, max_gt=16)
    a, b = ref.evaluate(frames, 7), ref.evaluate(frames, 7, img_fn=ref.evaluate_img_two_pass)
    assert a.keys() == b.keys() and len(a) > 20
    for key in a:
        for field in ("dtm", "dtIg", "gtIg"):
            assert np.array_equal(a[key][field], b[key][field]), (key, field)
    ra = ref.records(a, 10)
    codes = set(np.unique((ra["flags"][:, :, None] >> (2 * np.arange(10, dtype=np.uint32))) & 3))
    assert codes == {ref.TP, ref.FP, ref.IGNORED}


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_declared_exported_and_bound(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    for sym in ("frcnn_coco_eval_update", "frcnn_coco_eval_accumulate"):
        assert re.search(r"\b%s\s*\(" % sym, txt), sym
        assert re.search(r" T %s\b" % sym, out), sym
        assert sym in L.SIGNATURES
    assert "FRCNN_OP_COCO_EVAL = 13" in txt and L.OP_COCO_EVAL == 13
    assert (L.EVAL_TP, L.EVAL_FP, L.EVAL_IGNORED) == (ref.TP, ref.FP, ref.IGNORED)
    assert L.lib.frcnn_abi_version() == L.ABI_VERSION == 7


P = 0x1000          # a non-NULL pointer that is never dereferenced: every refusal below happens before a launch
U_NAMES = ("boxes", "labels", "scores", "count", "gtb", "gta", "gtl", "gtc", "ngt", "frame", "thr", "npig", "rs", "rl", "ri", "rr", "rf", "cursor",
           "err", "ws")


def _update(L, T=10, C=91, D=300, G=64, max_det=100, cap=1000, null=(), ws_bytes=1 << 30):
    a = {k: (None if k in null else P) for k in U_NAMES}
    return L.lib.frcnn_coco_eval_update(a["boxes"], a["labels"], a["scores"], a["count"], D, a["gtb"], a["gta"], a["gtl"], a["gtc"], a["ngt"], G,
                                        a["frame"], a["thr"], T, C, max_det, a["npig"], a["rs"], a["rl"], a["ri"], a["rr"], a["rf"], cap,
                                        a["cursor"], a["err"], a["ws"], ws_bytes, None)


def _acc(L, T=10, C=91, R=101, cap=1000, md=(1, 10, 100), null=(), ws_bytes=1 << 30):
    a = {k: (None if k in null else P) for k in ("lab", "rank", "fl", "n", "npig", "rthr", "prec", "rec", "ws")}
    return L.lib.frcnn_coco_eval_accumulate(a["lab"], a["rank"], a["fl"], a["n"], cap, a["npig"], a["rthr"], R, T, C, md[0], md[1], md[2], a["prec"],
                                            a["rec"], a["ws"], ws_bytes, None)


def test_update_refuses_null_pointers(L):
    for k in U_NAMES:
        assert _update(L, null=(k,)) == -1 and b"coco_eval_update" in L.lib.frcnn_last_error(), k


def test_accumulate_refuses_null_pointers(L):
    for k in ("lab", "rank", "fl", "n", "npig", "rthr", "prec", "rec", "ws"):
        assert _acc(L, null=(k,)) == -1 and b"coco_eval_accumulate" in L.lib.frcnn_last_error(), k


def test_limits_refused(L):
    assert _update(L, T=0) == -2 and _update(L, T=17) == -2 and _acc(L, T=0) == -2 and _acc(L, T=17) == -2
    assert _update(L, C=1) == -2 and _update(L, C=257) == -2 and _acc(L, C=1) == -2 and _acc(L, C=257) == -2
    assert _update(L, G=0) == -2 and _update(L, G=1025) == -2 and b"coco_eval_update" in L.lib.frcnn_last_error()
    assert _update(L, D=0) == -2 and _update(L, C=21, D=20 * 2048 + 1) == -2
    assert _update(L, max_det=0) == -2 and _update(L, max_det=101) == -2
    assert _acc(L, R=0) == -2 and _acc(L, R=257) == -2
    assert _update(L, cap=0) == -1 and _acc(L, cap=0) == -1 and _acc(L, md=(0, 10, 100)) == -1


def test_small_workspace_refused(L):
    assert _update(L, ws_bytes=16) == -3 and _acc(L, ws_bytes=256 + 32 * 1000 - 1) == -3


def test_workspace_bytes_zero_outside_the_limits(L):
    assert L.workspace_bytes(L.OP_COCO_EVAL, 9000, 128) >= 9000 * 8
    assert L.workspace_bytes(L.OP_COCO_EVAL, 255 * 2048, 1024) > 0
    assert L.workspace_bytes(L.OP_COCO_EVAL, 255 * 2048 + 1, 64) == 0
    assert L.workspace_bytes(L.OP_COCO_EVAL, 300, 1025) == 0
    assert L.workspace_bytes(L.OP_COCO_EVAL, 0, 64) == 0 and L.workspace_bytes(L.OP_COCO_EVAL, 300, 0) == 0


def test_evaluator_refuses_bad_configuration_without_a_device(L):
    from faster_rcnn_pytorch_amd import evaluation
    for kw in (dict(iou_thresholds=()), dict(iou_thresholds=[0.5] * 17), dict(gt_capacity=1025), dict(record_capacity=0),
               dict(max_dets=(1, 10)), dict(max_dets=(10, 1, 100)), dict(max_dets=(1, 10, 101))):
        with pytest.raises(ValueError):
            evaluation.CocoDetectionEvaluator(91, **kw)
    with pytest.raises(ValueError):
        evaluation.CocoDetectionEvaluator(257)
    with pytest.raises(ValueError):
        evaluation.CocoGroundTruth(1025, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.CocoDetectionEvaluator(91, device="cpu")
    gt = evaluation.CocoGroundTruth(2, "cpu").set([[1, 2, 3, 4], [5, 6, 7, 8], [0, 0, 1, 1]], [0, 1, 2], iscrowd=[0, 1, 0], orig_wh=(640, 480),
                                                  image_id=7)
    assert gt.n.tolist() == [3] and gt.frame.tolist() == [640, 480, 7]                  # n keeps the true count on overflow
    assert gt.boxes.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]] and gt.area.tolist() == [12, 56]
    assert gt.labels.tolist() == [0, 1] and gt.iscrowd.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------ frame-buffer layout
# what eval_update_kernel and coco_update_kernel read: a 16-byte head (w, h, image_id, n) and then the fields, each [capacity, width]
LAYOUTS = {"GroundTruth": (("boxes", np.float32, 4), ("labels", np.int32, 1), ("difficult", np.uint8, 1)),
           "CocoGroundTruth": (("boxes", np.float64, 4), ("area", np.float64, 1), ("labels", np.int32, 1), ("iscrowd", np.uint8, 1))}


@pytest.mark.parametrize("c", [1, 3, 64])
@pytest.mark.parametrize("cls", sorted(LAYOUTS))
def test_frame_buffer_bytes_are_head_then_fields_in_table_order(L, cls, c):
    """The raw bytes of the one allocation against a hand-packed expectation, for 0, c and c + 2 rows from host arrays: field k starts
    at 16 + sum(itemsize * width of the fields before it) * c, n keeps the true count on overflow, the rows past min(n, c) stay as
    they were (zero)."""
    from faster_rcnn_pytorch_amd import evaluation
    rng = np.random.RandomState(c)
    for n in (0, c, c + 2):
        cols = {"boxes": rng.randint(1, 4000, (n, 4)) / 8.0, "area": rng.randint(1, 10 ** 6, n) / 4.0, "labels": rng.randint(0, 90, n),
                "difficult": rng.randint(0, 2, n), "iscrowd": rng.randint(0, 2, n)}
        gt = getattr(evaluation, cls)(c, "cpu")
        if cls == "GroundTruth":
            gt.set(cols["boxes"], cols["labels"], cols["difficult"], (641 + n, 479), 70000 + n)
        else:
            gt.set(cols["boxes"], cols["labels"], cols["iscrowd"], cols["area"], orig_wh=(641 + n, 479), image_id=70000 + n)
        m = min(n, c)
        want = [np.array([641 + n, 479, 70000 + n, n], np.int32).view(np.uint8)]
        for name, dt, w in LAYOUTS[cls]:
            field = np.zeros((c, w), dt)
            field[:m] = np.asarray(cols[name]).reshape(n, w)[:m]
            want.append(field.view(np.uint8).reshape(-1))
            view = getattr(gt, name)
            assert tuple(view.shape) == ((c, w) if w > 1 else (c,)) and np.array_equal(view.numpy().reshape(c, w), field), name
        want = np.concatenate(want)
        raw = np.frombuffer(bytes(gt.frame.untyped_storage()), np.uint8)
        assert raw.size == 16 + sum(np.dtype(dt).itemsize * w for _, dt, w in LAYOUTS[cls]) * c
        assert np.array_equal(raw, want)
        assert gt.n.tolist() == [n] and gt.frame.tolist() == [641 + n, 479, 70000 + n] and gt.capacity == c
    if cls == "CocoGroundTruth":                                 # area = None is w * h of the box
        gt = evaluation.CocoGroundTruth(c, "cpu").set(cols["boxes"], cols["labels"], orig_wh=(8, 8))
        assert np.array_equal(gt.area.numpy(), (cols["boxes"][:, 2] * cols["boxes"][:, 3])[:c]) and gt.iscrowd.tolist() == [0] * c
