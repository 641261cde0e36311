"""CPU-only checks of the pooled COCO protocol (useCats = 0; csrc/coco_eval_pooled.hip, evaluation.CocoDetectionEvaluator(use_cats=False),
evaluation.ProposalEvaluator): hand-derived known answers on the restatement the GPU tests compare against
(tests/coco_eval_pooled_ref.py), its vectorised arg-max form against the literal sorted walk flag for flag, the one pin there is -- on
single-label sets the pooled restatement equals the per-category one of tests/coco_eval_ref.py --, and the new entry point declared,
exported, bound and refusing bad arguments without a device.

ONE = 1 / (1 + 2^-52): see tests/test_coco_eval_host.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import coco_eval_pooled_ref as pref
import coco_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1.0 / (1.0 + 2.0 ** -52)
ALL, SMALL, MEDIUM, LARGE = 0, 1, 2, 3
TP, FP, IG = ref.TP, ref.FP, ref.IGNORED
GT_M = [100, 100, 50, 50]                    # a medium ground truth (area 2500) and its exact detection
DET_M = [100, 100, 150, 150]
LITERAL = dict(img_fn=ref.evaluate_img, literal_iou=True)          # the known answers go through the literal walk and box_iou


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _codes(res, r, a=ALL):
    """The 2-bit codes of record r (in record order) for one area range, one per threshold."""
    return ((int(res["records"]["flags"][r, a]) >> (2 * np.arange(10))) & 3).tolist()


def _both_forms(frames, **kw):
    """run() through the literal walk, checked against the arg-max form before it is returned."""
    a, b = pref.run(frames, **dict(LITERAL, **kw)), pref.run(frames, **kw)
    for k in ("precision", "recall", "npig", "stats"):
        assert np.array_equal(a[k], b[k]), k
    for k in a["records"]:
        assert np.array_equal(a["records"][k], b["records"][k]), k
    return a


# ------------------------------------------------------------------------------------------------------------ known answers
def test_01_detection_on_a_ground_truth_of_another_label_is_fp_per_category_and_tp_pooled():
    """One detection of label 0 exactly on the one ground truth, which has label 1.  useCats = 1: category 0 has a detection and no
    ground truth -- unmatched, area 2500 inside 'all' -> FP at every threshold, npig = 0 -> its cells stay -1; category 1 has a ground
    truth and no detection -> recall 0, precision 0.  Pooled: one list each, IoU = 1 >= every threshold -> TP everywhere; tp = [1],
    fp = [0] -> rc = [1], pr = [ONE]; 'small' and 'large' have npig = 0."""
    f = ref.one_frame([DET_M], [0.9], [GT_M], labels=[0], gt_labels=[1])
    cats = ref.run([f], 3)
    assert ((cats["records"]["flags"][0, ALL] >> (2 * np.arange(10))) & 3).tolist() == [FP] * 10
    assert cats["npig"].tolist() == [[0, 0, 0, 0], [1, 0, 1, 0]] and cats["stats"][0] == 0.0 and cats["stats"][8] == 0.0
    res = _both_forms([f])
    assert _codes(res, 0) == [TP] * 10 and _codes(res, 0, MEDIUM) == [TP] * 10
    assert res["records"]["label"].tolist() == [0] and res["records"]["rank"].tolist() == [0]
    assert res["npig"].tolist() == [[1, 0, 1, 0]] and res["precision"].shape == (10, 101, 1, 4, 3)
    assert (res["precision"][:, :, 0, [ALL, MEDIUM], :] == ONE).all() and (res["recall"][:, 0, [ALL, MEDIUM], :] == 1.0).all()
    assert (res["precision"][:, :, 0, [SMALL, LARGE], :] == -1).all()
    assert res["stats"][[6, 7, 8, 10]].tolist() == [1, 1, 1, 1] and res["stats"][[3, 5, 9, 11]].tolist() == [-1] * 4


@pytest.mark.parametrize("swap", [False, True])
def test_02_equal_scores_go_label_ascending_whatever_the_positions(swap):
    """A = the ground truth's exact box with label 1, B = its upper half (IoU exactly 1/2) with label 0, both score 0.5.  The pooled
    list is [B, A] wherever they stand in the input, and the stable sort keeps it: rank 0 = B.  At t = 0.5 B takes the ground truth
    (0.5 >= 0.5) -> TP, and A finds it taken -> FP; at t >= 0.55 B is below t -> FP and A -> TP.  (Ordered by position with A first, A
    would be TP at every threshold.)"""
    A, B = DET_M, [100, 100, 150, 125]
    dets, labels = ([B, A], [0, 1]) if swap else ([A, B], [1, 0])
    res = _both_forms([ref.one_frame(dets, [0.5, 0.5], [GT_M], labels=labels, gt_labels=[0])])
    p = pref._prepare(ref.one_frame(dets, [0.5, 0.5], [GT_M], labels=labels, gt_labels=[0]), 1000)
    assert p["pos"].tolist() == ([0, 1] if swap else [1, 0])                 # rank -> original position: B first
    assert p["ious"][:, 0].tolist() == [0.5, 1.0]
    assert res["records"]["rank"].tolist() == [0, 1]
    assert _codes(res, 0) == [TP] + [FP] * 9 and _codes(res, 1) == [FP] + [TP] * 9


def test_03_of_two_equal_ious_the_later_ground_truth_in_pooled_order_wins():
    """gA = the upper half [0,0,10,5] of D = [0,0,10,10] with label 1 at position 0, gB = the lower half [0,5,10,5] with label 0 at
    position 1: IoU(D, gA) = IoU(D, gB) = 50 / 100 = 1/2.  Pooled order of the ground truths is [gB, gA]; `>=` keeps the later of equal
    IoUs, so at t = 0.5 D (score 0.9) takes gA.  E = gA's exact box (score 0.8) has IoU 1 with gA and 0 with gB: gA is taken -> FP at
    t = 0.5.  (In original order the later one is gB, and E would be TP.)  At t >= 0.55 D matches nothing -> FP, E -> TP."""
    f = ref.one_frame([[0, 0, 10, 10], [0, 0, 10, 5]], [0.9, 0.8], [[0, 0, 10, 5], [0, 5, 10, 5]], labels=[0, 0], gt_labels=[1, 0])
    p = pref._prepare(f, 1000)
    assert p["gpos"].tolist() == [1, 0] and p["ious"].tolist() == [[0.5, 0.5], [0.0, 1.0]]
    res = _both_forms([f])
    assert _codes(res, 0) == [TP] + [FP] * 9 and _codes(res, 1) == [FP] + [TP] * 9
    original = ref.run([dict(f, gt_labels=np.zeros(2, np.int32))], 2)          # one label: pooled order = original order
    assert ((int(original["records"]["flags"][1, ALL]) >> (2 * np.arange(10))) & 3).tolist() == [TP] * 10


def test_04_a_crowd_ground_truth_is_matched_twice():
    """A crowd ground truth [200,200,100,100] of label 1 and two detections of label 0 inside it: IoU with a crowd = intersection /
    detection area = 1 for both.  A crowd is ignored in every range, so both go to the second pass, a matched crowd is not skipped, and
    both detections are matched to an ignored ground truth -> IGNORED at every (range, threshold).  npig = 0 everywhere: every cell and
    every stat stays -1."""
    f = ref.one_frame([[210, 210, 250, 250], [220, 220, 260, 260]], [0.9, 0.8], [[200, 200, 100, 100]], iscrowd=[1], labels=[0, 0], gt_labels=[1])
    res = _both_forms([f])
    for r in range(2):
        for a in range(4):
            assert _codes(res, r, a) == [IG] * 10
    assert (res["npig"] == 0).all() and (res["precision"] == -1).all() and (res["stats"] == -1).all()


def test_05_all_ground_truths_ignored():
    """Two crowd ground truths (labels 0 and 2); X lies inside the first (IoU 1 -> matched, ignored), Y = [300,300,360,360] touches
    neither -> unmatched; its area 3600 lies inside 'all' and 'medium' -> FP there, outside 'small' and 'large' -> IGNORED there.  No
    ground truth counts: npig = 0, every precision / recall cell and every stat is -1."""
    f = ref.one_frame([[110, 110, 140, 140], [300, 300, 360, 360]], [0.9, 0.8], [GT_M, [10, 10, 40, 40]], iscrowd=[1, 1], labels=[1, 1],
                      gt_labels=[0, 2])
    res = _both_forms([f])
    assert all(_codes(res, 0, a) == [IG] * 10 for a in range(4))
    assert _codes(res, 1, ALL) == [FP] * 10 and _codes(res, 1, MEDIUM) == [FP] * 10
    assert _codes(res, 1, SMALL) == [IG] * 10 and _codes(res, 1, LARGE) == [IG] * 10
    assert (res["npig"] == 0).all() and (res["precision"] == -1).all() and (res["recall"] == -1).all() and (res["stats"] == -1).all()


def _frame_1003():
    """1003 detections with distinct descending scores (2000 - i) / 2048 and labels i % 3 -- so the pooled order is NOT the input order,
    and the score sort has to undo it --; those at ranks 99, 299, 999 and 1000 are the exact boxes of four medium ground truths, the
    rest is clutter far from them."""
    gts = [[16 + 64 * j, 16, 48, 48] for j in range(4)]
    dets = [[300 + (i % 10) * 8, 300 + (i // 10 % 16) * 8, 340 + (i % 10) * 8, 340 + (i // 10 % 16) * 8] for i in range(1003)]
    for j, r in enumerate((99, 299, 999, 1000)):
        x, y, w, h = gts[j]
        dets[r] = [x, y, x + w, y + h]
    return ref.one_frame(dets, [(2000 - i) / 2048.0 for i in range(1003)], gts, labels=[i % 3 for i in range(1003)], gt_labels=[2, 1, 0, 1])


def test_06_1003_detections_are_cut_at_100_300_1000():
    """maxDets[-1] = 1000 keeps ranks 0 .. 999: 1000 records, the match at rank 1000 is gone.  Four ground truths: the top 100 hold one
    match (rank 99) -> AR@100 = 1/4, the top 300 two -> AR@300 = 2/4, the top 1000 three -> AR@1000 = 3/4, at every threshold (IoU 1),
    so the means over the thresholds are those values exactly."""
    res = _both_forms([_frame_1003()])
    assert len(res["records"]["rank"]) == 1000 and res["records"]["rank"].tolist() == list(range(1000))
    assert res["records"]["score"].tolist() == [(2000 - i) / 2048.0 for i in range(1000)]
    tp_ranks = [r for r in range(1000) if _codes(res, r)[0] == TP]
    assert tp_ranks == [99, 299, 999] and res["npig"].tolist() == [[4, 0, 4, 0]]
    assert (res["recall"][:, 0, ALL, :] == np.array([0.25, 0.5, 0.75])).all()
    assert res["stats"][[6, 7, 8]].tolist() == [0.25, 0.5, 0.75] and res["stats"][10] == 0.75
    s = pref.proposal_summary(res)
    assert s["ar"].tolist() == [0.25, 0.5, 0.75] and s["ar_medium"] == 0.75 and s["ar_small"] == -1 and s["npig"].tolist() == [4, 0, 4, 0]


def test_07_an_empty_frame_contributes_nothing():
    """No detection and no ground truth: evaluate skips the frame; nothing is evaluated, every cell is -1.  Next to a real frame it
    changes nothing."""
    empty = ref.one_frame(np.zeros((0, 4)), [], np.zeros((0, 4)), image_id=4)
    res = _both_forms([empty])
    assert len(res["ev"]) == 0 and len(res["records"]["label"]) == 0 and (res["npig"] == 0).all() and (res["precision"] == -1).all()
    one = ref.one_frame([DET_M], [0.9], [GT_M], labels=[0], gt_labels=[1])
    a, b = _both_forms([one]), _both_forms([empty, one])
    assert np.array_equal(a["precision"], b["precision"]) and np.array_equal(a["stats"], b["stats"])


# ------------------------------------------------------------------------------------------------------------ the kernel's form
SMALL_SHAPES = [(40, 12), (0, 5), (7, 0), (90, 30), (25, 25), (60, 3), (1, 1), (33, 17)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_argmax_form_equals_the_literal_sorted_walk(seed):
    """The vectorised two-pass arg-max (with the vectorised IoU) against evaluateImg's literal walk over the sorted ground truths (with
    box_iou pair by pair), flag for flag, on frames whose integer grid makes exact IoU ties and exact threshold hits common."""
    frames = pref.make_set(seed, SMALL_SHAPES, num_labels=4)
    kinds = pref.kinds(frames)
    print(kinds)
    for k, v in kinds.items():
        assert v >= 1, k
    a = pref.evaluate(frames, max_det=50, img_fn=ref.evaluate_img, literal_iou=True)
    b = pref.evaluate(frames, max_det=50, img_fn=pref.evaluate_img_argmax)
    c = pref.evaluate(frames, max_det=50, img_fn=ref.evaluate_img_two_pass)
    assert a.keys() == b.keys() == c.keys() and len(a) == 4 * (len(SMALL_SHAPES))
    for key in a:
        for field in ("score", "pos", "dtm", "dtIg", "gtIg"):
            assert np.array_equal(a[key][field], b[key][field]) and np.array_equal(a[key][field], c[key][field]), (key, field)
    codes = set(np.unique((ref.records(a, 10)["flags"][:, :, None] >> (2 * np.arange(10, dtype=np.uint32))) & 3))
    assert codes == {TP, FP, IG}


# ------------------------------------------------------------------------------------------------------------ the pin
@pytest.mark.parametrize("seed", [3, 4])
def test_single_label_sets_equal_the_per_category_restatement(seed):
    """With one label the pooled lists ARE the category's lists, so at max_dets <= 100 the pooled restatement must equal
    coco_eval_ref.run bit for bit.  The only pin there is: pycocotools itself is not available."""
    frames = ref.make_set(seed, n_images=10, num_classes=3, max_det=150, max_gt=16)
    assert all((f["labels"] == 0).all() and (f["gt_labels"] == 0).all() for f in frames) and max(len(f["labels"]) for f in frames) > 100
    cats = ref.run(frames, 2)
    for kw in (LITERAL, {}):
        pooled = pref.run(frames, max_dets=ref.MAX_DETS, **kw)
        for k in ("precision", "recall", "npig", "stats"):
            assert pooled[k].shape == cats[k].shape and np.array_equal(pooled[k], cats[k]), k
        for k in cats["records"]:
            assert np.array_equal(pooled["records"][k], cats["records"][k]), k
    assert cats["stats"][0] > 0 and len(cats["records"]["label"]) > 100


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_symbol_declared_exported_and_bound(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    sym = "frcnn_coco_eval_update_pooled"
    assert re.search(r"\b%s\s*\(" % sym, txt) and re.search(r" T %s\b" % sym, out) and sym in L.SIGNATURES
    assert L.SIGNATURES[sym] == L.SIGNATURES["frcnn_coco_eval_update"]                      # the same arguments
    assert "FRCNN_OP_COCO_EVAL_POOLED = 15" in txt and L.OP_COCO_EVAL_POOLED == 15
    assert L.lib.frcnn_abi_version() == L.ABI_VERSION == 7                                  # entry points were only added


P = 0x1000          # a non-NULL pointer that is never dereferenced: every refusal below happens before a launch
U_NAMES = ("boxes", "labels", "scores", "count", "gtb", "gta", "gtl", "gtc", "ngt", "frame", "thr", "npig", "rs", "rl", "ri", "rr", "rf", "cursor",
           "err", "ws")


def _update(L, T=10, C=91, D=1000, G=64, max_det=1000, cap=1000, null=(), ws_bytes=1 << 30, ptr=None):
    a = {k: (None if k in null else P) for k in U_NAMES}
    a.update(ptr or {})
    return L.lib.frcnn_coco_eval_update_pooled(a["boxes"], a["labels"], a["scores"], a["count"], D, a["gtb"], a["gta"], a["gtl"], a["gtc"], a["ngt"],
                                               G, a["frame"], a["thr"], T, C, max_det, a["npig"], a["rs"], a["rl"], a["ri"], a["rr"], a["rf"], cap,
                                               a["cursor"], a["err"], a["ws"], ws_bytes, None)


def test_update_refuses_null_pointers(L):
    for k in U_NAMES:
        assert _update(L, null=(k,)) == -1 and b"coco_eval_update_pooled" in L.lib.frcnn_last_error(), k


def test_limits_refused(L):
    assert _update(L, T=0) == -2 and _update(L, T=17) == -2 and _update(L, C=1) == -2 and _update(L, C=257) == -2
    assert _update(L, G=0) == -2 and _update(L, G=1025) == -2 and b"coco_eval_update_pooled" in L.lib.frcnn_last_error()
    assert _update(L, D=0) == -2 and _update(L, C=21, D=20 * 2048 + 1) == -2 and _update(L, C=2, D=2049) == -2
    assert _update(L, max_det=0) == -2 and _update(L, max_det=2049) == -2
    assert _update(L, cap=0) == -1


def test_misalignment_refused(L):
    assert _update(L, ptr={"boxes": P + 8}) == -1 and b"aligned" in L.lib.frcnn_last_error()
    assert _update(L, ptr={"gtb": P + 4}) == -1 and _update(L, ptr={"gta": P + 4}) == -1


def test_small_workspace_refused(L):
    need = L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 1000, 64)
    assert _update(L, ws_bytes=need - 1) == -3 and b"workspace" in L.lib.frcnn_last_error() and _update(L, ws_bytes=16) == -3


def test_workspace_bytes_zero_outside_the_limits(L):
    small, big = L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 300, 128), L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 255 * 2048, 1024)
    fixed = 5 * 2048 * 8 + 2048 + 1024 * 4                       # the ranked boxes, their area bits, the ground truths' pooled order
    assert small >= 300 * 8 + fixed and big >= 255 * 2048 * 8 + fixed
    assert L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 255 * 2048 + 1, 64) == 0 and L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 300, 1025) == 0
    assert L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 0, 64) == 0 and L.workspace_bytes(L.OP_COCO_EVAL_POOLED, 300, 0) == 0


def test_evaluators_refuse_bad_configuration_without_a_device(L):
    from faster_rcnn_pytorch_amd import evaluation
    for kw in (dict(max_dets=(1, 10)), dict(max_dets=(300, 100, 1000)), dict(max_dets=(100, 300, 2049)), dict(max_dets=(0, 300, 1000)),
               dict(iou_thresholds=[0.5] * 17), dict(gt_capacity=1025)):
        with pytest.raises(ValueError):
            evaluation.CocoDetectionEvaluator(91, use_cats=False, **kw)
        with pytest.raises(ValueError):
            evaluation.ProposalEvaluator(**kw)
    with pytest.raises(ValueError):
        evaluation.CocoDetectionEvaluator(91, max_dets=(100, 300, 1000))                    # per category the cut stays at 100
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.CocoDetectionEvaluator(91, use_cats=False, max_dets=(100, 300, 2048), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.ProposalEvaluator(device="cpu")


def test_the_mode_is_no_longer_listed_as_not_built():
    for rel in ("README.md", "DESIGN.md", "docs/PARITY.md", "faster_rcnn_pytorch_amd/csrc/coco_eval.hip", "faster_rcnn_pytorch_amd/evaluation.py"):
        for line in open(os.path.join(ROOT, rel)).read().splitlines():
            assert not ("not built" in line.lower() and "usecats = 0" in line.lower() and "coco_eval_pooled" not in line), (rel, line)
