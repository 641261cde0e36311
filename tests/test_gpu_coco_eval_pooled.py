"""The pooled COCO protocol on the device (useCats = 0: csrc/coco_eval_pooled.hip, evaluation.CocoDetectionEvaluator(use_cats=False),
evaluation.ProposalEvaluator, FRCNN.proposals / detect(want_proposals=True), DetectGraph(proposal_evaluator=)) against its restatement
(tests/coco_eval_pooled_ref.py; known answers in tests/test_coco_eval_pooled_host.py).

Everything is compared with np.array_equal: the records in the defined order (scores, ranks, the flag word of every area range), npig,
precision, recall and the 12 stats.  Every device operation is an IEEE float64 + - * / in the order of the restatement, so there is no
tolerance to choose.  The evaluators, their ground-truth buffers and workspaces are built inside tests/guarded.py's context, once with
0xFF and once with 0x00 in every guard, fresh output and scratch byte: nothing is written outside a buffer, the workspace may hold
anything, and the two runs give the same bytes.  Rows at and above a frame's counts hold NaN boxes and wild labels."""
import numpy as np
import pytest
import torch

import coco_eval_pooled_ref as pref
import coco_eval_ref as ref
import test_gpu_coco_eval as tc
from guarded import run_both

pytestmark = pytest.mark.gpu
DEV = tc.DEV
NC = 6                                                           # labels 0 .. 4


def _mods():
    from faster_rcnn_pytorch_amd import evaluation, ops
    return evaluation, ops


def _feed(ev, gt, f, det_capacity=None, count=None, place=None):
    """gt.set, NaN boxes and wild labels behind the live ground truths, then one update on the frame's (placed) detections."""
    _, ops = _mods()
    tc._set_gt(gt, f)
    n = len(f["gt_labels"])
    if n < gt.capacity:
        gt.boxes[n:] = float("nan")
        gt.area[n:] = float("nan")
        gt.labels[n:] = 10 ** 6
        gt.iscrowd[n:] = 1
    d = tc._dets(f, det_capacity, count)
    if place is not None:
        d = ops.Detections(*[None if t is None else place(t) for t in d])
    ev.update(d, gt)


def _store(ev):
    """The defined part of a pooled evaluator's buffers.  A frame's slots are reserved by ONE atomic add and filled in rank order, so
    the raw columns up to the cursor are defined as they stand."""
    n = min(int(ev.cursor.item()), ev.record_capacity)
    d = {"rec." + k: t[:n] for k, t in zip(ev._keys(), ev._records())}
    d.update(npig=ev.npig, cursor=ev.cursor, error=ev.error)
    if ev.image_capacity:
        m = min(int(ev.led_count.item()), ev.image_capacity)
        d.update(led_image=ev.led_image[:m], led_range=ev.led_range[:m], led_delta=ev.led_delta[:m], led_count=ev.led_count)
    return d


def _guarded(frames, num_classes=NC, gt_capacity=128, det_capacity=None, counts=None, summarize=True, **kw):
    """One pooled evaluator over `frames` under both prefills; returns (records_sorted, summarize()) of the 0xFF run, or its raw store
    when summarize is off (error frames)."""
    evaluation, _ = _mods()
    kw.setdefault("record_capacity", 1 << 13)
    kw.setdefault("max_dets", pref.MAX_DETS)

    def case(g):
        ev = evaluation.CocoDetectionEvaluator(num_classes, gt_capacity=gt_capacity, device=DEV, use_cats=False, **kw)
        gt = evaluation.CocoGroundTruth(gt_capacity, DEV)
        for i, f in enumerate(frames):
            _feed(ev, gt, f, det_capacity, None if counts is None else counts[i], g.place)
        out = _store(ev)
        if summarize:
            res = ev.summarize()
            out.update({"summary." + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in res.items() if isinstance(v, np.ndarray)})
            out.update(_records=ev.records_sorted(), _res=res)
        return out
    a, _ = run_both(case, derived=lambda k: k.startswith("summary."))
    return a


def _check(frames, r, **kw):
    out = _guarded(frames, **kw)
    tc._same_records(out["_records"], r["records"])
    assert (out["_records"]["label"] == 0).all()
    tc._same_result(out["_res"], r)
    assert out["_res"]["npig"].shape == (1, 4) and out["_res"]["precision"].shape[2] == 1
    return out


def _three_codes(r, T):
    return set(np.unique((r["records"]["flags"][:, :, None] >> (2 * np.arange(T, dtype=np.uint32))) & 3)) == {ref.TP, ref.FP, ref.IGNORED}


# ------------------------------------------------------------------------------------------------------------ 1. the ranking's seams
MAX_DETS, D_CAP = (10, 50, 300), 700


@pytest.mark.parametrize("n", [0, 1, MAX_DETS[-1] - 1, MAX_DETS[-1], MAX_DETS[-1] + 1, D_CAP])
def test_live_count_around_the_cut(n):
    """A live count of 0, 1, max_det - 1, max_det, max_det + 1 and the capacity (the last two: the radix select) in a buffer of 700
    rows; 12 score values, so runs of equal scores straddle every cut and the order inside them is (label, position)."""
    frames = [pref.grid_frame(40 + n, n, 20, NC - 1, image_id=7), pref.grid_frame(41 + n, 33, 9, NC - 1, image_id=2)]
    r = pref.run(frames, max_dets=MAX_DETS)
    kept = min(n, MAX_DETS[-1])
    assert len(r["records"]["label"]) == kept + 33
    if n > MAX_DETS[-1]:                                         # a run of equal scores across the cut: some of it is kept, some is not
        sc = np.sort(frames[0]["scores"])[::-1]
        assert sc[MAX_DETS[-1] - 1] == sc[MAX_DETS[-1]]
    if n >= 300:
        assert _three_codes(r, 10) and pref.kinds(frames)["score_ties_across_labels"] >= 1
    _check(frames, r, det_capacity=D_CAP, max_dets=MAX_DETS, gt_capacity=32)


def test_2048_ranked_detections_selected_from_2600():
    """nd = max_det = 2048 (the LDS sort at its full width) selected from 2600 live rows, few ground truths, two thresholds."""
    frames = [pref.grid_frame(5, 2600, 6, NC - 1, image_id=1, n_scores=40)]
    r = pref.run(frames, thrs=(0.5, 0.75), max_dets=(100, 1000, 2048))
    assert len(r["records"]["label"]) == 2048 and r["stats"][8] > 0
    _check(frames, r, det_capacity=2600, max_dets=(100, 1000, 2048), gt_capacity=8, iou_thresholds=(0.5, 0.75))


# ------------------------------------------------------------------------------------------------------------ 2. the matching's seams
@pytest.mark.parametrize("G", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_ground_truth_count_at_wave_and_block_boundaries(G):
    """G around one wave, one pass of the 256 threads and the capacity; 40 detections, the ten default thresholds (40 chains)."""
    frames = [pref.grid_frame(300 + G, 40, G, NC - 1, image_id=3)]
    r = pref.run(frames)
    if G >= 63:
        k = pref.kinds(frames)
        assert k["iou_ties"] >= 1 and k["best_gt_has_another_label"] >= 1 and int(r["npig"][0, 0]) > 0
    _check(frames, r, gt_capacity=max(G, 1), record_capacity=256)


@pytest.mark.parametrize("T", [1, 10, 16])
def test_number_of_chains(T):
    """T = 1, 10, 16: 4, 40 and 64 workgroups ORing into the records' four flag words."""
    thr = {1: (0.5,), 10: ref.IOU_THRS, 16: np.linspace(0.05, 0.8, 16)}[T]
    frames = pref.make_set(7, [(120, 65), (0, 12), (30, 0), (300, 40)], NC - 1)
    r = pref.run(frames, thrs=thr)
    assert _three_codes(r, T)
    _check(frames, r, iou_thresholds=thr)


def test_1000_detections_1024_ground_truths():
    """The proposal evaluator's full shape: nd = 1000 ranked of 1000, G = 1024 (four ground truths per thread), two thresholds."""
    frames = [pref.grid_frame(11, 1000, 1024, NC - 1, image_id=9, n_scores=200)]
    r = pref.run(frames, thrs=(0.5, 0.75))
    k = pref.kinds(frames, thrs=np.array([0.5, 0.75]))
    assert k["iou_ties"] >= 1 and k["iou_equal_threshold"] >= 1 and _three_codes(r, 2) and len(r["records"]["label"]) == 1000
    _check(frames, r, gt_capacity=1024, iou_thresholds=(0.5, 0.75))


def test_known_answers_through_the_device():
    """The hand-derived cases of tests/test_coco_eval_pooled_host.py, whose expected flags are asserted there on the restatement."""
    import test_coco_eval_pooled_host as th
    A, B = th.DET_M, [100, 100, 150, 125]
    f = ref.one_frame
    cases = [f([th.DET_M], [0.9], [th.GT_M], labels=[0], gt_labels=[1]),
             f([A, B], [0.5, 0.5], [th.GT_M], labels=[1, 0], gt_labels=[0]),
             f([[0, 0, 10, 10], [0, 0, 10, 5]], [0.9, 0.8], [[0, 0, 10, 5], [0, 5, 10, 5]], labels=[0, 0], gt_labels=[1, 0]),
             f([[210, 210, 250, 250], [220, 220, 260, 260]], [0.9, 0.8], [[200, 200, 100, 100]], iscrowd=[1], labels=[0, 0], gt_labels=[1]),
             f([[110, 110, 140, 140], [300, 300, 360, 360]], [0.9, 0.8], [th.GT_M, [10, 10, 40, 40]], iscrowd=[1, 1], labels=[1, 1], gt_labels=[0, 2]),
             th._frame_1003(),
             f(np.zeros((0, 4)), [], np.zeros((0, 4)), image_id=4)]
    for i, frame in enumerate(cases):
        r = pref.run([frame])
        out = _check([frame], r, num_classes=4, gt_capacity=4, record_capacity=1024)
        if i == 0:
            assert ((int(out["_records"]["flags"][0, 0]) >> (2 * np.arange(10))) & 3).tolist() == [ref.TP] * 10
        if i == 5:
            assert out["_res"]["stats"][[6, 7, 8]].tolist() == [0.25, 0.5, 0.75] and out["_res"]["n_records"] == 1000


# ------------------------------------------------------------------------------------------------------------ 3. loud failure
ERRORS = {"abort": 1, "gt_overflow": 2, "count": 4, "det_label": 8, "gt_label": 8, "both_labels": 8, "abort+gt_overflow": 3, "count+gt_overflow": 6}


@pytest.mark.parametrize("kind", sorted(ERRORS))
def test_every_error_bit_alone_and_combined_records_nothing(kind):
    """Each bit of the frame's error word, alone and together with the others it can meet (a bad count ends the frame before its labels
    are looked at): the word is set, nothing is recorded, npig does not move; after reset() a good frame is scored."""
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    f = dict(pref.grid_frame(77, 50, 12, NC - 1, image_id=1))
    if "det_label" in kind or kind == "both_labels":
        f["labels"] = f["labels"].copy()
        f["labels"][3] = NC - 1                                  # labels 0 .. NC - 2
    if "gt_label" in kind or kind == "both_labels":
        f["gt_labels"] = f["gt_labels"].copy()
        f["gt_labels"][0] = -1
    gcap = 11 if "gt_overflow" in kind else 16
    count = -1 if "abort" in kind else (65 if "count" in kind else None)
    out = _guarded([f], gt_capacity=gcap, det_capacity=64, counts=[count], summarize=False, record_capacity=256)
    assert int(out["error"].item()) == ERRORS[kind] and int(out["cursor"].item()) == 0 and int(out["npig"].sum().item()) == 0
    ev = evaluation.CocoDetectionEvaluator(NC, record_capacity=256, gt_capacity=16, device=DEV, use_cats=False, max_dets=(1, 10, 100))
    _feed(ev, evaluation.CocoGroundTruth(gcap, DEV), f, 64, count)
    with pytest.raises(FrcnnError):
        ev.summarize()
    ev.reset()
    good = pref.grid_frame(77, 50, 12, NC - 1, image_id=1)
    _feed(ev, evaluation.CocoGroundTruth(16, DEV), good, 64)
    assert ev.summarize()["n_records"] == 50


def test_full_record_store_counts_the_dropped():
    evaluation, _ = _mods()
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    frames = pref.make_set(8, [(60, 10), (60, 10)], NC - 1)
    ev = evaluation.CocoDetectionEvaluator(NC, record_capacity=100, gt_capacity=16, device=DEV, use_cats=False, max_dets=(1, 10, 100))
    gt = evaluation.CocoGroundTruth(16, DEV)
    for f in frames:
        _feed(ev, gt, f)
    with pytest.raises(FrcnnError, match="20 of 120 records were dropped"):
        ev.summarize()


# ------------------------------------------------------------------------------------------------------------ 4. device against device
def test_single_label_frames_equal_the_per_category_kernel():
    """With one label and max_dets = (1, 10, 100) the pooled kernels and coco_update_kernel see the same lists: sorted records and
    summarize() are equal bit for bit."""
    evaluation, _ = _mods()
    frames = ref.make_set(3, n_images=10, num_classes=3, max_det=150, max_gt=16)
    assert all((f["labels"] == 0).all() for f in frames) and max(len(f["labels"]) for f in frames) > 100
    cats = tc._run(frames, 2, gt_capacity=16, det_capacity=160)
    pooled = evaluation.CocoDetectionEvaluator(2, record_capacity=1 << 14, gt_capacity=16, device=DEV, use_cats=False, max_dets=(1, 10, 100))
    gt = evaluation.CocoGroundTruth(16, DEV)
    for f in frames:
        _feed(pooled, gt, f, 160)
    tc._same_records(pooled.records_sorted(), cats.records_sorted())
    a, b = pooled.summarize(), cats.summarize()
    for k in ("precision", "recall", "npig", "stats"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["n_records"] == b["n_records"] > 100 and a["stats"][0] > 0
    tc._same_result(a, pref.run(frames, max_dets=(1, 10, 100)))


# ------------------------------------------------------------------------------------------------------------ 5. shards
def test_two_shards_with_an_overlapping_image_merge_to_one_evaluator():
    evaluation, _ = _mods()
    frames = pref.make_set(9, [(80, 20), (10, 3), (150, 30), (0, 4), (60, 60)], NC - 1)
    r = pref.run(frames, max_dets=(10, 50, 120))

    def ev(**kw):
        return evaluation.CocoDetectionEvaluator(NC, record_capacity=1 << 12, gt_capacity=64, device=DEV, use_cats=False, max_dets=(10, 50, 120),
                                                 image_capacity=8, **kw)
    a, b, one, gt = ev(), ev(), ev(), evaluation.CocoGroundTruth(64, DEV)
    for f in frames[:3]:
        _feed(a, gt, f)
    for f in frames[2:]:                                         # frames[2] is seen by both shards
        _feed(b, gt, f)
    for f in frames:
        _feed(one, gt, f)
    merged = ev().merge_shards([a, b.state()])
    tc._same_records(merged.records_sorted(), one.records_sorted())
    tc._same_records(merged.records_sorted(), r["records"])
    tc._same_result(merged.summarize(), r)
    synced = ev().merge_shards([a.state()]).synchronize_between_processes()          # no process group: deduplication only
    assert synced.summarize()["n_records"] == int(a.cursor.item())
    per_category = evaluation.CocoDetectionEvaluator(NC, record_capacity=1 << 12, gt_capacity=64, device=DEV, max_dets=(10, 50, 100), image_capacity=8)
    for bad in (lambda: ev().merge_shards([a, per_category]), lambda: per_category.merge_shards([a.state()]),
                lambda: evaluation.CocoDetectionEvaluator(NC, record_capacity=64, device=DEV, use_cats=False, max_dets=(10, 50, 120)).merge(
                    evaluation.CocoDetectionEvaluator(NC, record_capacity=64, device=DEV, max_dets=(10, 50, 100)))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------------------ 6. capture
def test_update_captured_once_and_replayed_on_three_frames_equals_eager():
    """A host sync inside update would raise during capture.  The static detections and the ground-truth buffer are rewritten between
    the replays."""
    evaluation, ops = _mods()
    frames = pref.make_set(10, [(200, 40), (0, 7), (450, 64)], NC - 1)
    kw = dict(record_capacity=1 << 12, gt_capacity=64, device=DEV, use_cats=False, max_dets=(10, 100, 300), image_capacity=4)
    eager, gt = evaluation.CocoDetectionEvaluator(NC, **kw), evaluation.CocoGroundTruth(64, DEV)
    for f in frames:
        _feed(eager, gt, f, 512)
    torch.cuda.synchronize()
    ev = evaluation.CocoDetectionEvaluator(NC, **kw)
    static = tc._dets(frames[0], 512)
    ev._workspace(512, 64)                                       # allocated outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(static, gt)
    assert int(ev.cursor.item()) == 0                            # the capture scores nothing
    for f in frames:
        d = tc._dets(f, 512)
        for dst, src in zip((static.boxes, static.labels, static.scores, static.count), (d.boxes, d.labels, d.scores, d.count)):
            dst.copy_(src)
        tc._set_gt(gt, f)
        graph.replay()
    tc._same_records(ev.records_sorted(), eager.records_sorted())
    a, b = ev.summarize(), eager.summarize()
    for k in ("precision", "recall", "npig", "stats"):
        assert np.array_equal(a[k], b[k]), k
    assert torch.equal(ev.led_image[:3], eager.led_image[:3]) and torch.equal(ev.led_range[:3], eager.led_range[:3])
    tc._same_result(a, pref.run(frames, max_dets=(10, 100, 300)))


# ------------------------------------------------------------------------------------------------------------ 7. the models
from test_gpu_detect import fpn, vgg                             # noqa: E402,F401  (module-scoped fixtures: both mirrors)

SHAPES = {"vgg": (600, 1000), "fpn": (800, 1344)}


def _same_detections(a, b):
    """The counts, and the live rows of the fixed-capacity fields (the rows behind the count are not defined)."""
    n = max(int(a.count.item()), 0)
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            rows = name in ("boxes", "labels", "scores", "prob")
            assert torch.equal(x[:n] if rows else x, y[:n] if rows else y), name


def _proposal_frames(m, hw, seeds=(21, 41, 42)):
    """Input frames, and for each a ground truth cut from its own proposals (so that matches exist), as frame dicts of the proposals."""
    xs, frames = [], []
    for k, seed in enumerate(seeds):
        x = torch.randn(1, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(seed)).to(DEV)
        p = m.proposals(x)
        n = int(p.count.item())
        assert n >= 8, "degenerate test frame"
        b = p.boxes[:n].cpu().numpy()
        w, h = tc.SIZES[k]
        pick = np.arange(0, n, max(n // (6 + k), 1))[:12]
        px = np.round(b[pick].astype(np.float64) * np.array([w, h, w, h]))
        gtb = np.stack([px[:, 0], px[:, 1], px[:, 2] - px[:, 0], px[:, 3] - px[:, 1]], 1)
        xs.append(x)
        frames.append({"image_id": 10 + k, "w": w, "h": h, "boxes": b, "labels": np.zeros(n, np.int32), "scores": p.scores[:n].cpu().numpy(),
                       "gt_boxes": gtb, "gt_area": gtb[:, 2] * gtb[:, 3], "gt_labels": (np.arange(len(pick)) % 5).astype(np.int32),
                       "gt_iscrowd": (np.arange(len(pick)) % 4 == 1).astype(np.uint8)})
    return xs, frames


@pytest.mark.parametrize("mirror", ["vgg", "fpn"])
def test_proposals_detect_and_detect_graph(mirror, request):
    """model.proposals(x) = _test_proposals' RoIs and count with the rank ramp; detect(want_proposals=True) = the plain detect and those
    proposals; DetectGraph(proposal_evaluator=) replayed over three frames = eager proposals + update = the restatement on the
    proposals brought to the host; without the argument DetectGraph's outputs are those of the eager detect."""
    evaluation, ops = _mods()
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    m, hw = request.getfixturevalue(mirror), SHAPES[mirror]
    xs, frames = _proposal_frames(m, hw)
    with torch.no_grad():
        _, rois, n_rois = m._test_proposals(xs[0])
    p = m.proposals(xs[0])
    P = rois.shape[0]
    n = int(n_rois.item())
    assert p.boxes.shape == rois.shape and torch.equal(p.boxes[:n], rois[:n]) and torch.equal(p.count, n_rois) and p.n_rois is p.count
    assert p.labels.dtype == torch.int32 and p.labels.shape == (P,)
    assert not p.labels.any() and p.scores.dtype == torch.float32 and p.scores.tolist() == [float(P - i) for i in range(P)]
    plain = m.detect(xs[0], tc.THRES)
    dets, props = m.detect(xs[0], tc.THRES, want_proposals=True)
    _same_detections(dets, plain)
    _same_detections(props, p)
    # eager proposals + update against the restatement
    max_dets = (10, 100, P)
    r = pref.run(frames, max_dets=max_dets)
    assert r["stats"][8] > 0 and len(r["records"]["label"]) == sum(len(f["labels"]) for f in frames)
    pe_e = evaluation.ProposalEvaluator(max_dets=max_dets, gt_capacity=16, record_capacity=1 << 13, device=DEV)
    gt = evaluation.CocoGroundTruth(16, DEV)
    for x, f in zip(xs, frames):
        tc._set_gt(gt, f)
        pe_e.update(m.proposals(x), gt)
    tc._same_records(pe_e.records_sorted(), r["records"])
    res = pe_e.summarize()
    want = pref.proposal_summary(r)
    assert sorted(res) == ["ar", "ar_large", "ar_medium", "ar_small", "n_records", "npig", "recall"]
    for k in ("ar", "recall", "npig"):
        assert np.array_equal(res[k], want[k]), k
    assert (res["ar_small"], res["ar_medium"], res["ar_large"]) == (want["ar_small"], want["ar_medium"], want["ar_large"])
    # one replay per frame scores the detections and the proposals
    pe_g = evaluation.ProposalEvaluator(max_dets=max_dets, gt_capacity=16, record_capacity=1 << 13, device=DEV)
    ev_g = evaluation.CocoDetectionEvaluator(m.num_classes, record_capacity=1 << 14, gt_capacity=16, device=DEV)
    ev_e = evaluation.CocoDetectionEvaluator(m.num_classes, record_capacity=1 << 14, gt_capacity=16, device=DEV)
    dg = DetectGraph(m, hw, threshold=tc.THRES, evaluator=ev_g, gt=gt, proposal_evaluator=pe_g)
    dg0 = DetectGraph(m, hw, threshold=tc.THRES)
    assert dg0.proposals is None and int(pe_g.cursor.item()) == 0
    for x, f in zip(xs, frames):
        tc._set_gt(gt, f)
        eager = m.detect(x, tc.THRES)
        ev_e.update(eager, gt)
        out = dg(x)
        _same_detections(out, eager)
        _same_detections(dg.proposals, m.proposals(x))
        _same_detections(dg0(x), eager)
    tc._same_records(pe_g.records_sorted(), pe_e.records_sorted())
    tc._same_records(ev_g.records_sorted(), ev_e.records_sorted())
    rg = pe_g.summarize()
    for k in ("ar", "recall", "npig"):
        assert np.array_equal(rg[k], res[k]), k
    with pytest.raises(ValueError):
        DetectGraph(m, hw, proposal_evaluator=pe_g)                                       # gt= is missing
    if mirror == "vgg":                                                                    # one mirror is enough: the proposals' update without a detection evaluator
        only = evaluation.ProposalEvaluator(max_dets=max_dets, gt_capacity=16, record_capacity=1 << 13, device=DEV)
        dgp = DetectGraph(m, hw, threshold=tc.THRES, gt=gt, proposal_evaluator=only)
        for x, f in zip(xs, frames):
            tc._set_gt(gt, f)
            dgp(x)
        tc._same_records(only.records_sorted(), pe_e.records_sorted())
