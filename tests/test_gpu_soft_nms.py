"""Soft-NMS on the device (csrc/detect_soft.hip, frcnn_detect_merge_soft) through ops.merge_detections(soft_nms=...), FRCNN.detect,
detect_tta, DetectGraph and TTADetectGraph.

Hard mode is held to frcnn_detect_merge bit for bit; linear mode to tests/soft_nms_ref.py bit for bit (pinned on the CPU by
tests/test_soft_nms_host.py): boxes, labels, scores, count, class counts and status.  Gaussian mode: labels, order and boxes identical,
scores within a relative (d + 1) * 2^-22 of the reference, d the decays the reference counts for that box -- each decay is one weight
rounded to fp32 (2^-24) on top of at most an ulp of the binary64 exp (2^-53) and one product rounding (2^-24), under 2^-22 together; the
bound is derived, not measured, and the inputs are the ones whose margin the host test holds above 1e-4.  Every call of the op runs
between guard bands (tests/guarded.py), once over 0xFF and once over 0x00; the rows at and above the count still hold the fill."""
import numpy as np
import pytest
import torch

import soft_nms_ref as ref
from guarded import run_both

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NEG_INF = float("-inf")
METHOD = {ref.HARD: "hard", ref.LINEAR: "linear", ref.GAUSSIAN: "gaussian"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dets(ops, s, place=lambda t: t):
    b, l, sc, n = s
    return ops.Detections(place(_t(np.asarray(b, F).reshape(-1, 4))), place(_t(np.asarray(l, np.int32))), place(_t(np.asarray(sc, F))),
                          place(_t(np.array([n], np.int32))), None, None, None)


def run(sets, flags, C, method=ref.LINEAR, nms_thr=0.3, sigma=0.5, floor=1e-3, min_score=0.0, vote_thr=None, capacity=None):
    """ops.merge_detections between guard bands (method None: without soft_nms, the greedy merge); returns numpy: the first count rows
    (none when count = -1), count, class_counts, status."""
    from faster_rcnn_pytorch_amd import ops
    soft = None if method is None else ops.SoftNMS(METHOD[method], sigma=sigma, score_floor=floor)

    def case(g):
        out = ops.merge_detections([_dets(ops, s, g.place) for s in sets], hflip=[bool(f & 1) for f in flags], vflip=[bool(f & 2) for f in flags],
                                   num_classes=C, min_score=min_score, nms_threshold=nms_thr, vote_threshold=vote_thr, capacity=capacity, soft_nms=soft)
        assert isinstance(out, ops.MergedDetections) and out.prob is None and out.labels.dtype == torch.int32 and out.status.dtype == torch.int32
        n = int(out.count.item())
        if n >= 0:                                                # rows at and above the count: as they were
            for t in (out.boxes, out.labels, out.scores):
                tail = t[n:].contiguous().view(torch.uint8)
                assert bool((tail == g.fill).all()), "a row at or above the count was written"
        n = max(n, 0)
        return {"boxes": out.boxes[:n], "labels": out.labels[:n], "scores": out.scores[:n], "count": out.count, "class_counts": out.class_counts,
                "status": out.status}
    out, _ = run_both(case)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, scores=True):
    """count, class counts and status first; the rows when the count is not -1."""
    assert int(got["count"][0]) == want["count"], (got["count"], want["count"], int(got["status"][0]), want["status"])
    assert int(got["status"][0]) == want["status"]
    assert np.array_equal(got["class_counts"], want["class_counts"])
    if want["count"] >= 0:
        assert np.array_equal(got["labels"], want["labels"])
        assert ref.same_bits(got["boxes"], want["boxes"])
        if scores:
            assert ref.same_bits(got["scores"], want["scores"])


def check(sets, flags, C, method=ref.LINEAR, **kw):
    cap = kw.get("capacity") if kw.get("capacity") is not None else min(sum(len(s[1]) for s in sets), (C - 1) * 2048)
    r = ref.soft_merge(sets, flags, C, method, nms_thr=kw.get("nms_thr", 0.3), sigma=kw.get("sigma", 0.5), floor=kw.get("floor", 1e-3),
                       min_score=kw.get("min_score", 0.0), vote_thr=kw.get("vote_thr"), out_capacity=cap)
    same(run(sets, flags, C, method, **kw), r)
    return r


def _flipped(sets, flags):
    """The sets stored as their views saw them, so that the merge brings them back."""
    return [(ref.flip(b, f), l, s, n) for (b, l, s, n), f in zip(sets, flags)]


def _set(boxes, scores):
    b = np.array(boxes, F).reshape(-1, 4)
    return b, np.zeros(len(b), np.int32), np.array(scores, F), len(b)


# ------------------------------------------------------------------------------------------------------------ 1. hard mode
@pytest.mark.parametrize("vote", [None, 0.8], ids=["novote", "vote"])
@pytest.mark.parametrize("K,C", [(1, 2), (1, 5), (3, 2), (3, 5)], ids=["K1_C2", "K1_C5", "K3_C2", "K3_C5"])
def test_hard_mode_is_the_greedy_merge_bit_for_bit(K, C, vote):
    rng = np.random.RandomState(10 * K + C)
    counts = [200, 40, 120][:K]
    flags = [0, 1, 2][:K]
    sets = _flipped(ref.random_sets(rng, K, C, [n + 9 for n in counts], counts, spread=0.15), flags)
    soft = run(sets, flags, C, ref.HARD, vote_thr=vote)
    hard = run(sets, flags, C, None, vote_thr=vote)
    n = int(hard["count"][0])
    assert 0 < n < sum(counts) and int(hard["status"][0]) == 0          # boxes were suppressed
    for k in ("count", "status", "class_counts", "labels", "scores", "boxes"):
        assert ref.same_bits(soft[k], hard[k]), k


# ------------------------------------------------------------------------------------------------------------ 2. linear mode, random sets
@pytest.mark.parametrize("vote", [None, 0.8], ids=["novote", "vote"])
@pytest.mark.parametrize("K,C,seed", [(2, 3, 21), (3, 5, 22)], ids=["K2_C3", "K3_C5"])
def test_linear_mode_on_random_sets(K, C, seed, vote):
    rng = np.random.RandomState(seed)
    per = 60 * (C - 1)                                            # ~60 rows per class and set
    flags = [0, 1, 2][:K]
    sets = _flipped(ref.random_sets(rng, K, C, [per + 9 + 3 * k for k in range(K)], [per + k for k in range(K)], spread=0.15), flags)
    r = check(sets, flags, C, ref.LINEAR, vote_thr=vote)
    assert r["count"] > 20 and r["status"] == 0 and (r["decays"] >= 2).mean() > 0.5          # most boxes were decayed several times
    if vote is not None:
        assert not ref.same_bits(r["boxes"], r["unvoted"])


# ------------------------------------------------------------------------------------------------------------ 3. ownership seams
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048])
def test_candidate_counts_at_the_ownership_seams(m):
    """One class of m candidates: thread t owns positions t, t + 256, ...; 64 lanes a wave, 256 threads, 8 slots a thread."""
    sets = ref.one_class(np.random.RandomState(1000 + m), m, spread=0.15)
    r = check(sets, [0], 2, ref.LINEAR)
    assert r["count"] >= 1 and (m < 63 or r["decays"].max() >= 2)


def test_a_full_class_that_emits_every_candidate():
    """2048 boxes two cells wide on a 64 x 32 grid of cells: each overlaps its row neighbours at IoU 1/3 and nothing else, so every box is
    decayed at most twice, none falls under the floor, and the scan runs all 2048 steps with every thread's eight slots live."""
    rng = np.random.RandomState(77)
    i = np.arange(2048)
    x, y = (i % 64) / 66.0, (i // 64) / 32.0
    b = np.stack([x, y, x + 2 / 66.0, y + 1 / 32.0], 1).astype(F)
    r = check([(b, np.zeros(2048, np.int32), (rng.rand(2048) * 0.9 + 0.05).astype(F), 2048)], [0], 2, ref.LINEAR)
    assert r["count"] == 2048 and r["decays"].max() == 2 and (r["decays"] > 0).mean() > 0.5


def test_2049_candidates_overflow_the_class():
    sets = ref.one_class(np.random.RandomState(3049), 2049)
    r = check(sets, [0], 2, ref.LINEAR)
    assert r["count"] == -1 and r["status"] == ref.CLASS_OVERFLOW and r["class_counts"].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------ 4. ties
A_, B_, C_BOX = [0, 0, .5, .5], [0, 0, .5, .25], [.75, .75, 1, 1]             # IoU(A, B) = 0.5 exactly; C touches neither


def test_equal_initial_scores_within_and_across_sets():
    a = (np.array([[0, 0, .25, .25], [.5, 0, .75, .25], [0, 0, .25, .25]], F), np.zeros(3, np.int32), np.full(3, .5, F), 3)
    b = (np.array([[0, .5, .25, .75], [0, 0, .25, .25]], F), np.zeros(2, np.int32), np.full(2, .5, F), 2)
    r = check([a, b], [0, 0], 2, ref.LINEAR, floor=-1.0)
    # the duplicates decay to 0.5 * (1 - 1) = 0 and come last, the earlier set's first
    assert r["boxes"].tolist() == [[0, 0, .25, .25], [.5, 0, .75, .25], [0, .5, .25, .75], [0, 0, .25, .25], [0, 0, .25, .25]]
    assert r["scores"].tolist() == [.5, .5, .5, 0, 0]
    r = check([b, a], [0, 0], 2, ref.LINEAR)                    # floor 1e-3: the duplicates drop; set order decides among equals
    assert r["boxes"].tolist() == [[0, .5, .25, .75], [0, 0, .25, .25], [.5, 0, .75, .25]]


def test_equal_working_scores_after_a_decay_emit_the_lower_position_first():
    r = check([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.LINEAR)          # B decays onto C's .25 exactly
    assert r["scores"].tolist() == [.75, .25, .25] and r["boxes"].tolist() == [A_, B_, C_BOX]
    r = check([_set([C_BOX, A_, B_], [.25, .75, .5])], [0], 2, ref.LINEAR)          # other rows, the same sorted positions
    assert r["boxes"].tolist() == [A_, B_, C_BOX]
    r = check([_set([A_, B_, C_BOX], [.75, .375, .25])], [0], 2, ref.LINEAR)        # and the decay reorders: B falls behind C
    assert r["scores"].tolist() == [.75, .25, .1875] and r["boxes"].tolist() == [A_, C_BOX, B_]


# ------------------------------------------------------------------------------------------------------------ 5. thresholds
def test_iou_exactly_at_the_threshold_decays_nothing():
    s = _set([[0, 0, .5, .5], [0, .125, .75, .875]], [.75, .25])              # IoU = fp32(0.3) exactly (tests/test_detect_merge_host.py)
    r = check([s], [0], 2, ref.LINEAR, nms_thr=0.3)
    assert r["scores"].tolist() == [.75, .25] and r["decays"].tolist() == [0, 0]
    r = check([s], [0], 2, ref.LINEAR, nms_thr=0.2999)
    assert r["decays"].tolist() == [0, 1] and r["scores"][1] < F(.25)
    r = check([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.LINEAR, nms_thr=0.5)
    assert r["scores"].tolist() == [.75, .5, .25]


def test_a_decayed_score_equal_to_the_floor_stays_and_one_ulp_below_it_drops():
    s = [_set([A_, B_, C_BOX], [.75, .5, .125])]
    r = check(s, [0], 2, ref.LINEAR, floor=0.25)
    assert r["scores"].tolist() == [.75, .25, .125]              # C lies under the floor but was never decayed
    r = check(s, [0], 2, ref.LINEAR, floor=float(np.nextafter(F(0.25), F(1))))
    assert r["scores"].tolist() == [.75, .125]


# ------------------------------------------------------------------------------------------------------------ 6. special boxes and scores
@pytest.mark.parametrize("method", [ref.LINEAR, ref.GAUSSIAN], ids=["linear", "gaussian"])
def test_nan_and_zero_area_boxes_are_not_decayed_and_decay_nothing(method):
    b = np.array([[.25, .25, .75, .75], [np.nan, .25, .75, .75], [.5, .25, .5, .75], [.25, .25, .75, .75], [.25, np.nan, .75, .75],
                  [.25, .5, .75, .5]], F)
    s = np.array([.9, .8, .7, .5, .4, .3], F)
    sets = [(b, np.zeros(6, np.int32), s, 6)]
    # row 3 duplicates row 0 and is the only row that is ever decayed (linear: to .5 * 0, under the floor, so it drops)
    same(run(sets, [0], 2, method, vote_thr=0.5), ref.soft_merge(sets, [0], 2, method, vote_thr=0.5), scores=method == ref.LINEAR)
    r = ref.soft_merge(sets, [0], 2, method, floor=-1.0)        # with a floor below every score it comes last
    assert r["decays"].tolist() == [0, 0, 0, 0, 0, 1]
    got = run(sets, [0], 2, method, floor=-1.0)
    same(got, r, scores=method == ref.LINEAR)
    special = [1, 2, 4, 5]
    assert ref.same_bits(got["scores"][[1, 2, 3, 4]], s[special]) and ref.same_bits(got["boxes"][[1, 2, 3, 4]], b[special])
    assert got["count"][0] == 6 and got["scores"][0] == F(.9) and got["scores"][5] < F(.5)


def test_minus_zero_scores_tie_with_plus_zero():
    b = np.array([[0, 0, .25, .25], [.5, 0, .75, .25], [0, .5, .25, .75]], F)
    z = (b, np.zeros(3, np.int32), np.array([0.0, -0.0, 0.0], F), 3)
    r = check([z], [0], 2, ref.LINEAR, min_score=-1.0)
    assert r["count"] == 3 and ref.same_bits(r["scores"], np.array([0.0, -0.0, 0.0], F)) and ref.same_bits(r["boxes"], b)          # row order


# ------------------------------------------------------------------------------------------------------------ 7. gaussian mode
@pytest.mark.parametrize("case", ref.gaussian_cases(), ids=lambda c: c[0])
def test_gaussian_mode_within_the_derived_bound(case):
    _, sets, flags, C, kw = case
    r = ref.soft_merge(sets, flags, C, ref.GAUSSIAN, out_capacity=sum(len(s[1]) for s in sets), **kw)
    got = run(sets, flags, C, ref.GAUSSIAN, **kw)
    same(got, r, scores=False)                                   # labels, order and boxes: a voted box depends on the order and the ORIGINAL scores alone
    g, w = got["scores"].astype(np.float64), r["scores"].astype(np.float64)
    rel = np.abs(g - w) / np.abs(w)
    bound = (r["decays"] + 1) * 2.0 ** -22
    print("gaussian %s: max rel err %.3g, max err / bound %.3g, max decays %d" % (case[0], rel.max(), (rel / bound).max(), r["decays"].max()))
    assert (rel <= bound).all(), (rel / bound).max()
    assert ref.same_bits(got["scores"][r["decays"] == 0], r["scores"][r["decays"] == 0])          # an undecayed box keeps its score's bits


# ------------------------------------------------------------------------------------------------------------ 8. flip, determinism
def test_a_mirrored_copy_merges_onto_the_originals_boxes():
    rng = np.random.RandomState(6)
    b, l, s, n = ref.random_sets(rng, 1, 4, [70], [64], dyadic=True, spread=0.15)[0]
    r = check([(b, l, s, n), (ref.flip(b, 1), l, s, n)], [0, 1], 4, ref.LINEAR, floor=-1.0)
    twice = ref.soft_merge([(b, l, s, n), (b, l, s, n)], [0, 0], 4, ref.LINEAR, floor=-1.0)
    assert r["count"] == 2 * n and ref.same_bits(r["boxes"], twice["boxes"]) and ref.same_bits(r["scores"], twice["scores"])
    have = {tuple(v) for v in b[:n].tolist()}
    assert all(tuple(v) in have for v in r["boxes"].tolist())    # two flips restore the bits of dyadic boxes


def test_two_calls_give_the_same_bits():
    rng = np.random.RandomState(8)
    sets = ref.random_sets(rng, 2, 4, [300, 300], [290, 280], spread=0.15)
    for method in (ref.LINEAR, ref.GAUSSIAN):
        a = run(sets, [0, 0], 4, method, vote_thr=0.8)
        b = run(sets, [0, 0], 4, method, vote_thr=0.8)
        assert a["count"][0] > 20 and all(ref.same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------ 9. model level
@pytest.fixture(scope="module")
def vgg():
    from faster_rcnn_pytorch_amd.model import FRCNN
    torch.manual_seed(0)
    m = FRCNN(num_classes=21, sampling="host").to(DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                        # the fixture recipe of tests/test_gpu_detect.py
        m.rpn.cls_layer.weight.mul_(30)
        m.rpn.reg_layer.weight.mul_(10)
        m.fast_rcnn_head.cls_head.weight.copy_(torch.randn(m.fast_rcnn_head.cls_head.weight.shape, generator=g) * 0.8)
        m.fast_rcnn_head.reg_head.weight.copy_(torch.randn(m.fast_rcnn_head.reg_head.weight.shape, generator=g) * 0.5)
    return m.eval()


H, W, THRES = 600, 1000, 0.05


def _frame(seed, h=H, w=W):
    return torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _host(det):
    return [t.clone() for t in det.to_host()] + [det.class_counts.cpu().clone(), det.status.cpu().clone()]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_detect_is_the_soft_merge_of_the_unsuppressed_post_process(vgg, method):
    from faster_rcnn_pytorch_amd import ops
    soft = ops.SoftNMS(method)
    x = _frame(21)
    with torch.no_grad():
        features, rois, n_rois = vgg._test_proposals(x)
        head_cls, head_reg = vgg._head(features, rois, x)
    cands = ops.detect_postprocess(head_cls, head_reg, rois, n_rois, THRES, float("inf"), want_prob=True)
    want = ops.merge_detections([cands], num_classes=21, min_score=NEG_INF, nms_threshold=0.3, soft_nms=soft)
    got, props = vgg.detect(x, THRES, soft_nms=soft, want_prob=True, want_proposals=True)
    plain = vgg.detect(x, THRES)
    assert type(plain) is ops.Detections and isinstance(got, ops.MergedDetections)
    n, nc, npl = int(got.count.item()), int(cands.count.item()), int(plain.count.item())
    assert 20 < npl < nc and 20 < n <= nc and int(got.status.item()) == 0
    assert _equal(_host(got), _host(want))
    assert torch.equal(got.prob, cands.prob) and torch.equal(got.n_rois, n_rois) and torch.equal(props.boxes, rois)
    if method == "linear":                                        # and the op against the restatement on the model's own candidates
        s = (cands.boxes.cpu().numpy(), cands.labels.cpu().numpy(), cands.scores.cpu().numpy(), nc)
        r = ref.soft_merge([s], [0], 21, ref.LINEAR, min_score=NEG_INF)
        gb, gl, gs = (t.numpy() for t in got.to_host())
        assert r["count"] == n and np.array_equal(gl, r["labels"]) and ref.same_bits(gs, r["scores"]) and ref.same_bits(gb, r["boxes"])
        hard = vgg.detect(x, THRES, soft_nms=ops.SoftNMS("hard"))          # the same scan in hard mode: plain detect's rows
        assert _equal(_host(hard)[:4], [t.clone() for t in plain.to_host()] + [plain.class_counts.cpu()])


def test_graphs_replay_what_the_eager_calls_give(vgg):
    from faster_rcnn_pytorch_amd import ops
    from faster_rcnn_pytorch_amd.inference import DetectGraph, TTADetectGraph
    soft = ops.SoftNMS("linear")
    xa, xb = _frame(41), _frame(42)
    ea, eb = _host(vgg.detect(xa, THRES, soft_nms=soft)), _host(vgg.detect(xb, THRES, soft_nms=soft))
    assert not _equal(ea, eb) and len(ea[1]) > 20 and len(eb[1]) > 20
    dg = DetectGraph(vgg, (H, W), threshold=THRES, soft_nms=soft)
    assert _equal(_host(dg(xa)), ea) and _equal(_host(dg(xb)), eb) and _equal(_host(dg(xa)), ea)          # a second frame, and the first again
    ta, tb = (_host(vgg.detect_tta(x, THRES, vote_threshold=0.8, soft_nms=soft)) for x in (xa, xb))
    assert not _equal(ta, ea) and not _equal(ta, tb) and len(ta[1]) > 20
    tg = TTADetectGraph(vgg, [(H, W)], threshold=THRES, vote_threshold=0.8, soft_nms=soft)
    assert _equal(_host(tg(xa)), ta) and _equal(_host(tg(xb)), tb) and _equal(_host(tg(xa)), ta)
    assert type(DetectGraph(vgg, (H, W), threshold=THRES)(xa)) is ops.Detections


def test_a_captured_evaluator_update_accepts_the_result(vgg):
    from faster_rcnn_pytorch_amd import evaluation, ops
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    soft = ops.SoftNMS("linear")
    x = _frame(41)
    d = vgg.detect(x, THRES, soft_nms=soft)
    b, l, _ = (t.numpy() for t in d.to_host())
    pick = np.arange(0, len(l), max(len(l) // 6, 1))[:12]
    truth = (np.round(b[pick].astype(np.float64) * np.array([500, 375, 500, 375])).astype(F), l[pick].astype(np.int32),
             (np.arange(len(pick)) % 4 == 1).astype(np.uint8), (500, 375), 10)
    gt = evaluation.GroundTruth(16, DEV)
    ev_e = evaluation.DetectionEvaluator(21, (0.5,), record_capacity=1 << 15, gt_capacity=16, device=DEV)
    ev_g = evaluation.DetectionEvaluator(21, (0.5,), record_capacity=1 << 15, gt_capacity=16, device=DEV)
    gt.set(*truth)
    ev_e.update(d, gt)
    dg = DetectGraph(vgg, (H, W), threshold=THRES, evaluator=ev_g, gt=gt, soft_nms=soft)
    assert ev_g.summarize()["n_records"] == 0                    # warm-up and capture score nothing
    gt.set(*truth)
    assert _equal(_host(dg(x)), _host(d))
    re_, rg = ev_e.records_sorted(), ev_g.records_sorted()
    assert len(re_["label"]) == len(l) and ((re_["flags"] & 3) == 1).sum() >= 4
    for key in ("label", "image_id", "position", "flags"):
        assert np.array_equal(re_[key], rg[key]), key
    assert np.array_equal(re_["score"].view(np.uint32), rg["score"].view(np.uint32))
