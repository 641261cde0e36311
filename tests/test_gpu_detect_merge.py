"""The merge of detection sets on the device (csrc/detect_merge.hip, ops.merge_detections), FRCNN.detect_tta and TTADetectGraph.

Every comparison of the op is bit for bit against tests/detect_merge_ref.py (pinned on the CPU by tests/test_detect_merge_host.py):
boxes, labels, scores, count, class counts and status.  Every call of the op runs between guard bands (tests/guarded.py), once over 0xFF
and once over 0x00: no byte outside the outputs and the exact-size workspace changes, and the defined part of the outputs does not
depend on what the buffers held.  Rows at and above the count are not looked at."""
import numpy as np
import pytest
import torch

import detect_merge_ref as ref
from guarded import run_both

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NEG_INF = float("-inf")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dets(ops, s, place=lambda t: t):
    b, l, sc, n = s
    return ops.Detections(place(_t(np.asarray(b, F).reshape(-1, 4))), place(_t(np.asarray(l, np.int32))), place(_t(np.asarray(sc, F))),
                          place(_t(np.array([n], np.int32))), None, None, None)


def run(sets, flags, C, min_score=0.0, nms_thr=0.3, vote_thr=None, capacity=None):
    """ops.merge_detections between guard bands; returns numpy: the first count rows (none when count = -1), count, class_counts, status."""
    from faster_rcnn_pytorch_amd import ops

    def case(g):
        out = ops.merge_detections([_dets(ops, s, g.place) for s in sets], hflip=[bool(f & 1) for f in flags], vflip=[bool(f & 2) for f in flags],
                                   num_classes=C, min_score=min_score, nms_threshold=nms_thr, vote_threshold=vote_thr, capacity=capacity)
        assert out.prob is None and out.labels.dtype == torch.int32 and out.status.dtype == torch.int32
        n = max(int(out.count.item()), 0)
        return {"boxes": out.boxes[:n], "labels": out.labels[:n], "scores": out.scores[:n], "count": out.count, "class_counts": out.class_counts,
                "status": out.status}
    out, _ = run_both(case)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want):
    """count, class counts and status first; the rows when the count is not -1."""
    assert int(got["count"][0]) == want["count"], (got["count"], want["count"], int(got["status"][0]), want["status"])
    assert int(got["status"][0]) == want["status"]
    assert np.array_equal(got["class_counts"], want["class_counts"])
    if want["count"] >= 0:
        assert np.array_equal(got["labels"], want["labels"])
        assert ref.same_bits(got["scores"], want["scores"]) and ref.same_bits(got["boxes"], want["boxes"])


def check(sets, flags, C, **kw):
    r = ref.merge(sets, flags, C, min_score=kw.get("min_score", 0.0), nms_thr=kw.get("nms_thr", 0.3), vote_thr=kw.get("vote_thr"),
                  out_capacity=kw.get("capacity") if kw.get("capacity") is not None else min(sum(len(s[1]) for s in sets), (C - 1) * 2048))
    same(run(sets, flags, C, **kw), r)
    return r


# ------------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("P,C,seed", [(7, 3, 3), (300, 21, 1)], ids=["7x3", "300x21"])
def test_one_set_from_the_post_process_comes_back_bit_for_bit(P, C, seed):
    from faster_rcnn_pytorch_amd import ops
    rng = np.random.RandomState(seed)                         # the input recipe of tests/test_gpu_detect.py
    hc, hr = (rng.randn(P, C) * 0.8).astype(F), (rng.randn(P, 4 * C) * 0.5).astype(F)
    c, wh = rng.rand(P, 2) * 0.8 + 0.1, rng.rand(P, 2) * 0.5 + 0.05
    rois = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(F)
    det = ops.detect_postprocess(_t(hc), _t(hr), _t(rois), _t(np.array([P], np.int32)), 0.05, 0.3)
    n = int(det.count.item())
    assert n > P // 2
    s = (det.boxes.cpu().numpy(), det.labels.cpu().numpy(), det.scores.cpu().numpy(), n)
    got = run([s], [0], C, min_score=NEG_INF)
    assert int(got["count"][0]) == n and int(got["status"][0]) == 0 and np.array_equal(got["class_counts"], det.class_counts.cpu().numpy())
    assert np.array_equal(got["labels"], s[1][:n]) and ref.same_bits(got["scores"], s[2][:n]) and ref.same_bits(got["boxes"], s[0][:n])


# ------------------------------------------------------------------------------------------------------------ 2. random sets
def _variant(sets, variant, C):
    sets = [(b.copy(), l.copy(), s.copy(), n) for b, l, s, n in sets]
    if variant == "one_empty":
        sets[1] = sets[1][:3] + (0,)
    elif variant == "all_empty":
        sets = [s[:3] + (0,) for s in sets]
    elif variant == "garbage_tail":                           # rows at and above the count: NaN boxes, NaN scores, labels out of range
        for b, l, s, n in sets:
            b[n:], s[n:], l[n:] = np.nan, np.nan, C + 5
            s[n::2] = 2.0
    return sets


@pytest.mark.parametrize("variant", ["plain", "one_empty", "all_empty", "garbage_tail"])
@pytest.mark.parametrize("vote", [None, 0.5], ids=["nms", "vote"])
@pytest.mark.parametrize("K,C,seed", [(2, 3, 11), (3, 21, 12)], ids=["K2_C3", "K3_C21"])
def test_random_sets(K, C, seed, vote, variant):
    rng = np.random.RandomState(seed)
    per = 40 if C == 3 else 300                               # ~20 / ~15 candidates per class and set
    sets = _variant(ref.random_sets(rng, K, C, [per + 9 + 3 * k for k in range(K)], [per + k for k in range(K)]), variant, C)
    flags = [0, 1, 2][:K]                                     # set 1 is a view mirrored in x, set 2 in y: stored mirrored, so that the merge brings them back
    sets = [(ref.flip(b, f), l, s, n) for (b, l, s, n), f in zip(sets, flags)]
    r = ref.merge(sets, flags, C, nms_thr=0.3, vote_thr=vote)
    if variant == "all_empty":
        assert r["count"] == 0
    else:                                                     # the case is not degenerate, by the reference alone
        assert r["count"] > 0 and r["suppressed"] > 0 and r["status"] == 0
        if vote is not None:
            assert max(r["voters"]) >= 2 and not ref.same_bits(r["boxes"], r["unvoted"])
    check(sets, flags, C, nms_thr=0.3, vote_thr=vote)


# ------------------------------------------------------------------------------------------------------------ 3. lane-order seams
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 129])
def test_voting_sums_at_the_lane_seams(m):
    """One class, m mutually overlapping candidates: one kept box, m voters.  Random scores and boxes: any other order of the binary64
    additions shows in the last bits.  Dyadic data: every order gives the same sums, and the naive float64 mean must match as well."""
    rng = np.random.RandomState(100 + m)
    j = rng.rand(m, 4) * 0.03
    b = (np.array([.25, .25, .75, .75]) + j * np.array([1, 1, -1, -1])).astype(F)
    sets = [(b, np.zeros(m, np.int32), (rng.rand(m) * 0.9 + 0.05).astype(F), m)]
    r = check(sets, [0], 2, vote_thr=0.5)
    assert r["count"] == 1 and r["voters"] == [m]
    dy = ref.dyadic_cluster(rng, m)
    r = check(dy, [0], 2, vote_thr=0.5)
    assert r["count"] == 1 and r["voters"] == [m]
    assert ref.same_bits(r["boxes"], ref.merge(dy, [0], 2, vote_thr=0.5, naive=True)["boxes"])


# ------------------------------------------------------------------------------------------------------------ 4. ties, flip, robustness
def test_ties_within_and_across_sets():
    a = (np.array([[0, 0, .25, .25], [.5, 0, .75, .25], [0, 0, .25, .25]], F), np.zeros(3, np.int32), np.full(3, .5, F), 3)
    b = (np.array([[0, .5, .25, .75], [0, 0, .25, .25]], F), np.zeros(2, np.int32), np.full(2, .5, F), 2)
    r = check([a, b], [0, 0], 2)
    assert r["boxes"].tolist() == [[0, 0, .25, .25], [.5, 0, .75, .25], [0, .5, .25, .75]] and r["suppressed"] == 2
    r = check([b, a], [0, 0], 2)                              # the duplicate box: the earlier set's copy survives
    assert r["boxes"].tolist() == [[0, .5, .25, .75], [0, 0, .25, .25], [.5, 0, .75, .25]]
    z = (a[0], a[1], np.array([0.0, -0.0, 0.0], F), 3)       # -0 counts as +0 in the order: rows 0, 1 in row order, row 2 suppressed by row 0
    r = check([z], [0], 2, min_score=-1.0)
    assert r["count"] == 2 and ref.same_bits(r["scores"], np.array([0.0, -0.0], F))


def test_flip():
    rng = np.random.RandomState(5)
    s = ref.random_sets(rng, 1, 5, [50], [45], dyadic=True)[0]
    for f in (1, 2, 3):
        r = check([s], [f], 5, nms_thr=1.5)                   # nothing suppressed: every live row comes back, mirrored
        assert r["count"] == 45
        order = np.lexsort((np.arange(45), -s[2][:45].astype(np.float64), s[1][:45]))
        assert ref.same_bits(r["boxes"], ref.flip(s[0][:45], f)[order])
        back = ref.merge([(r["boxes"], r["labels"], r["scores"], 45)], [f], 5, nms_thr=1.5)
        got = run([(r["boxes"], r["labels"], r["scores"], 45)], [f], 5, nms_thr=1.5)
        same(got, back)
        assert ref.same_bits(got["boxes"], s[0][:45][order])  # two flips restore the bits of dyadic boxes


def test_nan_zero_area_and_inf_rows_under_voting():
    b = np.array([[.25, .25, .75, .75], [.26, .25, .75, .75], [np.nan, .25, .75, .75], [.5, .25, .5, .75], [.25, .26, .75, .75],
                  [0, 0, .125, .125], [0, 0, .125, .126]], F)
    s = np.array([.9, .8, .7, .6, .5, np.inf, .4], F)
    r = check([(b, np.zeros(7, np.int32), s, 7)], [0], 2, vote_thr=0.5)
    # order: inf, .9, .8 (suppressed), NaN box, zero-area box, .5 (suppressed), .4 (suppressed by the inf row)
    assert r["count"] == 4 and ref.same_bits(r["unvoted"], b[[5, 0, 2, 3]])
    assert ref.same_bits(r["boxes"][[0, 2, 3]], b[[5, 2, 3]])  # the inf score (a non-finite sum), the NaN box and the zero-area box: unchanged bits
    assert r["voters"] == [2, 3, 1, 1] and not ref.same_bits(r["boxes"][1], b[0])


# ------------------------------------------------------------------------------------------------------------ 5. limits
def _grid(n):
    """n disjoint boxes on a 64 x 64 grid, scores descending."""
    i = np.arange(n)
    x, y = (i % 64) / 64.0, (i // 64) / 64.0
    b = np.stack([x, y, x + 1 / 128.0, y + 1 / 128.0], 1).astype(F)
    return b, np.zeros(n, np.int32), (1.0 - i / 4096.0).astype(F), n


def test_2048_candidates_in_a_class_pass_and_2049_do_not():
    g = _grid(2049)
    a, b = tuple(v[:1000] for v in g[:3]) + (1000,), tuple(v[1000:] for v in g[:3]) + (1048,)
    r = check([a, b], [0, 0], 3)
    assert r["count"] == 2048 and r["status"] == 0
    b = b[:3] + (1049,)
    r = check([a, b], [0, 0], 3)
    assert r["count"] == -1 and r["status"] == ref.CLASS_OVERFLOW and r["class_counts"].tolist() == [0, 0]


def test_capacity_counts_and_labels():
    rng = np.random.RandomState(7)
    sets = ref.random_sets(rng, 2, 4, [70, 70], [60, 64])
    r0 = ref.merge(sets, [0, 0], 4)
    r = check(sets, [0, 0], 4, capacity=r0["total"])          # exactly full
    assert r["count"] == r0["total"] and r["status"] == 0
    r = check(sets, [0, 0], 4, capacity=r0["total"] - 1)      # a kept total of out_capacity + 1
    assert r["count"] == -1 and r["status"] == ref.OUTPUT_OVERFLOW
    r = check([sets[0], sets[1][:3] + (-1,)], [0, 0], 4)      # an aborted scan upstream
    assert r["count"] == -1 and r["status"] == ref.UPSTREAM_ABORT and r["total"] > 0
    r = check([sets[0], sets[1][:3] + (75,)], [0, 0], 4)      # a count above the capacity: clipped and flagged
    assert r["count"] > 0 and r["status"] == ref.COUNT_CLIPPED
    sets[0][1][3] = 3                                         # a live label outside 0 .. C-2
    sets[1][1][5] = -1
    r = check(sets, [0, 0], 4)
    assert r["count"] > 0 and r["status"] == ref.LABEL_RANGE
    from faster_rcnn_pytorch_amd import _lib, ops
    out = ops.merge_detections([_dets(ops, sets[0]), _dets(ops, sets[1][:3] + (-1,))], num_classes=4)
    with pytest.raises(_lib.FrcnnError):
        out.to_host()
    assert ops.describe_merge_status(int(out.status.item())) != []


def test_fpn_shapes_on_the_op_alone():
    """C = 91 with the capacities of P = 1000 (90 000 rows per set): the default output capacity is the sets' sum."""
    rng = np.random.RandomState(9)
    sets = ref.random_sets(rng, 2, 91, [90000, 90000], [1400, 1300])
    sets[1] = (ref.flip(sets[1][0], 1),) + sets[1][1:]        # the second view is stored mirrored
    r = check(sets, [0, 1], 91, vote_thr=0.5)
    assert r["count"] > 90 and r["suppressed"] > 0 and max(r["voters"]) >= 2


# ------------------------------------------------------------------------------------------------------------ 6. model level
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


@pytest.mark.parametrize("vote", [None, 0.5], ids=["nms", "vote"])
def test_detect_tta_is_the_merge_of_two_detect_calls(vgg, vote):
    from faster_rcnn_pytorch_amd import ops
    x = _frame(21)
    a, b = vgg.detect(x, THRES), vgg.detect(x.flip(-1), THRES)
    want = ops.merge_detections([a, b], hflip=[False, True], num_classes=21, min_score=NEG_INF, nms_threshold=0.3, vote_threshold=vote)
    got = vgg.detect_tta(x, THRES, vote_threshold=vote)
    na, nb, n = int(a.count.item()), int(b.count.item()), int(got.count.item())
    assert na > 20 and nb > 20 and 20 < n < na + nb and int(got.status.item()) == 0          # some rows of the two views merge
    assert _equal(_host(got), _host(want))
    assert _equal(_host(vgg.detect_tta([(x, False), (x.flip(-1), True)], THRES, vote_threshold=vote)), _host(want))
    # and the op itself against the restatement on the model's own detections
    sets = [(d.boxes.cpu().numpy(), d.labels.cpu().numpy(), d.scores.cpu().numpy(), int(d.count.item())) for d in (a, b)]
    r = ref.merge(sets, [0, 1], 21, min_score=NEG_INF, nms_thr=0.3, vote_thr=vote)
    gb, gl, gs = (t.numpy() for t in got.to_host())
    assert r["count"] == n and np.array_equal(gl, r["labels"]) and ref.same_bits(gs, r["scores"]) and ref.same_bits(gb, r["boxes"])


def test_tta_graph_replays_equal_eager_detect_tta(vgg):
    from faster_rcnn_pytorch_amd.inference import TTADetectGraph
    xa, xb = _frame(41), _frame(42)
    ea, eb = _host(vgg.detect_tta(xa, THRES, vote_threshold=0.5)), _host(vgg.detect_tta(xb, THRES, vote_threshold=0.5))
    assert not _equal(ea, eb) and len(ea[1]) > 0 and len(eb[1]) > 0
    tg = TTADetectGraph(vgg, [(H, W)], threshold=THRES, vote_threshold=0.5)
    ra, rb, ra2, rb2 = _host(tg(xa)), _host(tg([xb])), _host(tg(xa)), _host(tg(xb))
    assert _equal(ra, ea) and _equal(rb, eb) and _equal(ra2, ra) and _equal(rb2, rb)
    tg.set_threshold(0.2)                        # read at replay time
    r2 = _host(tg(xa))
    assert _equal(r2, _host(vgg.detect_tta(xa, 0.2, vote_threshold=0.5))) and len(r2[1]) < len(ea[1])
    with pytest.raises(ValueError):
        tg(_frame(1, 320, 480))


def test_tta_graph_with_a_second_size_and_an_evaluator(vgg):
    """Two sizes, four views, and a captured DetectionEvaluator update on the merged set: its records equal the eager evaluator's."""
    from faster_rcnn_pytorch_amd import evaluation
    from faster_rcnn_pytorch_amd.inference import TTADetectGraph
    thr3 = (0.3, 0.5, 0.75)
    frames = [(_frame(41), _frame(51, 320, 480)), (_frame(42), _frame(52, 320, 480))]

    def views(xs):
        return [(xs[0], False), (xs[0].flip(-1), True), (xs[1], False), (xs[1].flip(-1), True)]
    gt = evaluation.GroundTruth(16, DEV)
    ev_e = evaluation.DetectionEvaluator(21, thr3, record_capacity=1 << 15, gt_capacity=16, device=DEV)
    ev_g = evaluation.DetectionEvaluator(21, thr3, record_capacity=1 << 15, gt_capacity=16, device=DEV)
    eager, gts = [], []
    for k, xs in enumerate(frames):
        d = vgg.detect_tta(views(xs), THRES)
        b, l, _ = (t.numpy() for t in d.to_host())
        assert len(l) >= 8, "degenerate test frame"
        pick = np.arange(0, len(l), max(len(l) // 6, 1))[:12]
        gts.append((np.round(b[pick].astype(np.float64) * np.array([500, 375, 500, 375])).astype(F), l[pick].astype(np.int32),
                    (np.arange(len(pick)) % 4 == 1).astype(np.uint8), (500, 375), 10 + k))
        gt.set(*gts[k])
        ev_e.update(d, gt)
        eager.append(_host(d))
    tg = TTADetectGraph(vgg, [(H, W), (320, 480)], threshold=THRES, evaluator=ev_g, gt=gt)
    assert ev_g.summarize()["n_records"] == 0   # warm-up and capture score nothing
    for k, xs in enumerate(frames):
        gt.set(*gts[k])
        assert _equal(_host(tg(list(xs))), eager[k])
    re_, rg = ev_e.records_sorted(), ev_g.records_sorted()
    assert len(re_["label"]) > 16 and ((re_["flags"] & 3) == 1).sum() >= 4
    for key in ("label", "image_id", "position", "flags"):
        assert np.array_equal(re_[key], rg[key]), key
    assert np.array_equal(re_["score"].view(np.uint32), rg["score"].view(np.uint32))
    with pytest.raises(ValueError):
        TTADetectGraph(vgg, [(H, W)], evaluator=ev_g)
