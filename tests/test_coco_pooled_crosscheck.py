"""pycocotools' own COCOeval with params.useCats = 0 and maxDets = [100, 300, 1000] against the pooled restatement
(tests/coco_eval_pooled_ref.py) and the device evaluator, exactly, on synthetic multi-label sets as COCO dicts.  Runs wherever pycocotools can
be imported and is SKIPPED elsewhere (the skip reason says so): the pooled order -- labels first, the stable score sort over it, the later of
equal IoUs -- is restated from the published algorithm and stays unpinned until this file has run (docs/PARITY.md)."""
import numpy as np
import pytest

pycocotools = pytest.importorskip(
    "pycocotools", reason="pycocotools is not installed (neither here nor on the GPU machine today): the pooled COCO protocol (useCats = 0) stays "
                          "unpinned (docs/PARITY.md)")

import coco_eval_pooled_ref as pref  # noqa: E402
import coco_eval_ref as ref  # noqa: E402

NC = 6
SETS = {31: [(120, 20), (0, 5), (400, 64), (7, 0), (1003, 30), (60, 60)], 32: [(300, 128), (33, 9), (1200, 12), (90, 30)]}


def _pycocotools(frames):
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    gt_dict, dets = ref.to_coco(frames, NC)
    gt = COCO()
    gt.dataset = gt_dict
    gt.createIndex()
    e = COCOeval(gt, gt.loadRes(dets) if dets else COCO(), "bbox")
    e.params.useCats = 0
    e.params.maxDets = list(pref.MAX_DETS)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


@pytest.fixture(scope="module", params=sorted(SETS))
def case(request):
    frames = pref.make_set(request.param, SETS[request.param], NC - 1)
    return frames, _pycocotools(frames)


def test_pooled_restatement_equals_pycocotools(case):
    frames, e = case
    r = pref.run(frames)
    assert np.array_equal(e.params.iouThrs, ref.IOU_THRS) and np.array_equal(e.params.recThrs, ref.REC_THRS)
    assert e.eval["precision"].shape == r["precision"].shape
    assert np.array_equal(e.eval["precision"], r["precision"]) and np.array_equal(e.eval["recall"], r["recall"])
    assert np.array_equal(np.asarray(e.stats, np.float64), r["stats"])


@pytest.mark.gpu
def test_pooled_device_equals_pycocotools(case):
    import test_gpu_coco_eval_pooled as g
    frames, e = case
    res = g._guarded(frames, gt_capacity=128, det_capacity=1280, max_dets=pref.MAX_DETS)["_res"]
    assert np.array_equal(e.eval["precision"], res["precision"]) and np.array_equal(e.eval["recall"], res["recall"])
    assert np.array_equal(np.asarray(e.stats, np.float64), res["stats"])
