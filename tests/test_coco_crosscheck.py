"""pycocotools' own COCOeval against the restatement (tests/coco_eval_ref.py) and the device evaluator, exactly, on the synthetic sets of
tests/test_gpu_coco_eval.py.  Runs wherever pycocotools can be imported and is SKIPPED elsewhere (the skip reason says so): the COCO
protocol of this project is restated from the published algorithm and stays unpinned until this file has run (docs/PARITY.md)."""
import numpy as np
import pytest

pycocotools = pytest.importorskip("pycocotools", reason="pycocotools is not installed: the COCO protocol stays unpinned (docs/PARITY.md)")

import coco_eval_ref as ref  # noqa: E402

SETS = {21: dict(num_classes=7, max_gt=24), 22: dict(num_classes=9, max_gt=128)}


def _pycocotools(frames, num_classes):
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    gt_dict, dets = ref.to_coco(frames, num_classes)
    gt = COCO()
    gt.dataset = gt_dict
    gt.createIndex()
    e = COCOeval(gt, gt.loadRes(dets), "bbox")
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


@pytest.fixture(scope="module", params=sorted(SETS))
def case(request):
    kw = SETS[request.param]
    frames = ref.make_set(request.param, n_images=20, **kw)
    return frames, kw["num_classes"], _pycocotools(frames, kw["num_classes"])


def test_restatement_equals_pycocotools(case):
    frames, nc, e = case
    r = ref.run(frames, nc)
    assert np.array_equal(e.params.iouThrs, ref.IOU_THRS) and np.array_equal(e.params.recThrs, ref.REC_THRS)
    assert np.array_equal(e.eval["precision"], r["precision"]) and np.array_equal(e.eval["recall"], r["recall"])
    assert np.array_equal(np.asarray(e.stats, np.float64), r["stats"])


@pytest.mark.gpu
def test_device_equals_pycocotools(case):
    import test_gpu_coco_eval as g
    frames, nc, e = case
    res = g._run(frames, nc, det_capacity=320).summarize()
    assert np.array_equal(e.eval["precision"], res["precision"]) and np.array_equal(e.eval["recall"], res["recall"])
    assert np.array_equal(np.asarray(e.stats, np.float64), res["stats"])
