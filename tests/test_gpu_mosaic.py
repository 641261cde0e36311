"""Mosaic augmentation on the device (csrc/mosaic.hip, transforms.mosaic / DeviceMosaicStage) against the golden results of the
reference's own code (tests/golden/mosaic.npz) and the restatement pinned to them (tests/mosaic_ref.py, tests/test_mosaic_host.py).
Every comparison is exact: the canvas is integers, the boxes are single binary32 operations in the reference's order."""
import hashlib

import numpy as np
import pytest
import torch

import mosaic_ref
from mosaic_ref import SMALL, full_inputs, small_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return mosaic_ref.load_golden()


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from faster_rcnn_pytorch_amd import transforms
    return transforms


def dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run(T, imgs, boxes, labels, regions, size, max_size):
    return T.mosaic(dev(imgs), dev(boxes), dev(labels), regions, size, max_size)


def check(res, ref):
    """A MosaicResult against (canvas, boxes, labels, fallback[, regions]) of the restatement or the golden file."""
    canvas, boxes, labels, fallback = ref[:4]
    n = len(boxes)
    assert int(res.count.item()) == n and res.count.dtype == torch.int32
    assert np.array_equal(res.fallback.cpu().numpy(), fallback)
    assert np.array_equal(res.canvas_u8.cpu().numpy(), canvas)
    assert np.array_equal(res.boxes[:n].cpu().numpy(), boxes) and np.array_equal(res.labels[:n].cpu().numpy(), labels)
    assert not res.boxes[n:].any() and not res.labels[n:].any()                    # rows at and above the count are zeros
    hc, hb, hl = res.to_host()
    assert np.array_equal(hc, canvas) and np.array_equal(hb, boxes) and np.array_equal(hl, labels)


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_equal_reference_and_restatement(T, gold, name):
    inp = small_inputs(gold, name)
    res = run(T, *inp)
    check(res, (gold[name + "_canvas"], gold[name + "_boxes_out"], gold[name + "_labels_out"], gold[name + "_fallback"]))
    check(res, mosaic_ref.mosaic_ref(*inp))
    if name == "small_capped":                       # tile 0's crop ends on the last row and column of its (max_size-capped) frame
        i, j, h, w = inp[3][0]
        assert (i + h, j + w) == mosaic_ref.first_resize_hw(40, 100, 48, 100) == (40, 100) and res.fallback[0].item() == 0


def test_full_size_equals_load_mosaic(T, gold):
    res = run(T, *full_inputs(gold))
    assert hashlib.sha256(res.canvas_u8.cpu().numpy().tobytes()).digest() == gold["full_sha_canvas"].tobytes()
    n = len(gold["full_boxes_out"])
    assert int(res.count.item()) == n and np.array_equal(res.fallback.cpu().numpy(), gold["full_fallback"])
    assert np.array_equal(res.boxes[:n].cpu().numpy(), gold["full_boxes_out"]) and np.array_equal(res.labels[:n].cpu().numpy(), gold["full_labels_out"])
    assert not res.boxes[n:].any() and not res.labels[n:].any()


def synthetic(counts, seed, drop_every=3, size=48):
    """64 x 64 sources (48 x 48 after the first resize), crop (8, 8, 32, 32); box k of a tile lies inside the crop, or -- every
    drop_every-th -- wholly left of it (dropped).  Labels number the boxes, so the order is checked too."""
    rng = np.random.RandomState(seed)
    imgs = [rng.randint(0, 256, (64, 64, 3)).astype(np.uint8) for _ in range(4)]
    boxes, labels, nxt = [], [], 0
    for n in counts:
        x1, y1 = rng.uniform(12, 24, n), rng.uniform(12, 24, n)
        b = np.stack([x1, y1, x1 + rng.uniform(3, 12, n), y1 + rng.uniform(3, 12, n)], 1)
        if drop_every:
            b[drop_every - 1::drop_every, 0::2] = np.stack([rng.uniform(0, 3, n), rng.uniform(4, 8, n)], 1)[drop_every - 1::drop_every]
        boxes.append((b * (64 / 48)).astype(np.float32))
        labels.append(np.arange(nxt, nxt + n, dtype=np.int64))
        nxt += n
    return imgs, boxes, labels, np.array([[8, 8, 32, 32]] * 4, np.int32), size, 1333


@pytest.mark.parametrize("counts", [(63, 64, 65, 255), (256, 257, 700, 1), (700, 0, 257, 64)])
def test_compaction_across_wave_and_workgroup_boundaries(T, counts):
    inp = synthetic(counts, seed=sum(counts))
    ref = mosaic_ref.mosaic_ref(*inp)
    assert len(ref[1]) == sum(n - n // 3 for n in counts) and ref[3].tolist() == [int(n == 0) for n in counts]
    starts = np.cumsum((0,) + counts)
    assert ref[2].tolist() == [int(starts[t]) + k for t in range(4) for k in range(counts[t]) if k % 3 != 2]      # every third box of a tile goes
    check(run(T, *inp), ref)


def test_no_boxes_at_all(T):
    imgs, _, _, regions, size, max_size = synthetic((0, 0, 0, 0), seed=3)
    empty_b, empty_l = [np.zeros((0, 4), np.float32)] * 4, [np.zeros(0, np.int64)] * 4
    res = run(T, imgs, empty_b, empty_l, regions, size, max_size)
    ref = mosaic_ref.mosaic_ref(imgs, empty_b, empty_l, regions, size, max_size)
    assert ref[3].all() and len(ref[1]) == 0
    check(res, ref)


@pytest.mark.parametrize("flip", [False, True])
def test_stage_equals_restatement_then_final_stage(T, gold, flip):
    imgs, boxes, labels, regions, size, max_size = small_inputs(gold, "small_mixed")
    stage = T.DeviceMosaicStage(size=size, max_size=max_size, min_crop=24, out_size=80, out_max_size=133)
    x, b, lab, count, meta = stage(dev(imgs), dev(boxes), dev(labels), regions, flip=flip)
    canvas, rb, rl, fallback, _ = mosaic_ref.mosaic_ref(imgs, boxes, labels, regions, size, max_size)
    xr, br, (oh, ow) = mosaic_ref.final_stage_ref(canvas, rb, flip, 80, 133)
    n = len(rb)
    assert (oh, ow) == (80, 80) and x.shape == (1, 3, 80, 80) and meta["size"] == (80, 80) and meta["orig_size"] == (96, 96)
    assert int(count.item()) == n and np.array_equal(meta["fallback"].cpu().numpy(), fallback)
    assert np.array_equal(x[0].cpu().numpy(), xr)
    assert np.array_equal(b[:n].cpu().numpy(), br) and np.array_equal(lab[:n].cpu().numpy(), rl)
    assert b.shape == (sum(len(v) for v in boxes), 4) and bool(torch.isfinite(b).all())


def test_capture_once_replay_on_other_device_contents(T, gold):
    """The graph is captured once; the replays differ from it in device memory only -- pixels, and boxes that turn tile 1's hand-back of
    the uncropped frame into a crop and tile 0's crop into a hand-back.  A decision taken on the host at capture time would replay the
    first set's regions; a host read-back would fail the capture."""
    imgs, boxes, labels, regions, size, max_size = small_inputs(gold, "small_mixed")
    counts = [len(b) for b in boxes]
    rng = np.random.RandomState(11)
    sets = [(imgs, boxes)]
    b_crop = [b.copy() for b in boxes]
    b_crop[1] = (np.array([[22, 42, 40, 60], [25, 45, 30, 50]]) * np.array([50 / 48, 70 / 67, 50 / 48, 70 / 67])).astype(np.float32)   # inside (40, 20, 26, 28)
    b_back = [b.copy() for b in boxes]
    b_back[0] = np.tile(np.array([[1, 2, 12, 20]], np.float32), (counts[0], 1))                    # left of (5, 24, 30, 40)
    for bs in (b_crop, b_back):
        sets.append(([rng.randint(0, 256, im.shape).astype(np.uint8) for im in imgs], bs))
    refs = [mosaic_ref.mosaic_ref(im, bs, labels, regions, size, max_size) for im, bs in sets]
    assert [r[3].tolist() for r in refs] == [[0, 1, 1, 0], [0, 0, 1, 0], [1, 1, 1, 0]]
    s_imgs, s_boxes, s_labels = dev(imgs), torch.from_numpy(np.concatenate(boxes)).cuda(), torch.from_numpy(np.concatenate(labels)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.mosaic(s_imgs, s_boxes, s_labels, regions, size, max_size, counts=counts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = T.mosaic(s_imgs, s_boxes, s_labels, regions, size, max_size, counts=counts)
    for (im, bs), ref in zip(sets[1:] + sets[:1], refs[1:] + refs[:1]):
        for dst, src in zip(s_imgs, im):
            dst.copy_(torch.from_numpy(src))
        s_boxes.copy_(torch.from_numpy(np.concatenate(bs)))
        g.replay()
        check(out, ref)
        eager = run(T, im, bs, labels, regions, size, max_size)
        check(eager, ref)
        assert torch.equal(out.boxes, eager.boxes) and torch.equal(out.labels, eager.labels) and torch.equal(out.canvas_u8, eager.canvas_u8)


def test_refuses_host_tensors_and_bad_regions(T, gold):
    imgs, boxes, labels, regions, size, max_size = small_inputs(gold, "small_mixed")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.mosaic([torch.from_numpy(a) for a in imgs], dev(boxes), dev(labels), regions, size, max_size)
    bad = regions.copy()
    bad[0] = (5, 24, 30, 49)                                                       # 24 + 49 > 72
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    with pytest.raises(FrcnnError, match="outside its resized frame"):
        T.mosaic(dev(imgs), dev(boxes), dev(labels), bad, size, max_size)
