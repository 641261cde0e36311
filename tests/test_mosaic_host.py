"""Mosaic augmentation, the part that needs no device: the restatement the GPU tests compare with (tests/mosaic_ref.py) against
golden results made by RUNNING the reference's own functions under Pillow (tests/golden/make_golden_mosaic.py), the host-side
size logic and region draw, and the C ABI's refusals."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import mosaic_ref

from mosaic_ref import SMALL, full_inputs, small_inputs


@pytest.fixture(scope="module")
def gold():
    return mosaic_ref.load_golden()


def test_golden_file_holds_every_adverse_kind(gold):
    assert sorted(gold["small_names"].tolist()) == sorted(SMALL)
    assert len(gold["adverse_names"]) == 17 and (gold["adverse_counts"] > 0).all()


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_reference_small(gold, name):
    canvas, boxes, labels, fallback, _ = mosaic_ref.mosaic_ref(*small_inputs(gold, name))
    assert np.array_equal(canvas, gold[name + "_canvas"])
    assert np.array_equal(boxes, gold[name + "_boxes_out"]) and boxes.dtype == np.float32
    assert np.array_equal(labels, gold[name + "_labels_out"])
    assert np.array_equal(fallback, gold[name + "_fallback"])


def test_restatement_equals_load_mosaic_full_size(gold):
    canvas, boxes, labels, fallback, _ = mosaic_ref.mosaic_ref(*full_inputs(gold))
    assert canvas.shape == (1200, 1200, 3)
    assert hashlib.sha256(np.ascontiguousarray(canvas).tobytes()).digest() == gold["full_sha_canvas"].tobytes()
    assert np.array_equal(boxes, gold["full_boxes_out"]) and np.array_equal(labels, gold["full_labels_out"])
    assert np.array_equal(fallback, gold["full_fallback"])


def test_size_logic_and_region_draw():
    from faster_rcnn_pytorch_amd import transforms as T
    # worked by hand from transforms_.py:93-114
    assert T.mosaic_resize_hw(375, 500, 600) == (600, 800) and T.mosaic_resize_hw(500, 375, 600) == (800, 600)
    assert T.mosaic_resize_hw(300, 1000, 600) == (400, 1333)          # 600 / 300 * 1000 > 1333 -> size = round(399.9) = 400
    assert T.mosaic_resize_hw(40, 100, 48, 100) == (40, 100) and T.mosaic_resize_hw(64, 64, 48) == (48, 48)
    for h in range(30, 200, 7):
        for w in range(30, 400, 11):
            for size, cap in ((48, 100), (48, 1333), (600, 1333), (37, None)):
                assert T.mosaic_resize_hw(h, w, size, cap) == mosaic_ref.first_resize_hw(h, w, size, cap)
    stage = T.DeviceMosaicStage()
    rng = random.Random(7)
    shapes = [(375, 500), (500, 375), (480, 640), (300, 1000)]
    for _ in range(250):                                               # 1 000 regions
        for (h, w), (i, j, ch, cw) in zip(shapes, stage.draw_regions(shapes, rng)):
            H1, W1 = T.mosaic_resize_hw(h, w, 600, 1333)
            assert 384 <= ch <= min(H1, 600) and 384 <= cw <= min(W1, 600) and 0 <= i <= H1 - ch and 0 <= j <= W1 - cw
    with pytest.raises(ValueError):
        stage.draw_regions([(100, 1000)])                              # capped to 133 x 1333: no room for a 384 crop


def test_cabi_refuses_bad_arguments_without_a_device():
    from faster_rcnn_pytorch_amd import _lib
    L = _lib.lib
    buf = (C.c_uint8 * 4096)()                                         # host memory behind every "device" pointer: a refusal never touches it
    p = C.cast(buf, C.c_void_p)
    srcs = (C.c_void_p * 4)(p, p, p, p)
    hw = np.array([[40, 60], [70, 50], [64, 64], [100, 130]], np.int32)           # -> 48 x 72, 67 x 48, 48 x 48, 48 x 62 at size 48
    reg = np.array([[5, 24, 30, 40], [40, 20, 26, 28], [0, 0, 24, 24], [0, 0, 48, 62]], np.int32)
    offs = np.array([0, 2, 2, 3, 5], np.int32)

    def call(srcs=srcs, hw=hw, size=48, max_size=1333, reg=reg, offs=offs, boxes=p, count=p, ws=p, nbytes=1 << 40):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a        # noqa: E731
        return L.frcnn_mosaic(srcs, ptr(hw), size, max_size, ptr(reg), boxes, p, ptr(offs), p, p, p, count, p, ws, nbytes, None)

    need = L.frcnn_mosaic_workspace(hw.ctypes.data_as(C.c_void_p), 48, 1333)
    assert need > 4 * (48 * 72 * 3)
    assert call(nbytes=need - 1) == -3 and b"workspace" in L.frcnn_last_error()                # everything valid but the workspace
    assert call(nbytes=0) == -3
    for kw in (dict(srcs=None), dict(hw=None), dict(reg=None), dict(offs=None), dict(count=None), dict(ws=None),
               dict(srcs=(C.c_void_p * 4)(p, p, None, p)), dict(boxes=None)):
        assert call(nbytes=0, **kw) == -1 and b"NULL" in L.frcnn_last_error(), kw
    for t, bad in ((0, [5, 24, 30, 49]), (0, [19, 24, 30, 40]), (1, [40, 20, 28, 28]), (2, [-1, 0, 24, 24]), (3, [0, -1, 48, 62]),
                   (3, [0, 0, 49, 62]), (3, [0, 1, 48, 62])):
        r = reg.copy()
        r[t] = bad
        assert call(nbytes=0, reg=r) == -1 and b"outside its resized frame" in L.frcnn_last_error(), bad
    for bad in ([5, 24, 0, 40], [5, 24, 30, 0], [5, 24, -3, 40]):
        r = reg.copy()
        r[0] = bad
        assert call(nbytes=0, reg=r) == -1 and b"must be >= 1" in L.frcnn_last_error(), bad
    for bad in ([0, 2, 1, 3, 5], [1, 2, 2, 3, 5], [0, 2, 2, 3, 2]):
        assert call(nbytes=0, offs=np.array(bad, np.int32)) == -1 and b"tile_offsets" in L.frcnn_last_error(), bad
    for bad in ([1 << 15, 60], [40, 1 << 15]):
        h2 = hw.copy()
        h2[1] = bad
        assert call(nbytes=0, hw=h2) == -1 and b"too large" in L.frcnn_last_error()
        assert L.frcnn_mosaic_workspace(h2.ctypes.data_as(C.c_void_p), 48, 1333) == 0
    assert call(nbytes=0, size=1 << 14) == -1 and call(nbytes=0, size=0) == -1
    assert L.frcnn_mosaic_workspace(None, 48, 1333) == 0
    # N = 0 needs no box pointers: the only complaint left is the workspace
    assert L.frcnn_mosaic(srcs, hw.ctypes.data_as(C.c_void_p), 48, 1333, reg.ctypes.data_as(C.c_void_p), None, None,
                          np.zeros(5, np.int32).ctypes.data_as(C.c_void_p), p, None, None, p, p, p, 0, None) == -3
    # the library's own size logic is the one Python and the restatement use: a region that fills the resized frame passes, one more row does not
    for h, w, size, cap in ((40, 100, 48, 100), (300, 1000, 600, 1333), (333, 500, 600, 1333), (111, 170, 37, 0)):
        H1, W1 = mosaic_ref.first_resize_hw(h, w, size, cap or None)
        h2, r = hw.copy(), reg.copy()
        h2[0], r[0] = (h, w), (0, 0, H1, W1)
        r[1:] = (0, 0, 1, 1)
        assert call(nbytes=0, hw=h2, reg=r, size=size, max_size=cap) == -3
        r[0] = (0, 0, H1 + 1, W1)
        assert call(nbytes=0, hw=h2, reg=r, size=size, max_size=cap) == -1
        r[0] = (0, 0, H1, W1 + 1)
        assert call(nbytes=0, hw=h2, reg=r, size=size, max_size=cap) == -1
