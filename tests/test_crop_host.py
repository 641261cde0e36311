"""The crop of the wired pipeline, the part that needs no device: the restatement the GPU tests compare with (tests/crop_ref.py) against
golden results made by RUNNING the reference's own functions under Pillow (tests/golden/make_golden_crop.py) and against Pillow itself,
the host-side draws, and the C ABI's refusals and declarations."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import crop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = crop_ref.case_names(crop_ref.load_golden())


@pytest.fixture(scope="module")
def gold():
    return crop_ref.load_golden()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def test_golden_file_holds_every_kind(gold):
    assert len(gold["kind_names"]) == 33 and (gold["kind_counts"] > 0).all()
    assert len(NAMES) == 30 and "center" in NAMES
    sizes = sorted(len(gold[n + "_boxes"]) for n in NAMES if n.startswith("list_") and n.endswith("_mixed"))
    assert sizes == [0, 1, 255, 256, 257, 700]
    assert len(gold["list_700_all_boxes_out"]) == 700 and len(gold["list_257_none_boxes_out"]) == 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "crop.npz")) < (1 << 20)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(gold, name):
    img, boxes, labels, area, crowd = crop_ref.crop_ref(*crop_ref.case_inputs(gold, name))
    assert np.array_equal(img, gold[name + "_img_out"]) and img.dtype == np.uint8
    assert np.array_equal(boxes, gold[name + "_boxes_out"]) and boxes.dtype == np.float32
    assert np.array_equal(labels, gold[name + "_labels_out"])
    assert np.array_equal(area, gold[name + "_area_out"]) and area.dtype == np.float32
    if int(gold[name + "_meta"][6]):
        assert np.array_equal(crowd, gold[name + "_iscrowd_out"])
    else:
        assert crowd is None
    assert not np.isnan(boxes).any() and (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()


def test_restatement_equals_the_classes_at_full_size(gold):
    img, boxes, labels, crowd = crop_ref.full_frame()
    region = tuple(int(v) for v in gold["full_region"])
    assert 384 <= region[2] <= 600 and 384 <= region[3] <= 600
    out, b, l, a, c = crop_ref.crop_ref(img, boxes, labels, crowd, (600, 800), region)
    assert sha(out) == gold["full_sha_crop"].tobytes()
    assert np.array_equal(b, gold["full_crop_boxes"]) and np.array_equal(l, gold["full_crop_labels"])
    assert np.array_equal(a, gold["full_crop_area"]) and np.array_equal(c, gold["full_crop_iscrowd"])
    from faster_rcnn_pytorch_amd.transforms import get_size
    oh, ow = get_size((region[3], region[2]), 800, 1333)
    assert (oh, ow) == tuple(gold["full_final_hw"])
    assert sha(crop_ref.resize_u8(out, (oh, ow))) == gold["full_sha_final"].tobytes()
    assert np.array_equal(crop_ref.resize_boxes(crop_ref.torch.from_numpy(b), (oh, ow), region[2:]).numpy(), gold["full_final_boxes"])


@pytest.mark.parametrize("branch", ["plain", "crop"])
@pytest.mark.parametrize("flip", [0, 1])
def test_stage_chain_restated_equals_reference(gold, branch, flip):
    """[resize, crop,] hflip, resize, ToTensor, Normalize through the reference's functions == crop_ref then final_stage_ref (no pad)."""
    img, boxes, labels = gold["stage_img"], gold["stage_boxes"], gold["stage_labels"]
    if branch == "crop":
        img, boxes, labels, _, _ = crop_ref.crop_ref(img, boxes, labels, None, tuple(gold["stage_resize_hw"]), tuple(gold["stage_region"]))
    x, b, _ = crop_ref.final_stage_ref(img, boxes, bool(flip), 48, 70, size_divisible=None)
    key = "stage_%s_flip%d" % (branch, flip)
    assert np.array_equal(x, gold[key + "_x"]) and np.array_equal(b, gold[key + "_boxes"]) and np.array_equal(labels, gold[key + "_labels"])


def test_restatement_image_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    for seed, (h, w), hw1, region in ((1, (64, 80), (48, 60), (5, 7, 30, 41)), (2, (37, 53), (61, 88), (31, 40, 30, 48)),
                                      (3, (64, 80), (20, 25), (5, 6, 9, 12)), (4, (40, 56), (40, 56), (21, 30, 19, 26)),
                                      (5, (120, 90), (33, 77), (0, 0, 33, 77))):
        img = crop_ref.seeded_case(seed, h, w, hw1, region, 0)[0]
        i, j, ch, cw = region
        pil = Image.fromarray(img, "RGB").resize((hw1[1], hw1[0]), Image.BILINEAR).crop((j, i, j + cw, i + ch))
        assert np.array_equal(crop_ref.crop_ref(img, np.zeros((0, 4), np.float32), np.zeros(0, np.int64), None, hw1, region)[0], np.array(pil))


def test_draws_and_center_crop_region(gold):
    from faster_rcnn_pytorch_amd import transforms as T
    rng = random.Random(11)
    seen_w, seen_i = set(), set()
    for _ in range(2000):
        i, j, ch, cw = T.draw_random_size_crop(56, 70, 24, 40, rng)
        assert 24 <= ch <= 40 and 24 <= cw <= 40 and 0 <= i <= 56 - ch and 0 <= j <= 70 - cw
        seen_w.add(cw), seen_i.add(i)
    assert seen_w == set(range(24, 41)) and min(seen_i) == 0 and max(seen_i) == 32                 # both ends of each range are reached
    for _ in range(200):
        i, j, ch, cw = T.draw_random_size_crop(30, 500, 24, 40, rng)                               # the frame caps the height
        assert 24 <= ch <= 30 and 24 <= cw <= 40 and 0 <= i <= 30 - ch and 0 <= j <= 500 - cw
        i, j, th, tw = T.draw_random_crop(45, 60, (40, 51), rng)
        assert (th, tw) == (40, 51) and 0 <= i <= 5 and 0 <= j <= 9
    assert T.draw_random_crop(45, 60, (45, 60), rng) == (0, 0, 45, 60)
    with pytest.raises(ValueError):
        T.draw_random_size_crop(20, 70, 24, 40, rng)
    with pytest.raises(ValueError):
        T.draw_random_crop(45, 60, (46, 60), rng)
    # CenterCrop: the golden case's region came out of the reference's class, both offsets on a half (2.5 -> 2, 4.5 -> 4)
    assert T.center_crop_region(45, 60, (40, 51)) == tuple(int(v) for v in gold["center_meta"][2:6]) == (2, 4, 40, 51)
    assert T.center_crop_region(47, 64, (40, 51)) == (4, 6, 40, 51)                                # 3.5 -> 4, 6.5 -> 6
    for h in range(40, 60):
        for w in range(51, 70):
            assert T.center_crop_region(h, w, (40, 51)) == crop_ref.center_crop_region(h, w, (40, 51))
    # the stage's plan: the recipe's order of draws, every field inside its range
    stage = T.DeviceMultiScaleStage(scales=(480, 512, 544), max_size=1333)
    branches = set()
    for _ in range(400):
        p = stage.draw(480, 640, rng)
        assert p.size in (480, 512, 544) and isinstance(p.flip, bool)
        branches.add(p.region is None)
        if p.region is not None:
            H1, W1 = p.resize_hw
            assert (H1, W1) in ((400, 533), (500, 666), (600, 800))
            i, j, ch, cw = p.region
            assert 384 <= ch <= min(H1, 600) and 384 <= cw <= min(W1, 600) and 0 <= i <= H1 - ch and 0 <= j <= W1 - cw
    assert branches == {True, False}


def test_cabi_refuses_bad_arguments_without_a_device():
    from faster_rcnn_pytorch_amd import _lib
    L = _lib.lib
    buf = (C.c_uint8 * (11 << 14))()                                       # host memory behind every "device" pointer: a refusal never touches it
    a = C.addressof(buf)
    src, out, boxes, boxes_out, labels, labels_out, crowd, crowd_out, area_out, count, ws = (C.c_void_p(a + (k << 14)) for k in range(11))
    base = dict(src=src, h=40, w=56, H1=61, W1=88, i=9, j=14, ch=30, cw=41, boxes=boxes, labels=labels, crowd=crowd, n=5, count_in=None, out=out,
                boxes_out=boxes_out, labels_out=labels_out, area_out=area_out, crowd_out=crowd_out, count=count, ws=ws, nbytes=1 << 40)

    def call(**kw):
        v = dict(base, **kw)
        return L.frcnn_resize_crop(v["src"], v["h"], v["w"], v["H1"], v["W1"], v["i"], v["j"], v["ch"], v["cw"], v["boxes"], v["labels"], v["crowd"],
                                   v["n"], v["count_in"], v["out"], v["boxes_out"], v["labels_out"], v["area_out"], v["crowd_out"], v["count"], v["ws"],
                                   v["nbytes"], None)

    need = L.frcnn_resize_crop_workspace(40, 56, 61, 88, 30, 41)
    assert need >= 30 * 41 * 3 and need < 40 * 88 * 3                # less than the whole frame's intermediate alone: only the region's share
    assert call(nbytes=need - 1) == -3 and b"workspace" in L.frcnn_last_error()                    # everything valid but the workspace
    assert call(nbytes=0) == -3
    assert call(nbytes=0, n=-1) == -1 and b"n = -1" in L.frcnn_last_error()
    for kw in (dict(src=None), dict(out=None), dict(count=None), dict(ws=None), dict(boxes=None), dict(labels=None), dict(boxes_out=None),
               dict(labels_out=None)):
        assert call(nbytes=0, **kw) == -1 and b"NULL" in L.frcnn_last_error(), kw
    for kw in (dict(crowd=None), dict(crowd_out=None)):
        assert call(nbytes=0, **kw) == -1 and b"iscrowd" in L.frcnn_last_error(), kw
    assert call(nbytes=0, crowd=None, crowd_out=None, area_out=None) == -3                         # both optional lists left out
    for kw in (dict(i=-1), dict(j=-1), dict(i=32), dict(j=48), dict(ch=62, i=0), dict(cw=89, j=0), dict(ch=53), dict(cw=75)):
        assert call(nbytes=0, **kw) == -1 and b"outside the resized frame" in L.frcnn_last_error(), kw
    for kw in (dict(i=31), dict(j=47), dict(i=0, j=0, ch=61, cw=88)):                             # ending on the last row / column is inside
        assert call(nbytes=0, **kw) == -3, kw
    for kw in (dict(ch=0), dict(cw=0), dict(ch=-3)):
        assert call(nbytes=0, **kw) == -1 and b"must be >= 1" in L.frcnn_last_error(), kw
    for kw in (dict(h=0), dict(w=0), dict(H1=0), dict(W1=0), dict(h=1 << 15), dict(w=1 << 15), dict(H1=1 << 15), dict(W1=1 << 15)):
        assert call(nbytes=0, **kw) == -1 and b"1 .. 32767" in L.frcnn_last_error(), kw
    assert call(nbytes=0, H1=32767, W1=32767) == -3
    assert call(nbytes=0, boxes=C.c_void_p(boxes.value + 4)) == -1 and b"aligned" in L.frcnn_last_error()
    assert call(nbytes=0, boxes_out=boxes) == -1 and b"overlaps" in L.frcnn_last_error()
    assert call(nbytes=0, out=src) == -1 and b"overlaps" in L.frcnn_last_error()
    assert call(nbytes=0, n=0, boxes=None, labels=None, crowd=None, boxes_out=None, labels_out=None, crowd_out=None, area_out=None) == -3
    for bad in ((0, 56, 61, 88, 30, 41), (40, 56, 61, 1 << 15, 30, 41), (40, 56, 61, 88, 62, 41), (40, 56, 61, 88, 30, 0)):
        assert L.frcnn_resize_crop_workspace(*bad) == 0, bad
    # the workspace follows the region, and a plain crop's is sized by the same rule
    assert L.frcnn_resize_crop_workspace(480, 640, 600, 800, 384, 384) < L.frcnn_resize_crop_workspace(480, 640, 600, 800, 600, 600)
    assert L.frcnn_resize_crop_workspace(48, 64, 48, 64, 20, 30) > 0


def test_header_exports_and_binding_agree_for_the_new_symbols():
    from faster_rcnn_pytorch_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("frcnn_resize_crop", "frcnn_resize_crop_workspace"):
        m = re.search(r"\b(\w+)\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, "%s is not declared in the header" % name
        assert re.search(r" T %s\n" % name, exported), "%s is not exported" % name
        res, args = _lib.SIGNATURES[name]
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                               # pointers bind as void *, int64_t / size_t / int by their width
            want = C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_size_t if p.startswith("size_t") else C.c_int
            assert a is want, (name, p, a)
        assert res is (C.c_size_t if m.group(1) == "size_t" else C.c_int)
    assert _lib.lib.frcnn_abi_version() == 7
