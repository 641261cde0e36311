"""The crop of the wired pipeline on the device (csrc/crop.hip, transforms.crop / DeviceMultiScaleStage) against the golden results of the
reference's own code (tests/golden/crop.npz) and the restatement pinned to them (tests/crop_ref.py, tests/test_crop_host.py).
Every comparison is exact: the image is integers, the boxes are single binary32 operations in the reference's order."""
import hashlib
import random

import numpy as np
import pytest
import torch

import crop_ref

pytestmark = pytest.mark.gpu
NAMES = crop_ref.case_names(crop_ref.load_golden())


@pytest.fixture(scope="module")
def gold():
    return crop_ref.load_golden()


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from faster_rcnn_pytorch_amd import transforms
    return transforms


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(T, img, boxes, labels, crowd, resize_hw, region, count=None):
    return T.crop(dev(img), dev(boxes), dev(labels), region, resize_hw, iscrowd=dev(crowd), count=count)


def check(res, ref, n_in):
    """A CropResult (or the same six tensors) against (image, boxes, labels, area, iscrowd or None)."""
    img, boxes, labels, area, crowd = ref
    img_d, b_d, l_d, a_d, c_d, count = res
    n = len(boxes)
    assert count.dtype == torch.int32 and int(count.item()) == n
    assert img_d.dtype == torch.uint8 and np.array_equal(img_d.cpu().numpy(), img)
    assert b_d.shape == (n_in, 4) and l_d.shape == (n_in,) and a_d.shape == (n_in,)
    assert np.array_equal(b_d[:n].cpu().numpy(), boxes) and np.array_equal(l_d[:n].cpu().numpy(), labels)
    assert np.array_equal(a_d[:n].cpu().numpy(), area)
    for t in (b_d, l_d, a_d):                                                       # rows at and above the count are zeros, not NaN, not 0xFF
        assert int(torch.count_nonzero(t[n:])) == 0 and not bool(torch.isnan(t[n:].float()).any())
    if crowd is None:
        assert c_d is None
    else:
        assert c_d.shape == (n_in,) and np.array_equal(c_d[:n].cpu().numpy(), crowd) and int(torch.count_nonzero(c_d[n:])) == 0


def raw(img, boxes, labels, crowd, resize_hw, region, count_in=None):
    """The C ABI itself, every output buffer prefilled with 0xFF bytes / NaN."""
    from faster_rcnn_pytorch_amd import _lib
    from faster_rcnn_pytorch_amd.ops import _ptr, _stream
    img_d, b_d, l_d, c_d = dev(img), dev(np.asarray(boxes, np.float32).reshape(-1, 4)), dev(labels), dev(crowd)
    h, w = img.shape[:2]
    H1, W1 = resize_hw or (h, w)
    i, j, ch, cw = region
    n = len(boxes)
    out = torch.full((ch, cw, 3), 0xFF, dtype=torch.uint8, device="cuda")
    b_o = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
    a_o = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    l_o = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    c_o = None if crowd is None else torch.full((n,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nb = int(_lib.lib.frcnn_resize_crop_workspace(h, w, H1, W1, ch, cw))
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.frcnn_resize_crop(_ptr(img_d), h, w, H1, W1, i, j, ch, cw, _ptr(b_d), _ptr(l_d), _ptr(c_d), n, _ptr(count_in), _ptr(out),
                                          _ptr(b_o), _ptr(l_o), _ptr(a_o), _ptr(c_o), _ptr(cnt), _ptr(ws), nb, _stream()), "resize_crop")
    return out, b_o, l_o, a_o, c_o, cnt


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases_equal_reference_and_restatement(T, gold, name):
    inp = crop_ref.case_inputs(gold, name)
    ref_gold = (gold[name + "_img_out"], gold[name + "_boxes_out"], gold[name + "_labels_out"], gold[name + "_area_out"],
                gold[name + "_iscrowd_out"] if inp[3] is not None else None)
    ref = crop_ref.crop_ref(*inp)
    n = len(inp[1])
    plain = not int(gold[name + "_meta"][8])
    res = run(T, inp[0], inp[1], inp[2], inp[3], None if plain else inp[4], inp[5])
    check(res, ref_gold, n)
    check(res, ref, n)
    check(raw(*inp), ref_gold, n)
    hi, hb, hl, ha, hc = res.to_host()
    assert np.array_equal(hi, ref_gold[0]) and np.array_equal(hb, ref_gold[1]) and np.array_equal(hl, ref_gold[2]) and np.array_equal(ha, ref_gold[3])
    assert (hc is None) == (inp[3] is None)


# (h, w), (H1, W1), region, boxes: more than one 256-column block, odd sizes, a strong down-scale, up- and down-scaling mixed, one axis equal
SEEDED = [((200, 400), (300, 620), (17, 33, 280, 555), 300), ((199, 333), (67, 111), (5, 9, 60, 100), 37), ((61, 97), (183, 50), (100, 3, 83, 47), 513),
          ((480, 640), (600, 800), (83, 117, 399, 465), 64), ((120, 300), (120, 450), (0, 150, 120, 300), 5), ((90, 70), (31, 70), (30, 0, 1, 70), 1)]


@pytest.mark.parametrize("k", range(len(SEEDED)))
def test_seeded_frames_equal_restatement_and_windowed_equals_full_resize_sliced(T, k):
    hw, hw1, region, n = SEEDED[k]
    img, boxes, labels, crowd = crop_ref.seeded_case(50 + k, hw[0], hw[1], hw1, region, n)
    ref = crop_ref.crop_ref(img, boxes, labels, crowd, hw1, region)
    assert len(ref[1]) <= n and (n < 5 or 0 < len(ref[1]) < n)
    res = run(T, img, boxes, labels, crowd, hw1, region)
    check(res, ref, n)
    check(raw(img, boxes, labels, crowd, hw1, region), ref, n)
    i, j, ch, cw = region
    full = run(T, img, boxes, labels, crowd, hw1, (0, 0) + hw1)                     # the whole resized frame through the same kernels
    assert torch.equal(full.img_u8[i:i + ch, j:j + cw], res.img_u8)
    assert np.array_equal(full.img_u8.cpu().numpy(), crop_ref.resize_u8(img, hw1))


@pytest.mark.parametrize("resize_hw", [None, (97, 203)])
def test_equal_size_is_a_byte_copy(T, resize_hw):
    img, boxes, labels, crowd = crop_ref.seeded_case(9, 97, 203, None, (13, 29, 71, 150), 40)
    d = dev(img)
    for region in ((13, 29, 71, 150), (0, 0, 97, 203), (96, 202, 1, 1), (0, 0, 1, 203)):
        i, j, ch, cw = region
        res = T.crop(d, dev(boxes), dev(labels), region, resize_hw)
        assert torch.equal(res.img_u8, d[i:i + ch, j:j + cw])
        check(res, crop_ref.crop_ref(img, boxes, labels, None, resize_hw, region), 40)


def test_a_device_count_hides_the_rows_behind_it(T):
    hw, hw1, region, n = (48, 64), (60, 80), (12, 16, 30, 40), 600
    img, boxes, labels, crowd = crop_ref.seeded_case(21, hw[0], hw[1], hw1, region, n)
    boxes[300:] = np.nan                                                            # rows behind the count may hold anything
    for live, eff in ((0, 0), (1, 1), (255, 255), (256, 256), (300, 300), (-5, 0)):
        cnt = torch.tensor([live], dtype=torch.int32, device="cuda")
        ref = crop_ref.crop_ref(img, boxes, labels, crowd, hw1, region, live=eff)
        check(run(T, img, boxes, labels, crowd, hw1, region, count=cnt), ref, n)
        check(raw(img, boxes, labels, crowd, hw1, region, count_in=cnt), ref, n)
    ok = boxes.copy()
    ok[300:] = boxes[:300]
    cnt = torch.tensor([100000], dtype=torch.int32, device="cuda")                  # a count above n is n
    check(run(T, img, ok, labels, crowd, hw1, region, count=cnt), crop_ref.crop_ref(img, ok, labels, crowd, hw1, region), n)


@pytest.mark.parametrize("branch", ["plain", "crop"])
@pytest.mark.parametrize("flip", [False, True])
def test_stage_equals_reference_chain(T, gold, branch, flip):
    img, boxes, labels = gold["stage_img"], gold["stage_boxes"], gold["stage_labels"]
    stage = T.DeviceMultiScaleStage(scales=(48,), max_size=70, crop_sizes=(56,), crop_min=24, crop_max=40)
    hw1, region = tuple(int(v) for v in gold["stage_resize_hw"]), tuple(int(v) for v in gold["stage_region"])
    plan = T.MultiScalePlan(flip, hw1, region, 48) if branch == "crop" else T.MultiScalePlan(flip, None, None, 48)
    x, b, lab, count, meta = stage(dev(img), dev(boxes), dev(labels), plan)
    key = "stage_%s_flip%d" % (branch, int(flip))
    xr, br, lr = gold[key + "_x"], gold[key + "_boxes"], gold[key + "_labels"]
    n = len(br)
    oh, ow = xr.shape[1:]
    assert meta["size"] == (oh, ow) and x.shape == (1, 3) + meta["padded"] and meta["padded"] == ((oh + 31) // 32 * 32, (ow + 31) // 32 * 32)
    assert int(count.item()) == n and (n == len(boxes)) == (branch == "plain")
    assert np.array_equal(x[0, :, :oh, :ow].cpu().numpy(), xr)
    assert int(torch.count_nonzero(x[0, :, oh:])) == 0 and int(torch.count_nonzero(x[0, :, :, ow:])) == 0
    assert np.array_equal(b[:n].cpu().numpy(), br) and np.array_equal(lab[:n].cpu().numpy(), lr)
    assert b.shape == (len(boxes), 4) and bool(torch.isfinite(b).all())             # the padding rows are zeros all the way through
    # and the restatement of the same chain, pad included
    ci, cb = (img, boxes) if branch == "plain" else crop_ref.crop_ref(img, boxes, labels, None, hw1, region)[:2]
    xs, bs, _ = crop_ref.final_stage_ref(ci, cb, flip, 48, 70)
    assert np.array_equal(x[0].cpu().numpy(), xs) and np.array_equal(b[:n].cpu().numpy(), bs)
    drawn = stage.draw(64, 80, random.Random(3 + int(flip)))
    out = stage(dev(img), dev(boxes), dev(labels), drawn)                           # a drawn plan runs
    assert out[0].shape[:2] == (1, 3) and int(out[3].item()) <= len(boxes)


def test_full_size_crop_branch_equals_the_classes(T, gold):
    img, boxes, labels, crowd = crop_ref.full_frame()
    region = tuple(int(v) for v in gold["full_region"])
    res = run(T, img, boxes, labels, crowd, (600, 800), region)
    assert hashlib.sha256(res.img_u8.cpu().numpy().tobytes()).digest() == gold["full_sha_crop"].tobytes()
    n = len(gold["full_crop_boxes"])
    assert int(res.count.item()) == n
    assert np.array_equal(res.boxes[:n].cpu().numpy(), gold["full_crop_boxes"]) and np.array_equal(res.labels[:n].cpu().numpy(), gold["full_crop_labels"])
    assert np.array_equal(res.area[:n].cpu().numpy(), gold["full_crop_area"]) and np.array_equal(res.iscrowd[:n].cpu().numpy(), gold["full_crop_iscrowd"])
    oh, ow = (int(v) for v in gold["full_final_hw"])
    _, u8 = T.preprocess_image(res.img_u8, (oh, ow), want_u8=True)
    assert hashlib.sha256(u8.cpu().numpy().tobytes()).digest() == gold["full_sha_final"].tobytes()


def test_capture_once_replay_on_another_frame(T):
    """Captured once, replayed on a second frame of the same shape with other boxes: the survivors are counted on the device at replay time."""
    hw, hw1, region, n = (64, 80), (56, 70), (9, 21, 33, 38), 300
    sets = [crop_ref.seeded_case(s, hw[0], hw[1], hw1, region, n) for s in (31, 32)]
    sets[1][1][::2, 0::2] -= 200.0                                                  # the second frame loses half its boxes to the left
    refs = [crop_ref.crop_ref(im, b, l, c, hw1, region) for im, b, l, c in sets]
    assert len(refs[0][1]) != len(refs[1][1]) and min(len(refs[0][1]), len(refs[1][1])) > 0
    s_img, s_b, s_l, s_c = (dev(a) for a in sets[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.crop(s_img, s_b, s_l, region, hw1, iscrowd=s_c)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = T.crop(s_img, s_b, s_l, region, hw1, iscrowd=s_c)
    counts = []
    for (im, b, l, c), ref in zip(sets[::-1], refs[::-1]):
        s_img.copy_(torch.from_numpy(im)), s_b.copy_(torch.from_numpy(b)), s_l.copy_(torch.from_numpy(l)), s_c.copy_(torch.from_numpy(c))
        g.replay()
        check(out, ref, n)
        eager = run(T, im, b, l, c, hw1, region)
        for t_g, t_e in zip(out, eager):
            assert torch.equal(t_g, t_e)
        counts.append(int(out.count.item()))
    assert counts[0] != counts[1]


def test_refusals_raise(T):
    from faster_rcnn_pytorch_amd import _lib
    img, boxes, labels, crowd = crop_ref.seeded_case(3, 40, 56, (61, 88), (9, 14, 30, 41), 8)
    d, b, l = dev(img), dev(boxes), dev(labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.crop(torch.from_numpy(img), b, l, (9, 14, 30, 41), (61, 88))
    for region in ((9, 14, 30, 75), (32, 14, 30, 41), (-1, 14, 30, 41), (0, 0, 62, 88)):
        with pytest.raises(_lib.FrcnnError, match="outside the resized frame"):
            T.crop(d, b, l, region, (61, 88))
    with pytest.raises(_lib.FrcnnError, match="outside the resized frame"):
        T.crop(d, b, l, (9, 14, 30, 43))                                            # a plain crop: the frame itself is 40 x 56
    for region in ((9, 14, 0, 41), (9, 14, 30, -2)):
        with pytest.raises(_lib.FrcnnError, match="must be >= 1"):
            T.crop(d, b, l, region, (61, 88))
    for hw1 in ((0, 88), (61, 1 << 15)):
        with pytest.raises(_lib.FrcnnError, match="1 .. 32767"):
            T.crop(d, b, l, (0, 0, 1, 1), hw1)
    with pytest.raises(ValueError, match="rows"):
        T.crop(d, b, l[:5], (9, 14, 30, 41), (61, 88))
    from faster_rcnn_pytorch_amd.ops import _ptr, _stream
    out, cnt, ws = torch.empty((30, 41, 3), dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    need = int(_lib.lib.frcnn_resize_crop_workspace(40, 56, 61, 88, 30, 41))
    args = (_ptr(d), 40, 56, 61, 88, 9, 14, 30, 41, None, None, None, 0, None, _ptr(out), None, None, None, None, _ptr(cnt), _ptr(ws))
    assert _lib.lib.frcnn_resize_crop(*args, need - 1, _stream()) == -3 and b"workspace" in _lib.lib.frcnn_last_error()
    assert _lib.lib.frcnn_resize_crop(*args, need, _stream()) == 0 and int(cnt.item()) == 0          # n = 0 with a workspace of exactly the size asked
    assert np.array_equal(out.cpu().numpy(), crop_ref.crop_ref(img, boxes[:0], labels[:0], None, (61, 88), (9, 14, 30, 41))[0])
