"""Photometric distortion and zoom-out on the device (csrc/photometric.hip; transforms.photometric_distort / zoom_out /
DeviceAugmentStage) against the results of the reference's own code under Pillow (tests/golden/photometric.npz) and the restatement
pinned to them (tests/photometric_ref.py, tests/test_photometric_host.py).  Every comparison is exact: the outputs are bytes, the boxes
one binary32 addition."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import photometric_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from faster_rcnn_pytorch_amd import transforms
    return transforms


@pytest.fixture(scope="module")
def L(T):
    from faster_rcnn_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def cube_dev(T):
    return torch.from_numpy(R.cube()).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(f):
    return int(np.array(f, np.float32).view(np.int32))


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_photometric(L, img, plan, ws=None):
    """The C ABI itself; output and workspace prefilled with 0xFF."""
    h, w = img.shape[:2]
    nb = int(L.lib.frcnn_photometric_workspace(h, w))
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda") if ws is None else ws
    out = torch.full_like(img, 0xFF)
    L.check(L.lib.frcnn_photometric(vp(img), h, w, vp(plan), vp(out), vp(ws), nb, stream()), "photometric")
    return out


def raw_zoom_out(L, img, boxes, new_hw, top_left):
    h, w = img.shape[:2]
    nb = int(L.lib.frcnn_zoom_out_workspace(h, w, int(new_hw[0]), int(new_hw[1])))
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    canvas = torch.full((int(new_hw[0]), int(new_hw[1]), 3), 0xFF, dtype=torch.uint8, device="cuda")
    n = int(boxes.shape[0])
    bo = torch.full_like(boxes, float("nan"))
    L.check(L.lib.frcnn_zoom_out(vp(img), h, w, int(new_hw[0]), int(new_hw[1]), int(top_left[0]), int(top_left[1]), vp(boxes) if n else None, n,
                                 vp(canvas), vp(bo) if n else None, vp(ws), nb, stream()), "zoom_out")
    return canvas, bo


def expect_photometric(gold, name, out):
    out = out.cpu().numpy()
    if name + "_out" in gold.files:
        assert np.array_equal(out, gold[name + "_out"]), name
    else:
        if hashlib.sha256(out.tobytes()).digest() != gold[name + "_sha"].tobytes():
            ref = R.photometric(R.case_input(gold, name), gold[name + "_order"], gold[name + "_factors"])
            bad = np.argwhere((out != ref).any(-1))
            raise AssertionError("%s: %d pixels differ, the first at %s" % (name, len(bad), bad[:1].tolist()))


def test_every_photometric_golden_case_through_the_package_and_the_c_abi(T, L, gold):
    for name in gold["p_names"].tolist():
        img = dev(R.case_input(gold, name))
        plan = T.photometric_plan(gold[name + "_order"].tolist(), gold[name + "_factors"])
        expect_photometric(gold, name, T.photometric_distort(img, plan))
        expect_photometric(gold, name, T.photometric_distort(img, dev(plan)))
        expect_photometric(gold, name, raw_photometric(L, img, dev(plan)))


def test_every_zoom_out_golden_case_through_the_package_and_the_c_abi(T, L, gold):
    for name in gold["z_names"].tolist():
        img, boxes = dev(gold[name + "_img"]), dev(gold[name + "_boxes"])
        for canvas, bo in (T.zoom_out(img, boxes, gold[name + "_new_hw"], gold[name + "_top_left"]),
                           raw_zoom_out(L, img, boxes, gold[name + "_new_hw"], gold[name + "_top_left"])):
            assert np.array_equal(canvas.cpu().numpy(), gold[name + "_canvas"]), name
            assert np.array_equal(bo.cpu().numpy(), gold[name + "_boxes_out"]), name
    canvas, bo = T.zoom_out(dev(gold["z_origin_img"]), None, gold["z_origin_new_hw"], gold["z_origin_top_left"])
    assert bo is None and np.array_equal(canvas.cpu().numpy(), gold["z_origin_canvas"])


CUBE = [("hue_0", (R.HUE, 0)), ("hue_13", (R.HUE, 13)), ("hue_243", (R.HUE, 243)), ("saturation_0.5", (R.SATURATION, bits(0.5))),
        ("saturation_1.0", (R.SATURATION, bits(1.0))), ("saturation_1.5", (R.SATURATION, bits(1.5))), ("brightness_0.5", (R.BRIGHTNESS, bits(0.5))),
        ("brightness_1.5", (R.BRIGHTNESS, bits(1.5)))]


@pytest.mark.parametrize("name,slot", CUBE, ids=[c[0] for c in CUBE])
def test_every_colour_equals_pillow(T, gold, cube_dev, name, slot):
    plan = np.array([slot[0], slot[1], -1, 0, -1, 0, -1, 0], np.int32)
    out = T.photometric_distort(cube_dev, dev(plan)).cpu().numpy()
    if hashlib.sha256(out.tobytes()).digest() != gold["cube_" + name].tobytes():
        ref = R.apply_plan(R.cube(), plan)                                   # only to say where
        bad = np.argwhere((out != ref).any(-1))
        raise AssertionError("%s: %d colours differ from the restatement, the first at %s" % (name, len(bad), bad[:1].tolist()))


def test_two_frames_back_to_back_on_one_workspace(L, gold):
    a, b = dev(R.seeded_frame(31, 75, 93)), dev(np.full((75, 93, 3), 255, np.uint8))
    pa, pb = R.plan((2, 1, 0, 3), {0: 1.3, 1: 0.6, 2: 0.9, 3: 0.04}), R.plan((0, 3, 1, 2), {0: 0.7, 1: 1.4, 2: 1.2, 3: -0.03})
    ws = torch.full((int(L.lib.frcnn_photometric_workspace(75, 93)),), 0xFF, dtype=torch.uint8, device="cuda")
    oa = raw_photometric(L, a, dev(pa), ws)                                  # no synchronisation in between: stream order alone
    ob = raw_photometric(L, b, dev(pb), ws)
    oa2 = raw_photometric(L, a, dev(pa), ws)
    assert np.array_equal(oa.cpu().numpy(), R.apply_plan(a.cpu().numpy(), pa))
    assert np.array_equal(ob.cpu().numpy(), R.apply_plan(b.cpu().numpy(), pb))
    assert torch.equal(oa, oa2)
    za, zb = dev(R.seeded_frame(32, 40, 51)), dev(np.full((40, 51, 3), 7, np.uint8))
    ca, _ = raw_zoom_out(L, za, torch.zeros((0, 4), device="cuda"), (64, 77), (5, 9))
    cb, _ = raw_zoom_out(L, zb, torch.zeros((0, 4), device="cuda"), (64, 77), (24, 26))
    assert np.array_equal(ca.cpu().numpy(), R.zoom_out(za.cpu().numpy(), np.zeros((0, 4)), (64, 77), (5, 9))[0])
    assert np.array_equal(cb.cpu().numpy(), np.full((64, 77, 3), 7, np.uint8))


def test_luma_sum_past_32_bits(T):
    """4105 x 4105 pixels of L = 255 sum to 4 297 011 375 > 2^32: the mean is 255 and contrast leaves the frame as it is.  A 32-bit
    accumulator finds a mean of 0 and halves every byte."""
    assert 4105 * 4105 * 255 == 4297011375 > 1 << 32
    img = torch.full((4105, 4105, 3), 255, dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(img)
    T.photometric_distort(img, dev(R.plan((R.CONTRAST,), {R.CONTRAST: 0.5})), out=out)
    assert bool((out == 255).all())


def test_plans_written_on_the_device(T):
    img = R.seeded_frame(41, 45, 67)
    d_img, d_plan = dev(img), torch.empty(8, dtype=torch.int32, device="cuda")
    plans = {
        "skipped slot": [R.SATURATION, bits(1.3), 17, bits(0.5), R.CONTRAST, bits(0.8), R.HUE, 250],
        "repeated op": [R.BRIGHTNESS, bits(1.2), R.HUE, 9, R.BRIGHTNESS, bits(0.5), R.CONTRAST, bits(1.4)],
        "contrast first": [R.CONTRAST, bits(1.5), R.HUE, 3, R.SATURATION, bits(0.6), R.BRIGHTNESS, bits(0.9)],
        "contrast last": [R.HUE, 255, R.BRIGHTNESS, bits(1.45), R.SATURATION, bits(1.5), R.CONTRAST, bits(0.5)],
        "negative op, contrast only": [-3, 0, R.CONTRAST, bits(0.75), 4, 0, R.CONTRAST, bits(1.5)],
        "all skipped": [-1, 0, 4, bits(0.5), 1 << 20, 0, -2147483648, 7],
    }
    for what, plan in plans.items():
        d_plan.copy_(torch.tensor(plan, dtype=torch.int32))
        out = T.photometric_distort(d_img, d_plan).cpu().numpy()
        assert np.array_equal(out, R.apply_plan(img, plan)), what
    assert np.array_equal(out, img)                                          # the all-skip plan: the output is the input


def test_capture_once_replay_with_three_plans(T):
    img, boxes = R.seeded_frame(43, 61, 83), np.array([[3, 4, 30.5, 40.25], [10, 0, 83, 61]], np.float32)
    plans = [R.plan((1, 0, 3, 2), {0: 0.8, 1: 1.3, 2: 0.7, 3: 0.05}), R.plan((3, 2, 1, 0), {0: 1.5, 1: 0.5, 2: 1.0, 3: -0.06}),
             np.array([2, bits(1.1), -1, 0, -1, 0, -1, 0], np.int32)]
    d_img, d_boxes, d_plan = dev(img), dev(boxes), dev(plans[0])

    def run():
        return T.zoom_out(T.photometric_distort(d_img, d_plan), d_boxes, (100, 141), (17, 40))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        canvas, bo = run()
    for plan in plans[1:] + plans[:1]:
        d_plan.copy_(torch.from_numpy(plan))
        g.replay()
        rc, rb = R.zoom_out(R.apply_plan(img, plan), boxes, (100, 141), (17, 40))
        assert np.array_equal(canvas.cpu().numpy(), rc) and np.array_equal(bo.cpu().numpy(), rb)
        ec, eb = run()
        assert torch.equal(ec, canvas) and torch.equal(eb, bo)


STAGE = [((37, 53), (2, 0, 3, 1), ((60, 90), (11, 20)), False),           # everything, no cap
         ((30, 100), (1, 3, 0, 2), ((40, 130), (10, 30)), True),          # 80 / 40 * 130 > 133: max_size caps the resize
         ((64, 48), None, ((64, 48), (0, 0)), True),                      # no photometric distortion, a zoom-out of scale 1
         ((45, 45), (3, 1, 2, 0), None, False)]                           # no zoom-out


@pytest.mark.parametrize("k", range(len(STAGE)))
def test_augment_stage_equals_restatement_then_oracle_preprocess(T, k):
    from oracle import oracle as orc
    (h, w), order, zoom, flip = STAGE[k]
    rng = np.random.RandomState(50 + k)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    x1, y1 = rng.uniform(0, w / 2, 6), rng.uniform(0, h / 2, 6)
    boxes = np.stack([x1, y1, x1 + rng.uniform(2, w / 2, 6), y1 + rng.uniform(2, h / 2, 6)], 1).astype(np.float32)
    plan = None if order is None else T.photometric_plan(order, {0: rng.uniform(0.5, 1.5), 1: rng.uniform(0.5, 1.5), 2: rng.uniform(0.5, 1.5),
                                                                   3: rng.uniform(-18 / 255., 18 / 255.)})
    stage = T.DeviceAugmentStage(size=80, max_size=133, size_divisible=32)
    x, b, meta = stage(dev(img), dev(boxes), plan=plan, zoom=zoom, flip=flip)
    ref_img = img if plan is None else R.apply_plan(img, plan)
    ref_boxes = boxes
    if zoom is not None:
        ref_img, ref_boxes = R.zoom_out(ref_img, boxes, zoom[0], zoom[1])
    H, W = ref_img.shape[:2]
    oh, ow = T.get_size((W, H), 80, 133)
    ph, pw = T.padded_size(oh, ow, 32)
    if k == 1:
        assert (oh, ow) == (41, 133)                                         # capped: not 80 on the short side
    assert meta == {"size": (oh, ow), "padded": (ph, pw), "orig_size": (H, W)} and x.shape == (1, 3, ph, pw)
    assert np.array_equal(x[0].cpu().numpy(), orc.preprocess_image(ref_img, (oh, ow), (ph, pw), flip)[1])
    assert np.array_equal(b.cpu().numpy(), orc.preprocess_boxes(ref_boxes, (W, H), (ow, oh), flip))


def test_error_codes_of_the_four_entry_points(T, L):
    lib = L.lib
    img, out, plan = torch.zeros((8, 9, 3), dtype=torch.uint8, device="cuda"), torch.zeros((8, 9, 3), dtype=torch.uint8, device="cuda"), dev(np.full(8, -1, np.int32))
    canvas = torch.zeros((16, 20, 3), dtype=torch.uint8, device="cuda")
    boxes, bo = torch.zeros((2, 4), device="cuda"), torch.zeros((2, 4), device="cuda")
    nb = int(lib.frcnn_photometric_workspace(8, 9))
    nz = int(lib.frcnn_zoom_out_workspace(8, 9, 16, 20))
    ws = torch.zeros(max(nb, nz), dtype=torch.uint8, device="cuda")
    assert nb > 0 and nz > 0
    for hw in ((0, 9), (8, 0), (32768, 9), (8, 32768), (-1, 9)):
        assert lib.frcnn_photometric_workspace(*hw) == 0
        assert lib.frcnn_photometric(vp(img), hw[0], hw[1], vp(plan), vp(out), vp(ws), nb, stream()) == -1
    assert lib.frcnn_photometric_workspace(32767, 32767) > 0
    for args in ((None, 8, 9, vp(plan), vp(out), vp(ws)), (vp(img), 8, 9, None, vp(out), vp(ws)), (vp(img), 8, 9, vp(plan), None, vp(ws)),
                 (vp(img), 8, 9, vp(plan), vp(out), None)):
        assert lib.frcnn_photometric(*args, nb, stream()) == -1 and b"NULL" in lib.frcnn_last_error()
    assert lib.frcnn_photometric(vp(img), 8, 9, vp(plan), vp(img), vp(ws), nb, stream()) == -1 and b"overlaps" in lib.frcnn_last_error()
    assert lib.frcnn_photometric(vp(img), 8, 9, vp(plan), vp(out), vp(ws), nb - 1, stream()) == -3
    zo = lambda **kw: lib.frcnn_zoom_out(*[kw.get(k, d) for k, d in (("src", vp(img)), ("h", 8), ("w", 9), ("new_h", 16), ("new_w", 20), ("top", 3), ("left", 4),  # noqa: E731
                                                                    ("boxes", vp(boxes)), ("n", 2), ("canvas", vp(canvas)), ("boxes_out", vp(bo)),
                                                                    ("ws", vp(ws)), ("nb", nz), ("stream", stream()))])
    for bad in (dict(src=None), dict(canvas=None), dict(ws=None), dict(boxes=None), dict(boxes_out=None), dict(n=-1), dict(h=0), dict(w=32768),
                dict(new_h=32768), dict(new_w=0), dict(new_h=7), dict(new_w=8), dict(top=-1), dict(top=9), dict(left=-1), dict(left=12),
                dict(canvas=vp(img))):
        assert zo(**bad) == -1, bad
    assert zo(nb=nz - 1) == -3
    for shape in ((0, 9, 16, 20), (8, 9, 7, 20), (8, 9, 16, 8), (8, 9, 32768, 20)):
        assert lib.frcnn_zoom_out_workspace(*shape) == 0
    assert zo(top=8, left=11) == 0 and zo(n=0, boxes=None, boxes_out=None) == 0          # the extreme paste; no boxes is legal
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.photometric_distort(torch.zeros((4, 4, 3), dtype=torch.uint8), plan)
    with pytest.raises(L.FrcnnError, match="leaves the canvas"):
        T.zoom_out(img, boxes, (16, 20), (9, 0))
