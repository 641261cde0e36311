"""tests/photometric_ref.py (the numpy restatement of photometric_distort_ and zoom_out_ the GPU tests compare the kernels with) held to
the results of the reference's own code under Pillow (tests/golden/photometric.npz, written by tests/golden/make_golden_photometric.py)
with np.array_equal, the whole-colour-cube hashes included; where Pillow is importable, to Pillow directly as well.  No GPU."""
import hashlib

import numpy as np
import pytest

import photometric_ref as R


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


@pytest.fixture(scope="module")
def cube():
    return R.cube()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def test_golden_file_holds_the_required_kinds(gold):
    counts = dict(zip(gold["required_names"].tolist(), gold["required_counts"].tolist()))
    assert len(counts) == 27 and all(v > 0 for v in counts.values()), counts
    assert counts["orders_on_37x53"] == 24
    assert len({tuple(gold["p_order%02d_order" % k]) for k in range(24)}) == 24


def test_photometric_cases_equal_the_reference(gold):
    for name in gold["p_names"].tolist():
        out = R.photometric(R.case_input(gold, name), gold[name + "_order"], gold[name + "_factors"])
        if name + "_out" in gold.files:
            assert np.array_equal(out, gold[name + "_out"]), name
        else:
            assert sha(out) == gold[name + "_sha"].tobytes(), name


def test_two_pixel_mean_of_ten_and_a_half_rounds_up(gold):
    img = gold["p_two_pixels_img"]
    assert R.luma(img).tolist() == [[10, 11]] and R.contrast_mean(img) == 11
    assert np.array_equal(R.contrast(img, 0.0), np.full_like(img, 11))


def test_zoom_out_cases_equal_the_reference(gold):
    for name in gold["z_names"].tolist():
        canvas, boxes = R.zoom_out(gold[name + "_img"], gold[name + "_boxes"], gold[name + "_new_hw"], gold[name + "_top_left"])
        assert np.array_equal(canvas, gold[name + "_canvas"]), name
        assert boxes.dtype == np.float32 and np.array_equal(boxes, gold[name + "_boxes_out"]), name
    assert R.median(gold["z_half_img"]) == (200, 240, 84)              # the upper level of the half-and-half channel


@pytest.mark.parametrize("shift", [0, 13, 243])
def test_hue_on_every_colour(gold, cube, shift):
    assert sha(R.hue(cube, shift)) == gold["cube_hue_%d" % shift].tobytes()


def test_a_hue_shift_of_zero_is_not_the_identity(cube):
    assert not np.array_equal(R.hue(cube[:64], 0), cube[:64])


@pytest.mark.parametrize("f", [0.5, 1.0, 1.5])
def test_saturation_on_every_colour(gold, cube, f):
    assert sha(R.saturation(cube, f)) == gold["cube_saturation_%.1f" % f].tobytes()


@pytest.mark.parametrize("f", [0.5, 1.5])
def test_brightness_on_every_colour(gold, cube, f):
    assert sha(R.brightness(cube, f)) == gold["cube_brightness_%.1f" % f].tobytes()


@pytest.mark.parametrize("f", [0.5, 1.0, 1.5])
def test_blend_on_every_level_and_byte(gold, f):
    level, byte = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert np.array_equal(R.blend(level, byte, f), gold["contrast_table_%.1f" % f])


def test_plan_rules():
    img = R.seeded_frame(5, 9, 11)
    bits = lambda f: int(np.array(f, np.float32).view(np.int32))      # noqa: E731
    assert np.array_equal(R.apply_plan(img, [-1, 0, 4, 0, 99, 7, -7, 1]), img)                                     # all skipped
    assert np.array_equal(R.apply_plan(img, [0, bits(1.2), 0, bits(0.5), -1, 0, -1, 0]), R.brightness(img, 1.2))   # a repeated op
    assert R.hue_shift(-18 / 255.) in (238, 239) and R.hue_shift(0.0) == 0 and R.hue_shift(-0.9 / 255.) == 0 and R.hue_shift(13.5 / 255.) == 13


def test_package_plan_equals_the_restatement():
    import random

    from faster_rcnn_pytorch_amd import transforms as T
    rng = random.Random(9)
    for _ in range(50):
        order, factors = T.draw_photometric(rng)
        assert sorted(order) == [0, 1, 2, 3] and all(0.5 <= factors[op] <= 1.5 for op in (0, 1, 2)) and abs(factors[3]) <= 18 / 255.
        assert np.array_equal(T.photometric_plan(order, factors), R.plan(order, factors))
        (nh, nw), (top, left) = T.draw_zoom_out(37, 53, 3, rng)
        assert 37 <= nh <= 111 and 53 <= nw <= 159 and 0 <= top <= nh - 37 and 0 <= left <= nw - 53
    with pytest.raises(ValueError, match="at most once"):
        T.photometric_plan([0, 0], {0: 1.0})
    assert T.photometric_plan([3], {3: -13.5 / 255.}).tolist() == [3, 243, -1, -1, -1, -1, -1, -1]


def test_restatement_equals_pillow_directly():
    """Pillow itself, where it is importable (any version: a difference here means Pillow changed, the golden file says for which)."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageStat
    img = R.seeded_frame(77, 45, 61)
    im = Image.fromarray(img, "RGB")
    assert np.array_equal(R.rgb_to_hsv(img), np.array(im.convert("HSV")))
    assert np.array_equal(R.hsv_to_rgb(img), np.array(Image.fromarray(img, "HSV").convert("RGB")))
    assert np.array_equal(R.luma(img), np.array(im.convert("L")))
    for f in (0.5, 0.83, 1.0, 1.37, 1.5):
        assert np.array_equal(R.brightness(img, f), np.array(ImageEnhance.Brightness(im).enhance(f)))
        assert np.array_equal(R.contrast(img, f), np.array(ImageEnhance.Contrast(im).enhance(f)))
        assert np.array_equal(R.saturation(img, f), np.array(ImageEnhance.Color(im).enhance(f)))
    assert list(R.median(img)) == list(ImageStat.Stat(im).median)
