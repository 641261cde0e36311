#!/usr/bin/env python
"""Generates tests/golden/photometric.npz by RUNNING the reference's own photometric_distort_ and zoom_out_ (datasets/transforms_.py:38-58,
130-147) under Pillow -- the way make_golden_mosaic.py runs its mosaic code.  Re-run:

    python tests/golden/make_golden_photometric.py          # FRCNN_REFERENCE=<checkout of the reference>

datasets/transforms_.py imports torchvision (not installed) and calls F.adjust_brightness / adjust_contrast / adjust_saturation /
adjust_hue.  This script registers a stub `torchvision.transforms(.functional)` whose four functions are what torchvision's PIL backend
does for a PIL image, TAKEN FROM ITS DOCUMENTATION, not run here: ImageEnhance.Brightness / Contrast / Color(img).enhance(f), and for
the hue: split img.convert("HSV"), add uint8(int32(f * 255)) to the H plane with uint8 wrap-around, merge, convert("RGB").
ImageStat.Stat._getmedian, which zoom_out_ calls, no longer exists in Pillow 12.2: it is aliased here to the `median` property, which
runs the same rule (the first level whose cumulative count exceeds count // 2).  random.shuffle / uniform / randint are wrapped: they
RECORD every draw, and return a scripted draw where a case needs one (all 24 orders, factors of exactly 0.5 / 1.0 / 1.5, the extreme
paste positions).  Nothing of the reference is stored: only inputs, draws and results.

  p_*     photometric cases: input (whole when small -- once for the 24 orders --, else the seed of photometric_ref.seeded_frame), order, factors, output (whole, or a
          sha256 when large)
  z_*     zoom-out cases: input, boxes, new_hw, top_left, canvas, boxes_out
  cube_*  Pillow itself on the 4096 x 4096 frame that holds every colour once: sha256 of the hue / saturation / brightness results
  contrast_table_*  Image.blend over all (degenerate level, byte) pairs, 65 536 bytes per factor
The REQUIRED kinds are counted and asserted."""
import hashlib
import importlib.util
import itertools
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageStat

REF = os.environ.get("FRCNN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(OUT)]
import photometric_ref as R  # noqa: E402  (tests/photometric_ref.py: hue_shift, seeded_frame, cube and luma only to BUILD and COUNT the cases)

OP_OF = {"adjust_brightness": 0, "adjust_contrast": 1, "adjust_saturation": 2, "adjust_hue": 3}
DRAWS = {"order": None, "uniform": [], "randint": []}          # what the wrapped generator returned, in call order
SCRIPT = {"order": None, "uniform": [], "randint": []}         # what it must return next (empty: a real draw)
_shuffle, _uniform, _randint = random.shuffle, random.uniform, random.randint


def shuffle(x):
    if SCRIPT["order"] is not None:
        x.sort(key=lambda d: SCRIPT["order"].index(OP_OF[d.__name__]))
        SCRIPT["order"] = None
    else:
        _shuffle(x)
    DRAWS["order"] = [OP_OF[d.__name__] for d in x]


def uniform(a, b):
    v = SCRIPT["uniform"].pop(0) if SCRIPT["uniform"] else _uniform(a, b)
    assert a <= v <= b
    DRAWS["uniform"].append(v)
    return v


def randint(a, b):
    v = SCRIPT["randint"].pop(0) if SCRIPT["randint"] else _randint(a, b)
    v = b if v == "max" else v
    assert a <= v <= b
    DRAWS["randint"].append(v)
    return v


def adjust_hue(img, f):
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.int32(f * 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def load_reference():
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")

    def adjust_brightness(img, f):
        return ImageEnhance.Brightness(img).enhance(f)

    def adjust_contrast(img, f):
        return ImageEnhance.Contrast(img).enhance(f)

    def adjust_saturation(img, f):
        return ImageEnhance.Color(img).enhance(f)
    tvf.adjust_brightness, tvf.adjust_contrast, tvf.adjust_saturation, tvf.adjust_hue = adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue
    tvt.functional, tv.transforms = tvf, tvt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    if not hasattr(ImageStat.Stat, "_getmedian"):
        ImageStat.Stat._getmedian = lambda self: self.median
    random.shuffle, random.uniform, random.randint = shuffle, uniform, randint          # transforms_.py calls random.<name> at call time
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    spec = importlib.util.spec_from_file_location("datasets.transforms_", os.path.join(REF, "datasets", "transforms_.py"))
    tr = importlib.util.module_from_spec(spec)
    sys.modules["datasets.transforms_"] = tr
    spec.loader.exec_module(tr)
    return tr


def run_photometric(tr, img, order=None, factors=None):
    """photometric_distort_ on a uint8 array -> (output array, order drawn, factors drawn as [4] indexed by op)."""
    DRAWS["order"], DRAWS["uniform"] = None, []
    if order is not None:
        SCRIPT["order"] = list(order)
    if factors is not None:
        SCRIPT["uniform"] = [factors[op] for op in (order if order is not None else [])]
        assert order is not None
    out, _, _ = tr.photometric_distort_(Image.fromarray(img, "RGB"), None, None)
    assert not SCRIPT["uniform"] and len(DRAWS["uniform"]) == 4
    fac = np.zeros(4, np.float64)
    for op, f in zip(DRAWS["order"], DRAWS["uniform"]):
        fac[op] = f
    return np.array(out), np.array(DRAWS["order"], np.int32), fac


def run_zoom(tr, img, boxes, max_scale, scale=None, left=None, top=None):
    DRAWS["uniform"], DRAWS["randint"] = [], []
    SCRIPT["uniform"] = [] if scale is None else [scale]
    SCRIPT["randint"] = [] if left is None else [left, top]
    out, b, _ = tr.zoom_out_(Image.fromarray(img, "RGB"), torch.from_numpy(boxes.copy()), None, max_scale)
    (left, top) = DRAWS["randint"]
    canvas = np.array(out)
    return canvas, b.numpy(), np.array(canvas.shape[:2], np.int32), np.array([top, left], np.int32), DRAWS["uniform"][0]


STORE_INPUT_BYTES, STORE_OUTPUT_BYTES = 16384, 110000
REQUIRED = ("orders_on_37x53", "shape_1x1", "shape_1x7", "shape_5x3", "shape_64x64", "shape_257x129", "shape_301x517", "one_colour_frame",
            "grey_frame", "factor_exactly_0.5", "factor_exactly_1.0", "factor_exactly_1.5", "factor_below_1", "factor_above_1", "hue_shift_0",
            "hue_factor_negative", "two_pixels_mean_10.5_rounds_to_11", "zoom_left_top_zero", "zoom_left_top_max", "zoom_scale_1",
            "zoom_odd_canvas_width", "zoom_channel_split_half_and_half", "zoom_bimodal_channel", "zoom_three_different_medians",
            "zoom_n_0", "zoom_n_1", "zoom_n_700")


def main():
    tr = load_reference()
    random.seed(2025)
    rng = np.random.RandomState(57)
    out, n = {}, dict.fromkeys(REQUIRED, 0)
    p_names = []

    def photometric_case(name, img=None, seed=None, hw=None, order=None, factors=None, store_img=True):
        if img is None:
            img = R.seeded_frame(seed, *hw)
        res, order, fac = run_photometric(tr, img, order, factors)
        p_names.append(name)
        if seed is not None and img.nbytes > STORE_INPUT_BYTES:
            out[name + "_seed"] = np.array([seed, img.shape[0], img.shape[1]], np.int64)
        elif store_img:
            out[name + "_img"] = img
        out[name + "_order"], out[name + "_factors"] = order, fac
        if res.nbytes > STORE_OUTPUT_BYTES:
            out[name + "_sha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(res).tobytes()).digest(), np.uint8)
        else:
            out[name + "_out"] = res
        h, w = img.shape[:2]
        if "shape_%dx%d" % (h, w) in n:
            n["shape_%dx%d" % (h, w)] += 1
        flat = img.reshape(-1, 3)
        n["one_colour_frame"] += bool((flat == flat[0]).all()) and len(flat) > 1
        n["grey_frame"] += bool((flat[:, 0] == flat[:, 1]).all() and (flat[:, 1] == flat[:, 2]).all()) and len(np.unique(flat[:, 0])) > 2
        for op in (0, 1, 2):
            for v in (0.5, 1.0, 1.5):
                n["factor_exactly_%.1f" % v] += fac[op] == v
            n["factor_below_1"] += fac[op] < 1
            n["factor_above_1"] += fac[op] > 1
        n["hue_shift_0"] += R.hue_shift(fac[3]) == 0
        n["hue_factor_negative"] += fac[3] < 0 and R.hue_shift(fac[3]) != 0
        return res, order, fac

    base = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    for k, order in enumerate(itertools.permutations(range(4))):
        photometric_case("p_order%02d" % k, base, order=order, store_img=False)
        n["orders_on_37x53"] += 1
    out["p_order_img"] = base                                          # the 24 order cases share one input
    assert len({tuple(out["p_order%02d_order" % k]) for k in range(24)}) == 24
    for h, w in ((1, 1), (1, 7), (5, 3), (64, 64), (257, 129), (301, 517)):
        photometric_case("p_shape_%dx%d" % (h, w), seed=1000 + h, hw=(h, w))
    photometric_case("p_one_colour", np.tile(np.array([200, 30, 90], np.uint8), (5, 7, 1)))
    g = rng.randint(0, 256, (6, 5)).astype(np.uint8)
    photometric_case("p_grey", np.stack([g, g, g], -1))
    photometric_case("p_exact_a", base[:9, :11].copy(), order=(2, 0, 3, 1), factors={0: 0.5, 1: 1.0, 2: 1.5, 3: 0.0})
    photometric_case("p_exact_b", base[9:20, 5:18].copy(), order=(1, 3, 2, 0), factors={0: 1.5, 1: 0.5, 2: 1.0, 3: -18 / 255.})
    photometric_case("p_exact_c", base[20:30, 7:20].copy(), order=(3, 2, 1, 0), factors={0: 1.0, 1: 1.5, 2: 0.5, 3: 18 / 255.})
    two = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)
    assert R.luma(two).tolist() == [[10, 11]] and ImageStat.Stat(Image.fromarray(two, "RGB").convert("L")).mean[0] == 10.5
    photometric_case("p_two_pixels", two, order=(1, 0, 2, 3), factors={0: 1.25, 1: 0.5, 2: 0.8, 3: 0.02})
    assert int(ImageStat.Stat(Image.fromarray(two, "RGB").convert("L")).mean[0] + 0.5) == 11
    assert np.array_equal(np.array(ImageEnhance.Contrast(Image.fromarray(two, "RGB")).enhance(0.0)), np.full_like(two, 11))
    n["two_pixels_mean_10.5_rounds_to_11"] += 1
    out["p_names"] = np.array(p_names)

    # ---- zoom-out ----
    z_names = []

    def boxes_for(img, k):
        h, w = img.shape[:2]
        x1, y1 = rng.uniform(0, w * 0.6, k), rng.uniform(0, h * 0.6, k)
        return np.stack([x1, y1, x1 + rng.uniform(1, w * 0.4, k), y1 + rng.uniform(1, h * 0.4, k)], 1).astype(np.float32).reshape(-1, 4)

    def zoom_case(name, img, k, max_scale=3, **script):
        b = boxes_for(img, k)
        canvas, bo, new_hw, top_left, scale = run_zoom(tr, img, b, max_scale, **script)
        z_names.append(name)
        out[name + "_img"], out[name + "_boxes"], out[name + "_new_hw"], out[name + "_top_left"] = img, b, new_hw, top_left
        out[name + "_canvas"], out[name + "_boxes_out"], out[name + "_scale"] = canvas, bo, np.array([scale], np.float64)
        h, w = img.shape[:2]
        assert tuple(new_hw) == (int(scale * h), int(scale * w)) and bo.dtype == np.float32 and bo.shape == b.shape
        top, left = (int(v) for v in top_left)
        n["zoom_left_top_zero"] += (top, left) == (0, 0) and tuple(new_hw) != (h, w)
        n["zoom_left_top_max"] += (top, left) == (new_hw[0] - h, new_hw[1] - w) and top > 0 and left > 0
        n["zoom_scale_1"] += tuple(new_hw) == (h, w)
        n["zoom_odd_canvas_width"] += new_hw[1] % 2 == 1
        if "zoom_n_%d" % k in n:
            n["zoom_n_%d" % k] += 1
        flat = img.reshape(-1, 3)
        med = R.median(img)
        assert list(med) == list(ImageStat.Stat(Image.fromarray(img, "RGB")).median)
        for c in range(3):
            lv, cnt = np.unique(flat[:, c], return_counts=True)
            n["zoom_channel_split_half_and_half"] += len(lv) == 2 and cnt[0] == cnt[1] and med[c] == lv[1]
            n["zoom_bimodal_channel"] += len(lv) == 2 and cnt[0] != cnt[1]
        n["zoom_three_different_medians"] += len(set(med)) == 3

    zoom_case("z_origin", rng.randint(0, 256, (20, 31, 3)).astype(np.uint8), 1, scale=1.7, left=0, top=0)
    zoom_case("z_max", rng.randint(0, 256, (17, 23, 3)).astype(np.uint8), 700, scale=2.31, left="max", top="max")
    zoom_case("z_scale1", rng.randint(0, 256, (9, 14, 3)).astype(np.uint8), 0, scale=1.0)
    half = np.empty((4, 6, 3), np.uint8)
    half[..., 0] = np.array([50] * 12 + [200] * 12).reshape(4, 6)[:, rng.permutation(6)]
    half[..., 1] = np.array([10] * 9 + [240] * 15).reshape(4, 6)
    half[..., 2] = np.arange(24).reshape(4, 6) * 7
    zoom_case("z_half", half, 1, scale=2.5)
    zoom_case("z_random", rng.randint(0, 256, (33, 47, 3)).astype(np.uint8), 5)
    zoom_case("z_wide", (rng.randint(0, 256, (12, 70, 3)) // 3 + np.array([0, 60, 150])).astype(np.uint8), 3)
    out["z_names"] = np.array(z_names)

    # ---- Pillow itself on every colour, and the blend on every (level, byte) pair ----
    cube = R.cube()
    im = Image.fromarray(cube, "RGB")
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(np.array(a)).tobytes()).digest(), np.uint8)      # noqa: E731
    for shift, f in ((0, 0.0), (13, 13.5 / 255.), (243, -13.5 / 255.)):
        assert R.hue_shift(f) == shift
        out["cube_hue_%d" % shift] = sha(adjust_hue(im, f))
    for f in (0.5, 1.0, 1.5):
        out["cube_saturation_%.1f" % f] = sha(ImageEnhance.Color(im).enhance(f))
    for f in (0.5, 1.5):
        out["cube_brightness_%.1f" % f] = sha(ImageEnhance.Brightness(im).enhance(f))
    ramp = Image.fromarray(np.arange(256, dtype=np.uint8)[None], "L")
    for f in (0.5, 1.0, 1.5):
        out["contrast_table_%.1f" % f] = np.stack([np.array(Image.blend(Image.new("L", (256, 1), m), ramp, f))[0] for m in range(256)])
    missing = [k for k, v in n.items() if v == 0]
    assert not missing, "the cases lack: %s" % missing
    out["required_names"], out["required_counts"] = np.array(REQUIRED), np.array([int(n[k]) for k in REQUIRED], np.int64)
    path = os.path.join(OUT, "photometric.npz")
    np.savez_compressed(path, **out)
    print("wrote photometric.npz: %d arrays, %d bytes; Pillow %s; counts %s" % (len(out), os.path.getsize(path), Image.__version__, {k: int(v) for k, v in n.items()}))


if __name__ == "__main__":
    main()
