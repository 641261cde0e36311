#!/usr/bin/env python
"""Generates tests/golden/mosaic.npz by RUNNING the reference's own mosaic code (datasets/mosaic_transform.py on
datasets/transforms_.py) with Pillow -- the way make_golden_voc_eval.py runs the reference's evaluator.  Re-run:

    python tests/golden/make_golden_mosaic.py          # FRCNN_REFERENCE=<checkout of the reference>

datasets/transforms_.py imports torchvision (not installed) for F.crop, F.resize, F.hflip and T.RandomCrop.get_params only.  This
script registers a stub `torchvision.transforms(.functional)` of its own in sys.modules: the three F calls are the PIL calls
torchvision makes for a PIL image (img.crop((j, i, j + w, i + h)), img.resize((w, h), BILINEAR), transpose(FLIP_LEFT_RIGHT)), and
get_params draws the corner uniformly and RECORDS the region it returns.  The two reference files are loaded by path under a
synthetic `datasets` package (a plain `import datasets` finds an unrelated installed package).  Nothing of the reference is stored:
only inputs, recorded regions and results.

Two kinds of case:
  small_*  size 48, crops of 24..48 (load_mosaic hardcodes 384, so the tiles are composed here from the reference's Resize, crop_,
           Resize, shift_mosaic_boxes and get_concat_*); inputs, canvas, boxes, labels, regions, fallback flags stored whole.  The
           adverse kinds listed in ADVERSE are counted and asserted.
  full     size 600 through load_mosaic itself; the four frames are regenerated from seeds, the canvas is stored as a sha256."""
import hashlib
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

REF = os.environ.get("FRCNN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
RECORDED = []                                     # regions get_params returned, in call order
CROPS = []                                        # per crop_ call: 1 when it handed back the uncropped image


def load_reference():
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tvf.crop = lambda img, i, j, h, w: img.crop((j, i, j + w, i + h))
    tvf.resize = lambda img, size: img.resize((size[1], size[0]), Image.BILINEAR)
    tvf.hflip = lambda img: img.transpose(Image.FLIP_LEFT_RIGHT)

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            region = (0, 0, h, w) if (w == tw and h == th) else (random.randint(0, h - th), random.randint(0, w - tw), th, tw)
            RECORDED.append(region)
            return region
    tvt.RandomCrop, tvt.functional, tv.transforms = RandomCrop, tvf, tvt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    mods = {}
    for name in ("transforms_", "mosaic_transform"):
        spec = importlib.util.spec_from_file_location("datasets." + name, os.path.join(REF, "datasets", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["datasets." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    tr = mods["transforms_"]
    inner = tr.crop_

    def crop_recording(image, boxes, labels, region, min_overlap_ratio=0.3):
        out = inner(image, boxes, labels, region, min_overlap_ratio)
        CROPS.append(int(out[0] is image))
        return out
    tr.crop_ = crop_recording                     # RandomSizeCrop looks crop_ up in its module at call time
    return tr, mods["mosaic_transform"]


def reference_small(tr, mo, imgs, boxes, labels, regions, size, max_size):
    tiles, bs, ls = [], [], []
    del CROPS[:]
    for k in range(4):
        im, b, l = Image.fromarray(imgs[k], "RGB"), torch.from_numpy(boxes[k].copy()), torch.from_numpy(labels[k].copy())
        im, b, l = tr.Resize(size, max_size=max_size)(im, b, l)
        im, b, l = tr.crop_(im, b, l, tuple(int(v) for v in regions[k]))
        im, b, l = tr.Resize((size, size))(im, b, l)
        b = mo.shift_mosaic_boxes(boxes=b, shift_x=(k & 1) * size, shift_y=(k >> 1) * size)
        tiles.append(im), bs.append(b), ls.append(l)
    canvas = mo.get_concat_v_cut_center(mo.get_concat_h_cut_center(tiles[0], tiles[1]), mo.get_concat_h_cut_center(tiles[2], tiles[3]))
    return np.array(canvas), torch.cat(bs).numpy(), torch.cat(ls).numpy(), np.array(CROPS, np.uint8)


# ---- the small cases ---------------------------------------------------------------------------------------------
sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]           # tests/ and the repository root (mosaic_ref imports oracle)
import mosaic_ref  # noqa: E402  (tests/mosaic_ref.py: first_resize_hw / scale_boxes / crop_keep only to PLACE and COUNT the adverse boxes; full_frame: the seeded frames)


def to_source(box_resized, hw, hw1):
    """A box wanted at these resized coordinates, as source coordinates (the float32 product lands near, not on, the target)."""
    sy, sx = hw[0] / hw1[0], hw[1] / hw1[1]
    return [box_resized[0] * sx, box_resized[1] * sy, box_resized[2] * sx, box_resized[3] * sy]


def near_threshold_box(rng, hw, hw1, region, above):
    """A box cut by the region's left edge whose kept-area ratio is within 1e-3 of 0.3, on the asked side (found by seeded search)."""
    i, j, h, w = region
    for _ in range(100000):
        width = rng.uniform(8, min(20, j / 0.7))
        x1 = j - 0.7 * width + rng.uniform(-0.02, 0.02)
        y1 = i + rng.uniform(1, h / 2 - 1)
        src = np.array([to_source([x1, y1, x1 + width, y1 + rng.uniform(4, h / 2 - 1)], hw, hw1)], np.float32)
        b1 = mosaic_ref.scale_boxes(torch.from_numpy(src), hw1, hw)
        c, keep = mosaic_ref.crop_keep(b1, region)
        r = float(((c[0, 2] - c[0, 0]) * (c[0, 3] - c[0, 1])) / ((b1[0, 2] - b1[0, 0]) * (b1[0, 3] - b1[0, 1])))
        if (0.3 < r < 0.301 and above and bool(keep[0])) or (0.299 < r <= 0.3 and not above and not bool(keep[0])):
            return src[0]
    raise AssertionError("no box found")


def small_cases():
    rng = np.random.RandomState(31)
    cases = {}

    def frame(h, w):
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)

    def rand_boxes(n, hw, hw1, region):
        """n boxes well inside the region (all kept)."""
        i, j, h, w = region
        out = []
        for _ in range(n):
            x1, y1 = j + rng.uniform(0, w / 2), i + rng.uniform(0, h / 2)
            out.append(to_source([x1, y1, x1 + rng.uniform(4, w / 2 - 1), y1 + rng.uniform(4, h / 2 - 1)], hw, hw1))
        return out

    # -- mixed: landscape (up-scaling crop, the adverse boxes), portrait (every box lost), square (no boxes), crop == whole frame
    size, max_size = 48, 1333
    hws = [(40, 60), (70, 50), (64, 64), (100, 130)]
    hw1 = [mosaic_ref.first_resize_hw(h, w, size, max_size) for h, w in hws]
    assert hw1 == [(48, 72), (67, 48), (48, 48), (48, 62)], hw1
    regions = [(5, 24, 30, 40), (40, 20, 26, 28), (0, 0, 24, 24), (0, 0, 48, 62)]
    b0 = rand_boxes(3, hws[0], hw1[0], regions[0])
    b0.insert(1, near_threshold_box(rng, hws[0], hw1[0], regions[0], above=True))
    b0.insert(3, near_threshold_box(rng, hws[0], hw1[0], regions[0], above=False))
    b0.append(to_source([2, 8, 20, 30], hws[0], hw1[0]))                  # left of the region: both x clamp to 0 -> a side of exactly 0
    b0.append(to_source([66, 8, 71, 30], hws[0], hw1[0]))                 # right of it: both x become w
    b0.append([30.0, 10.0, 30.0, 25.0])                                   # zero-area source box inside the region: 0 / 0 = NaN
    b0 += rand_boxes(1, hws[0], hw1[0], regions[0])
    b1 = [to_source([2, 2, 30, 20], hws[1], hw1[1]), to_source([1, 5, 15, 38], hws[1], hw1[1])]       # above / left of the crop
    b3 = rand_boxes(4, hws[3], hw1[3], regions[3])
    cases["small_mixed"] = dict(size=size, max_size=max_size, imgs=[frame(*s) for s in hws], regions=regions,
                                boxes=[b0, b1, [], b3])
    # -- capped: a wide source that max_size = 100 caps; a region on every border, one ending on the frame's last row and column
    size, max_size = 48, 100
    hws = [(40, 100), (50, 37), (48, 80), (90, 61)]
    hw1 = [mosaic_ref.first_resize_hw(h, w, size, max_size) for h, w in hws]
    assert hw1[0] == (40, 100) and mosaic_ref.first_resize_hw(40, 100, size, 1333) == (48, 120), hw1
    regions = [(hw1[0][0] - 25, hw1[0][1] - 31, 25, 31), (0, 0, 30, 24), (hw1[2][0] - 24, 0, 24, 40), (0, hw1[3][1] - 29, 33, 29)]
    cases["small_capped"] = dict(size=size, max_size=max_size, imgs=[frame(*s) for s in hws], regions=regions,
                                 boxes=[rand_boxes(2, hws[k], hw1[k], regions[k]) + [to_source([0, 0, 9, 9], hws[k], hw1[k])] for k in range(4)])
    # -- down: larger sources, an odd size, strong first down-scale; tile 3 falls back to a frame that is then squeezed
    size, max_size = 37, 1333
    hws = [(111, 170), (150, 97), (74, 74), (120, 200)]
    hw1 = [mosaic_ref.first_resize_hw(h, w, size, max_size) for h, w in hws]
    regions = [(3, 9, 24, 37), (20, 5, 30, 25), (0, 0, 37, 37), (6, 20, 27, 35)]
    cases["small_down"] = dict(size=size, max_size=max_size, imgs=[frame(*s) for s in hws], regions=regions,
                               boxes=[rand_boxes(2, hws[0], hw1[0], regions[0]), rand_boxes(3, hws[1], hw1[1], regions[1]),
                                      rand_boxes(2, hws[2], hw1[2], regions[2]), [to_source([1, 1, 12, 5], hws[3], hw1[3])]])
    for c in cases.values():
        c["boxes"] = [np.asarray(b, np.float32).reshape(-1, 4) for b in c["boxes"]]
        c["labels"] = [rng.randint(0, 20, len(b)).astype(np.int64) for b in c["boxes"]]
        c["regions"] = np.asarray(c["regions"], np.int32)
    return cases


ADVERSE = ("landscape", "portrait", "square", "capped_by_max_size", "tile_loses_every_box", "tile_without_boxes", "ratio_just_above_0.3",
           "ratio_just_below_0.3", "clamped_side_exactly_zero", "zero_area_source_box_nan", "crop_is_whole_frame", "region_at_top",
           "region_at_left", "region_at_bottom", "region_at_right", "region_ends_on_last_pixel", "second_resize_up_and_down_in_one_mosaic")


def count_adverse(cases, results):
    n = dict.fromkeys(ADVERSE, 0)
    for name, c in cases.items():
        fallback = results[name][3]
        up = down = False
        for k in range(4):
            h, w = c["imgs"][k].shape[:2]
            H1, W1 = mosaic_ref.first_resize_hw(h, w, c["size"], c["max_size"])
            i, j, rh, rw = (int(v) for v in c["regions"][k])
            n["landscape"] += w > h
            n["portrait"] += h > w
            n["square"] += h == w
            n["capped_by_max_size"] += (H1, W1) != mosaic_ref.first_resize_hw(h, w, c["size"], None)
            n["tile_loses_every_box"] += bool(fallback[k]) and len(c["boxes"][k]) > 0
            n["tile_without_boxes"] += len(c["boxes"][k]) == 0
            n["crop_is_whole_frame"] += (i, j, rh, rw) == (0, 0, H1, W1) and not fallback[k]
            n["region_at_top"] += i == 0
            n["region_at_left"] += j == 0
            n["region_at_bottom"] += i + rh == H1
            n["region_at_right"] += j + rw == W1
            n["region_ends_on_last_pixel"] += i + rh == H1 and j + rw == W1 and (i, j) != (0, 0)
            uh, uw = (H1, W1) if fallback[k] else (rh, rw)
            up |= uh < c["size"] or uw < c["size"]
            down |= uh > c["size"] or uw > c["size"]
            b1 = mosaic_ref.scale_boxes(torch.from_numpy(c["boxes"][k]), (H1, W1), (h, w))
            cb, keep = mosaic_ref.crop_keep(b1, c["regions"][k])
            ratio = ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])) / ((b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]))
            n["ratio_just_above_0.3"] += int(((ratio > 0.3) & (ratio < 0.301) & keep).sum())
            n["ratio_just_below_0.3"] += int(((ratio <= 0.3) & (ratio > 0.299) & ~keep).sum())
            n["clamped_side_exactly_zero"] += int((((cb[:, 2] - cb[:, 0]) == 0) | ((cb[:, 3] - cb[:, 1]) == 0)).sum())
            n["zero_area_source_box_nan"] += int((torch.isnan(ratio) & ~keep).sum())
        n["second_resize_up_and_down_in_one_mosaic"] += up and down
    missing = [k for k, v in n.items() if v == 0]
    assert not missing, "the small cases lack: %s" % missing
    return n


# ---- the full-size case through load_mosaic itself ------------------------------------------------------------------
def reference_full(mo):
    random.seed(2024)
    del RECORDED[:], CROPS[:]
    order = [0]
    img, boxes, labels = mosaic_ref.full_frame(0)

    def load_image(index):
        order.append(index)
        return Image.fromarray(mosaic_ref.full_frame(index)[0], "RGB")
    canvas, b, l = mo.load_mosaic(None, len(mosaic_ref.FULL_SHAPES), 600, load_image, lambda index: index,
                                  lambda index: (mosaic_ref.full_frame(index)[1].tolist(), mosaic_ref.full_frame(index)[2].tolist()),
                                  Image.fromarray(img, "RGB"), torch.from_numpy(boxes), torch.from_numpy(labels))
    assert len(order) == 4 and len(RECORDED) == 4 and len(CROPS) == 4
    return np.array(order, np.int64), np.array(RECORDED, np.int32), np.array(canvas), b.numpy(), l.numpy(), np.array(CROPS, np.uint8)


def main():
    tr, mo = load_reference()
    out = {}
    cases = small_cases()
    results = {}
    for name, c in cases.items():
        results[name] = reference_small(tr, mo, c["imgs"], c["boxes"], c["labels"], c["regions"], c["size"], c["max_size"])
        canvas, b, l, fb = results[name]
        assert canvas.shape == (2 * c["size"], 2 * c["size"], 3) and canvas.dtype == np.uint8 and b.dtype == np.float32 and l.dtype == np.int64
        out[name + "_meta"] = np.array([c["size"], c["max_size"]], np.int64)
        out[name + "_regions"] = c["regions"]
        for k in range(4):
            out["%s_img%d" % (name, k)], out["%s_boxes%d" % (name, k)], out["%s_labels%d" % (name, k)] = c["imgs"][k], c["boxes"][k], c["labels"][k]
        out[name + "_canvas"], out[name + "_boxes_out"], out[name + "_labels_out"], out[name + "_fallback"] = canvas, b, l, fb
    counts = count_adverse(cases, results)
    out["small_names"] = np.array(sorted(cases))
    out["adverse_names"], out["adverse_counts"] = np.array(ADVERSE), np.array([counts[k] for k in ADVERSE], np.int64)
    order, regions, canvas, b, l, fb = reference_full(mo)
    assert canvas.shape == (1200, 1200, 3)
    out["full_order"], out["full_regions"], out["full_boxes_out"], out["full_labels_out"], out["full_fallback"] = order, regions, b, l, fb
    out["full_sha_canvas"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(canvas).tobytes()).digest(), np.uint8)
    np.savez_compressed(os.path.join(OUT, "mosaic.npz"), **out)
    print("wrote mosaic.npz: %d arrays; Pillow %s; adverse counts %s; full: frames %s, fallback %s, %d boxes" %
          (len(out), Image.__version__, counts, order.tolist(), fb.tolist(), len(b)))


if __name__ == "__main__":
    main()
