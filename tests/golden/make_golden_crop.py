#!/usr/bin/env python
"""Generates tests/golden/crop.npz by RUNNING the reference's own crop, resize, hflip, RandomSizeCrop, CenterCrop, ToTensor and Normalize
(new_datasets/transforms.py) with Pillow -- the way make_golden_mosaic.py runs datasets/transforms_.py.  Re-run:

    python tests/golden/make_golden_crop.py          # FRCNN_REFERENCE=<checkout of the reference>

new_datasets/transforms.py imports torchvision (not installed) for F.crop, F.resize, F.hflip, F.to_tensor, F.normalize and
T.RandomCrop.get_params, and util.box_ops / util.misc, which want torchvision.__version__ and torchvision.ops.boxes.box_area at import.
This script registers a stub torchvision of its own in sys.modules: the F calls are the PIL / torch calls torchvision makes for a PIL
image (img.crop((j, i, j + w, i + h)), img.resize((w, h), BILINEAR), transpose(FLIP_LEFT_RIGHT), from_numpy().permute().float().div(255),
sub(mean).div(std)), and get_params draws the corner uniformly and RECORDS the region it returns.  The reference file is loaded by path
under a synthetic `new_datasets` package.  Nothing of the reference is stored: only inputs, recorded regions and results.

Cases (frames of at most 64 x 80 unless said otherwise), all stored whole:
  small cases  resize (up, down, down by more than 2, equal size, none) then crop; the KINDS below are counted and asserted
  list cases   0, 1, 255, 256, 257 and 700 boxes (the compaction's chunk seams); one list keeps every box, one keeps none
  center       CenterCrop whose round() falls on a half, through the class itself
  stage_*      the chain DeviceMultiScaleStage runs, on both branches, flip off and on: [resize, crop,] hflip, resize, ToTensor, Normalize
  full         a 480 x 640 frame: RandomResize([600]), a seeded RandomSizeCrop(384, 600), RandomResize([800], 1333), through the classes;
               the images are stored as sha256, the boxes whole."""
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def load_reference():
    names = ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.ops", "torchvision.ops.boxes")
    tv, tvt, tvf, tvo, tvb = (types.ModuleType(n) for n in names)
    tv.__version__ = "0.15.0"
    tvb.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    tvf.crop = lambda img, i, j, h, w: img.crop((j, i, j + w, i + h))
    tvf.resize = lambda img, size: img.resize((size[1], size[0]), Image.BILINEAR)
    tvf.hflip = lambda img: img.transpose(Image.FLIP_LEFT_RIGHT)
    tvf.to_tensor = lambda img: torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().float().div(255)
    tvf.normalize = lambda t, mean, std: t.sub(torch.tensor(mean)[:, None, None]).div(torch.tensor(std)[:, None, None])

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            region = (0, 0, h, w) if (w == tw and h == th) else (random.randint(0, h - th), random.randint(0, w - tw), th, tw)
            RECORDED.append(region)
            return region
    tvt.RandomCrop, tvt.functional, tv.transforms, tvo.boxes, tv.ops = RandomCrop, tvf, tvt, tvb, tvo
    sys.modules.update(dict(zip(names, (tv, tvt, tvf, tvo, tvb))))
    if REF not in sys.path:
        sys.path.insert(0, REF)                   # util.box_ops, util.misc
    pkg = types.ModuleType("new_datasets")
    pkg.__path__ = [os.path.join(REF, "new_datasets")]
    sys.modules["new_datasets"] = pkg
    spec = importlib.util.spec_from_file_location("new_datasets.transforms", os.path.join(REF, "new_datasets", "transforms.py"))
    tr = importlib.util.module_from_spec(spec)
    sys.modules["new_datasets.transforms"] = tr
    spec.loader.exec_module(tr)
    return tr


sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]           # tests/ and the repository root (crop_ref imports oracle)
import crop_ref  # noqa: E402  (tests/crop_ref.py: resize_boxes / crop_boxes only to COUNT the kinds of box; seeded_case for the lists, full_frame)


def target_of(boxes, labels, area, iscrowd):
    """The reference's crop reads target["iscrowd"] unconditionally (transforms.py:25, 53-54: a KeyError without it), so a case WITHOUT
    iscrowd hands it zeros and drops what comes back; an absent area is really absent (crop makes its own, :33-35)."""
    t = {"boxes": torch.from_numpy(boxes.copy()), "labels": torch.from_numpy(labels.copy())}
    if area is not None:
        t["area"] = torch.from_numpy(area.copy())
    t["iscrowd"] = torch.from_numpy(iscrowd.copy()) if iscrowd is not None else torch.zeros(len(labels), dtype=torch.int64)
    return t


def reference_crop(tr, c):
    """resize (skipped for resize_hw None: a plain crop) then crop, through the reference's functions."""
    img, t = Image.fromarray(c["img"], "RGB"), target_of(c["boxes"], c["labels"], c["area"], c["iscrowd"])
    if c["resize_hw"] is not None:
        img, t = tr.resize(img, t, (c["resize_hw"][1], c["resize_hw"][0]))               # a (w, h) tuple is taken as is
        assert img.size == (c["resize_hw"][1], c["resize_hw"][0])
    img, t = tr.crop(img, t, tuple(int(v) for v in c["region"]))
    assert t["boxes"].dtype == torch.float32 and t["area"].dtype == torch.float32 and t["labels"].dtype == torch.int64
    assert t["size"].tolist() == list(c["region"][2:])
    return np.array(img), t["boxes"].numpy(), t["labels"].numpy(), t["area"].numpy(), t["iscrowd"].numpy() if c["iscrowd"] is not None else None


def to_source(b, hw, hw1):
    """A box wanted at these resized coordinates, as source coordinates (the float32 product lands near, not on, the target)."""
    sy, sx = hw[0] / hw1[0], hw[1] / hw1[1]
    return [b[0] * sx, b[1] * sy, b[2] * sx, b[3] * sy]


def adverse_boxes(region, hw, hw1):
    """Every kind of box around a region, in coordinates of the resized frame mapped to the source.  With hw1 == hw the map is exact."""
    i, j, h, w = region
    H1, W1 = hw1
    x0, y0, x1, y1 = j, i, j + w, i + h
    mx, my = j + w / 2.0, i + h / 2.0
    bs = [[x0 + w / 4.0, y0 + h / 4.0, mx, my],                               # wholly inside
          [x0 - 9, y0 + 1, x0 - 2, my], [x1 + 2, y0 + 1, x1 + 9, my],         # wholly outside: left, right
          [x0 + 1, y0 - 9, mx, y0 - 2], [x0 + 1, y1 + 2, mx, y1 + 9],         # above, below
          [x0 - 5, y0 + 1, mx, my], [mx, y0 + 1, x1 + 5, my],                 # cut: left, right
          [x0 + 1, y0 - 5, mx, my], [x0 + 1, my, mx, y1 + 5],                 # cut: top, bottom
          [x0 - 6, y0 + 1, x0, my], [x1, y0 + 1, x1 + 6, my],                 # touch the left / right edge from outside: clipped to zero width
          [x0 + 1, y0 - 6, mx, y0], [x0 + 1, y1, mx, y1 + 6],                 # touch the top / bottom edge: clipped to zero height
          [mx, my, x1, y1], [x0, y0, mx, my],                                 # end exactly on the region's far / near edges
          [mx, y0 + 1, mx, my], [x0 + 1, my, mx, my],                         # zero area at the source
          [np.nan, y0 + 1, mx, my], [x0 + 1, y0 + 1, mx, np.nan],             # a NaN coordinate
          [mx, y0 + 1, x0 + 1, my], [x0 + 1, my, mx, y0 + 1]]                 # x2 < x1, y2 < y1
    return np.array([to_source(b, hw, hw1) for b in bs], np.float32)


def small_cases():
    rng = np.random.RandomState(47)
    cases = {}

    def add(name, hw, hw1, region, boxes=None, area=True, iscrowd=True):
        H1, W1 = hw1 or hw
        b = adverse_boxes(region, hw, (H1, W1)) if boxes is None else boxes
        n = len(b)
        cases[name] = dict(img=rng.randint(0, 256, hw + (3,)).astype(np.uint8), resize_hw=hw1, region=region, boxes=b,
                           labels=rng.randint(0, 90, n).astype(np.int64), area=rng.uniform(1, 500, n).astype(np.float32) if area else None,
                           iscrowd=rng.randint(0, 2, n).astype(np.int64) if iscrowd else None)

    add("plain_mid", (48, 64), None, (10, 12, 20, 30))                                   # no resize at all: exact coordinates
    add("plain_no_area", (48, 64), None, (10, 12, 20, 30), area=False, iscrowd=False)
    add("plain_only_iscrowd", (48, 64), None, (7, 9, 21, 33), area=False)
    add("plain_only_area", (48, 64), None, (7, 9, 21, 33), iscrowd=False)
    add("equal_top_left", (40, 56), (40, 56), (0, 0, 17, 23))                            # resize to an equal size (Pillow copies)
    add("equal_last_pixel", (40, 56), (40, 56), (21, 30, 19, 26))                        # ends on the last row and column
    add("equal_whole", (33, 47), (33, 47), (0, 0, 33, 47))
    add("equal_1x1", (33, 47), (33, 47), (16, 23, 1, 1))
    add("up_mid", (37, 53), (61, 88), (9, 14, 30, 41))
    add("up_bottom_right", (37, 53), (61, 88), (31, 40, 30, 48))
    add("up_top", (37, 53), (61, 88), (0, 20, 25, 31), area=False)
    add("down_left", (64, 80), (48, 60), (11, 0, 25, 31))
    add("down_bottom", (64, 80), (48, 60), (30, 13, 18, 40), iscrowd=False)
    add("down_whole", (64, 80), (48, 60), (0, 0, 48, 60))
    add("down3_mid", (64, 80), (20, 25), (5, 6, 9, 12))                                  # scale 3.2: seven-tap windows that reach past the region
    add("down3_right", (64, 80), (20, 25), (0, 13, 20, 12))
    add("down3_1x1", (64, 80), (20, 25), (19, 24, 1, 1))
    add("mixed_wide", (50, 40), (35, 72), (3, 20, 30, 50))                               # down-scaled rows, up-scaled columns
    add("same_w", (50, 80), (100, 80), (40, 8, 37, 64))                                  # one axis at scale 1 through the resampler
    return cases


KINDS = ("inside", "outside_left", "outside_right", "outside_top", "outside_bottom", "cut_left", "cut_right", "cut_top", "cut_bottom",
         "clipped_to_zero_width", "clipped_to_zero_height", "ends_on_edge_x", "ends_on_edge_y", "zero_area_at_source", "nan_coordinate",
         "x2_below_x1", "region_at_top", "region_at_left", "region_at_bottom", "region_at_right", "region_ends_on_last_pixel",
         "region_is_whole_frame", "region_1x1", "resize_up", "resize_down", "resize_equal", "no_resize", "resize_down_more_than_2",
         "window_reaches_outside_region", "with_area", "without_area", "with_iscrowd", "without_iscrowd")


def count_kinds(cases):
    n = dict.fromkeys(KINDS, 0)
    for c in cases.values():
        h, w = c["img"].shape[:2]
        H1, W1 = c["resize_hw"] or (h, w)
        i, j, ch, cw = c["region"]
        n["region_at_top"] += i == 0
        n["region_at_left"] += j == 0
        n["region_at_bottom"] += i + ch == H1
        n["region_at_right"] += j + cw == W1
        n["region_ends_on_last_pixel"] += i + ch == H1 and j + cw == W1 and (i, j) != (0, 0)
        n["region_is_whole_frame"] += (i, j, ch, cw) == (0, 0, H1, W1)
        n["region_1x1"] += (ch, cw) == (1, 1)
        n["no_resize"] += c["resize_hw"] is None
        n["resize_equal"] += c["resize_hw"] == (h, w)
        n["resize_up"] += H1 > h and W1 > w
        n["resize_down"] += H1 < h and W1 < w
        n["resize_down_more_than_2"] += h > 2 * H1 and w > 2 * W1
        n["window_reaches_outside_region"] += h > 2 * H1 and w > 2 * W1 and i > 0 and j > 0 and i + ch < H1 and j + cw < W1
        n["with_area"] += c["area"] is not None
        n["without_area"] += c["area"] is None
        n["with_iscrowd"] += c["iscrowd"] is not None
        n["without_iscrowd"] += c["iscrowd"] is None
        src = torch.from_numpy(c["boxes"])
        s = crop_ref.resize_boxes(src, (H1, W1), (h, w)) - torch.as_tensor([j, i, j, i])            # shifted, before the clip
        cb, _, keep = crop_ref.crop_boxes(crop_ref.resize_boxes(src, (H1, W1), (h, w)), c["region"])
        ok = ~torch.isnan(s).any(1) & (src[:, 2] > src[:, 0]) & (src[:, 3] > src[:, 1])
        n["inside"] += int((keep & (cb == s).all(1) & (s[:, 2] < cw) & (s[:, 3] < ch) & (s[:, 0] > 0) & (s[:, 1] > 0)).sum())
        n["outside_left"] += int((ok & ~keep & (s[:, 2] < 0)).sum())
        n["outside_right"] += int((ok & ~keep & (s[:, 0] > cw)).sum())
        n["outside_top"] += int((ok & ~keep & (s[:, 3] < 0)).sum())
        n["outside_bottom"] += int((ok & ~keep & (s[:, 1] > ch)).sum())
        n["cut_left"] += int((keep & (s[:, 0] < 0)).sum())
        n["cut_right"] += int((keep & (s[:, 2] > cw)).sum())
        n["cut_top"] += int((keep & (s[:, 1] < 0)).sum())
        n["cut_bottom"] += int((keep & (s[:, 3] > ch)).sum())
        n["clipped_to_zero_width"] += int((ok & ~keep & (cb[:, 2] == cb[:, 0]) & ((s[:, 2] == 0) | (s[:, 0] == cw))).sum())
        n["clipped_to_zero_height"] += int((ok & ~keep & (cb[:, 3] == cb[:, 1]) & ((s[:, 3] == 0) | (s[:, 1] == ch))).sum())
        n["ends_on_edge_x"] += int((keep & ((s[:, 2] == cw) | (s[:, 0] == 0))).sum())
        n["ends_on_edge_y"] += int((keep & ((s[:, 3] == ch) | (s[:, 1] == 0))).sum())
        n["zero_area_at_source"] += int((~keep & ~torch.isnan(s).any(1) & ((src[:, 2] == src[:, 0]) | (src[:, 3] == src[:, 1]))).sum())
        n["nan_coordinate"] += int((~keep & torch.isnan(s).any(1)).sum())
        n["x2_below_x1"] += int((~keep & ~torch.isnan(s).any(1) & ((src[:, 2] < src[:, 0]) | (src[:, 3] < src[:, 1]))).sum())
    missing = [k for k, v in n.items() if v == 0]
    assert not missing, "the small cases lack: %s" % missing
    return n


LIST_SIZES = (0, 1, 255, 256, 257, 700)


def list_cases():
    """The compaction's chunk seams on a 48 x 64 frame resized to 60 x 80, region (12, 16, 30, 40).  keep: 'mixed' (crop_ref.seeded_case),
    'all' (every box inside), 'none' (every box left of the region)."""
    cases = {}
    hw, hw1, region = (48, 64), (60, 80), (12, 16, 30, 40)
    for n in LIST_SIZES:
        for keep in ("mixed",) + (("all", "none") if n in (257, 700) else ()):
            img, b, lab, crowd = crop_ref.seeded_case(1000 + n, hw[0], hw[1], hw1, region, n)
            rng = np.random.RandomState(2000 + n)
            if keep != "mixed":
                x1, y1 = rng.uniform(18, 40, n), rng.uniform(14, 30, n)
                b = np.stack([x1, y1, x1 + rng.uniform(1, 14, n), y1 + rng.uniform(1, 10, n)], 1)
                if keep == "none":
                    b[:, 0::2] -= 40
                b = np.array([to_source(r, hw, hw1) for r in b], np.float32).reshape(-1, 4)
            cases["list_%d_%s" % (n, keep)] = dict(img=img, resize_hw=hw1, region=region, boxes=b, labels=np.arange(n, dtype=np.int64),
                                                   area=rng.uniform(1, 500, n).astype(np.float32), iscrowd=crowd)
    return cases


def center_case(tr):
    """CenterCrop((40, 51)) on a 45 x 60 frame: (45 - 40) / 2 = 2.5 and (60 - 51) / 2 = 4.5, both halves; round() goes to even."""
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (45, 60, 3)).astype(np.uint8)
    seen = []
    inner = tr.crop

    def recording(image, target, region):
        seen.append(tuple(int(v) for v in region))
        return inner(image, target, region)
    tr.crop = recording
    boxes = adverse_boxes((2, 4, 40, 51), (45, 60), (45, 60))
    c = dict(img=img, resize_hw=None, boxes=boxes, labels=rng.randint(0, 90, len(boxes)).astype(np.int64), area=None,
             iscrowd=rng.randint(0, 2, len(boxes)).astype(np.int64))
    out_img, t = tr.CenterCrop((40, 51))(Image.fromarray(img, "RGB"), target_of(boxes, c["labels"], None, c["iscrowd"]))
    tr.crop = inner
    assert seen == [(2, 4, 40, 51)], seen
    c["region"] = seen[0]
    return c, (np.array(out_img), t["boxes"].numpy(), t["labels"].numpy(), t["area"].numpy(), t["iscrowd"].numpy())


STAGE = dict(scales=(48,), max_size=70, crop_sizes=(56,), crop_min=24, crop_max=40)        # the small stage of the stage_* cases


def stage_cases(tr):
    """[resize(56), crop(region),] hflip, resize(48, max_size=70), ToTensor, Normalize on a 64 x 80 frame, through the reference's
    functions and classes, in the order DeviceMultiScaleStage runs them."""
    rng = np.random.RandomState(77)
    img = rng.randint(0, 256, (64, 80, 3)).astype(np.uint8)
    region = (9, 21, 33, 38)                                              # in the 56 x 70 frame
    boxes = adverse_boxes(region, (64, 80), (56, 70))
    boxes = boxes[~np.isnan(boxes).any(1)]                                # the plain branch keeps every row: keep its output comparable
    labels = rng.randint(0, 90, len(boxes)).astype(np.int64)
    out = {"stage_img": img, "stage_boxes": boxes, "stage_labels": labels, "stage_region": np.array(region, np.int32),
           "stage_resize_hw": np.array([56, 70], np.int32)}
    for branch in ("plain", "crop"):
        for flip in (0, 1):
            im, t = Image.fromarray(img, "RGB"), target_of(boxes, labels, None, None)
            if branch == "crop":
                im, t = tr.RandomResize([STAGE["crop_sizes"][0]])(im, t)
                assert im.size == (70, 56)
                im, t = tr.crop(im, t, region)
            if flip:
                im, t = tr.hflip(im, t)
            im, t = tr.RandomResize([STAGE["scales"][0]], max_size=STAGE["max_size"])(im, t)
            x, t = tr.ToTensor()(im, t)
            x, t = tr.Normalize(MEAN, STD)(x, t)
            key = "stage_%s_flip%d" % (branch, flip)
            out[key + "_x"], out[key + "_boxes"], out[key + "_labels"] = x.numpy(), t["boxes"].numpy(), t["labels"].numpy()
    assert out["stage_plain_flip0_x"].shape == (3, 48, 60) and len(out["stage_crop_flip0_boxes"]) < len(boxes)
    return out


def full_case(tr):
    img, boxes, labels, crowd = crop_ref.full_frame()
    random.seed(384600)
    del RECORDED[:]
    im, t = Image.fromarray(img, "RGB"), target_of(boxes, labels, None, crowd)
    im, t = tr.RandomResize([600])(im, t)
    assert im.size == (800, 600)
    im, t = tr.RandomSizeCrop(384, 600)(im, t)
    assert len(RECORDED) == 1
    crop_img, cb, cl, ca, cc = np.array(im), t["boxes"].numpy(), t["labels"].numpy(), t["area"].numpy(), t["iscrowd"].numpy()
    im, t = tr.RandomResize([800], max_size=1333)(im, t)
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)        # noqa: E731
    assert 0 < len(cb) < 24
    return {"full_region": np.array(RECORDED[0], np.int32), "full_sha_crop": sha(crop_img), "full_crop_boxes": cb, "full_crop_labels": cl,
            "full_crop_area": ca, "full_crop_iscrowd": cc, "full_sha_final": sha(np.array(im)), "full_final_hw": np.array(im.size[::-1], np.int32),
            "full_final_boxes": t["boxes"].numpy(), "full_final_area": t["area"].numpy()}


def main():
    tr = load_reference()
    out = {}
    cases = small_cases()
    counts = count_kinds(cases)
    lists = list_cases()
    cases.update(lists)
    results = {name: reference_crop(tr, c) for name, c in cases.items()}
    cases["center"], results["center"] = center_case(tr)
    kept = {name: len(results[name][1]) for name in lists}
    assert sorted(int(k.split("_")[1]) for k in lists if k.endswith("mixed")) == sorted(LIST_SIZES)
    assert kept["list_700_all"] == 700 and kept["list_257_all"] == 257 and kept["list_700_none"] == 0 and kept["list_257_none"] == 0
    assert all(0 < kept["list_%d_mixed" % n] < n for n in LIST_SIZES if n > 1)
    # area in the target or not, the crop's area is the clipped box's: the same boxes with and without give the same result
    for a, b in (("plain_mid", "plain_no_area"), ("plain_only_iscrowd", "plain_only_area")):
        assert np.array_equal(cases[a]["boxes"], cases[b]["boxes"], equal_nan=True) and np.array_equal(results[a][3], results[b][3])
    for name, c in cases.items():
        img, b, l, a, crowd = results[name]
        i, j, ch, cw = c["region"]
        h, w = c["img"].shape[:2]
        H1, W1 = c["resize_hw"] or (h, w)
        assert img.shape == (ch, cw, 3) and img.dtype == np.uint8 and len(b) == len(l) == len(a)
        out[name + "_meta"] = np.array([H1, W1, i, j, ch, cw, c["iscrowd"] is not None, c["area"] is not None, c["resize_hw"] is not None], np.int64)
        out[name + "_img"], out[name + "_boxes"], out[name + "_labels"] = c["img"], c["boxes"], c["labels"]
        if c["iscrowd"] is not None:
            out[name + "_iscrowd"], out[name + "_iscrowd_out"] = c["iscrowd"], crowd
        out[name + "_img_out"], out[name + "_boxes_out"], out[name + "_labels_out"], out[name + "_area_out"] = img, b, l, a
    out["case_names"] = np.array(sorted(cases))
    out["kind_names"], out["kind_counts"] = np.array(KINDS), np.array([counts[k] for k in KINDS], np.int64)
    out.update(stage_cases(tr))
    out.update(full_case(tr))
    path = os.path.join(OUT, "crop.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    print("wrote crop.npz: %d arrays, %d bytes; Pillow %s; %d cases; kinds %s; kept %s; full region %s, %d boxes" %
          (len(out), os.path.getsize(path), Image.__version__, len(cases), counts, kept, out["full_region"].tolist(), len(out["full_crop_boxes"])))


if __name__ == "__main__":
    main()
